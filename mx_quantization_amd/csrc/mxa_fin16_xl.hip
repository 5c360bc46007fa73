// Launches of the chunked 16-row finishing kernel (mxa_finish16_xl.hpp: rows of 1,025 .. 4,096
// keys, k <= 64, float32).  Compiled twice (build_native.py): MXA_F16XL_W4=0 the MXINT8-P
// instantiations (launch_finish16_xl_w8), MXA_F16XL_W4=1 the MXINT4-P ones (launch_finish16_xl_w4).
// A third compilation, MXA_F16XL_XDT=1 (MXINT8 P), holds the float16 / bfloat16 instantiations
// (launch_finish16_xl_x1: mxa_attention_dt).
#include "mxa_finish16_xl.hpp"
#include "mxa_launch.hpp"

#ifndef MXA_F16XL_W4
#define MXA_F16XL_W4 0
#endif
#ifndef MXA_F16XL_XDT
#define MXA_F16XL_XDT 0
#endif
#if MXA_F16XL_XDT
#define MXA_F16XL_FN launch_finish16_xl_x1
#elif MXA_F16XL_W4
#define MXA_F16XL_FN launch_finish16_xl_w4
#else
#define MXA_F16XL_FN launch_finish16_xl_w8
#endif

namespace mxa {

constexpr bool kF16XlW4 = MXA_F16XL_W4 != 0;
constexpr bool kF16XlXdt = MXA_F16XL_XDT != 0;
static_assert(!(kF16XlW4 && kF16XlXdt), "MXINT4 P: float32 only");

// the LDS bytes of a workgroup of w waves
static auto finish16_xl_lds_of(const Rows2Args& ra) {
  return [D = ra.D, ntb = ra.ntb](int w) { return fin16_xl_lds(D, ntb, w).total; };
}
template <int NB, int KS, bool EXTRA>
static int launch_finish16_xl_x(const Rows2Args& ra, int BH, hipStream_t stream) {
  constexpr auto kernel = &finish16_xl_kernel<NB, KS + (kF16XlXdt ? kFin16XlDtKS : 0), EXTRA, kF16XlW4>;
  return launch_finish_waves<kernel>(ra, kFin16, finish16_xl_lds_of(ra), BH, stream);
}
template <int NB>
static int launch_finish16_xl_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  // EXTRA: a bias, the debug true scores or bfloatX rounding (float16 / bfloat16 always round)
  const bool extra = kF16XlXdt || ra.bias || ra.true_out || (ra.bfloat != 0 && ra.bfloat != 32);
  auto ks = [&](auto ks_c) {
    constexpr int KS = decltype(ks_c)::value;
    if (extra) return launch_finish16_xl_x<NB, KS, true>(ra, BH, stream);
    if constexpr (!kF16XlXdt) return launch_finish16_xl_x<NB, KS, false>(ra, BH, stream);
    return (int)MXA_ERR_UNSUPPORTED;
  };
  // four lanes per row: slots ceil(k / 4), the sizes of finish16_kernel
  const int n = (ra.k_top + 3) / 4;
  if (n <= 5) return ks(std::integral_constant<int, 5>{});
  if (n <= 8) return ks(std::integral_constant<int, 8>{});
  if (n <= 12) return ks(std::integral_constant<int, 12>{});
  return ks(std::integral_constant<int, 16>{});
}

int MXA_F16XL_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  // (launch_rows chooses the unit by the call's dtypes; the plan pass runs before they are bound)
  // (any kept-index list of 1 .. 64 keys: finish_choice decides which k reach it -- mxa_attention_nth's every one)
  if (!xl_rows(ra.T) || ra.T > kXlRowsT || ra.k_top < 1 || ra.k_top > 64 || ra.xo_codes || (!kF16XlXdt && (ra.s_dt != kF32 || ra.in_dt != kF32))) return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return finish_tile_plan(kFin16, ra.N, BH, finish16_xl_lds_of(ra), finish_wave_cap(2), &w, &r);
  }
  return dispatch_nbd(ra.nbd, [&](auto nb) { return launch_finish16_xl_nb<decltype(nb)::value>(ra, BH, stream); });
}

}  // namespace mxa
