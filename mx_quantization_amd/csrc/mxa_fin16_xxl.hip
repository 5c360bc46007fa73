// Launches of the 16-row finishing kernel of rows of 4,097 .. 16,384 keys (mxa_finish16_xxl.hpp: k <= 64,
// float32).  Compiled twice (build_native.py): MXA_F16XXL_W4=0 the MXINT8-P instantiations
// (launch_finish16_xxl_w8), MXA_F16XXL_W4=1 the MXINT4-P ones (launch_finish16_xxl_w4).
#include "mxa_finish16_xxl.hpp"
#include "mxa_launch.hpp"

#ifndef MXA_F16XXL_W4
#define MXA_F16XXL_W4 0
#endif
#if MXA_F16XXL_W4
#define MXA_F16XXL_FN launch_finish16_xxl_w4
#else
#define MXA_F16XXL_FN launch_finish16_xxl_w8
#endif

namespace mxa {

constexpr bool kF16XxlW4 = MXA_F16XXL_W4 != 0;

// the LDS bytes of a workgroup of w waves: two chunks of V block scales and w chunk areas, whatever T is
static auto finish16_xxl_lds_of(const Rows2Args& ra) {
  return [D = ra.D](int w) { return fin16_xxl_lds(D, w).total; };
}
template <int NB, int KS, bool EXTRA>
static int launch_finish16_xxl_x(const Rows2Args& ra, int BH, hipStream_t stream) {
  constexpr auto kernel = &finish16_xxl_kernel<NB, KS, EXTRA, kF16XxlW4>;
  return launch_finish_waves<kernel>(ra, kFin16, finish16_xxl_lds_of(ra), BH, stream);
}
template <int NB>
static int launch_finish16_xxl_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  // EXTRA: a bias, the debug true scores or bfloatX rounding
  const bool extra = ra.bias || ra.true_out || (ra.bfloat != 0 && ra.bfloat != 32);
  auto ks = [&](auto ks_c) {
    constexpr int KS = decltype(ks_c)::value;
    return extra ? launch_finish16_xxl_x<NB, KS, true>(ra, BH, stream) : launch_finish16_xxl_x<NB, KS, false>(ra, BH, stream);
  };
  // four lanes per row: slots ceil(k / 4), the sizes of finish16_kernel
  const int n = (ra.k_top + 3) / 4;
  if (n <= 5) return ks(std::integral_constant<int, 5>{});
  if (n <= 8) return ks(std::integral_constant<int, 8>{});
  if (n <= 12) return ks(std::integral_constant<int, 12>{});
  return ks(std::integral_constant<int, 16>{});
}

int MXA_F16XXL_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  if (!xxl_rows_ok(ra.T, ra.k_top) || ra.xo_codes || ra.s_dt != kF32 || ra.in_dt != kF32) return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return finish_tile_plan(kFin16, ra.N, BH, finish16_xxl_lds_of(ra), finish_wave_cap(2), &w, &r);
  }
  return dispatch_nbd(ra.nbd, [&](auto nb) { return launch_finish16_xxl_nb<decltype(nb)::value>(ra, BH, stream); });
}

}  // namespace mxa
