// Launches of the 16-row finishing kernel (mxa_finish16.hpp: k <= 64).  Compiled twice
// (build_native.py): MXA_F16_XDT=0 the float32 instantiations (launch_finish16_x0),
// MXA_F16_XDT=1 the float16 / bfloat16 ones (launch_finish16_x1), so that they build in
// parallel with the other finishing kernels.  A third compilation, MXA_F16_LONG=1 (float32
// only), holds the LONG instantiations for rows of 513 .. 1,024 keys (launch_finish16_l0).
// MXA_F16_W4=1 (float32 only, with or without MXA_F16_LONG): the MXINT4-P instantiations of
// mxa_attention_bits at width 4 (launch_finish16_x0w4, launch_finish16_l0w4).
// MXA_F16_LXO=1 (float32, MXINT8 P): the LONG instantiations that write the proj Linear's MX input codes
// (launch_finish16_l0xo: the fused blocks on rows of 513 .. 1,024 keys), and nothing else -- a unit of
// its own, so that every other unit keeps the code it had.
#include "mxa_finish16.hpp"
#include "mxa_launch.hpp"

#ifndef MXA_F16_XDT
#define MXA_F16_XDT 0
#endif
#ifndef MXA_F16_LONG
#define MXA_F16_LONG 0
#endif
#ifndef MXA_F16_W4
#define MXA_F16_W4 0
#endif
#ifndef MXA_F16_LXO
#define MXA_F16_LXO 0
#endif
#if MXA_F16_LXO
#undef MXA_F16_LONG
#define MXA_F16_LONG 1
#define MXA_F16_FN launch_finish16_l0xo
#elif MXA_F16_W4 && MXA_F16_LONG
#define MXA_F16_FN launch_finish16_l0w4
#elif MXA_F16_W4
#define MXA_F16_FN launch_finish16_x0w4
#elif MXA_F16_LONG
#define MXA_F16_FN launch_finish16_l0
#elif MXA_F16_XDT
#define MXA_F16_FN launch_finish16_x1
#else
#define MXA_F16_FN launch_finish16_x0
#endif

namespace mxa {

constexpr bool kF16Xdt = MXA_F16_XDT != 0;
constexpr bool kF16Long = MXA_F16_LONG != 0;
constexpr bool kF16W4 = MXA_F16_W4 != 0;
constexpr bool kF16Lxo = MXA_F16_LXO != 0;
static_assert(!(kF16Xdt && (kF16Long || kF16W4)), "long rows, MXINT4 P: float32 only");
static_assert(!(kF16Lxo && (kF16Xdt || kF16W4)), "the proj's codes on long rows: float32, MXINT8 P");

// waves per workgroup by finish_tile_plan (mxa_launch.hpp) from the waves per SIMD the
// kernel's registers allow
static int finish16_plan(const Rows2Args& ra, int BH, int regs_waves_per_simd, int* waves, int* rows_per_wg) {
  const bool xo = ra.xo_codes != nullptr;
  auto lds = [&](int w) { return fin16_lds(ra.T, ra.D, ra.kst, ra.nbd, ra.vst, ra.ntb, w, xo, kF16Long).total; };
  return finish_tile_plan(kFin16, ra.N, BH, lds, finish_wave_cap(regs_waves_per_simd), waves, rows_per_wg);
}
template <int NB, int KS, bool EXTRA, bool XO = false>
static int launch_finish16_x(const Rows2Args& ra0, int BH, hipStream_t stream) {
  Rows2Args ra = ra0;
  constexpr auto kernel = &finish16_kernel<NB, KS + (kF16Long ? kFin16LongKS : 0) + (kF16W4 ? kFin16Bits4KS : 0), kF16Xdt, EXTRA, XO>;
  int rc = finish16_plan(ra, BH, kernel_waves_per_simd<kernel>(), &ra.waves, &ra.rows_per_wg);
  if (rc) return rc;
  const size_t lds = fin16_lds(ra.T, ra.D, ra.kst, ra.nbd, ra.vst, ra.ntb, ra.waves, XO, kF16Long).total;
  return launch_finish_tiles<kernel>(ra, BH, lds, stream);
}
template <int NB, int KS>
static int launch_finish16_ks(const Rows2Args& ra, int BH, hipStream_t stream) {
  // EXTRA: a bias, the debug true scores or bfloatX rounding (float16 / bfloat16 always round)
  const bool extra = kF16Xdt || ra.bias || ra.true_out || (ra.bfloat != 0 && ra.bfloat != 32);
  if (ra.xo_codes) {  // the proj Linear's MX input codes: float32, D % 32 == 0, k <= 32
    if constexpr (!kF16Xdt && kF16Long == kF16Lxo && !kF16W4 && KS <= 8) {
      if (ra.D % 32) return MXA_ERR_UNSUPPORTED;
      return extra ? launch_finish16_x<NB, KS, true, true>(ra, BH, stream) : launch_finish16_x<NB, KS, false, true>(ra, BH, stream);
    }
    return MXA_ERR_UNSUPPORTED;
  }
  if constexpr (!kF16Lxo) {
    if (extra) return launch_finish16_x<NB, KS, true>(ra, BH, stream);
    if constexpr (!kF16Xdt) return launch_finish16_x<NB, KS, false>(ra, BH, stream);
  }
  return MXA_ERR_UNSUPPORTED;
}
template <int NB>
static int launch_finish16_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  // four lanes per row: slots ceil(k / 4) (DeiT / PixArt k = 20: 5, DeiT k = 30: 8)
  const int ks = (ra.k_top + 3) / 4;
  if (ks <= 5) return launch_finish16_ks<NB, 5>(ra, BH, stream);
  if (ks <= 8) return launch_finish16_ks<NB, 8>(ra, BH, stream);
  if (ks <= 12) return launch_finish16_ks<NB, 12>(ra, BH, stream);
  if (ks <= 16) return launch_finish16_ks<NB, 16>(ra, BH, stream);
  return MXA_ERR_UNSUPPORTED;  // k > 64: the 32-row kernel
}

int MXA_F16_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  if (ra.xo_codes && (kF16Xdt || kF16Long != kF16Lxo || kF16W4 || ra.k_top > 32 || ra.D % 32)) return MXA_ERR_UNSUPPORTED;
  if (kF16Lxo && !ra.xo_codes) return MXA_ERR_UNSUPPORTED;
  if (kF16W4 && (ra.s_dt != kF32 || ra.in_dt != kF32)) return MXA_ERR_UNSUPPORTED;
  if (kF16Long != long_rows(ra.T)) return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return ra.k_top <= 64 ? finish16_plan(ra, BH, 2, &w, &r) : MXA_ERR_UNSUPPORTED;
  }
  switch (ra.nbd) {
    case 1: return launch_finish16_nb<1>(ra, BH, stream);
    case 2: return launch_finish16_nb<2>(ra, BH, stream);
    case 3: return launch_finish16_nb<3>(ra, BH, stream);
    default: return launch_finish16_nb<4>(ra, BH, stream);
  }
}

}  // namespace mxa
