// Launches of the finishing kernel with every key's score on MFMA (mxa_finish_qk.hpp).
// Compiled twice (build_native.py): MXA_FQ_XDT=0 the float32 instantiations
// (launch_finish_qk_x0), MXA_FQ_XDT=1 the float16 / bfloat16 ones (launch_finish_qk_x1),
// so that the two build in parallel.  MXA_FQ_W4=1 (float32 only): the MXINT4-P instantiations
// of mxa_attention_bits at width 4 (launch_finish_qk_x0w4).
#include "mxa_finish_qk.hpp"
#include "mxa_launch.hpp"

#ifndef MXA_FQ_XDT
#define MXA_FQ_XDT 0
#endif
#ifndef MXA_FQ_W4
#define MXA_FQ_W4 0
#endif
#if MXA_FQ_W4
#define MXA_FQ_FN launch_finish_qk_x0w4
#elif MXA_FQ_XDT
#define MXA_FQ_FN launch_finish_qk_x1
#else
#define MXA_FQ_FN launch_finish_qk_x0
#endif

namespace mxa {

constexpr bool kXdt = MXA_FQ_XDT != 0;
constexpr bool kW4 = MXA_FQ_W4 != 0;
static_assert(!(kXdt && kW4), "MXINT4 P: float32 only");

// ---- finishing kernel, every key's score on MFMA (mxa_finish_qk.hpp) ------------------
// key blocks the kernel's registers hold (template NTB): 4 or 8
static int fq_ntb_max(int ntb) { return ntb <= 4 ? 4 : 8; }
// waves per workgroup by finish_tile_plan (mxa_launch.hpp): LDS per workgroup only, none per wave
static int finish_qk_plan(const Rows2Args& ra, int nb, int BH, int regs_waves_per_simd, int* waves, int* rows_per_wg) {
  const size_t t = fq_lds(ra.ntb, nb, fq_ntb_max(ra.ntb), ra.D).total;
  return finish_tile_plan(kFqRows, ra.N, BH, [t](int) { return t; }, finish_wave_cap(regs_waves_per_simd), waves,
                          rows_per_wg);
}
template <int NB, int NTB, bool XDT, bool EXTRA>
static int launch_finish_qk_x(Rows2Args ra, int BH, hipStream_t stream) {
  constexpr auto kernel = &finish_qk_kernel<NB, NTB + (kW4 ? kFqBits4NTB : 0), XDT, EXTRA>;
  int rc = finish_qk_plan(ra, NB, BH, kernel_waves_per_simd<kernel>(), &ra.waves, &ra.rows_per_wg);
  if (rc) return rc;
  return launch_finish_tiles<kernel>(ra, BH, fq_lds(ra.ntb, NB, NTB, ra.D).total, stream);
}
template <int NB, int NTB, bool XDT>
static int launch_finish_qk_xdt(const Rows2Args& ra, int BH, hipStream_t stream) {
  if ((!ra.mask_out && !ra.dense) || fq_ntb_max(ra.ntb) != NTB || ra.nbd != NB || ra.dpad != 32 * NB) return MXA_ERR_ARG;
  // EXTRA: a bias, the debug true scores or bfloatX rounding
  const bool extra = ra.bias || ra.true_out || (ra.bfloat != 0 && ra.bfloat != 32);
  return extra ? launch_finish_qk_x<NB, NTB, XDT, true>(ra, BH, stream) : launch_finish_qk_x<NB, NTB, XDT, false>(ra, BH, stream);
}
template <int NB>
static int launch_finish_qk_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  if (ra.ntb <= 4) return launch_finish_qk_xdt<NB, 4, kXdt>(ra, BH, stream);
  return launch_finish_qk_xdt<NB, 8, kXdt>(ra, BH, stream);
}

int MXA_FQ_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  if (kW4 && (ra.s_dt != kF32 || ra.in_dt != kF32)) return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return finish_qk_plan(ra, ra.nbd, BH, 2, &w, &r);
  }
  switch (ra.nbd) {
    case 1: return launch_finish_qk_nb<1>(ra, BH, stream);
    case 2: return launch_finish_qk_nb<2>(ra, BH, stream);
    case 3: return launch_finish_qk_nb<3>(ra, BH, stream);
    default: return launch_finish_qk_nb<4>(ra, BH, stream);
  }
}

}  // namespace mxa
