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
template <int NB, int NTB>
static int launch_finish_qk_ntb(const Rows2Args& ra, int BH, hipStream_t stream) {
  if ((!ra.mask_out && !ra.dense) || ra.nbd != NB || ra.dpad != 32 * NB) return MXA_ERR_ARG;
  constexpr int NTBW = NTB + (kW4 ? kFqBits4NTB : 0);
  const size_t lds = fq_lds(ra.ntb, NB, NTB, ra.D).total;
  if (finish_mfma_extra(ra)) return launch_finish_mfma<&finish_qk_kernel<NB, NTBW, kXdt, true>>(ra, kFqRows, lds, BH, stream);
  return launch_finish_mfma<&finish_qk_kernel<NB, NTBW, kXdt, false>>(ra, kFqRows, lds, BH, stream);
}

int MXA_FQ_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  if (kW4 && (ra.s_dt != kF32 || ra.in_dt != kF32)) return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return finish_mfma_plan(ra, kFqRows, fq_lds(ra.ntb, ra.nbd, fq_ntb_max(ra.ntb), ra.D).total, BH, 2, &w, &r);
  }
  return dispatch_nbd(ra.nbd, [&](auto nb) {
    constexpr int NB = decltype(nb)::value;
    return ra.ntb <= 4 ? launch_finish_qk_ntb<NB, 4>(ra, BH, stream) : launch_finish_qk_ntb<NB, 8>(ra, BH, stream);
  });
}

}  // namespace mxa
