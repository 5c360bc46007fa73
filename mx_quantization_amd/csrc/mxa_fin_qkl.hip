// Launches of the tiled MFMA finishing kernel for rows of 513 .. 1,024 keys
// (mxa_finish_qk_long.hpp).  Compiled twice (build_native.py): MXA_FQL_W4=0 the MXINT8-P
// instantiations (launch_finish_qk_long_w8), MXA_FQL_W4=1 the MXINT4-P ones
// (launch_finish_qk_long_w4), so that the two build in parallel.
#include "mxa_finish_qk_long.hpp"
#include "mxa_launch.hpp"

#ifndef MXA_FQL_W4
#define MXA_FQL_W4 0
#endif
#if MXA_FQL_W4
#define MXA_FQL_FN launch_finish_qk_long_w4
#else
#define MXA_FQL_FN launch_finish_qk_long_w8
#endif

namespace mxa {

constexpr bool kW4 = MXA_FQL_W4 != 0;

template <int NB>
static int launch_finish_qk_long_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  if ((!ra.mask_out && !ra.dense) || ra.dpad != 32 * NB) return MXA_ERR_ARG;
  const size_t lds = fql_lds(NB, ra.D).total;
  if (finish_mfma_extra(ra)) return launch_finish_mfma<&finish_qk_long_kernel<NB, kW4, true>>(ra, kFqRows, lds, BH, stream);
  return launch_finish_mfma<&finish_qk_long_kernel<NB, kW4, false>>(ra, kFqRows, lds, BH, stream);
}

int MXA_FQL_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  if (ra.s_dt != kF32 || ra.in_dt != kF32 || ra.xo_codes) return MXA_ERR_UNSUPPORTED;
  if (ra.T > kFqlT || ra.ntb > kFqlNTB || ra.nbd < 1 || ra.nbd > 4 || ra.D > 32 * ra.nbd) return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return finish_mfma_plan(ra, kFqRows, fql_lds(ra.nbd, ra.D).total, BH, 2, &w, &r);
  }
  return dispatch_nbd(ra.nbd, [&](auto nb) { return launch_finish_qk_long_nb<decltype(nb)::value>(ra, BH, stream); });
}

}  // namespace mxa
