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

// waves per workgroup by finish_tile_plan (mxa_launch.hpp): LDS per workgroup only, none per wave
static int finish_qk_long_plan(const Rows2Args& ra, int BH, int regs_waves_per_simd, int* waves, int* rows_per_wg) {
  const size_t t = fql_lds(ra.nbd, ra.D).total;
  return finish_tile_plan(kFqRows, ra.N, BH, [t](int) { return t; }, finish_wave_cap(regs_waves_per_simd), waves,
                          rows_per_wg);
}
template <int NB, bool EXTRA>
static int launch_finish_qk_long_x(Rows2Args ra, int BH, hipStream_t stream) {
  constexpr auto kernel = &finish_qk_long_kernel<NB, kW4, EXTRA>;
  int rc = finish_qk_long_plan(ra, BH, kernel_waves_per_simd<kernel>(), &ra.waves, &ra.rows_per_wg);
  if (rc) return rc;
  return launch_finish_tiles<kernel>(ra, BH, fql_lds(NB, ra.D).total, stream);
}
template <int NB>
static int launch_finish_qk_long_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  if ((!ra.mask_out && !ra.dense) || ra.dpad != 32 * NB) return MXA_ERR_ARG;
  // EXTRA: a bias, the debug true scores or bfloatX rounding
  const bool extra = ra.bias || ra.true_out || (ra.bfloat != 0 && ra.bfloat != 32);
  return extra ? launch_finish_qk_long_x<NB, true>(ra, BH, stream) : launch_finish_qk_long_x<NB, false>(ra, BH, stream);
}

int MXA_FQL_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  if (ra.s_dt != kF32 || ra.in_dt != kF32 || ra.xo_codes) return MXA_ERR_UNSUPPORTED;
  if (ra.T > kFqlT || ra.ntb > kFqlNTB || ra.nbd < 1 || ra.nbd > 4 || ra.D > 32 * ra.nbd) return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return finish_qk_long_plan(ra, BH, 2, &w, &r);
  }
  switch (ra.nbd) {
    case 1: return launch_finish_qk_long_nb<1>(ra, BH, stream);
    case 2: return launch_finish_qk_long_nb<2>(ra, BH, stream);
    case 3: return launch_finish_qk_long_nb<3>(ra, BH, stream);
    default: return launch_finish_qk_long_nb<4>(ra, BH, stream);
  }
}

}  // namespace mxa
