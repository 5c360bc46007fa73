// Launches of the long rows' selection kernel (mxa_select_long.hpp: rows of 513 .. 1,024
// keys).  Compiled once per score mode (MXA_SELL_PART 1..6, as mxa_sel.hip; part 0 holds the
// dispatcher: build_native.py) so that hipcc builds the instantiations in parallel.
#include "mxa_select_long.hpp"

#ifndef MXA_SELL_PART
#define MXA_SELL_PART 0
#endif

namespace mxa {

int launch_select_long_p1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // ex_pred
int launch_select_long_p2(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // EXION
int launch_select_long_p3(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // MXINT4 / partial
int launch_select_long_p4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // true_ex
int launch_select_long_p5(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // ELSA
int launch_select_long_p6(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // the true scores

#if MXA_SELL_PART == 0
int launch_select_long(const Rows2Args& ra, int mode, int BH, hipStream_t stream, bool plan) {
  if (ra.T > kLongRowsT || ra.k_top > ra.T) return MXA_ERR_UNSUPPORTED;
  switch (mode) {
    case kModeExSign: return launch_select_long_p1(ra, BH, stream, plan);
    case kModeOpMul: return launch_select_long_p2(ra, BH, stream, plan);
    case kModeOpExp: return launch_select_long_p3(ra, BH, stream, plan);
    case kModeTrueEx: return launch_select_long_p4(ra, BH, stream, plan);
    case kModeElsa: return launch_select_long_p5(ra, BH, stream, plan);
    default: return launch_select_long_p6(ra, BH, stream, plan);
  }
}
#else
// one head's rows in chunks of 32 (16 while the grid has fewer than 2048 workgroups): the
// staged tables are shared by eight (four) rows per wave
template <int MODE>
static int launch_select_long_m(const Rows2Args& ra0, int BH, hipStream_t stream, bool plan) {
  Rows2Args ra = ra0;
  ra.kst = ra.dpad;  // the code modes read the K operands in place (sel_stage_long)
  const size_t lds = sel_lds_long(MODE, ra.T, ra.D, ra.kst, ra.nbd).rows + (size_t)kSelLongWaves * wrow_bytes(ra.T);
  if (lds > 160 * 1024) return MXA_ERR_UNSUPPORTED;
  if (plan) return MXA_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&select_long_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return MXA_ERR_LAUNCH;
  ra.rows_per_wg = (int64_t)BH * ((ra.N + kSelRows - 1) / kSelRows) < 2048 ? 16 : kSelRows;
  const unsigned gy = (unsigned)((ra.N + ra.rows_per_wg - 1) / ra.rows_per_wg);
  hipLaunchKernelGGL(select_long_kernel<MODE>, dim3((unsigned)BH, gy), dim3(64 * kSelLongWaves), lds, stream, ra);
  return launch_status();
}
constexpr int kPartMode[7] = {0, kModeExSign, kModeOpMul, kModeOpExp, kModeTrueEx, kModeElsa, kModeTrue};
#define MXA_SELL_FN2(i) launch_select_long_p##i
#define MXA_SELL_FN(i) MXA_SELL_FN2(i)
int MXA_SELL_FN(MXA_SELL_PART)(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  return launch_select_long_m<kPartMode[MXA_SELL_PART]>(ra, BH, stream, plan);
}
#endif

}  // namespace mxa
