// Launches of the selection kernel for rows of 1,025 .. 4,096 keys outside std::partial_sort's regime
// (mxa_select_xl_nth.hpp) and the standalone mxa_topk_xl_nth on the same body.  Compiled once per score
// mode (MXA_SELN_PART 1..5, as mxa_sel_xl.hip; part 0 holds the dispatcher and mxa_topk_xl_nth:
// build_native.py).
#include "mxa_select_xl_nth.hpp"

#ifndef MXA_SELN_PART
#define MXA_SELN_PART 0
#endif

namespace mxa {

int launch_select_xl_nth_p1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // ex_pred
int launch_select_xl_nth_p2(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // EXION
int launch_select_xl_nth_p3(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // MXINT4 / partial
int launch_select_xl_nth_p4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // true_ex
int launch_select_xl_nth_p5(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // the true scores

#if MXA_SELN_PART == 0
// k == 0: an all-zero mask, cleared by a kernel (a captured graph replays a kernel node)
__global__ void clear_words_nth_kernel(uint32_t* p, int64_t words) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) p[i] = 0u;
}

// the standalone top-k on the same body (mxa_topk_xl_nth): wave w of a workgroup takes row nw blockIdx.x + w
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void topk_xl_nth_kernel(GrpTopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63), nw = (int)(blockDim.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * nw + wave;
  if (row >= a.rows) return;
  const WRow g = carve_wxrow(smem + (size_t)wave * wxrow_bytes(a.n), a.n);
  const int64_t src = row * a.ld;
  for (int j = lane; j < a.n; j += 64) g.A[j] = pack_ki(order_key(load_dt(a.vals, src + j, a.dt)), (uint32_t)j);
  wave_lds_sync();
  wave_topk_xl(g, a.n, a.k);
  for (int p = lane; p < a.k; p += 64) {
    const uint32_t ix = (uint32_t)g.A[p];
    a.out_idx[row * a.k + p] = (int64_t)ix;
    if (a.out_vals) store_dt(a.out_vals, row * a.k + p, load_dt(a.vals, src + ix, a.dt), a.dt);
  }
  if (a.out_mask)
    sel_mask_words(a.out_mask, row, (a.n + 31) / 32, (lu32*)g.SL, true, lane, 64, a.k, [&](int p) { return (uint32_t)g.A[p]; });
}

int launch_select_xl_nth(const Rows2Args& ra, int mode, int BH, hipStream_t stream, bool plan) {
  if (!xl_rows(ra.T) || ra.T > kXlRowsT || ra.k_top < 1 || ra.k_top > ra.T) return MXA_ERR_UNSUPPORTED;
  switch (mode) {
    case kModeExSign: return launch_select_xl_nth_p1(ra, BH, stream, plan);
    case kModeOpMul: return launch_select_xl_nth_p2(ra, BH, stream, plan);
    case kModeOpExp: return launch_select_xl_nth_p3(ra, BH, stream, plan);
    case kModeTrueEx: return launch_select_xl_nth_p4(ra, BH, stream, plan);
    case kModeElsa: return MXA_ERR_UNSUPPORTED;
    default: return launch_select_xl_nth_p5(ra, BH, stream, plan);
  }
}
#else
template <int MODE, bool STAGED>
static int launch_select_xl_nth_s(const Rows2Args& ra, int BH, const SelNthPlan& pl, hipStream_t stream) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&select_xl_nth_kernel<MODE, STAGED>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds) != hipSuccess)
    return MXA_ERR_LAUNCH;
  const unsigned gy = (unsigned)((ra.N + ra.rows_per_wg - 1) / ra.rows_per_wg);
  hipLaunchKernelGGL((select_xl_nth_kernel<MODE, STAGED>), dim3((unsigned)BH, gy), dim3(64 * pl.waves), pl.lds, stream, ra);
  return launch_status();
}
template <int MODE>
static int launch_select_xl_nth_m(const Rows2Args& ra0, int BH, hipStream_t stream, bool plan) {
  Rows2Args ra = ra0;
  ra.kst = ra.dpad;  // the code modes read the K operands in place (sel_stage_long)
  const SelNthPlan pl = sel_nth_plan(MODE, ra.T, ra.D, ra.kst, ra.nbd);
  if (pl.waves < 1 || pl.lds > 160 * 1024) return MXA_ERR_UNSUPPORTED;
  if (plan) return MXA_OK;
  ra.rows_per_wg = (int64_t)BH * ((ra.N + kSelRows - 1) / kSelRows) < 2048 ? 16 : kSelRows;
  if constexpr (MODE == kModeExSign) {
    if (pl.staged) return launch_select_xl_nth_s<MODE, true>(ra, BH, pl, stream);
  }
  return launch_select_xl_nth_s<MODE, false>(ra, BH, pl, stream);
}
constexpr int kPartMode[6] = {0, kModeExSign, kModeOpMul, kModeOpExp, kModeTrueEx, kModeTrue};
#define MXA_SELN_FN2(i) launch_select_xl_nth_p##i
#define MXA_SELN_FN(i) MXA_SELN_FN2(i)
int MXA_SELN_FN(MXA_SELN_PART)(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  return launch_select_xl_nth_m<kPartMode[MXA_SELN_PART]>(ra, BH, stream, plan);
}
#endif

}  // namespace mxa

#if MXA_SELN_PART == 0
using namespace mxa;

extern "C" int mxa_topk_xl_nth(const void* vals, int64_t rows, int32_t n, int64_t ld, int32_t k, int64_t* out_idx,
                               void* out_vals, uint32_t* out_mask, int32_t dtype, hipStream_t stream) {
  // (rows of at most 1,024 values: mxa_topk; partial_sort's regime: the streaming kernel)
  if (n <= kLongRowsT || xl_rows_ok(n, k)) return mxa_topk_xl(vals, rows, n, ld, k, out_idx, out_vals, out_mask, dtype, stream);
  if (!vals || (!out_idx && k > 0) || rows < 0 || ld < n || k < 0 || k > n) return MXA_ERR_ARG;
  if (dtype != kF32 && dtype != kF16 && dtype != kBF16) return MXA_ERR_ARG;
  if (n > kWxMaxN) return MXA_ERR_UNSUPPORTED;
  if (rows == 0) return MXA_OK;
  if (k == 0) {  // nothing kept, as mxa_topk
    if (!out_mask) return MXA_OK;
    const int64_t words = rows * (int64_t)((n + 31) / 32);
    hipLaunchKernelGGL(clear_words_nth_kernel, dim3((unsigned)std::min<int64_t>((words + 255) / 256, 4096)), dim3(256), 0,
                       stream, out_mask, words);
    return launch_status();
  }
  const GrpTopkArgs ga{vals, rows, ld, n, k, out_idx, out_vals, out_mask, dtype};
  const int waves = sel_nth_plan(kModeTrue, n, 0, 0, 0).waves;  // (no tables: the rows alone)
  const size_t lds = (size_t)waves * wxrow_bytes(n);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_xl_nth_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return MXA_ERR_LAUNCH;
  hipLaunchKernelGGL(topk_xl_nth_kernel, dim3((unsigned)((rows + waves - 1) / waves)), dim3(64 * waves), lds, stream, ga);
  return launch_status();
}
#endif
