// Launches of the selection kernel for rows of 1,025 .. 4,096 keys (mxa_select_xl.hpp) and the
// standalone mxa_topk_xl on the same streaming body.  Compiled once per score mode (MXA_SELX_PART
// 1..5, as mxa_sel_long.hip; part 0 holds the dispatcher and mxa_topk_xl: build_native.py).
#include "mxa_select_xl.hpp"

#ifndef MXA_SELX_PART
#define MXA_SELX_PART 0
#endif

namespace mxa {

int launch_select_xl_p1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // ex_pred
int launch_select_xl_p2(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // EXION
int launch_select_xl_p3(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // MXINT4 / partial
int launch_select_xl_p4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // true_ex
int launch_select_xl_p5(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // the true scores

#if MXA_SELX_PART == 0
// the standalone top-k on the same body: waves of a 256-thread workgroup take rows 4 blockIdx.x + wave
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void topk_xl_kernel(GrpTopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= a.rows) return;
  lu32* strip = (lu32*)(smem + (size_t)wave * xl_strip_bytes(a.n));
  const int64_t src = row * a.ld;
  for (int j = lane; j < a.n; j += 64) strip[j] = order_key(load_dt(a.vals, src + j, a.dt));
  wave_lds_sync();
  const XlHeap h = xl_select(strip, a.n, a.k, lane);
  if (lane < a.k) {
    a.out_idx[row * a.k + lane] = (int64_t)h.idx;
    if (a.out_vals) store_dt(a.out_vals, row * a.k + lane, load_dt(a.vals, src + h.idx, a.dt), a.dt);
  }
  if (a.out_mask)
    sel_mask_words(a.out_mask, row, (a.n + 31) / 32, strip, true, lane, 64, a.k, [&](int) { return h.idx; });
}

int launch_select_xl(const Rows2Args& ra, int mode, int BH, hipStream_t stream, bool plan) {
  if (!xl_rows_ok(ra.T, ra.k_top)) return MXA_ERR_UNSUPPORTED;
  switch (mode) {
    case kModeExSign: return launch_select_xl_p1(ra, BH, stream, plan);
    case kModeOpMul: return launch_select_xl_p2(ra, BH, stream, plan);
    case kModeOpExp: return launch_select_xl_p3(ra, BH, stream, plan);
    case kModeTrueEx: return launch_select_xl_p4(ra, BH, stream, plan);
    case kModeElsa: return MXA_ERR_UNSUPPORTED;
    default: return launch_select_xl_p5(ra, BH, stream, plan);
  }
}
#else
template <int MODE, bool STAGED>
static int launch_select_xl_s(const Rows2Args& ra, int BH, size_t lds, hipStream_t stream) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&select_xl_kernel<MODE, STAGED>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return MXA_ERR_LAUNCH;
  const unsigned gy = (unsigned)((ra.N + ra.rows_per_wg - 1) / ra.rows_per_wg);
  hipLaunchKernelGGL((select_xl_kernel<MODE, STAGED>), dim3((unsigned)BH, gy), dim3(64 * kSelXlWaves), lds, stream, ra);
  return launch_status();
}
// ex_pred's tables: staged while tables + strips leave two workgroups per CU (80 KB each); else
// read from the workspace (nbd >= 3), or staged at one workgroup per CU (the key records of nbd <= 2)
template <int MODE>
static int launch_select_xl_m(const Rows2Args& ra0, int BH, hipStream_t stream, bool plan) {
  Rows2Args ra = ra0;
  ra.kst = ra.dpad;  // the code modes read the K operands in place (sel_stage_long)
  const size_t strips = (size_t)kSelXlWaves * xl_strip_bytes(ra.T);
  const size_t staged = sel_lds_long(MODE, ra.T, ra.D, ra.kst, ra.nbd).rows + strips;
  const bool stage = MODE == kModeExSign && (staged <= 80 * 1024 || ra.nbd <= 2);
  const size_t lds = stage ? staged : strips;
  if (lds > 160 * 1024) return MXA_ERR_UNSUPPORTED;
  if (plan) return MXA_OK;
  ra.rows_per_wg = (int64_t)BH * ((ra.N + kSelRows - 1) / kSelRows) < 2048 ? 16 : kSelRows;
  if constexpr (MODE == kModeExSign) {
    if (stage) return launch_select_xl_s<MODE, true>(ra, BH, lds, stream);
  }
  return launch_select_xl_s<MODE, false>(ra, BH, lds, stream);
}
constexpr int kPartMode[6] = {0, kModeExSign, kModeOpMul, kModeOpExp, kModeTrueEx, kModeTrue};
#define MXA_SELX_FN2(i) launch_select_xl_p##i
#define MXA_SELX_FN(i) MXA_SELX_FN2(i)
int MXA_SELX_FN(MXA_SELX_PART)(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  return launch_select_xl_m<kPartMode[MXA_SELX_PART]>(ra, BH, stream, plan);
}
#endif

}  // namespace mxa

#if MXA_SELX_PART == 0
using namespace mxa;

extern "C" int mxa_topk_xl(const void* vals, int64_t rows, int32_t n, int64_t ld, int32_t k, int64_t* out_idx,
                           void* out_vals, uint32_t* out_mask, int32_t dtype, hipStream_t stream) {
  if (n <= kLongRowsT) return mxa_topk(vals, rows, n, ld, k, out_idx, out_vals, out_mask, dtype, stream);
  if (!vals || (!out_idx && k > 0) || rows < 0 || ld < n || k < 0 || k > n) return MXA_ERR_ARG;
  if (dtype != kF32 && dtype != kF16 && dtype != kBF16) return MXA_ERR_ARG;
  if (!xl_rows_ok(n, k)) return MXA_ERR_UNSUPPORTED;
  if (rows == 0) return MXA_OK;
  const GrpTopkArgs ga{vals, rows, ld, n, k, out_idx, out_vals, out_mask, dtype};
  const size_t lds = (size_t)4 * xl_strip_bytes(n);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_xl_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return MXA_ERR_LAUNCH;
  hipLaunchKernelGGL(topk_xl_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), lds, stream, ga);
  return launch_status();
}
#endif
