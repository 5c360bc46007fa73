// Launches of the selection kernel for rows of 4,097 .. 16,384 keys (mxa_select_xxl.hpp) and the
// standalone mxa_topk_xxl on the same chunked streaming body.  Compiled once per score mode
// (MXA_SELXX_PART 1..5, as mxa_sel_xl.hip; part 0 holds the dispatcher and mxa_topk_xxl: build_native.py).
#include "mxa_select_xxl.hpp"

#ifndef MXA_SELXX_PART
#define MXA_SELXX_PART 0
#endif

namespace mxa {

int launch_select_xxl_p1(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // ex_pred
int launch_select_xxl_p2(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // EXION
int launch_select_xxl_p3(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // MXINT4 / partial
int launch_select_xxl_p4(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // true_ex
int launch_select_xxl_p5(const Rows2Args& ra, int BH, hipStream_t stream, bool plan);  // the true scores

#if MXA_SELXX_PART == 0
// the standalone top-k on the same body (topk_xl_kernel's pattern): waves of a 256-thread workgroup take
// rows 4 blockIdx.x + wave; the chunk's values are loaded, keyed and written to the strip by the feeder
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void topk_xxl_kernel(GrpTopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= a.rows) return;
  lu32* strip = (lu32*)(smem + (size_t)wave * kXxlStripBytes);
  const int64_t src = row * a.ld;
  const XlHeap h = xxl_select(strip, a.n, a.k, lane, [&](int c0, int nc) {
    for (int j = lane; j < nc; j += 64) strip[j] = order_key(load_dt(a.vals, src + c0 + j, a.dt));
  });
  if (lane < a.k) {
    a.out_idx[row * a.k + lane] = (int64_t)h.idx;
    if (a.out_vals) store_dt(a.out_vals, row * a.k + lane, load_dt(a.vals, src + h.idx, a.dt), a.dt);
  }
  if (a.out_mask)
    sel_mask_words(a.out_mask, row, (a.n + 31) / 32, strip, true, lane, 64, a.k, [&](int) { return h.idx; });
}

int launch_select_xxl(const Rows2Args& ra, int mode, int BH, hipStream_t stream, bool plan) {
  if (!xxl_rows_ok(ra.T, ra.k_top)) return MXA_ERR_UNSUPPORTED;
  switch (mode) {
    case kModeExSign: return launch_select_xxl_p1(ra, BH, stream, plan);
    case kModeOpMul: return launch_select_xxl_p2(ra, BH, stream, plan);
    case kModeOpExp: return launch_select_xxl_p3(ra, BH, stream, plan);
    case kModeTrueEx: return launch_select_xxl_p4(ra, BH, stream, plan);
    case kModeElsa: return MXA_ERR_UNSUPPORTED;
    default: return launch_select_xxl_p5(ra, BH, stream, plan);
  }
}
#else
// 16 KB of LDS whatever T is: nothing to plan
template <int MODE>
static int launch_select_xxl_m(const Rows2Args& ra0, int BH, hipStream_t stream, bool plan) {
  if (plan) return MXA_OK;
  Rows2Args ra = ra0;
  ra.kst = ra.dpad;  // every table is read in place
  ra.rows_per_wg = (int64_t)BH * ((ra.N + kSelRows - 1) / kSelRows) < 2048 ? 16 : kSelRows;
  const unsigned gy = (unsigned)((ra.N + ra.rows_per_wg - 1) / ra.rows_per_wg);
  hipLaunchKernelGGL((select_xxl_kernel<MODE>), dim3((unsigned)BH, gy), dim3(64 * kSelXxlWaves),
                     kSelXxlWaves * kXxlStripBytes, stream, ra);
  return launch_status();
}
constexpr int kPartMode[6] = {0, kModeExSign, kModeOpMul, kModeOpExp, kModeTrueEx, kModeTrue};
#define MXA_SELXX_FN2(i) launch_select_xxl_p##i
#define MXA_SELXX_FN(i) MXA_SELXX_FN2(i)
int MXA_SELXX_FN(MXA_SELXX_PART)(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  return launch_select_xxl_m<kPartMode[MXA_SELXX_PART]>(ra, BH, stream, plan);
}
#endif

}  // namespace mxa

#if MXA_SELXX_PART == 0
using namespace mxa;

extern "C" int mxa_topk_xxl(const void* vals, int64_t rows, int32_t n, int64_t ld, int32_t k, int64_t* out_idx,
                            void* out_vals, uint32_t* out_mask, int32_t dtype, hipStream_t stream) {
  if (n <= kXlRowsT) return mxa_topk_xl_nth(vals, rows, n, ld, k, out_idx, out_vals, out_mask, dtype, stream);
  if (!vals || (!out_idx && k > 0) || rows < 0 || ld < n || k < 0 || k > n) return MXA_ERR_ARG;
  if (dtype != kF32 && dtype != kF16 && dtype != kBF16) return MXA_ERR_ARG;
  if (!xxl_rows_ok(n, k)) return MXA_ERR_UNSUPPORTED;
  if (rows == 0) return MXA_OK;
  if ((rows + 3) / 4 > INT32_MAX) return MXA_ERR_UNSUPPORTED;
  const GrpTopkArgs ga{vals, rows, ld, n, k, out_idx, out_vals, out_mask, dtype};
  hipLaunchKernelGGL(topk_xxl_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 4 * kXxlStripBytes, stream, ga);
  return launch_status();
}
#endif
