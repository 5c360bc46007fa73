// Selection kernel for rows of 1,025 .. 4,096 keys OUTSIDE std::partial_sort's regime (k > 64 or
// k * 64 > T: torch's CPU topk takes std::nth_element + std::sort there, TopKImpl.h:45-86) -- the reference's
// default k_top = 20 on rows of 1,025 .. 1,279 keys, --k 30 up to 1,919, k = 64 below 4,096, and every k > 64
// (PixArt-Sigma at 1024 x 1024 with self_k = 154).  select_xl_kernel's streaming heap does not apply; this is
// select_long_kernel's shape stretched to 4,096 keys:
//
//   scores   sel_scores as it is (lane stride 64); the sink writes pack_ki(order key, position) into the
//            wave's 64-bit mirror (mxa_topk_wave_xl.hpp carve_wxrow)
//   top-k    wave_topk_xl on the mirror
//   out      the kept indices through kept_put, the prune-mask words through sel_mask_words (its scratch: the
//            slot tables, dead by then).  The masked MFMA finishing kernel of k_top > 64 reads the words, so
//            for such a call a.mask_out is always set (the caller's, else the workspace's: rows2_bind)
//
// One wave per query row; the waves per workgroup follow the row's LDS (sel_nth_plan): 50,688 B at 4,096 keys
// is one wave per workgroup, three workgroups per CU; 13.7 KB at 1,025 keys is four waves.  The key-side
// tables follow select_xl_kernel's rules with that per-row figure: the code modes read the K operands in
// place through L2; ex_pred stages its tables while tables + rows leave two workgroups per CU, else reads
// them from the workspace (nbd >= 3) or stages the key records at one workgroup per CU (nbd <= 2).
#pragma once
#include "mxa_select_xl.hpp"
#include "mxa_topk_wave_xl.hpp"

namespace mxa {

static_assert(kXlRowsT == kWxMaxN, "the xl rows' bound is the chunked wave top-k's");

// the launch of one call: waves per workgroup (0: nothing fits), ex_pred's tables staged or not, LDS bytes
struct SelNthPlan { int waves; bool staged; size_t lds; };
inline SelNthPlan sel_nth_plan(int mode, int T, int D, int kst, int nbd) {
  const size_t row = wxrow_bytes(T);
  const size_t tabs = mode == kModeExSign ? sel_lds_long(mode, T, D, kst, nbd).rows : 0;
  auto waves_in = [row](size_t budget, size_t t) { return budget > t ? (int)std::min<size_t>(4, (budget - t) / row) : 0; };
  SelNthPlan p{};
  p.waves = waves_in(80 * 1024, tabs);
  p.staged = mode == kModeExSign && p.waves >= 1;
  if (!p.staged && mode == kModeExSign && nbd <= 2) {  // the key records exist in LDS only
    p.waves = waves_in(160 * 1024, tabs);
    p.staged = true;
  } else if (!p.staged) {
    p.waves = waves_in(80 * 1024, 0);
  }
  p.lds = (p.staged ? tabs : 0) + (size_t)p.waves * row;
  return p;
}

template <int MODE, bool STAGED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void select_xl_nth_kernel(Rows2Args a) {
  static_assert(MODE != kModeElsa && (STAGED ? MODE == kModeExSign : true), "ELSA stops at 1,024 keys; only ex_pred stages");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63), nw = (int)(blockDim.x >> 6);
  const int bh = blockIdx.x;
  const int T = a.T, k = a.k_top;
  const int r0 = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r0 + a.rows_per_wg);
  SelTabs t{};
  size_t tabs = 0;
  if constexpr (STAGED) {
    const SelLds L = sel_lds_long(MODE, T, a.D, a.kst, a.nbd);
    t = sel_stage_long<MODE>(a, smem, L, bh);
    tabs = L.rows;
  } else if constexpr (MODE == kModeExSign) {  // nbd >= 3: the tables where rows_prep left them
    const int64_t kb = (int64_t)bh * T;
    t.tex = const_cast<int16_t*>(a.ksA + kb * a.nbd);
    t.tsg = const_cast<uint32_t*>(a.ksg + kb * a.nbd);
  } else {
    t = sel_stage_long<MODE>(a, smem, SelLds{}, bh);
  }
  const WRow g = carve_wxrow(smem + tabs + (size_t)wave * wxrow_bytes(T), T);
  for (int r = r0 + wave; r < r_end; r += nw) {
    sel_scores<MODE>(a, t, bh, r, lane, 64, [&](int j, float, uint32_t key, auto) { g.A[j] = pack_ki(key, (uint32_t)j); });
    wave_lds_sync();
    wave_topk_xl(g, T, k);
    const int64_t grow = (int64_t)bh * a.N + r;
    for (int p = lane; p < k; p += 64) kept_put(a, grow * k + p, (int)(uint32_t)g.A[p]);
    if (a.mask_out)
      sel_mask_words(a.mask_out, grow, (T + 31) / 32, (lu32*)g.SL, true, lane, 64, k, [&](int p) { return (uint32_t)g.A[p]; });
    wave_lds_sync();  // the next row's scores overwrite the mirror
  }
}

}  // namespace mxa
