// Selection kernel for rows of 1,025 .. 4,096 keys (PixArt-Sigma at 1024 x 1024: 3,840 .. 4,096
// latent tokens), top-k with k <= 64 and k * 64 <= T: the regime in which torch.topk on CPU
// (TopKImpl.h:45-86) takes std::partial_sort -- __heap_select over the row, then __sort_heap.
// That is a streaming algorithm, so the row needs no 64-bit mirror and no partition window:
//
//   scores   sel_scores as it is (lane stride 64); the sink writes the 32-bit order key alone
//            into the wave's LDS strip key[T] (16 KB at 4,096 keys); the index is the position
//   heap     the k <= 64 heap elements one per lane -- a key VGPR and an index VGPR, heap
//            position = lane.  The walk (hole, second, parent, every compare) is wave-uniform
//            scalar code; elements are read by v_readlane with a scalar lane index and written by a
//            select on the lane number.
//            xl_push_heap / xl_adjust_heap are ln_push_heap / ln_adjust_heap (mxa_order.hpp)
//            operation for operation, lgt on the keys: a tie never enters the heap
//   scan     64 keys per step: ballot(key > heap[0].key); the lowest set lane is the next
//            element __heap_select would take (the smallest position); __pop_heap's
//            __adjust_heap(first, 0, k, value) with it (the value __pop_heap writes back to
//            a[i] is never read again: not stored); then only the lanes above it are compared
//            with the new top
//   sort     __sort_heap on the lanes; lane p then holds the p-th kept index
//
// One wave per query row, four waves per workgroup (as select_long_kernel).  The key-side tables:
// the code modes read the K operands in place through L2 (sel_stage_long); ex_pred's sign words
// and block exponents are staged (STAGED) when tables + strips leave two workgroups per CU, and
// are otherwise read from the workspace through SelTabs (nbd >= 3: the int16 exponents and sign
// words as rows_prep left them; nbd <= 2 needs the key records, which exist in LDS only, and
// always fits: at most 64 KB beside 64 KB of strips).  The host decides per launch
// (mxa_sel_xl.hip).
#pragma once
#include "mxa_select_long.hpp"

namespace mxa {

constexpr int kSelXlWaves = 4;  // one query row per wave at a time
__host__ __device__ constexpr size_t xl_strip_bytes(int T) { return ((size_t)T * 4 + 15) & ~(size_t)15; }

// the heap: lane p holds the element at heap position p.  Reads are v_readlane with a scalar lane
// index; a write to position `to` is a select on lane == to (the toolchain has no writelane builtin:
// one compare and a v_cndmask per field, against v_writelane and its m0 move)
struct XlHeap { uint32_t key, idx; int lane; };
__device__ __forceinline__ uint32_t xl_get(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ void xl_put(XlHeap& h, int to, uint32_t vk, uint32_t vi) {  // f[to] = v
  const bool me = h.lane == to;
  h.key = me ? vk : h.key;
  h.idx = me ? vi : h.idx;
}
__device__ __forceinline__ void xl_move(XlHeap& h, int to, int from) {  // f[to] = f[from]
  xl_put(h, to, xl_get(h.key, from), xl_get(h.idx, from));
}
// ln_push_heap (stl_heap.h __push_heap) with the value (vk, vi)
__device__ __forceinline__ void xl_push_heap(XlHeap& h, int hole, int top, uint32_t vk, uint32_t vi) {
  int parent = (hole - 1) / 2;
  while (hole > top && xl_get(h.key, parent) > vk) {
    xl_move(h, hole, parent);
    hole = parent;
    parent = (hole - 1) / 2;
  }
  xl_put(h, hole, vk, vi);
}
// ln_adjust_heap (__adjust_heap)
__device__ __forceinline__ void xl_adjust_heap(XlHeap& h, int hole, int len, uint32_t vk, uint32_t vi) {
  const int top = hole;
  int second = hole;
  while (second < (len - 1) / 2) {
    second = 2 * (second + 1);
    if (xl_get(h.key, second) > xl_get(h.key, second - 1)) second--;
    xl_move(h, hole, second);
    hole = second;
  }
  if ((len & 1) == 0 && second == (len - 2) / 2) {
    second = 2 * (second + 1);
    xl_move(h, hole, second - 1);
    hole = second - 1;
  }
  xl_push_heap(h, hole, top, vk, vi);
}

// partial_sort(a, a + k, a + T) of the elements (strip[j], j): ln_heap_select, then ln_sort_heap.
// Lane p < k returns the p-th element.  1 <= k <= 64 <= T; every lane of the wave calls it.
__device__ __forceinline__ XlHeap xl_select(const lu32* strip, int T, int k, int lane) {
  XlHeap h;
  h.key = lane < k ? strip[lane] : 0u;
  h.idx = (uint32_t)lane;
  h.lane = lane;
  if (k >= 2) {  // __make_heap
    int parent = (k - 2) / 2;
    while (true) {
      xl_adjust_heap(h, parent, k, xl_get(h.key, parent), xl_get(h.idx, parent));
      if (parent == 0) break;
      parent--;
    }
  }
  uint32_t top = xl_get(h.key, 0);
  for (int base = k; base < T; base += 64) {
    const int j = base + lane;
    const uint32_t kv = j < T ? strip[j] : 0u;  // (0 is below every real key: mxa_order.hpp)
    uint64_t pend = __builtin_amdgcn_ballot_w64(kv > top);
    while (pend) {
      const int l = __builtin_ctzll(pend);
      xl_adjust_heap(h, 0, k, xl_get(kv, l), (uint32_t)(base + l));
      top = xl_get(h.key, 0);
      pend = __builtin_amdgcn_ballot_w64(kv > top) & ~((2ull << l) - 1ull);
    }
  }
  for (int last = k - 1; last >= 1; --last) {  // __sort_heap: __pop_heap(first, last, last)
    const uint32_t vk = xl_get(h.key, last), vi = xl_get(h.idx, last);
    xl_move(h, last, 0);
    xl_adjust_heap(h, 0, last, vk, vi);
  }
  return h;
}

template <int MODE, bool STAGED>
__global__ __launch_bounds__(64 * kSelXlWaves) __attribute__((amdgpu_waves_per_eu(2, 8))) void select_xl_kernel(Rows2Args a) {
  static_assert(MODE != kModeElsa && (STAGED ? MODE == kModeExSign : true), "ELSA stops at 1,024 keys; only ex_pred stages");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int bh = blockIdx.x;
  const int T = a.T, k = a.k_top;
  const int r0 = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r0 + a.rows_per_wg);
  SelTabs t{};
  size_t strips = 0;
  if constexpr (STAGED) {
    const SelLds L = sel_lds_long(MODE, T, a.D, a.kst, a.nbd);
    t = sel_stage_long<MODE>(a, smem, L, bh);
    strips = L.rows;
  } else if constexpr (MODE == kModeExSign) {  // nbd >= 3: the tables where rows_prep left them
    const int64_t kb = (int64_t)bh * T;
    t.tex = const_cast<int16_t*>(a.ksA + kb * a.nbd);
    t.tsg = const_cast<uint32_t*>(a.ksg + kb * a.nbd);
  } else {
    t = sel_stage_long<MODE>(a, smem, SelLds{}, bh);
  }
  lu32* strip = (lu32*)(smem + strips + (size_t)wave * xl_strip_bytes(T));
  for (int r = r0 + wave; r < r_end; r += kSelXlWaves) {
    sel_scores<MODE>(a, t, bh, r, lane, 64, [&](int j, float, uint32_t key, auto) { strip[j] = key; });
    wave_lds_sync();
    const XlHeap h = xl_select(strip, T, k, lane);
    const int64_t grow = (int64_t)bh * a.N + r;
    if (lane < k) kept_put(a, grow * k + lane, (int)h.idx);
    if (a.mask_out)  // (the strip is dead: its first words are the scratch)
      sel_mask_words(a.mask_out, grow, (T + 31) / 32, strip, true, lane, 64, k, [&](int) { return h.idx; });
    wave_lds_sync();  // the next row's keys overwrite the strip
  }
}

}  // namespace mxa
