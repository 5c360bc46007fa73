// Selection kernel for rows of 4,097 .. 16,384 keys (PixArt-Sigma's 2K checkpoint: 128 x 128 = 16,384
// latent tokens), top-k with k <= 64 and k * 64 <= T -- torch.topk on CPU takes std::partial_sort there
// (TopKImpl.h:45-86): __make_heap over the first k elements, ONE in-order scan, __sort_heap.  The scan
// never looks back, so the row is consumed chunk by chunk and no LDS area grows with T:
//
//   strip    one CHUNK of order keys per wave (1,024 keys, 4 KB) where select_xl_kernel keeps the whole
//            row (64 KB a wave at 16,384 keys: four waves would need 256 KB of the 160 KB)
//   walk     per chunk, in ascending key order: the score pass writes the chunk's keys into the strip, then
//            the scan consumes them.  A key's score depends on that key alone, so the order keys -- and with
//            them every heap movement -- are the ones the unchunked kernel produces.  The scan's 64-key steps
//            restart at each chunk's first key; a step only groups consecutive positions (the lowest pending
//            lane is always the smallest position whose key beats the top), so the grouping changes nothing
//   heap     select_xl_kernel's as it is: one element per lane, wave-uniform scalar walk, xl_push_heap /
//            xl_adjust_heap (mxa_select_xl.hpp) replaying libstdc++ operation for operation
//   scores   per key what sel_scores computes at a lane stride of 64 (its general, exact loops): the same
//            helpers (expred_score, g_dot, g_dot_trueex), the same roundings, bias and sinks, the query row's
//            operands loaded once per row and kept across the chunks
//   tables   every key-side table is read where rows_prep left it, through L2: the code modes as
//            select_long_kernel does, and ex_pred's int16 block exponents and sign words too (at every nbd:
//            expred_score reads the raw exponents, which is what the nbd <= 2 key records decode to).  They
//            cannot be staged whole (288 KB at D = 72); staged per chunk they would cost 18 KB a wave beside
//            a 4 KB strip, or a workgroup barrier per chunk to share one copy among four waves on four
//            different rows.  A head's tables stay L2-resident while its rows are scored
//
// One wave per query row, four waves per workgroup, 16 KB of LDS per workgroup: the waves per CU are set by
// the registers (eight workgroups at 128 KB), not by LDS.
#pragma once
#include "mxa_select_xl.hpp"

namespace mxa {

constexpr int kSelXxlWaves = 4;          // one query row per wave at a time
constexpr int kXxlSelChunk = 1024;       // keys per chunk of the strip
constexpr size_t kXxlStripBytes = (size_t)kXxlSelChunk * 4;
static_assert(kXxlRowsT / 32 <= kXxlSelChunk, "the strip is the prune-mask words' scratch afterwards");

// partial_sort(a, a + k, a + T) of the elements (key(j), j) as xl_select computes it, the keys produced chunk
// by chunk: fill(c0, nc) writes the keys of positions c0 .. c0 + nc - 1 to strip[0 .. nc).  Lane p < k returns
// the p-th element.  1 <= k <= 64 <= T; every lane of the wave calls it.
template <typename Fill>
__device__ __forceinline__ XlHeap xxl_select(lu32* strip, int T, int k, int lane, Fill&& fill) {
  XlHeap h;
  h.key = 0u;
  h.idx = (uint32_t)lane;
  h.lane = lane;
  uint32_t top = 0u;
  for (int c0 = 0; c0 < T; c0 += kXxlSelChunk) {
    const int nc = min(kXxlSelChunk, T - c0);
    fill(c0, nc);
    wave_lds_sync();
    int lo = 0;
    if (c0 == 0) {  // the first k elements (k <= 64 < nc): __make_heap
      h.key = lane < k ? strip[lane] : 0u;
      if (k >= 2) {
        int parent = (k - 2) / 2;
        while (true) {
          xl_adjust_heap(h, parent, k, xl_get(h.key, parent), xl_get(h.idx, parent));
          if (parent == 0) break;
          parent--;
        }
      }
      top = xl_get(h.key, 0);
      lo = k;
    }
    for (int base = lo; base < nc; base += 64) {  // __heap_select's scan, 64 keys per step
      const int j = base + lane;
      const uint32_t kv = j < nc ? strip[j] : 0u;  // (0 is below every real key: mxa_order.hpp)
      uint64_t pend = __builtin_amdgcn_ballot_w64(kv > top);
      while (pend) {
        const int l = __builtin_ctzll(pend);
        xl_adjust_heap(h, 0, k, xl_get(kv, l), (uint32_t)(c0 + base + l));
        top = xl_get(h.key, 0);
        pend = __builtin_amdgcn_ballot_w64(kv > top) & ~((2ull << l) - 1ull);
      }
    }
    wave_lds_sync();  // the next chunk's keys overwrite the strip
  }
  for (int last = k - 1; last >= 1; --last) {  // __sort_heap: __pop_heap(first, last, last)
    const uint32_t vk = xl_get(h.key, last), vi = xl_get(h.idx, last);
    xl_move(h, last, 0);
    xl_adjust_heap(h, 0, last, vk, vi);
  }
  return h;
}

// The selection of query row r of head bh: the scores of sel_scores<MODE> (lane stride 64, tables in the
// workspace), their order keys through the strip into xxl_select.  true_out / pred_out are written here.
template <int MODE>
__device__ __forceinline__ XlHeap xxl_select_row(const Rows2Args& a, int bh, int r, int lane, lu32* strip) {
  static_assert(MODE != kModeElsa, "ELSA stops at 1,024 keys");
  const int T = a.T, D = a.D, nbd = a.nbd;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const int64_t kb = (int64_t)bh * T;
  const int64_t grow = (int64_t)bh * a.N + r;
  const int64_t brow = a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)r * a.bs2 : -1;
  const int sum_dt = MODE != kModeTrue && a.in_dt == kF32 ? (int)kF32 : a.s_dt;  // (sel_scores' rule)
  // key j's score v as the caller ranks it: rounded, + bias, to the sinks, its order key into the strip
  auto emit = [&](int j, int c0, float v) {
    v = round_dt(v, a.s_dt);
    if (brow >= 0) v = round_dt(v + load_dt(a.bias, brow + (int64_t)j * a.bs3, a.in_dt), sum_dt);
    if (MODE == kModeTrue) {
      if (a.true_out) a.true_out[grow * T + j] = v;
    } else if (a.pred_out) {
      a.pred_out[grow * T + j] = v;
    }
    strip[j - c0] = order_key(v);
  };
  if constexpr (MODE == kModeExSign) {
    uint32_t sq[kMaxNB];
    int eq[kMaxNB];
#pragma unroll
    for (int b = 0; b < kMaxNB; ++b) {
      sq[b] = b < nbd ? a.qsg[grow * nbd + b] : 0u;
      eq[b] = b < nbd ? exp_from16(a.qsA[grow * nbd + b]) : 0;
    }
    const int16_t* kex = a.ksA + kb * nbd;
    const uint32_t* ksg = a.ksg + kb * nbd;
    return xxl_select(strip, T, a.k_top, lane, [&](int c0, int nc) {
      auto keys = [&](auto nbd_c) {
        constexpr int NBD = decltype(nbd_c)::value;
        for (int j = c0 + lane; j < c0 + nc; j += 64) emit(j, c0, expred_score<NBD>(sq, eq, kex + j * NBD, ksg + j * NBD, D));
      };
      switch (nbd) {
        case 1: keys(std::integral_constant<int, 1>{}); break;
        case 2: keys(std::integral_constant<int, 2>{}); break;
        case 3: keys(std::integral_constant<int, 3>{}); break;
        default: keys(std::integral_constant<int, 4>{}); break;
      }
    });
  } else {
    const int8_t* qsrc = (MODE == kModeTrue ? a.qc : a.qop) + grow * a.dpad;
    const int16_t* qesrc = (MODE == kModeTrue ? a.qsT : a.qsA) + grow * nbd;
    const int8_t* kcd = (MODE == kModeTrue ? a.kc : a.kop) + kb * a.dpad;
    const int16_t* kex = (MODE == kModeTrue ? a.ksT : a.ksA) + kb * nbd;
    uint4 qv[2 * kMaxNB];
    uint4 qz[MODE == kModeTrueEx ? 2 * kMaxNB : 1];
    int qe[kMaxNB];
#pragma unroll
    for (int b = 0; b < kMaxNB; ++b) {
      qv[2 * b] = b < nbd ? *reinterpret_cast<const uint4*>(qsrc + 32 * b) : make_uint4(0, 0, 0, 0);
      qv[2 * b + 1] = b < nbd ? *reinterpret_cast<const uint4*>(qsrc + 32 * b + 16) : make_uint4(0, 0, 0, 0);
      if constexpr (MODE == kModeTrueEx) {
        const int8_t* zsrc = a.qz + grow * a.dpad;
        qz[2 * b] = b < nbd ? *reinterpret_cast<const uint4*>(zsrc + 32 * b) : make_uint4(0, 0, 0, 0);
        qz[2 * b + 1] = b < nbd ? *reinterpret_cast<const uint4*>(zsrc + 32 * b + 16) : make_uint4(0, 0, 0, 0);
      }
      qe[b] = b < nbd ? exp_from16(qesrc[b]) : 0;
    }
    return xxl_select(strip, T, a.k_top, lane, [&](int c0, int nc) {
      for (int j = c0 + lane; j < c0 + nc; j += 64) {
        bool nan = false;
        double acc;
        if constexpr (MODE == kModeTrueEx)
          acc = g_dot_trueex(qv, qz, qe, nbd, kcd + (size_t)j * a.dpad, a.kz + (kb + j) * a.dpad, kex + j * nbd, nan);
        else
          acc = g_dot<MODE == kModeOpMul>(qv, qe, nbd, kcd + (size_t)j * a.dpad, kex + j * nbd, nan);
        float v = nan ? __uint_as_float(0x7FC00000u) : (float)acc;
        // true = quantize_elemwise(fl32(QK^T)) * scale   (matmul.py:88-91, caller)
        if (MODE == kModeTrue) v = round_bfloat(round_dt(v, a.s_dt), a.bfloat, kRoundNearest, 1, a.s_dt) * a.scale;
        emit(j, c0, v);
      }
    });
  }
}

// (waves per SIMD: the heap and a query row's operands fit 128 VGPRs -- four workgroups of four waves per
// SIMD row of the CU is the floor aimed at; LDS would allow ten workgroups)
template <int MODE>
__global__ __launch_bounds__(64 * kSelXxlWaves) __attribute__((amdgpu_waves_per_eu(4, 8))) void select_xxl_kernel(Rows2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int bh = blockIdx.x;
  const int k = a.k_top;
  const int r0 = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r0 + a.rows_per_wg);
  lu32* strip = (lu32*)(smem + (size_t)wave * kXxlStripBytes);
  for (int r = r0 + wave; r < r_end; r += kSelXxlWaves) {
    const XlHeap h = xxl_select_row<MODE>(a, bh, r, lane, strip);
    const int64_t grow = (int64_t)bh * a.N + r;
    if (lane < k) kept_put(a, grow * k + lane, (int)h.idx);
    if (a.mask_out)  // (the strip is dead: its first words are the scratch)
      sel_mask_words(a.mask_out, grow, (a.T + 31) / 32, strip, true, lane, 64, k, [&](int) { return h.idx; });
    wave_lds_sync();  // the next row's keys overwrite the strip
  }
}

}  // namespace mxa
