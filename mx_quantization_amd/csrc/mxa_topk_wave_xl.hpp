// The one-wave-per-row exact-order top-k (mxa_topk_wave.hpp) for rows of up to 4,096 positions:
//     std::nth_element(begin, begin + k - 1, end, cmp); std::sort(begin, begin + k - 1, cmp)
// (torch's CPU topk outside std::partial_sort's regime, TopKImpl.h:45-86, libstdc++ 11) on (order key,
// index) pairs, for every 1 <= k <= n <= kWxMaxN.  The element movements are wave_topk's: median of three,
// the rank-form __unguarded_partition, the depth limit 2 lg n with __heap_select / __sort_heap on lane 0
// (mxa_order.hpp), the stable rank of the final <= 16-element segments.  Three things differ at this length:
//
//   the window  A partition step over r positions is ceil(r / 64) keys per lane, up to 64.  Ranges of at
//               most 1,024 positions take w_partition<16> of mxa_topk_wave.hpp as it is (its E ladder: narrow
//               ranges, narrow steps -- and after the first two or three steps of a row every range is
//               narrow).  Wider ranges walk the window in chunks of 16 registers (wx_part_chunked): the
//               median swap is stored first, so both passes read the mirror as the partition sees it and
//               no mask needs the swap patched in; pass 1 counts the right stops over all chunks; pass 2
//               reads each chunk again and carries baseL, baseR, ncut and nsw across chunks as scalars.
//               The register count stays the 1,024 form's (16 window registers), the code size one more
//               body of the widest step.
//   the widths  positions take 13 bits: the pending-range word is f | l << 13 | d << 26 (d <= 24, at most 24
//               ranges pending: still one VGPR's lanes); the boundary bits are 128 words; the final rank
//               phase computes the ranks of ALL positions into the slot tables (dead by then, u16 per
//               position) before any element moves, then moves the elements 64 at a time with the next 64
//               already read: a segment has <= 16 elements, so a store of chunk e lands in chunks e - 1 ..
//               e + 1, whose sources are in registers by then.
//   LDS         sized from n: the mirror 8 (n + 64) bytes, the two slot tables 4 n, 512 B of boundary words
//               and 512 B of trash slots -- 50,688 B at 4,096 positions (three rows per CU), 14,312 B at
//               1,100.  The two slot tables stay two: a key equal to the pivot is a left AND a right stop,
//               so the two lists together can hold up to 2 (r - 1) positions of a range of r; one r-entry
//               table would have the lists overlap before the swap count is known.
#pragma once
#include "mxa_topk_wave.hpp"

namespace mxa {

constexpr int kWxMaxN = 4096;  // positions < 4,096: 13-bit fields (l may be 4,096), 128 boundary words
__host__ __device__ constexpr size_t wxrow_bytes(int n) {
  return (size_t)8 * wrow_mirror(n) + (((size_t)4 * n + 15) & ~(size_t)15) + 512 + 512;
}
// (WRow of mxa_topk_wave.hpp with 128 boundary words)
__device__ __forceinline__ WRow carve_wxrow(unsigned char* base, int n) {
  WRow g;
  g.A = (lu64*)(wl32*)base;
  g.SL = (wl16*)(base + (size_t)8 * wrow_mirror(n));
  g.SR = g.SL + n;
  g.BW = (wl32*)(base + (size_t)8 * wrow_mirror(n) + (((size_t)4 * n + 15) & ~(size_t)15));
  g.TR = (lu64*)(g.BW + 128);
  return g;
}

// w_part_e for a range of more than 1,024 positions: the window in chunks of 16 registers
__device__ __forceinline__ int wx_part_chunked(const WRow& g, int f, int l, uint32_t lane) {
  const int E = (l - f + 63) >> 6;  // 17 .. 64
  const int mid = f + ((l - f) >> 1);
  const int cpos = f + (lane == 1 ? 1 : 0) + (lane == 2 ? mid - f : 0) + (lane >= 3 ? l - 1 - f : 0);
  const uint64_t cv = g.A[cpos];
  const uint32_t ch = (uint32_t)(cv >> 32), cl = (uint32_t)cv;
  const uint32_t kf = w_readlane(ch, 0), ka = w_readlane(ch, 1), kb = w_readlane(ch, 2), kc = w_readlane(ch, 3);
  // __move_median_to_first(f, f+1, mid, l-1) with cmp = greater (stl_algo.h:79-99)
  int ms;
  if (ka > kb) ms = kb > kc ? 2 : (ka > kc ? 3 : 1);
  else ms = ka > kc ? 1 : (kb > kc ? 3 : 2);
  const int m = ms == 1 ? f + 1 : ms == 2 ? mid : l - 1;
  const uint32_t p = ms == 1 ? ka : ms == 2 ? kb : kc;
  {  // iter_swap(f, m): lane 0 writes A[f] = old m, lane 1 writes A[m] = old f
    const uint32_t xml = w_readlane(cl, ms), xfl = w_readlane(cl, 0);
    lu64* dst = lane == 0 ? g.A + f : lane == 1 ? g.A + m : g.TR + lane;
    *dst = lane == 0 ? pack_ki(p, xml) : pack_ki(kf, xfl);
  }
  wave_lds_sync();  // the window below is the swapped row
  const wl32* wk = (const wl32*)(g.A + f + lane) + 1;
  // pass 1: the right stops' count (position f is never a stop)
  int totR = 0;
  for (int e0 = 0; e0 < E; e0 += 16) {
    uint32_t K[16];
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e0 + e < E) K[e] = wk[128 * (e0 + e)];
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e0 + e < E) totR += __popcll(w_ballot(K[e] >= p) & w_rng(e0 + e == 0 ? 1 : 0, l - f - 64 * (e0 + e)));
  }
  // pass 2: w_part_e's, the bases carried from chunk to chunk
  wl16* const slb = g.SL - 1;
  wl16* const srb = g.SR + totR;
  wl16* const trash = (wl16*)(g.TR + lane);
  int baseL = 0, baseR = 0, ncut = 0, nsw = 0;
  for (int e0 = 0; e0 < E; e0 += 16) {
    uint32_t K[16];
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (e0 + e < E) K[e] = wk[128 * (e0 + e)];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (e0 + e < E) {
        const uint64_t rng = w_rng(e0 + e == 0 ? 1 : 0, l - f - 64 * (e0 + e));
        const uint64_t Lm = w_ballot(K[e] <= p) & rng;
        const uint64_t R = w_ballot(K[e] >= p) & rng;
        const uint32_t PLi = w_mbcnt(Lm >> 1, (uint32_t)baseL + (uint32_t)(Lm & 1));
        const uint32_t PRi = w_mbcnt(R >> 1, (uint32_t)baseR + (uint32_t)(R & 1));
        const uint16_t z = (uint16_t)(f + 64 * (e0 + e) + (int)lane);
        *(w_lanebit(Lm) ? slb + PLi : trash) = z;
        *(w_lanebit(R) ? srb - PRi : trash) = z;
        const uint64_t ok = w_ballot(PLi + PRi <= (uint32_t)totR) & rng;
        ncut += __popcll(ok);
        nsw += __popcll(ok & Lm);
        baseL += __popcll(Lm);
        baseR += __popcll(R);
      }
    }
  }
  wave_lds_sync();
  for (int t = (int)lane; t < nsw; t += 64) {
    const int x = g.SL[t], y = g.SR[t];
    const uint64_t ax = g.A[x], ay = g.A[y];
    g.A[x] = ay;
    g.A[y] = ax;
  }
  wave_lds_sync();
  return f + 1 + ncut;
}
__device__ __forceinline__ int wx_partition(const WRow& g, int f, int l, uint32_t lane) {
  if (l - f <= kWMaxN) return w_partition<kWMaxN / 64>(g, f, l, lane);
  return wx_part_chunked(g, f, l, lane);
}

// std::nth_element(begin, begin + k - 1, end) then std::sort(begin, begin + k - 1) (std::partial_sort when
// k * 64 <= n) on the wave's row of carve_wxrow; afterwards A[p], p < k, holds torch's p-th index in its low
// word.  n, k wave-uniform; n <= kWxMaxN.  wave_topk's text but for the widths and the final rank phase.
__device__ __forceinline__ void wave_topk_xl(const WRow& g, int n, int k) {
  const uint32_t lane = w_lane();
  if (k <= 0) return;
  if (k * 64 <= n) {  // std::partial_sort(begin, begin + k, end)
    if (lane == 0) {
      ln_heap_select(g.A, 0, k, n);
      ln_sort_heap(g.A, 0, k);
    }
    wave_lds_sync();
    return;
  }
  const int nth = k - 1, m = k - 1;
  {  // std::__introselect(0, nth, n, 2 lg n)
    int f = 0, l = n, d = 2 * ilog2(n);
    bool heap = false;
    while (l - f > 3) {
      if (d == 0) {
        heap = true;
        break;
      }
      --d;
      const int cut = wx_partition(g, f, l, lane);
      if (cut <= nth) f = cut;
      else l = cut;
    }
    if (heap) {  // __heap_select(f, nth + 1, l); iter_swap(f, nth)
      if (lane == 0) {
        ln_heap_select(g.A, f, nth + 1, l);
        const uint64_t t = g.A[f];
        g.A[f] = g.A[nth];
        g.A[nth] = t;
      }
    } else if (l - f > 1 && lane == 0) {
      ln_insertion_sort(g.A, f, l);
    }
    wave_lds_sync();
  }
  if (m < 2) return;
  // std::sort(0, m): __introsort_loop(0, m, 2 lg m), threshold 16; the pending ranges on a stack, one per
  // lane of a VGPR; every cut starts a final segment (boundary bits BW, plus 0 and m)
  g.BW[lane] = lane == 0 ? 1u : 0u;
  g.BW[64 + lane] = 0u;
  wave_lds_sync();
  if (lane == 0) w_mark(g, m);
  int maxlen = 0;  // longest final segment that is not heap-sorted
  {
    uint32_t stk = 0;  // lane s: pending range s (f | l << 13 | d << 26)
    int sp = 0;
    int f = 0, l = m, d = 2 * ilog2(m);
    while (true) {
      while (l - f > 16 && d > 0) {
        --d;
        const int cut = wx_partition(g, f, l, lane);
        if (lane == 0) w_mark(g, cut);
        stk = lane == (uint32_t)sp ? (uint32_t)cut | ((uint32_t)l << 13) | ((uint32_t)d << 26) : stk;
        ++sp;
        l = cut;
      }
      if (l - f > 16) {  // depth limit: std::__partial_sort(f, l, l) -- final as it stands
        if (lane == 0) {
          ln_heap_select(g.A, f, l, l);
          ln_sort_heap(g.A, f, l);
        }
        for (int c = f + 1 + (int)lane; c < l; c += 64) w_mark(g, c);  // singletons: rank = identity
        wave_lds_sync();
      } else {
        maxlen = max(maxlen, l - f);
      }
      if (sp == 0) break;
      --sp;
      const uint32_t s = w_readlane(stk, sp);
      f = (int)(s & 8191u);
      l = (int)((s >> 13) & 8191u);
      d = (int)(s >> 26);
    }
  }
  if (maxlen < 2) return;  // every segment a singleton or heap-sorted
  wave_lds_sync();
  // stable rank of each position z < m within its segment [s, t) (wave_topk's composite and its 96-bit
  // boundary window), for ALL positions before any element moves: the ranks go into the slot tables
  const wl32* A32 = (const wl32*)g.A;
  wl16* const RK = g.SL;  // [2 n] u16, m < n
  for (int z = (int)lane; z < m; z += 64) {
    const uint32_t kz = A32[2 * z + 1];
    const int w = z >> 5, o = z & 31;
    const uint32_t b0 = w > 0 ? g.BW[w - 1] : 0u, b1 = g.BW[w], b2 = w < 127 ? g.BW[w + 1] : 0u;
    const uint64_t lowin = ((uint64_t)b1 << 32 | b0) & (~0ull >> (31 - o));  // bits <= 32 + o
    const int s = z - (32 + o - (63 - (int)__clzll(lowin)));
    const uint64_t hiwin = ((uint64_t)b2 << 32 | b1) >> o >> 1;  // bit 0 <-> position z + 1
    const int t = z + 1 + (int)__ffsll((long long)hiwin) - 1;
    const uint64_t cz = ((uint64_t)kz << 32) | (uint32_t)(0xFFFF - z);
    uint32_t r = (uint32_t)s;
    for (int j = 0; j < maxlen; ++j) {
      const int wp = min(s + j, m - 1);
      const uint64_t cw = ((uint64_t)A32[2 * wp + 1] << 32) | (uint32_t)(0xFFFF - wp);
      r += (s + j < t && cw > cz) ? 1u : 0u;
    }
    RK[z] = (uint16_t)r;
  }
  wave_lds_sync();
  // the moves, 64 positions at a time; the next 64 sources are read before this chunk's stores
  uint64_t xn = g.A[min((int)lane, m - 1)];
  for (int z0 = 0; z0 < m; z0 += 64) {
    const uint64_t x = xn;
    const int z = z0 + (int)lane;
    if (z0 + 64 < m) xn = g.A[min(z + 64, m - 1)];
    wave_lds_sync();
    if (z < m) g.A[RK[z]] = x;
  }
  wave_lds_sync();
}

}  // namespace mxa
