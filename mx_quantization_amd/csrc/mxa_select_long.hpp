// Selection kernel for rows of 513 .. 1,024 keys (PixArt 512x512 self-attention: 1,024
// tokens): the approximate (or true) scores of mxa_select.hpp's sel_scores fed straight into
// the one-wave-per-row top-k of mxa_topk_wave.hpp.
//
// Per workgroup (one head, a chunk of its query rows; four waves): wave w takes rows r0 + w,
// r0 + w + 4, ...  Lane l scores keys l, l + 64, ... and writes pack_ki(order_key(v), j) into
// the wave's WRow mirror; wave_topk<16> orders it; the kept indices go out through kept_put,
// the prune-mask words through sel_mask_words, as in topk_wave_kernel.  k_top == 0: the
// scores alone.
//
// The key-side tables (SelTabs):
//   ex_pred   sign words + block exponents in LDS (at most 24 KB for 1,024 keys); for nbd <= 2
//             the key records of sel_lds without the 16 range-flag words, which cover 512 keys
//             only: with a lane stride of 64 sel_scores takes its general, exact loop
//   ELSA      hash words + cosine table in LDS (sel_stage as it is)
//   MXINT4 / EXION / partial_* / true_ex / the true scores: nothing staged.  The code tables
//             are T (dpad + 16) bytes, 115 KB (D = 72) to 147 KB (D = 128) and twice that for
//             true_ex, next to 54 KB of row areas: SelTabs points at the K operands in the
//             workspace (row stride dpad) and sel_scores reads them through L2, where a head's
//             operands (<= 256 KB) stay resident while its 1,024 rows are scored.
#pragma once
#include "mxa_launch.hpp"
#include "mxa_select.hpp"

namespace mxa {

static_assert(kLongRowsT == kWMaxN, "the long rows' bound is the wave top-k's");
constexpr int kSelLongWaves = 4;  // one query row per wave at a time

// LDS of the long rows' score tables: those of sel_lds for the modes that stage any
__host__ __device__ inline SelLds sel_lds_long(int mode, int T, int D, int kst, int nbd) {
  if (mode == kModeExSign || mode == kModeElsa) return sel_lds(mode, T, D, kst, nbd);
  return SelLds{};
}

template <int MODE>
__device__ __forceinline__ SelTabs sel_stage_long(const Rows2Args& a, unsigned char* smem, const SelLds& L, int bh) {
  if constexpr (MODE == kModeElsa) {
    return sel_stage<MODE>(a, smem, L, bh);
  } else if constexpr (MODE == kModeExSign) {
    if (a.nbd > 2) return sel_stage<MODE>(a, smem, L, bh);
    SelTabs t{};  // the key records (sel_lds), no range flags
    t.trec = reinterpret_cast<uint32_t*>(__builtin_assume_aligned(smem + L.ex, 16));
    const int nbd = a.nbd;
    const int64_t kb = (int64_t)bh * a.T;
    for (int i = threadIdx.x; i < a.T * nbd; i += blockDim.x) {
      const int j = nbd == 2 ? i >> 1 : i, b = i - j * nbd;
      t.trec[2 * nbd * j + b] = a.ksg[kb * nbd + i];
      t.trec[2 * nbd * j + nbd + b] = expred_rec_word(a.ksA[kb * nbd + i]);
    }
    __syncthreads();
    return t;
  } else {  // the K operands where rows_prep left them (a.kst == a.dpad: launch_select_long)
    SelTabs t{};
    const int64_t kb = (int64_t)bh * a.T;
    t.tcd = const_cast<int8_t*>((MODE == kModeTrue ? a.kc : a.kop) + kb * a.dpad);
    t.tex = const_cast<int16_t*>((MODE == kModeTrue ? a.ksT : a.ksA) + kb * a.nbd);
    if (MODE == kModeTrueEx) t.tz = const_cast<int8_t*>(a.kz + kb * a.dpad);
    return t;
  }
}

template <int MODE>
__global__ __launch_bounds__(64 * kSelLongWaves) __attribute__((amdgpu_waves_per_eu(2, 8))) void select_long_kernel(Rows2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int bh = blockIdx.x;
  const int T = a.T, k = a.k_top;
  const int r0 = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r0 + a.rows_per_wg);
  const SelLds L = sel_lds_long(MODE, T, a.D, a.kst, a.nbd);
  const SelTabs t = sel_stage_long<MODE>(a, smem, L, bh);
  const WRow g = carve_wrow(smem + L.rows + (size_t)wave * wrow_bytes(T), T);
  for (int r = r0 + wave; r < r_end; r += kSelLongWaves) {
    sel_scores<MODE>(a, t, bh, r, lane, 64, [&](int j, float, uint32_t key, auto) { g.A[j] = pack_ki(key, (uint32_t)j); });
    if (k <= 0) continue;  // scores only
    wave_lds_sync();
    wave_topk<kWMaxN / 64>(g, T, k);
    const int64_t grow = (int64_t)bh * a.N + r;
    for (int p = lane; p < k; p += 64) kept_put(a, grow * k + p, (int)(uint32_t)g.A[p]);
    if (a.mask_out)
      sel_mask_words(a.mask_out, grow, (T + 31) / 32, (lu32*)g.SL, true, lane, 64, k, [&](int p) { return (uint32_t)g.A[p]; });
    wave_lds_sync();  // the next row's scores overwrite the mirror
  }
}

}  // namespace mxa
