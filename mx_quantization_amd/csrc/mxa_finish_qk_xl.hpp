// finish_qk_long_kernel's chunked sibling for DENSE rows of 1,025 .. 4,096 keys (mxa_attention_xl_full:
// top_k=False at 1024 x 1024, MX_transformer_block.py:656, :704-705; MX_pixart_transformer_2d.py:214),
// every key's score and P.V on v_mfma_i32_16x16x32_i8; float32, or (XDT, mxa_attention_dt) float16 /
// bfloat16 tensors or scores.
//
// finish_qk_long_kernel (mxa_finish_qk_long.hpp) keeps the exact epilogue's per-key terms of the WHOLE
// row in LDS (fql_lds, strides fixed at 1,024 keys).  Stretched to 4,096 keys that is 114 KB at NB = 3,
// D = 72 and 146 KB at NB = 4, D = 128: one workgroup per CU.  Here the LDS holds the terms of ONE
// CHUNK of 1,024 keys (32 key blocks) at a time, in the same layout, so a workgroup needs what the
// sibling needs (29 .. 37 KB) whatever T is.  The price is that the waves of a workgroup, each on a
// 16-row tile of its own of the same head, walk the chunks IN LOCKSTEP:
//   for each round of tiles (one trip count for the whole workgroup, see `rounds`)
//     for each of the three passes (maximum; sum; codes and P.V)
//       for each chunk: barrier, the workgroup stages the chunk's key terms (pass 3: and its V block
//       scales), barrier, the tile terms, barrier; then every wave takes the chunk's key blocks.
// A wave whose round has no tile left walks the chunks on a clamped row with no key kept and stores
// nothing: every barrier is reached by every wave.
// The arithmetic is finish_qk_long_kernel's, addition for addition: the scores are recomputed in each
// pass from one MFMA per (16 keys, 32-element block) and fq_tile_scores / fq_finish_score; pass 2 sums
// into ONE fp32 accumulator per lane over its 8 keys of every block in ascending block order over the
// whole row (no per-chunk partial sums), then fq_fsum4; pass 3 adds one fmaf per key block into the
// output accumulators in ascending block order; no running rescale.  A row of T keys whose keys from
// 1,024 on are masked to -inf therefore gives the bytes finish_qk_long_kernel gives on its first
// 1,024 keys.  The indices into LDS (key, tile, block) are chunk-local; the key handed to
// fq_finish_score (bias, true_out), the K codes and the V^T codes are addressed by the key's place in
// the row.  The K codes and V^T codes stay in the workspace (L2); sweep's loads run a pair of key
// blocks ahead, across chunk borders too (a chunk holds an even number of blocks, so no pair straddles
// one).  The dense form's kept bits of a lane are "key < T"; the MASKED form (k_top > 64 outside
// partial_sort's regime, mxa_attention_nth: MXA_FIN_MFMA_XL) reads the selection's prune-mask words the way
// finish_qk_long_kernel does, a block's byte of the row's word a pair of key blocks ahead with the K operands --
// so a chunk's mask words travel with that chunk's per-key terms -- and everything else is the dense form's.
// Reference: microxscaling/mx/matmul.py:68-76, :85-88.
#pragma once
#include "mxa_finish_qk_long.hpp"

namespace mxa {

// NB: 32-element blocks per head dim; W4: P is MXINT4; EXTRA: a bias, the debug true-score output or
// bfloatX rounding (finish_qk_long_kernel's)
// XDT (MXINT8 P, NBX = NB + kFqDtNB): finish_qk_long_kernel's XDT rules inside the lockstep walk.  The dtypes
// are kernel arguments, so every branch on them is uniform over the workgroup, and none of them encloses a
// barrier: stage() and the trip counts of rounds, passes, chunks and blocks do not read them
// MASKED (float32): NBX = NB + kFqXlMaskNB, as XDT an offset of the block count that the dense instantiations
// do not use, so that they keep their names and code
// MASKED with XDT (MXINT8 P, k_top > kGxlMaxK at float16 / bfloat16, mxa_attention_nth_dt): both offsets, NBX = NB +
// kFqDtNB + kFqXlMaskNB.  The mask words only choose which scores are -inf, and the XDT rules work on the scores
// that remain, so the two forms meet without a line of their own
constexpr int kFqXlMaskNB = 16;
template <int NBX, bool W4, bool EXTRA>
__global__ __launch_bounds__(512) void finish_qk_xl_kernel(Rows2Args a) {
  constexpr int NB = NBX % kFqDtNB;
  constexpr bool MASKED = NBX >= kFqXlMaskNB;
  constexpr bool XDT = (NBX % kFqXlMaskNB) >= kFqDtNB;
  static_assert(kFqXlMaskNB == 2 * kFqDtNB && NB >= 1 && NB <= 4 && NBX < 2 * kFqXlMaskNB, "NBX: NB + the two offsets");
  static_assert(!(W4 && XDT), "MXINT4 P: float32");
  const int sdt = XDT ? a.s_dt : (int)kF32, idt = XDT ? a.in_dt : (int)kF32;
  constexpr bool kRound = XDT || EXTRA;
  constexpr int kes = kFqlT;  // keys per chunk = the LDS tables' key stride
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x;
  const int T = a.T, D = a.D, ntb = a.ntb;
  const int nch = (ntb + kFqlNTB - 1) / kFqlNTB;  // chunks of the row
  const int b_ = bh / a.H, h_ = bh % a.H;
  const FqlLds L = fql_lds(NB, D);
  int16_t* tke = reinterpret_cast<int16_t*>(smem + L.ke);
  int* tkx = reinterpret_cast<int*>(smem + L.kx);
  int* ttg = reinterpret_cast<int*>(smem + L.tg);
  float* tvs = reinterpret_cast<float*>(smem + L.vs);

  const int64_t kb = (int64_t)bh * T;
  // chunk ch's tables, by the whole workgroup: the per-key terms of its keys (chunk-local index), the
  // tile terms and, vscales (pass 3), the V block scales [ceil(D / 16)][32][16] of its key blocks.
  // The first barrier: every wave is done with the tables of the chunk before
  auto stage = [&](int ch, bool vscales) {
    const int cT = min(kFqlT, T - kFqlT * ch), nbc = min(kFqlNTB, ntb - kFqlNTB * ch);
    __syncthreads();
    fq_stage_key_terms<NB, kes>(a.ksT, cT, kb + (int64_t)kFqlT * ch, 32 * nbc, tke, tkx);
    if (vscales) {
      const int16_t* vssrc = a.vs + ((int64_t)bh * ntb + kFqlNTB * ch) * D;
      for (int i = threadIdx.x; i < nbc * D; i += blockDim.x) {
        const int tb = i / D, dd = i - tb * D;
        tvs[((dd >> 4) * kFqlNTB + tb) * 16 + (dd & 15)] = scale_f(exp_from16(vssrc[i]));
      }
    }
    __syncthreads();
    fq_stage_tile_terms<kes, kFqlNTB>(nbc, tkx, ttg);
    __syncthreads();
  };

  const int8_t* vbase = a.vt + (int64_t)bh * D * a.tpad + 8 * g;  // [ntb][D][32] per head
  const int r_beg = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r_beg + a.rows_per_wg);
  // THE loop bound of the workgroup: its tiles over its waves, rounded up -- the same for every wave,
  // because every round holds 9 nch barriers (blockDim.x = 64 a.waves)
  const int wg_tiles = (max(r_end - r_beg, 0) + kFqRows - 1) / kFqRows;
  const int rounds = (wg_tiles + a.waves - 1) / a.waves;
  for (int round = 0; round < rounds; ++round) {
    const int r0 = r_beg + kFqRows * (round * a.waves + wave);
    const bool has_tile = r0 < r_end;  // (wave-uniform) else: the walk on a clamped row, nothing kept or stored
    const int r = r0 + q;
    const bool valid = has_tile && r < r_end;
    const int crow = valid ? r : (has_tile ? r0 : r_beg);
    const int64_t grow = (int64_t)bh * a.N + crow;
    const int64_t brow = EXTRA && a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)crow * a.bs2 : -1;
    const FqQuery<NB> Q = fq_load_query<NB>(a.qc, a.qsT, grow, g);

    // the row's kept bits of keys 32 blk + 8 g .. + 7: every key < T (MASKED: the row's mask word of the block;
    // a.ntb == ceil(T / 32) words per row, mxa_fin_qkxl.hip)
    auto kept_bits = [&](int blk) -> uint32_t {
      if (!valid || blk >= ntb) return 0u;
      if constexpr (MASKED) return (a.mask_out[grow * ntb + blk] >> (8 * g)) & 0xFFu;
      return fq_dense_bits(T, blk, g);
    };
    auto load_k = [&](int tile, int64_t* ka) { fql_load_k<NB>(a.kc, kb, T, tile, q, g, ka); };
    // the scores of the lane's keys 32 blk + 8 g + 4 t + i (i = 0..3) from key tile 2 blk + t's A
    // operands, a dropped key -inf; blk: the block's number in the row, cb: its chunk's first block
    auto scores = [&](int blk, int cb, int t, const int64_t* ka, uint32_t kbits, bool first, float* sv) {
      v4iq_ c[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const v4iq_ zero = {0, 0, 0, 0};
        c[b] = __builtin_amdgcn_mfma_i32_16x16x32_i8(ka[b], Q.qb[b], zero, 0, 0, 0);
      }
      const int lkey0 = 32 * (blk - cb) + 8 * g + 4 * t;  // in the chunk's tables
      const int key0 = 32 * blk + 8 * g + 4 * t;          // in the row
      float sc[4];
      fq_tile_scores<NB, kes, kFqlNTB>(c, Q, 2 * (blk - cb) + t, lkey0, tke, tkx, ttg, sc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float s = fq_finish_score<EXTRA, kRound>(sc[i], a.scale, a.bfloat, T, a.bias, a.bs3, a.true_out, key0 + i, brow, grow, valid, first, sdt, idt);
        sv[i] = (kbits >> (4 * t + i)) & 1u ? s : -INFINITY;
      }
    };

    // one pass over the row's key blocks in ascending order, chunk by chunk: body(blk, cb, kbits, ka of
    // tile 2 blk, ka of tile 2 blk + 1).  The K operands are loaded one pair of blocks -- four key tiles
    // -- ahead of their MFMAs (finish_qk_long_kernel's sweep); the pair in flight at a chunk's end is the
    // next chunk's first
    auto sweep = [&](bool vscales, auto&& body) {
      int64_t kc[4][NB], kn[4][NB];
      uint32_t mc[2], mn[2];
#pragma unroll
      for (int u = 0; u < 4; ++u) load_k(u, kc[u]);
      mc[0] = kept_bits(0);
      mc[1] = kept_bits(1);
      for (int ch = 0; ch < nch; ++ch) {
        stage(ch, vscales);
        const int cb = kFqlNTB * ch, ce = min(ntb, cb + kFqlNTB);
        for (int b0 = cb; b0 < ce; b0 += 2) {
#pragma unroll
          for (int u = 0; u < 4; ++u) load_k(2 * (b0 + 2) + u, kn[u]);
          mn[0] = kept_bits(b0 + 2);
          mn[1] = kept_bits(b0 + 3);
          body(b0, cb, mc[0], kc[0], kc[1]);
          if (b0 + 1 < ntb) body(b0 + 1, cb, mc[1], kc[2], kc[3]);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int b = 0; b < NB; ++b) kc[u][b] = kn[u][b];
          mc[0] = mn[0];
          mc[1] = mn[1];
        }
      }
    };

    // ---- pass 1: the maximum over the keys --------------------------------------------------
    float mx = -INFINITY;
    sweep(false, [&](int blk, int cb, uint32_t kbits, const int64_t* ka0, const int64_t* ka1) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float sv[4];
        scores(blk, cb, t, t ? ka1 : ka0, kbits, true, sv);
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = fmaxf(mx, sv[i]);
      }
    });
    mx = fq_fmax4(mx);
    // a row whose max is -inf: exp(v - mx) is NaN for every key; the dropped keys are put back to 0
    const bool mx_inf = mx == -INFINITY;

    // ---- pass 2: the sum, one accumulator per lane in ascending key-block order over the row ----
    float sum = 0.0f;
    sweep(false, [&](int blk, int cb, uint32_t kbits, const int64_t* ka0, const int64_t* ka1) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float sv[4];
        scores(blk, cb, t, t ? ka1 : ka0, kbits, false, sv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float e = __builtin_amdgcn_exp2f((sv[i] - mx) * 1.4426950408889634f);
          if (mx_inf && !((kbits >> (4 * t + i)) & 1u)) e = 0.0f;
          sum += e;
        }
      }
    });
    sum = fq_fsum4(sum);
    const bool nan_sum = sum != sum;  // (a NaN score: the dropped keys' p back to 0)
    const float rs = 1.0f / sum;      // p = e / sum by div_by_sum

    // ---- pass 3: per key block P codes, then P.V: O^T = V^T . P^T (finish_qk_kernel's maps) --
    // (the P block coding and the output store: finish_qk_long_kernel's text, see mxa_finish_qk.hpp)
    constexpr int NDT = 2 * NB;  // 16-column tiles of D <= 32 NB
    float acc[NDT][4];
#pragma unroll
    for (int u = 0; u < NDT; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f;
    sweep(true, [&](int blk, int cb, uint32_t kbits, const int64_t* ka0, const int64_t* ka1) {
      int64_t va[NDT];  // the block's V^T operands, in flight through its scores
#pragma unroll
      for (int u = 0; u < NDT; ++u)
        if (16 * u < D) va[u] = *reinterpret_cast<const int64_t*>(vbase + ((int64_t)blk * D + min(16 * u + q, D - 1)) * 32);
      float p[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float sv[4];
        scores(blk, cb, t, t ? ka1 : ka0, kbits, false, sv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = __builtin_amdgcn_exp2f((sv[i] - mx) * 1.4426950408889634f);
          const float q1 = div_by_sum(e, sum, rs);
          float pv = kRound ? round_dt(round_bfloat(q1, a.bfloat, kRoundNearest, 1, sdt), sdt) : q1;
          if (nan_sum && !((kbits >> (4 * t + i)) & 1u)) pv = 0.0f;
          p[4 * t + i] = pv;
        }
      }
      uint32_t bm = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) bm = max(bm, __float_as_uint(p[j]) & 0x7FFFFFFFu);
        bm = fq_umax4(bm);
        const PBlock pb = p_block(bm, a.flush_p, sdt, kPUnit<W4>);
        const int es = pb.es;
        const bool fl = pb.flush;
        const float sP = pb.sP;
        uint32_t lo = 0u, hi = 0u;
        if (es != kExpNaN) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            uint32_t code;
            const float x = fl ? p[j] * 0.0f : p[j];
            if (XDT) code = (uint32_t)(int)round_code(x, es, 8, kRoundNearest, sdt) & 0xFFu;
            else code = (uint32_t)p_code_bits_f32<W4>(x, pow2f(-es));
            if (j < 4) lo |= code << (8 * j);
            else hi |= code << (8 * (j - 4));
          }
        }
        const int64_t pc = (int64_t)(((uint64_t)hi << 32) | lo);
#pragma unroll
      for (int u = 0; u < NDT; ++u)
        if (16 * u < D) fq_pv_mfma(va[u], pc, sP, tvs + (u * kFqlNTB + (blk - cb)) * 16 + 4 * g, acc[u]);
    });
    // ---- the tile's output rows -------------------------------------------------------------
    if (valid) fq_store_tile<NDT>(a.out, b_ * a.os0 + h_ * a.os1 + (int64_t)r * a.os2, D, g, a.bfloat, sdt, acc);
  }
}

}  // namespace mxa
