// finish_qk_kernel's tiled sibling for rows of 513 .. 1,024 keys (mxa_attention_full): the
// top-k path with k > 64 and the dense branch (top_k=False), every key's score and P.V on
// v_mfma_i32_16x16x32_i8, float32.
//
// finish_qk_kernel (mxa_finish_qk.hpp) holds a row's scores in registers (T <= 256) and the
// head's K and V^T codes in LDS; neither fits 1,024 keys.  The reference quantizes
// softmax(true scores) itself (MX_transformer_block.py:704-705 dense, :700-702 top-k), so the
// row's maximum and sum must be final before any P is coded: no running rescale.  This kernel
// therefore makes THREE PASSES over the key blocks of a tile of 16 query rows (one wave, lane
// (q, g) = (lane % 16, lane / 16) owning keys 32 b + 8 g .. + 7 of query row q, as there) and
// recomputes the scores in each:
//   1. the maximum over the kept keys (and the debug true scores, once per key);
//   2. the sum of exp2((v - mx) log2 e): one fp32 accumulator per lane over its 8 keys of
//      every block in ascending block order, then fq_fsum4 -- a chain of 8 ntb + 2 additions;
//   3. per block p = div_by_sum(e, sum), MX(P) (fq_umax4, p_block, the same code functions),
//      one MFMA per 16 output columns and one fmaf per block into the output accumulators, in
//      ascending block order (n_add = ntb).
// Every rule is finish_qk_kernel's: the exact epilogue (fast shifted-int32 form under the same
// test, else fq_exact), true_score / bias, -inf for a dropped key, the rows whose maximum is
// -inf or whose sum is NaN.  The operands stay where the builders left them: the K codes are
// the MFMA A operand straight from the workspace (8 bytes at (kb + key) dpad + 32 b + 8 g, as
// select_long_kernel and finish16_kernel's LONG variant read K in place), the V^T codes are
// read as finish16_kernel reads them (one contiguous 512-B run per MFMA).  The K operands and mask
// words are loaded a pair of key blocks ahead of their MFMAs (sweep).  LDS holds only the
// per-key terms of the exact epilogue and the V block scales (37 KB at NB = 4).
// Reference: microxscaling/mx/matmul.py:68-76, :85-88; caller
// workloads/PixArt/models/MX_transformer_block.py:656, :679-717.
#pragma once
#include "mxa_finish_qk.hpp"

namespace mxa {

constexpr int kFqlT = 1024;           // the longest row
constexpr int kFqlNTB = kFqlT / 32;   // its key blocks

// LDS per workgroup (nothing per wave), strides fixed: K exponents [NB][1024] (int16, key
// order), the exact epilogue's key terms [3][1024] (int32: smallest block exponent, the
// blocks' offsets from it as bytes, the spread), per 16-key tile [2][64] (smallest exponent,
// largest spread: the fast-path test), V block scales as floats [ceil(D / 16)][32][16]
struct FqlLds {
  size_t ke, kx, tg, vs, total;
};
__host__ __device__ inline FqlLds fql_lds(int nb, int D) {
  FqlLds L;
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  size_t o = 0;
  L.ke = o;
  o += al((size_t)nb * kFqlT * 2);
  L.kx = o;
  o += al((size_t)3 * kFqlT * 4);
  L.tg = o;
  o += al((size_t)2 * 2 * kFqlNTB * 4);
  L.vs = o;
  o += al((size_t)((D + 15) / 16) * kFqlNTB * 16 * 4);
  L.total = o;
  return L;
}

// MXA_FQL_OCC: a tools-only build that asks the register allocator for that many waves per SIMD, for
// same-box A/Bs (build_native defines); the product leaves the choice to the compiler
#ifdef MXA_FQL_OCC
#define MXA_FQL_ATTR __attribute__((amdgpu_waves_per_eu(MXA_FQL_OCC, 8)))
#else
#define MXA_FQL_ATTR
#endif

// NB: 32-element blocks per head dim; W4: P is MXINT4 (finish_qk_kernel's W4); EXTRA: a bias,
// the debug true-score output or bfloatX rounding
template <int NB, bool W4, bool EXTRA>
__global__ __launch_bounds__(512) MXA_FQL_ATTR void finish_qk_long_kernel(Rows2Args a) {
  constexpr int sdt = (int)kF32, idt = (int)kF32;
  constexpr bool kRound = EXTRA;
  constexpr int kes = kFqlT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x;
  const int T = a.T, D = a.D, ntb = a.ntb, ntw = (a.T + 31) / 32;
  const int tpad = 32 * ntb;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const FqlLds L = fql_lds(NB, D);
  int16_t* tke = reinterpret_cast<int16_t*>(smem + L.ke);
  int* tkx = reinterpret_cast<int*>(smem + L.kx);
  int* ttg = reinterpret_cast<int*>(smem + L.tg);
  float* tvs = reinterpret_cast<float*>(smem + L.vs);

  // ---- stage the head's per-key terms and V block scales -------------------------------
  const int64_t kb = (int64_t)bh * T;
  fq_stage_key_terms<NB, kes>(a.ksT, T, kb, tpad, tke, tkx);
  fq_stage_v_scales<kFqlNTB>(a.vs, ntb, D, bh, tvs);
  __syncthreads();
  fq_stage_tile_terms<kes, kFqlNTB>(ntb, tkx, ttg);
  __syncthreads();

  const int8_t* vbase = a.vt + (int64_t)bh * D * a.tpad + 8 * g;  // [ntb][D][32] per head
  const int r_beg = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r_beg + a.rows_per_wg);
  for (int r0 = r_beg + kFqRows * wave; r0 < r_end; r0 += kFqRows * a.waves) {
    const int r = r0 + q;
    const bool valid = r < r_end;
    const int64_t grow = (int64_t)bh * a.N + (valid ? r : r0);
    const int64_t brow = EXTRA && a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)(valid ? r : r0) * a.bs2 : -1;
    const FqQuery<NB> Q = fq_load_query<NB>(a.qc, a.qsT, grow, g);

    // the row's kept bits of keys 32 blk + 8 g .. + 7 (the dense branch: every key < T)
    auto kept_bits = [&](int blk) -> uint32_t {
      if (!valid || blk >= ntb) return 0u;
      if (a.dense) return (1u << min(max(T - (32 * blk + 8 * g), 0), 8)) - 1u;
      return (a.mask_out[grow * ntw + blk] >> (8 * g)) & 0xFFu;
    };
    // key tile `tile`'s A operands of this lane (row fq_key_of_row(16 tile + q)); a key >= T -- a
    // ragged last block, or a tile past the row -- reads nothing and gives zero codes
    auto load_k = [&](int tile, int64_t* ka) {
      const int akey = fq_key_of_row(16 * tile + q);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        ka[b] = 0;
        if (akey < T) ka[b] = *reinterpret_cast<const int64_t*>(a.kc + (kb + akey) * (32 * NB) + 32 * b + 8 * g);
      }
    };
    // the scores of the lane's keys 32 blk + 8 g + 4 t + i (i = 0..3) of key tile 2 blk + t from
    // its A operands ka, a dropped key -inf; first: the pass that writes the debug true scores
    auto scores = [&](int blk, int t, const int64_t* ka, uint32_t kbits, bool first, float* sv) {
      const int tile = 2 * blk + t;
      v4iq_ c[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const v4iq_ zero = {0, 0, 0, 0};
        c[b] = __builtin_amdgcn_mfma_i32_16x16x32_i8(ka[b], Q.qb[b], zero, 0, 0, 0);
      }
      const int key0 = 32 * blk + 8 * g + 4 * t;
      float sc[4];
      fq_tile_scores<NB, kes, kFqlNTB>(c, Q, tile, key0, tke, tkx, ttg, sc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float s = fq_finish_score<EXTRA, kRound>(sc[i], a.scale, a.bfloat, T, a.bias, a.bs3, a.true_out, key0 + i, brow, grow, valid, first, sdt, idt);
        sv[i] = (kbits >> (4 * t + i)) & 1u ? s : -INFINITY;
      }
    };

    // one pass over the row's key blocks in ascending order, body(blk, kbits, ka of tile 2 blk,
    // ka of tile 2 blk + 1).  The K operands and mask bits come from L2 and a wave has few
    // neighbours to hide that behind (2,048 tiles at the PixArt shape: two waves per SIMD), so
    // they are loaded one pair of blocks -- four key tiles -- ahead of their MFMAs
    auto sweep = [&](auto&& body) {
      int64_t kc[4][NB], kn[4][NB];
      uint32_t mc[2], mn[2];
#pragma unroll
      for (int u = 0; u < 4; ++u) load_k(u, kc[u]);
      mc[0] = kept_bits(0);
      mc[1] = kept_bits(1);
      for (int b0 = 0; b0 < ntb; b0 += 2) {
#pragma unroll
        for (int u = 0; u < 4; ++u) load_k(2 * (b0 + 2) + u, kn[u]);
        mn[0] = kept_bits(b0 + 2);
        mn[1] = kept_bits(b0 + 3);
        body(b0, mc[0], kc[0], kc[1]);
        if (b0 + 1 < ntb) body(b0 + 1, mc[1], kc[2], kc[3]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int b = 0; b < NB; ++b) kc[u][b] = kn[u][b];
        mc[0] = mn[0];
        mc[1] = mn[1];
      }
    };

    // ---- pass 1: the maximum over the kept keys ------------------------------------------
    float mx = -INFINITY;
    sweep([&](int blk, uint32_t kbits, const int64_t* ka0, const int64_t* ka1) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float sv[4];
        scores(blk, t, t ? ka1 : ka0, kbits, true, sv);
#pragma unroll
        for (int i = 0; i < 4; ++i) mx = fmaxf(mx, sv[i]);
      }
    });
    mx = fq_fmax4(mx);
    // a row whose max is -inf (every kept score -inf): exp(v - mx) is NaN for every key; the
    // dropped keys are put back to 0 from the mask bits (finish_qk_kernel)
    const bool mx_inf = mx == -INFINITY;

    // ---- pass 2: the sum, one accumulator per lane in ascending key-block order ------------
    float sum = 0.0f;
    sweep([&](int blk, uint32_t kbits, const int64_t* ka0, const int64_t* ka1) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float sv[4];
        scores(blk, t, t ? ka1 : ka0, kbits, false, sv);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float e = __builtin_amdgcn_exp2f((sv[i] - mx) * 1.4426950408889634f);
          if (mx_inf && !((kbits >> (4 * t + i)) & 1u)) e = 0.0f;
          sum += e;
        }
      }
    });
    sum = fq_fsum4(sum);
    const bool nan_sum = sum != sum;  // (a NaN kept score: the dropped keys' p back to 0)
    const float rs = 1.0f / sum;      // p = e / sum by div_by_sum

    // ---- pass 3: per key block P codes, then P.V: O^T = V^T . P^T (finish_qk_kernel's maps) --
    constexpr int NDT = 2 * NB;  // 16-column tiles of D <= 32 NB
    float acc[NDT][4];
#pragma unroll
    for (int u = 0; u < NDT; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f;
    sweep([&](int blk, uint32_t kbits, const int64_t* ka0, const int64_t* ka1) {
      int64_t va[NDT];  // the block's V^T operands, in flight through its scores
#pragma unroll
      for (int u = 0; u < NDT; ++u)
        if (16 * u < D) va[u] = *reinterpret_cast<const int64_t*>(vbase + ((int64_t)blk * D + min(16 * u + q, D - 1)) * 32);
      float p[8];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float sv[4];
        scores(blk, t, t ? ka1 : ka0, kbits, false, sv);
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
            const float x = fl ? p[j] * 0.0f : p[j];
            const uint32_t code = (uint32_t)p_code_bits_f32<W4>(x, pow2f(-es));
            if (j < 4) lo |= code << (8 * j);
            else hi |= code << (8 * (j - 4));
          }
        }
        const int64_t pc = (int64_t)(((uint64_t)hi << 32) | lo);
#pragma unroll
      for (int u = 0; u < NDT; ++u)
        if (16 * u < D) fq_pv_mfma(va[u], pc, sP, tvs + (u * kFqlNTB + blk) * 16 + 4 * g, acc[u]);
    });
    // ---- the tile's output rows -------------------------------------------------------------
    if (valid) {
      const int64_t ob = b_ * a.os0 + h_ * a.os1 + (int64_t)r * a.os2;
#pragma unroll
      for (int u = 0; u < NDT; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int dd = 16 * u + 4 * g + i;
          if (dd < D) store_dt(a.out, ob + dd, round_bfloat(round_dt(acc[u][i], sdt), a.bfloat, kRoundNearest, 1, sdt), sdt);
        }
    }
  }
}

}  // namespace mxa
