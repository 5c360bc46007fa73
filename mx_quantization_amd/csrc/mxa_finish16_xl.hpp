// Finishing kernel of the top-k path for rows of 1,025 .. 4,096 keys (k <= 64): finish16_kernel's
// LONG form (mxa_finish16.hpp) with the keys walked in CHUNKS of 1,024.
//
// The LONG instantiation sizes its per-wave LDS by T -- the 16 x (tpad + 16) P code tile, sP
// [ntb][16] and bm [16][ntb]: about 82 KB per wave at 4,096 keys.  Here the per-wave area is that
// of one chunk of 32 MX blocks (16 x 1,040 code bytes, sP [32][16], bm [16][32]: 20,736 B) whatever
// T is; beside it only the V block scales grow with T ([ntb][D] floats: 36 KB at D = 72).
// Per tile of 16 query rows (one wave, four lanes per row, slots ph, ph + 4, ...):
//   1. once: the kept keys' true scores (the K rows gathered from the workspace, as LONG does) and
//      the softmax; the (index, p) slots stay in registers across the chunks;
//   2. per chunk c: the slots whose key lies in [1024 c, 1024 c + 1024) give their block maxima
//      (LDS atomic max), the block scales and code multipliers follow, the codes go into the
//      chunk's tile; then P.V on v_mfma_i32_16x16x32_i8 per 32-key block with finish16_kernel's
//      per-block epilogue, the V^T operands prefetched two blocks ahead across chunk borders;
//      the written positions are cleared.
// The MX blocks of P along the keys are 32 keys, so none straddles a chunk: every block's scale,
// codes, int32 sum and fp32 epilogue are those of the unchunked kernel, in the same block order.
// No key block is skipped: a block no row keeps still multiplies its zero codes with V's block
// scale, so a non-finite scale reaches every row's output column as in the reference's dense
// 0 * NaN.  (At the Sigma shape 16 rows x 20 keys touch most of the 128 blocks anyway.)
// A kernel of its own, so that no finish16_kernel instantiation's registers move (see there).
// P is MXINT8 or (W4) MXINT4.  float32, or (XDT, MXINT8 P: mxa_attention_dt) float16 / bfloat16 tensors or
// scores with finish16_kernel's XDT rules: the dtype roundings at run time, P's shared exponents taken in the
// score dtype, each chunk's bm holding the block word (es + 1024 and the flush flag) for p_code_word.  Block
// scales are per block, so the chunking cannot change a code there either.
#pragma once
#include "mxa_finish16.hpp"

namespace mxa {

constexpr int kXlChunkBlocks = 32;                      // MX blocks of P per chunk
constexpr int kXlChunk = 32 * kXlChunkBlocks;           // keys per chunk
constexpr int kXlVst = kXlChunk + 16;                   // the code tile's row stride (16 pad columns)
constexpr int kFin16XlDtKS = 64;                        // finish16_xl_kernel's KSX of an XDT instantiation: KS + this

// LDS: the V block scales as floats [ntb][D], then per wave the chunk's P code tile [16][kXlVst],
// its block scales sP [32][16] (float) and block maxima / code multipliers bm [16][32] (u32)
struct Fin16XlLds { size_t ve, waves, sp, bm, per_wave, total; };
__host__ __device__ inline Fin16XlLds fin16_xl_lds(int D, int ntb, int waves) {
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  Fin16XlLds L;
  L.ve = 0;
  L.waves = al((size_t)ntb * D * 4);
  L.sp = (size_t)kFin16 * kXlVst;
  L.bm = L.sp + (size_t)kXlChunkBlocks * kFin16 * 4;
  L.per_wave = L.bm + (size_t)kFin16 * kXlChunkBlocks * 4;
  L.total = L.waves + (size_t)waves * L.per_wave;
  return L;
}

// NB: 32-blocks per head dim; KS: kept slots per lane (k <= 4 KS); EXTRA: a bias, the debug
// true-score output or bfloatX rounding; W4: MXINT4 P
// XDT travels in the slot count, KSX = KS + kFin16XlDtKS, as LONG does in finish16_kernel: the float32
// instantiations keep the names and the code they had.  Its occupancy targets are the float32 form's: the
// run-time roundings sit outside the per-block P.V loop (the scores, the softmax and one code per slot and
// chunk), so they add no registers that live across it
template <int NB, int KSX, bool EXTRA, bool W4>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NB <= 2 && KSX % kFin16XlDtKS <= 12 ? kFin16Occ : (NB * (KSX % kFin16XlDtKS) <= 64 ? 3 : 2), 8))) void finish16_xl_kernel(Rows2Args a) {
  constexpr int KS = KSX % kFin16XlDtKS;
  constexpr bool XDT = KSX >= kFin16XlDtKS;
  static_assert(!(W4 && XDT) && (!XDT || EXTRA), "MXINT4 P: float32; float16 / bfloat16 always round");
  constexpr bool kRound = EXTRA;
  const int sdt = XDT ? a.s_dt : (int)kF32, idt = XDT ? a.in_dt : (int)kF32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bh = blockIdx.x;
  const int T = a.T, D = a.D, ntb = a.ntb, k = a.k_top;
  constexpr int nbd = NB;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const Fin16XlLds L = fin16_xl_lds(D, ntb, a.waves);
  float* tvs = reinterpret_cast<float*>(smem + L.ve);
  unsigned char* wb = smem + L.waves + (size_t)wave * L.per_wave;
  int8_t* ptile = reinterpret_cast<int8_t*>(wb);
  float* sP = reinterpret_cast<float*>(wb + L.sp);
  uint32_t* bmw = reinterpret_cast<uint32_t*>(wb + L.bm);  // [16][32]
  const int pr = lane >> 2, ph = lane & 3;  // the lane's tile row and slot phase

  const int r_beg = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r_beg + a.rows_per_wg);
  uint32_t* bm = bmw + pr * kXlChunkBlocks;
  const int pad = kXlChunk + ph;  // the code column of a slot outside the chunk (never read by the MFMA)
  const int ln = lane & 15, kg = lane >> 4;
  const int8_t* vbase = a.vt + (int64_t)bh * D * a.tpad + 8 * kg;
  constexpr int NDT = 2 * NB;  // 16-column tiles of D <= 32 NB
  int64_t bv[NDT], bw[NDT];  // V^T operands of key blocks b, b + 1 (in flight ahead of use)
  auto load_v = [&](int b, int64_t* dst) {
#pragma unroll
    for (int u = 0; u < NDT; ++u)
      if (16 * u < D) dst[u] = *reinterpret_cast<const int64_t*>(vbase + ((int64_t)b * D + min(16 * u + ln, D - 1)) * 32);
  };
  int ixn[KS];  // the next tile's kept indices, loaded while the current tile finishes
  auto load_ix = [&](int r0n) {
    const int rn = r0n + pr;
    const int64_t gn = (int64_t)bh * a.N + (rn < r_end ? rn : r_beg);
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const int s = ph + 4 * t;
      ixn[t] = rn < r_end && s < k ? kept_get(a, gn * k + s) : 0;
    }
  };
  load_ix(r_beg + kFin16 * wave);  // (in flight through the staging)

  // ---- stage the V block scales; clear the code tile and the block maxima -------------------
  const int64_t kb = (int64_t)bh * T;
  {
    const int16_t* vssrc = a.vs + (int64_t)bh * ntb * D;
    for (int i = threadIdx.x; i < ntb * D; i += blockDim.x) tvs[i] = scale_f(exp_from16(vssrc[i]));
    for (int i = lane; i < kFin16 * kXlVst / 16; i += 64) reinterpret_cast<uint4*>(ptile)[i] = make_uint4(0, 0, 0, 0);
    for (int i = lane; i < kFin16 * kXlChunkBlocks; i += 64) bmw[i] = 0u;
  }
  __syncthreads();

  for (int r0 = r_beg + kFin16 * wave; r0 < r_end; r0 += kFin16 * a.waves) {
    const int r = r0 + pr;
    const bool valid = r < r_end;
    const int64_t grow = (int64_t)bh * a.N + (valid ? r : r0);
    const int64_t brow = EXTRA && a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)(valid ? r : r0) * a.bs2 : -1;
    // the first two key blocks' V^T operands, in flight through the scores and softmax (ntb >= 33)
    load_v(0, bv);
    load_v(1, bw);
    uint4 qv[2 * NB];
    int qe[NB];
    load_query_row<NB>(a, grow, qv, qe);
    int ix[KS];
    bool on[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      on[t] = valid && ph + 4 * t < k;
      ix[t] = ixn[t];
    }
    auto true_of = [&](int j) -> float {  // the true score of key j (+ bias: EXTRA only)
      const float acc = true_dot<NB>(qv, qe, a.kc + (kb + j) * a.dpad, a.ksT + (kb + j) * nbd);
      const float t = true_score<kRound>(acc, a.scale, a.bfloat, sdt);
      return kRound && brow >= 0 ? true_score_bias(t, a.bias, brow + (int64_t)j * a.bs3, idt, sdt) : t;
    };
    if (EXTRA && a.true_out && valid)  // debug output: every key's true score
      for (int j = ph; j < T; j += 4) a.true_out[grow * T + j] = true_of(j);

    // ---- 1. kept scores and softmax: p in v[], once per tile ----------------------------------
    float v[KS];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const float s = true_of(ix[t]);
      v[t] = on[t] ? s : -INFINITY;
      mx = fmaxf(mx, v[t]);
    }
    mx = fin16_qmax(mx);
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      v[t] = on[t] ? __builtin_amdgcn_exp2f((v[t] - mx) * 1.4426950408889634f) : 0.0f;
      sum += v[t];
    }
    sum = fin16_qsum(sum);
    const float rs = 1.0f / sum;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      float p = div_by_sum(v[t], sum, rs);
      if (kRound) p = round_dt(round_bfloat(p, a.bfloat, kRoundNearest, 1, sdt), sdt);
      v[t] = p;
    }

    float acc[NDT][4];
#pragma unroll
    for (int u = 0; u < NDT; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f;
    if (r0 + kFin16 * a.waves < r_end) load_ix(r0 + kFin16 * a.waves);

    // ---- 2. per chunk of 32 key blocks: MX(P) into the chunk's tile, then P.V ------------------
    for (int cb = 0; cb < ntb; cb += kXlChunkBlocks) {
      const int nbc = min(kXlChunkBlocks, ntb - cb);
      // the block maxima of the chunk's slots (a slot outside it adds max(., 0): no change)
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        const bool in = on[t] && (ix[t] >> 5) - cb >= 0 && (ix[t] >> 5) - cb < kXlChunkBlocks;
        atomicMax(&bm[(ix[t] >> 5) & (kXlChunkBlocks - 1)], in ? __float_as_uint(v[t]) & 0x7FFFFFFFu : 0u);
      }
      wave_lds_sync();
      // per block: the scale sP (NaN for a NaN block) and the code multiplier 2^-es (0 for a NaN
      // or flushed block; XDT: the block word of p_code_word), finish16_kernel's rule
      for (int bk = ph; bk < kXlChunkBlocks; bk += 4) {
        int e_raw;
        const int es = scale_exponent_dt(bm[bk], 127, sdt, &e_raw);
        const bool fl = a.flush_p && !(e_raw != kExpNaN && e_raw > -127);
        sP[bk * kFin16 + pr] = scale_f(es == kExpNaN ? kExpNaN : es - kPUnit<W4>);
        if (XDT) bm[bk] = (es == kExpNaN ? 0u : (uint32_t)(es + 1024)) | (fl ? 0x10000u : 0u);
        else bm[bk] = __float_as_uint(es == kExpNaN || fl ? 0.0f : pow2f(-es));
      }
      wave_lds_sync();
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        const bool in = on[t] && (ix[t] >> 5) - cb >= 0 && (ix[t] >> 5) - cb < kXlChunkBlocks;
        const uint32_t e = bm[(ix[t] >> 5) & (kXlChunkBlocks - 1)];
        // (a slot outside the chunk codes against a block that is not its own: the result goes to the pad)
        const int code = XDT ? p_code_word(v[t], e, sdt) : (int)p_code_bits_f32<W4>(v[t], __uint_as_float(e));
        ptile[pr * kXlVst + (in ? ix[t] & (kXlChunk - 1) : pad)] = (int8_t)code;
      }
      wave_lds_sync();
      // P.V, key block outer (the lane maps of finish16_kernel); b: the block's number in the row
      for (int b = cb; b < cb + nbc; ++b) {
        int64_t bn[NDT];
        if (b + 2 < ntb) load_v(b + 2, bn);  // two blocks ahead
        const int64_t av = *reinterpret_cast<const int64_t*>(ptile + ln * kXlVst + 32 * (b - cb) + 8 * kg);
        const float4 s4 = *reinterpret_cast<const float4*>(sP + (b - cb) * kFin16 + 4 * kg);
#pragma unroll
        for (int u = 0; u < NDT; ++u) {
          if (16 * u < D) {
            const v4i16_ zero = {0, 0, 0, 0};
            const v4i16_ c = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, bv[u], zero, 0, 0, 0);
            const float sv = tvs[b * D + min(16 * u + ln, D - 1)];
            acc[u][0] = fmaf((float)c[0], s4.x * sv, acc[u][0]);
            acc[u][1] = fmaf((float)c[1], s4.y * sv, acc[u][1]);
            acc[u][2] = fmaf((float)c[2], s4.z * sv, acc[u][2]);
            acc[u][3] = fmaf((float)c[3], s4.w * sv, acc[u][3]);
          }
        }
#pragma unroll
        for (int u = 0; u < NDT; ++u) {
          bv[u] = bw[u];
          bw[u] = bn[u];
        }
      }
      wave_lds_sync();  // every lane's MFMA reads of the tile are done
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        const bool in = on[t] && (ix[t] >> 5) - cb >= 0 && (ix[t] >> 5) - cb < kXlChunkBlocks;
        ptile[pr * kXlVst + (in ? ix[t] & (kXlChunk - 1) : pad)] = 0;
      }
      for (int bk = ph; bk < kXlChunkBlocks; bk += 4) bm[bk] = 0u;
      wave_lds_sync();
    }

    // ---- 3. output rows (64-B segments per row) ---------------------------------------------
#pragma unroll
    for (int u = 0; u < NDT; ++u) {
      if (16 * u + ln < D) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rr = r0 + 4 * kg + i;
          if (rr < r_end)
            store_dt(a.out, b_ * a.os0 + h_ * a.os1 + (int64_t)rr * a.os2 + 16 * u + ln,
                     kRound ? round_bfloat(round_dt(acc[u][i], sdt), a.bfloat, kRoundNearest, 1, sdt) : acc[u][i], sdt);
        }
      }
    }
  }
}

}  // namespace mxa
