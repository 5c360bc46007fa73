// Finishing kernel of the top-k path for rows of 4,097 .. 16,384 keys (k <= 64): finish16_xl_kernel's
// per-tile scheme (mxa_finish16_xl.hpp) with NO LDS table that grows with T.
//
// finish16_xl_kernel stages every V block scale of the head, [ntb][D] floats: 147,456 B at 16,384 keys and
// D = 72, more than a workgroup can have beside one wave's chunk area.  Here the V block scales are staged
// PER CHUNK of 32 key blocks, [32][D] floats (9,216 B at D = 72), shared by the workgroup's waves and
// double-buffered: while the waves multiply chunk c, the workgroup's threads hold chunk c + 1's raw int16
// exponents in registers (loaded before the chunk's work, converted and written to the other buffer behind
// its P.V), so the loads' latency lies under the MFMA loop.  One __syncthreads per chunk publishes the next
// buffer and retires the current one.  All waves of a workgroup therefore walk the chunks in step: the
// workgroup runs `rounds` rounds of one tile per wave, and a wave whose tile lies past the workgroup's last
// row still stages and meets every barrier (it only skips the tile's own work).
// Reading the scales straight from L2 instead would put a dependent global load per 16-column tile into
// every block's epilogue (the scale multiplies the MFMA's result) on a kernel that runs at 1..2 waves per
// SIMD: nothing hides it.  Staged, the epilogue reads LDS as finish16_xl_kernel's does.
//
// Per tile of 16 query rows (one wave, four lanes per row, slots ph, ph + 4, ...) everything else is
// finish16_xl_kernel's: the kept keys' true scores and the softmax once, the slots (full 32-bit key index,
// p) in registers across the chunks; per chunk the block maxima by LDS atomic max, the block scales, the
// codes into the chunk's tile, P.V on v_mfma_i32_16x16x32_i8 per 32-key block with the per-block fp32
// epilogue, V^T prefetched two blocks ahead across chunk borders, the written positions cleared.  The block
// order and the epilogue are the unchunked kernel's; no key block is skipped (a block no row keeps still
// multiplies its zero codes with V's block scale: a NaN scale poisons that output column, the reference's
// dense 0 * NaN).  float32 tensors and scores; P is MXINT8 or (W4) MXINT4.
#pragma once
#include "mxa_finish16_xl.hpp"

namespace mxa {

constexpr int kXxlStage = 12;  // raw V block exponents a thread holds for the next chunk (the rest: staged behind P.V)

// LDS: the V block scales of two chunks as floats [2][32][D], then per wave finish16_xl_kernel's chunk area
struct Fin16XxlLds { size_t ve, ve_buf, waves, sp, bm, per_wave, total; };
__host__ __device__ inline Fin16XxlLds fin16_xxl_lds(int D, int waves) {
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  Fin16XxlLds L;
  L.ve = 0;
  L.ve_buf = al((size_t)kXlChunkBlocks * D * 4);
  L.waves = 2 * L.ve_buf;
  L.sp = (size_t)kFin16 * kXlVst;
  L.bm = L.sp + (size_t)kXlChunkBlocks * kFin16 * 4;
  L.per_wave = L.bm + (size_t)kFin16 * kXlChunkBlocks * 4;
  L.total = L.waves + (size_t)waves * L.per_wave;
  return L;
}

// NB: 32-blocks per head dim; KS: kept slots per lane (k <= 4 KS); EXTRA: a bias, the debug true-score
// output or bfloatX rounding; W4: MXINT4 P.  (LDS holds the kernel to at most seven waves per CU, so the
// register allocation aims at two waves per SIMD, 256 VGPRs: PixArt's NB = 3, KS = 5 takes 251 and no
// scratch, the widest form -- NB = 4, KS = 16 -- 504 B; the figures per instantiation: DESIGN.md section 4)
template <int NB, int KS, bool EXTRA, bool W4>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 8))) void finish16_xxl_kernel(Rows2Args a) {
  constexpr bool kRound = EXTRA;
  constexpr int sdt = kF32, idt = kF32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bh = blockIdx.x;
  const int T = a.T, D = a.D, ntb = a.ntb, k = a.k_top;
  constexpr int nbd = NB;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const Fin16XxlLds L = fin16_xxl_lds(D, a.waves);
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

  // ---- the V block scales of one chunk (key blocks cb .. cb + 31 of the ntb): [32][D] floats in buffer `to`.
  // stage_load takes a thread's first kXxlStage exponents into registers; stage_store converts and writes
  // them, and stages what is left (few waves, a wide head) in one go
  const int16_t* vssrc = a.vs + (int64_t)bh * ntb * D;
  const int nthr = (int)blockDim.x;
  auto buf = [&](int to) { return reinterpret_cast<float*>(smem + L.ve + (size_t)to * L.ve_buf); };
  auto stage_load = [&](int cb, int16_t* raw) {
    const int cnt = min(kXlChunkBlocks, ntb - cb) * D;
#pragma unroll
    for (int t = 0; t < kXxlStage; ++t) {
      const int i = (int)threadIdx.x + t * nthr;
      raw[t] = i < cnt ? vssrc[(int64_t)cb * D + i] : (int16_t)0;
    }
  };
  auto stage_store = [&](int cb, const int16_t* raw, int to) {
    const int cnt = min(kXlChunkBlocks, ntb - cb) * D;
    float* tv = buf(to);
#pragma unroll
    for (int t = 0; t < kXxlStage; ++t) {
      const int i = (int)threadIdx.x + t * nthr;
      if (i < cnt) tv[i] = scale_f(exp_from16(raw[t]));
    }
    for (int i = (int)threadIdx.x + kXxlStage * nthr; i < cnt; i += nthr) tv[i] = scale_f(exp_from16(vssrc[(int64_t)cb * D + i]));
  };
  {  // the first chunk; clear the code tile and the block maxima
    int16_t raw[kXxlStage];
    stage_load(0, raw);
    for (int i = lane; i < kFin16 * kXlVst / 16; i += 64) reinterpret_cast<uint4*>(ptile)[i] = make_uint4(0, 0, 0, 0);
    for (int i = lane; i < kFin16 * kXlChunkBlocks; i += 64) bmw[i] = 0u;
    stage_store(0, raw, 0);
  }
  __syncthreads();

  const int64_t kb = (int64_t)bh * T;
  const int tiles = (r_end - r_beg + kFin16 - 1) / kFin16, rounds = (tiles + a.waves - 1) / a.waves;
  int cur = 0;  // the buffer that holds the chunk being multiplied
  for (int round = 0; round < rounds; ++round) {
    const int r0 = r_beg + kFin16 * (wave + round * a.waves);
    const bool tile = r0 < r_end;  // (wave-uniform) a wave without a tile only stages and meets the barriers
    const int r = r0 + pr;
    const bool valid = r < r_end;
    const int64_t grow = (int64_t)bh * a.N + (valid ? r : (tile ? r0 : r_beg));
    const int64_t brow = EXTRA && a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)(valid ? r : (tile ? r0 : r_beg)) * a.bs2 : -1;
    int ix[KS];
    bool on[KS];
    float v[KS];
    float acc[NDT][4];
#pragma unroll
    for (int u = 0; u < NDT; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      on[t] = false;
      ix[t] = 0;
      v[t] = 0.0f;
    }
    if (tile) {
      // the first two key blocks' V^T operands, in flight through the scores and softmax (ntb >= 129)
      load_v(0, bv);
      load_v(1, bw);
      uint4 qv[2 * NB];
      int qe[NB];
      load_query_row<NB>(a, grow, qv, qe);
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        on[t] = valid && ph + 4 * t < k;
        ix[t] = ixn[t];
      }
      auto true_of = [&](int j) -> float {  // the true score of key j (+ bias: EXTRA only)
        const float dot = true_dot<NB>(qv, qe, a.kc + (kb + j) * a.dpad, a.ksT + (kb + j) * nbd);
        const float t = true_score<kRound>(dot, a.scale, a.bfloat, sdt);
        return kRound && brow >= 0 ? true_score_bias(t, a.bias, brow + (int64_t)j * a.bs3, idt, sdt) : t;
      };
      if (EXTRA && a.true_out && valid)  // debug output: every key's true score
        for (int j = ph; j < T; j += 4) a.true_out[grow * T + j] = true_of(j);

      // ---- 1. kept scores and softmax: p in v[], once per tile --------------------------------
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
      if (r0 + kFin16 * a.waves < r_end) load_ix(r0 + kFin16 * a.waves);
    }

    // ---- 2. per chunk of 32 key blocks: MX(P) into the chunk's tile, then P.V --------------------
    for (int cb = 0; cb < ntb; cb += kXlChunkBlocks) {
      // the chunk the workgroup multiplies next: this tile's next one, else the next round's first
      const int nxt = cb + kXlChunkBlocks < ntb ? cb + kXlChunkBlocks : (round + 1 < rounds ? 0 : -1);
      int16_t raw[kXxlStage];
      if (nxt >= 0) stage_load(nxt, raw);
      if (tile) {
        const float* tvs = buf(cur);
        const int nbc = min(kXlChunkBlocks, ntb - cb);
        // the block maxima of the chunk's slots (a slot outside it adds max(., 0): no change)
#pragma unroll
        for (int t = 0; t < KS; ++t) {
          const bool in = on[t] && (ix[t] >> 5) - cb >= 0 && (ix[t] >> 5) - cb < kXlChunkBlocks;
          atomicMax(&bm[(ix[t] >> 5) & (kXlChunkBlocks - 1)], in ? __float_as_uint(v[t]) & 0x7FFFFFFFu : 0u);
        }
        wave_lds_sync();
        // per block: the scale sP (NaN for a NaN block) and the code multiplier 2^-es (0 for a NaN or
        // flushed block), finish16_kernel's rule
        for (int bk = ph; bk < kXlChunkBlocks; bk += 4) {
          int e_raw;
          const int es = scale_exponent_dt(bm[bk], 127, sdt, &e_raw);
          const bool fl = a.flush_p && !(e_raw != kExpNaN && e_raw > -127);
          sP[bk * kFin16 + pr] = scale_f(es == kExpNaN ? kExpNaN : es - kPUnit<W4>);
          bm[bk] = __float_as_uint(es == kExpNaN || fl ? 0.0f : pow2f(-es));
        }
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < KS; ++t) {
          const bool in = on[t] && (ix[t] >> 5) - cb >= 0 && (ix[t] >> 5) - cb < kXlChunkBlocks;
          const uint32_t e = bm[(ix[t] >> 5) & (kXlChunkBlocks - 1)];
          // (a slot outside the chunk codes against a block that is not its own: the result goes to the pad)
          const int code = (int)p_code_bits_f32<W4>(v[t], __uint_as_float(e));
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
              const float sv = tvs[(b - cb) * D + min(16 * u + ln, D - 1)];
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
      // the next chunk's scales into the other buffer (its last readers passed the previous barrier);
      // the barrier publishes it and retires this chunk's
      if (nxt >= 0) stage_store(nxt, raw, cur ^ 1);
      __syncthreads();
      cur ^= 1;
    }

    // ---- 3. output rows (64-B segments per row) -----------------------------------------------
    if (tile) {
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
}

}  // namespace mxa
