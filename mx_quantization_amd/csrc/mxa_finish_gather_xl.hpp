// Finishing kernel of the top-k path for rows of 1,025 .. 4,096 keys with 65 <= k <= 256 kept keys, float16 /
// bfloat16 tensors or scores (mxa_attention_nth_dt: PixArt-Sigma at 1024 x 1024 in 16 bits, self_k = 154).
//
// finish16_xl_kernel (mxa_finish16_xl.hpp) computes only the kept keys' scores, but holds a row's slots in
// registers -- v[KS], ix[KS], on[KS], four lanes per row -- and ends at k = 64 (k = 256 would be 64 slots per
// lane); the masked finish_qk_xl_kernel finishes 3 x T scores per row to use k of them, each with the run-time
// rounding chain of the 16-bit dtypes.  Here the slots live in LDS: a per-wave SLOT TABLE of 16 rows x 256 words
// beside finish16_xl_kernel's chunk area (the P code tile [16][kXlVst], sP [32][16], bm [16][32]).
// One word per slot: bits 0..14 the key (T <= 4,096), bit 15 set for a slot past k or of a row past the end, bits
// 16..31 a value of the SCORE DTYPE's 16 bits -- first the true score, which true_score<true> / true_score_bias
// have already rounded to that dtype, then (from the slot's chunk on) p, which round_dt has.  The score dtype of a
// call that is not float32 throughout is always float16 or bfloat16 (rows2_bind: s_dt = the autocast dtype, else
// the tensors'), so no slot needs more than 16 bits and nothing is rounded that finish16_xl_kernel's XDT form
// does not round.  The row stride is 260 words: slot s of row r lies in bank (4 r + s) mod 64, so the wave's 64
// lanes (row r = lane / 4, phase s mod 4 = lane % 4) touch 64 banks in every access.
// Per tile of 16 query rows (one wave, four lanes per row, slots ph, ph + 4, ...):
//   pass 1   groups of 64 slots per row (16 per lane): the kept indices loaded, then the K rows gathered from the
//            workspace (true_dot<NB>); the words stored, the running maximum kept;
//   pass 2   the sum of exp2f((s - mx) log2 e) over the table, then the quad sum;
//   chunk c  (1,024 keys = 32 MX blocks of P) the slots whose key lies in it: p = round_dt(round_bfloat(
//            div_by_sum(e, sum))) replaces the score in the word and goes into the block maximum (LDS atomicMax);
//            per block scale_exponent_dt, sP and the block word; per slot p_code_word into the code tile; P.V on
//            v_mfma_i32_16x16x32_i8 per 32-key block with the fmaf epilogue, the V^T operands two blocks ahead
//            across chunk borders; the written codes and the block words cleared.
// Per element this is finish16_xl_kernel's XDT arithmetic; what differs is where a slot waits and how many there
// are.  The chunk walk, the lane maps of the MFMA and the output store are that kernel's lines.  No key block is
// skipped (0 x a NaN V scale still reaches the row).  The one __syncthreads stands behind the V-scale staging,
// before any per-wave loop.
#pragma once
#include "mxa_finish16_xl.hpp"

namespace mxa {

constexpr int kGxlSlots = 256;          // slots per row of the table
constexpr int kGxlSst = kGxlSlots + 4;  // its row stride in words
constexpr int kGxlGroup = 16;           // slots per lane of a pass-1 group (64 per row)
constexpr uint32_t kGxlOff = 0x8000u;   // the word of a slot that holds no key

// LDS: finish16_xl_kernel's (the V block scales, then per wave the chunk area), each wave's slot table behind
// its chunk area
struct GxlLds { size_t ve, waves, sp, bm, slots, per_wave, total; };
__host__ __device__ inline GxlLds gxl_lds(int D, int ntb, int waves) {
  const Fin16XlLds F = fin16_xl_lds(D, ntb, 1);
  GxlLds L;
  L.ve = F.ve; L.waves = F.waves; L.sp = F.sp; L.bm = F.bm;
  L.slots = F.per_wave;
  L.per_wave = L.slots + (size_t)kFin16 * kGxlSst * 4;
  L.total = L.waves + (size_t)waves * L.per_wave;
  return L;
}

// the 16 bits of a value already rounded to the score dtype (float16 / bfloat16), and back
__device__ __forceinline__ uint32_t gxl_pack(float x, int sdt) { return (uint32_t)f_to_dt_bits(x, sdt) << 16; }
__device__ __forceinline__ float gxl_value(uint32_t w, int sdt) {
  return sdt == kF16 ? f16_bits_to_f((uint16_t)(w >> 16)) : bf16_bits_to_f((uint16_t)(w >> 16));
}

// NB: 32-blocks per head dim.  Float16 / bfloat16 tensors or scores, MXINT8 P: always the rounding form (a bias,
// the debug true-score output and bfloatX rounding need no instantiation of their own)
template <int NB>
__global__ __launch_bounds__(512) void finish_gather_xl_kernel(Rows2Args a) {
  const int sdt = a.s_dt, idt = a.in_dt;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bh = blockIdx.x;
  const int T = a.T, D = a.D, ntb = a.ntb, k = a.k_top;
  constexpr int nbd = NB;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const GxlLds L = gxl_lds(D, ntb, a.waves);
  float* tvs = reinterpret_cast<float*>(smem + L.ve);
  unsigned char* wb = smem + L.waves + (size_t)wave * L.per_wave;
  int8_t* ptile = reinterpret_cast<int8_t*>(wb);
  float* sP = reinterpret_cast<float*>(wb + L.sp);
  uint32_t* bmw = reinterpret_cast<uint32_t*>(wb + L.bm);  // [16][32]
  const int pr = lane >> 2, ph = lane & 3;  // the lane's tile row and slot phase
  uint32_t* bm = bmw + pr * kXlChunkBlocks;
  uint32_t* slot = reinterpret_cast<uint32_t*>(wb + L.slots) + pr * kGxlSst + ph;  // the lane's slots: slot[4 t]
  int8_t* prow = ptile + pr * kXlVst;
  const int nsl = (k + 3) >> 2;  // slots per lane (k <= kGxlSlots: <= 64)

  const int r_beg = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r_beg + a.rows_per_wg);
  const int ln = lane & 15, kg = lane >> 4;
  const int8_t* vbase = a.vt + (int64_t)bh * D * a.tpad + 8 * kg;
  constexpr int NDT = 2 * NB;  // 16-column tiles of D <= 32 NB
  int64_t bv[NDT], bw[NDT];  // V^T operands of key blocks b, b + 1 (in flight ahead of use)
  auto load_v = [&](int b, int64_t* dst) {
#pragma unroll
    for (int u = 0; u < NDT; ++u)
      if (16 * u < D) dst[u] = *reinterpret_cast<const int64_t*>(vbase + ((int64_t)b * D + min(16 * u + ln, D - 1)) * 32);
  };

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
    const int64_t brow = a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)(valid ? r : r0) * a.bs2 : -1;
    // the first two key blocks' V^T operands, in flight through the scores and softmax (ntb >= 33)
    load_v(0, bv);
    load_v(1, bw);
    uint4 qv[2 * NB];
    int qe[NB];
    load_query_row<NB>(a, grow, qv, qe);
    auto true_of = [&](int j) -> float {  // the true score of key j (+ bias), in the score dtype
      const float acc = true_dot<NB>(qv, qe, a.kc + (kb + j) * a.dpad, a.ksT + (kb + j) * nbd);
      const float t = true_score<true>(acc, a.scale, a.bfloat, sdt);
      return brow >= 0 ? true_score_bias(t, a.bias, brow + (int64_t)j * a.bs3, idt, sdt) : t;
    };
    if (a.true_out && valid)  // debug output: every key's true score
      for (int j = ph; j < T; j += 4) a.true_out[grow * T + j] = true_of(j);

    // ---- pass 1: the kept keys' scores into the table, 16 slots per lane at a time -------------
    float mx = -INFINITY;
    for (int t0 = 0; t0 < nsl; t0 += kGxlGroup) {
      int ix[kGxlGroup];
#pragma unroll
      for (int t = 0; t < kGxlGroup; ++t) {
        const int s = ph + 4 * (t0 + t);
        ix[t] = valid && s < k ? kept_get(a, grow * k + s) : -1;
      }
#pragma unroll
      for (int t = 0; t < kGxlGroup; ++t) {
        if (t0 + t < nsl) {  // (uniform over the wave)
          const float s = true_of(max(ix[t], 0));  // (an empty slot scores key 0, as finish16_xl_kernel's do)
          slot[4 * (t0 + t)] = ix[t] >= 0 ? (uint32_t)ix[t] | gxl_pack(s, sdt) : kGxlOff;
          mx = fmaxf(mx, ix[t] >= 0 ? s : -INFINITY);
        }
      }
    }
    mx = fin16_qmax(mx);
    // ---- pass 2: the sum, per lane in ascending slot order, then over the row's four lanes -----
    auto exp_of = [&](uint32_t w) { return __builtin_amdgcn_exp2f((gxl_value(w, sdt) - mx) * 1.4426950408889634f); };
    float sum = 0.0f;
    for (int t = 0; t < nsl; ++t) {
      const uint32_t w = slot[4 * t];
      sum += w & kGxlOff ? 0.0f : exp_of(w);
    }
    sum = fin16_qsum(sum);
    const float rs = 1.0f / sum;

    float acc[NDT][4];
#pragma unroll
    for (int u = 0; u < NDT; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f;

    // ---- per chunk of 32 key blocks: MX(P) into the chunk's tile, then P.V ---------------------
    for (int cb = 0; cb < ntb; cb += kXlChunkBlocks) {
      const int nbc = min(kXlChunkBlocks, ntb - cb);
      // a slot of this chunk: its block's number in the chunk, else -1 (the block of an empty slot reads as 1,024)
      auto block_in = [&](uint32_t w) {
        const int bl = (int)((w & 0xFFFFu) >> 5) - cb;
        return bl >= 0 && bl < kXlChunkBlocks ? bl : -1;
      };
      // p of the chunk's slots (it replaces the score in the word) and their block maxima
      for (int t = 0; t < nsl; ++t) {
        const uint32_t w = slot[4 * t];
        const int bl = block_in(w);
        if (bl >= 0) {
          const float p = round_dt(round_bfloat(div_by_sum(exp_of(w), sum, rs), a.bfloat, kRoundNearest, 1, sdt), sdt);
          slot[4 * t] = (w & 0xFFFFu) | gxl_pack(p, sdt);
          atomicMax(&bm[bl], __float_as_uint(p) & 0x7FFFFFFFu);
        }
      }
      wave_lds_sync();
      // per block: the scale sP (NaN for a NaN block) and the block word of p_code_word, finish16_kernel's XDT rule
      for (int bk = ph; bk < kXlChunkBlocks; bk += 4) {
        int e_raw;
        const int es = scale_exponent_dt(bm[bk], 127, sdt, &e_raw);
        const bool fl = a.flush_p && !(e_raw != kExpNaN && e_raw > -127);
        sP[bk * kFin16 + pr] = scale_f(es == kExpNaN ? kExpNaN : es - kPUnit<false>);
        bm[bk] = (es == kExpNaN ? 0u : (uint32_t)(es + 1024)) | (fl ? 0x10000u : 0u);
      }
      wave_lds_sync();
      for (int t = 0; t < nsl; ++t) {
        const uint32_t w = slot[4 * t];
        const int bl = block_in(w);
        if (bl >= 0) prow[w & (kXlChunk - 1)] = (int8_t)p_code_word(gxl_value(w, sdt), bm[bl], sdt);
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
      for (int t = 0; t < nsl; ++t) {
        const uint32_t w = slot[4 * t];
        if (block_in(w) >= 0) prow[w & (kXlChunk - 1)] = 0;
      }
      for (int bk = ph; bk < kXlChunkBlocks; bk += 4) bm[bk] = 0u;
      wave_lds_sync();
    }

    // ---- output rows (64-B segments per row) -------------------------------------------------
#pragma unroll
    for (int u = 0; u < NDT; ++u) {
      if (16 * u + ln < D) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rr = r0 + 4 * kg + i;
          if (rr < r_end)
            store_dt(a.out, b_ * a.os0 + h_ * a.os1 + (int64_t)rr * a.os2 + 16 * u + ln,
                     round_bfloat(round_dt(acc[u][i], sdt), a.bfloat, kRoundNearest, 1, sdt), sdt);
        }
      }
    }
  }
}

}  // namespace mxa
