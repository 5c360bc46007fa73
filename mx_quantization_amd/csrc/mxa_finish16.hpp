// Finishing kernel of the top-k path for small k (k <= 64: DeiT's 20 / 30, PixArt's 20),
// 16-ROW TILES: for every query row and its k kept keys (the selection kernel's indices) the
// true scores, softmax, MX(P) along keys and P.V, with P.V on v_mfma_i32_16x16x32_i8.
//
// Per workgroup (one head, or a chunk of its query rows): the head's K codes + exponents and
// the V block scales (as floats) staged in LDS once.  Per wave, tiles of 16 query rows, four
// lanes per row, lane slots ph, ph + 4, ... (KS of them: k <= 4 KS):
//   1. the kept key's true score fl32(exact sum) * scale (+ bias) by v_dot4 over the LDS codes
//      (exact block epilogue); softmax over the kept scores (quad DPP); P
//      MX-quantized along keys: block maxima by LDS atomic max, the block's code multiplier
//      2^-es, the codes into the tile's dense code rows (zero elsewhere);
//   2. P.V for the tile, key block outer: per 32-key MX block the P operand and row scales
//      once, then per 16 output columns ONE v_mfma_i32_16x16x32_i8 (K = 32 = one block: each
//      block keeps its exact int32 sum), epilogue acc += C * (sP[row][b] * sV[b][d]) in fp32
//      (P.V is a tolerance-only product); the V^T operands (token-block-major
//      codes: one contiguous 512-B run per MFMA) straight from HBM / L2, two blocks ahead
//      of their MFMAs (the first two issued at the tile's start, in flight through step 1);
//      the next tile's kept indices loaded during this tile's P.V;
//   3. the tile's output rows go out; the written code positions are cleared.
// Every slot runs the same instructions (an unused slot -- k < 4 KS, or a row past the end --
// scores key 0 and writes its code to a pad column), so the per-slot work has no branches.
// exp / divide: the softmax on v_exp_f32 (2^((v - mx) log2 e)) and a corrected reciprocal
// (P is a tolerance-only operand, as in mxa_finish_qk.hpp).
// (The proj Linear's MX input codes, XO: here for k <= 32; for larger k they stay on the
// 32-row kernel, whose 32 x 32 output blocks are whole MX blocks of the rows.)
// Reference: microxscaling/mx/matmul.py:68-76 (MX P.V), callers
// workloads/deit/scripts/main.py:124-152, workloads/DiT/models.py:195-225,
// workloads/PixArt/models/MX_transformer_block.py:679-717, :826-859.
#pragma once
#include "mxa_finish.hpp"

namespace mxa {

constexpr int kFin16 = 16;  // query rows per MFMA tile (one wave)
constexpr int kFin16Occ = 4;  // waves per SIMD the register allocation aims at
constexpr int kFin16LongKS = 64;  // finish16_kernel's KSL of a LONG instantiation: KS + this
constexpr int kFin16Bits4KS = 128;  // ... and of an MXINT4-P instantiation: + this
// Measured (DeiT-base, same box): the V^T codes staged in LDS per workgroup instead of read
// from L2: 0.172 vs 0.166 ms (3 workgroups per CU instead of 4; PixArt 0.019 vs 0.021); the
// next tile's query codes loaded one tile ahead: 0.193 ms (registers).  Phase timing (tools
// builds): without the V^T loads 0.125 ms, without the score gathers 0.138, neither 0.104.

typedef int v4i16_ __attribute__((ext_vector_type(4)));

// LDS: tables (K codes, K exponents, V block scales as floats [ntb][D]), then per wave the P
// code tile [16][vst] (columns >= tpad: the unused slots' pad), the P block scales sP
// [ntb][16] (float), the block maxima / code multipliers bm [16][ntb] (u32)
struct Fin16Lds {
  size_t kc, ke, vt, ve, waves, per_wave, sp, bm, total;
};
// xo: the per-wave area also holds the 16 x (D + 1) fp32 output tile being MX-quantized for
// the proj Linear (over the code tile, sP and bm, which are rewritten afterwards)
// long_k: rows of more than 512 keys -- no K tables (the kept keys' rows are read from the
// workspace), so the size does not grow with T D
__host__ __device__ inline Fin16Lds fin16_lds(int T, int D, int kst, int nbd, int vst, int ntb, int waves,
                                              bool xo = false, bool long_k = false) {
  Fin16Lds L;
  size_t o = 0;
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  L.kc = o;
  if (!long_k) o += al((size_t)T * kst);
  L.ke = o;
  if (!long_k) o += al((size_t)T * nbd * 2);
  L.ve = o;
  o += al((size_t)ntb * D * 4);
  L.vt = o;
  L.waves = o;
  L.sp = al((size_t)kFin16 * vst);
  L.bm = L.sp + al((size_t)ntb * kFin16 * 4);
  L.per_wave = L.bm + al((size_t)kFin16 * ntb * 4);
  if (xo && L.per_wave < al((size_t)kFin16 * (D + 1) * 4)) L.per_wave = al((size_t)kFin16 * (D + 1) * 4);
  L.total = o + (size_t)waves * L.per_wave;
  return L;
}

// NB: 32-blocks per head dim; KS: kept slots per lane (k <= 4 KS); XDT: float16 / bfloat16
// inputs or scores (the dtype roundings at run time); EXTRA: a bias, the debug true-score
// output or bfloatX rounding (else the scores and P are plain float32); XO: the output rows
// go to the proj Linear as MX codes along C (Rows2Args::xo_codes; float32, D % 32 == 0):
// the tile's 16 x D block is transposed through LDS and every 32-column block of every row
// quantized by rows_prep's per-block body (two lanes per block, all 64 lanes for D = 64);
// LONG: rows of 513 .. 1,024 keys -- the head's K table is not staged: a kept key's codes and
// exponents are read where rows_prep left them (k of T rows per query row, L2-resident)
// (LONG travels in the slot count, KSL = KS + kFin16LongKS: the short rows' instantiations keep
// the names and the code they had -- a kernel of its own around a shared body changed the
// register allocation of 49 of them, and the committed profiles name them)
// W4: P is MXINT4 (mxa_attention_bits at width 4: codes floor(p 2^(2 - es) + 1/2) <= 7, block
// scale 2^(es - 2); the int8 MFMA and its epilogue as they are) -- it travels in the slot count
// too, KSL = KS (+ kFin16LongKS) + kFin16Bits4KS; float32, no proj codes
// LONG with XO (the fused blocks of mxa_attention_proj_full, MXINT8 P): the XO epilogue works on the tile's
// 16 x D output wherever the K rows came from; the per-wave area of a LONG call (16 x (tpad + 16) code
// bytes alone, >= 8,960 B at T = 513) holds the 16 x (D + 1) fp32 tile (8,256 B at D = 128)
template <int NB, int KSL, bool XDT, bool EXTRA, bool XO = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(NB <= 2 && KSL % kFin16LongKS <= 12 ? kFin16Occ : (NB * (KSL % kFin16LongKS) <= 64 ? 3 : 2), 8))) void finish16_kernel(Rows2Args a) {
  constexpr int KS = KSL % kFin16LongKS;
  constexpr bool LONG = KSL % kFin16Bits4KS >= kFin16LongKS;
  constexpr bool W4 = KSL >= kFin16Bits4KS;
  static_assert(!((LONG || W4) && XDT) && !(W4 && XO), "long rows, MXINT4 P: float32; MXINT4 P: no proj codes");
  constexpr bool kRound = XDT || EXTRA;
  const int sdt = XDT ? a.s_dt : (int)kF32, idt = XDT ? a.in_dt : (int)kF32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int bh = blockIdx.x;
  const int T = a.T, D = a.D, kst = a.kst, vst = a.vst, ntb = a.ntb, k = a.k_top;
  constexpr int nbd = NB;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const Fin16Lds L = fin16_lds(T, D, kst, nbd, vst, ntb, a.waves, XO, LONG);
  int8_t* tkc = reinterpret_cast<int8_t*>(smem + L.kc);
  int16_t* tke = reinterpret_cast<int16_t*>(smem + L.ke);
  float* tvs = reinterpret_cast<float*>(smem + L.ve);
  unsigned char* wb = smem + L.waves + (size_t)wave * L.per_wave;
  int8_t* ptile = reinterpret_cast<int8_t*>(wb);
  float* sP = reinterpret_cast<float*>(wb + L.sp);
  uint32_t* bmw = reinterpret_cast<uint32_t*>(wb + L.bm);  // [16][ntb]
  const int pr = lane >> 2, ph = lane & 3;  // the lane's tile row and slot phase

  const int r_beg = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r_beg + a.rows_per_wg);
  uint32_t* bm = bmw + pr * ntb;
  const int pad = a.tpad + ph;  // an unused slot's code column (never read by the MFMA)
  const int ln = lane & 15, kg = lane >> 4;
  const int8_t* vbase = a.vt + (int64_t)bh * D * a.tpad + 8 * kg;
  constexpr int NDT = 2 * NB;  // 16-column tiles of D <= 32 NB
  int64_t bv[NDT], bw[NDT];  // V^T operands of key blocks b, b + 1 (in flight ahead of use)
  auto load_v = [&](int b, int64_t* dst) {
#pragma unroll
    for (int u = 0; u < NDT; ++u)
      if (16 * u < D) dst[u] = *reinterpret_cast<const int64_t*>(vbase + ((int64_t)b * D + min(16 * u + ln, D - 1)) * 32);
  };
  // the next tile's kept indices, loaded while the current tile finishes (the query codes are
  // loaded at the tile's start: one tile ahead they cost more registers than they save)
  int ixn[KS];
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

  // ---- stage the head's K table and V block scales; clear the code tile ---------------
  const int64_t kb = (int64_t)bh * T;
  {
    if constexpr (!LONG) stage_k_table<NB>(a, kb, tkc, tke);
    const int16_t* vssrc = a.vs + (int64_t)bh * ntb * D;
    for (int i = threadIdx.x; i < ntb * D; i += blockDim.x) tvs[i] = scale_f(exp_from16(vssrc[i]));
    for (int i = lane; i < kFin16 * vst / 16; i += 64) reinterpret_cast<uint4*>(ptile)[i] = make_uint4(0, 0, 0, 0);
    for (int i = lane; i < kFin16 * ntb; i += 64) bmw[i] = 0u;
  }
  __syncthreads();

  for (int r0 = r_beg + kFin16 * wave; r0 < r_end; r0 += kFin16 * a.waves) {
    const int r = r0 + pr;
    const bool valid = r < r_end;
    const int64_t grow = (int64_t)bh * a.N + (valid ? r : r0);
    const int64_t brow = EXTRA && a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)(valid ? r : r0) * a.bs2 : -1;
    // the first two key blocks' V^T operands, in flight through the scores and softmax
    load_v(0, bv);
    if (ntb > 1) load_v(1, bw);
    // the row's query codes / exponents and its kept indices
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
      const float acc = LONG ? true_dot<NB>(qv, qe, a.kc + (kb + j) * a.dpad, a.ksT + (kb + j) * nbd)
                             : true_dot<NB>(qv, qe, tkc + (size_t)j * kst, tke + j * nbd);
      const float t = true_score<kRound>(acc, a.scale, a.bfloat, sdt);
      return kRound && brow >= 0 ? true_score_bias(t, a.bias, brow + (int64_t)j * a.bs3, idt, sdt) : t;
    };
    if (EXTRA && a.true_out && valid)  // debug output: every key's true score
      for (int j = ph; j < T; j += 4) a.true_out[grow * T + j] = true_of(j);

    // ---- 1. kept scores, softmax, MX(P) into the code tile ------------------------------
    float v[KS];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const float s = true_of(ix[t]);
      v[t] = on[t] ? s : -INFINITY;
      mx = fmaxf(mx, v[t]);
    }
    auto qmax = [](float x) {
      uint32_t u = __float_as_uint(x);
      auto op = [](uint32_t p, uint32_t q) { return __float_as_uint(fmaxf(__uint_as_float(p), __uint_as_float(q))); };
      u = op(u, dpp_u32<0xB1>(u));
      return __uint_as_float(op(u, dpp_u32<0x4E>(u)));
    };
    auto qsum = [](float x) {
      uint32_t u = __float_as_uint(x);
      auto op = [](uint32_t p, uint32_t q) { return __float_as_uint(__uint_as_float(p) + __uint_as_float(q)); };
      u = op(u, dpp_u32<0xB1>(u));
      return __uint_as_float(op(u, dpp_u32<0x4E>(u)));
    };
    mx = qmax(mx);
    // exp(v - mx) as 2^((v - mx) log2 e) (the difference first: folding mx log2 e into an
    // fma loses the argument for large scores); an unused slot adds 0 (also where mx = -inf)
    float sum = 0.0f;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      v[t] = on[t] ? __builtin_amdgcn_exp2f((v[t] - mx) * 1.4426950408889634f) : 0.0f;
      sum += v[t];
    }
    sum = qsum(sum);
    const float rs = 1.0f / sum;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      float p = div_by_sum(v[t], sum, rs);
      if (kRound) p = round_dt(round_bfloat(p, a.bfloat, kRoundNearest, 1, sdt), sdt);
      v[t] = p;
      // zeros.scatter_(idx, softmax) -> MXINT8 along keys: the block maxima (an unused slot
      // adds max(., 0) to block 0: no change)
      atomicMax(&bm[ix[t] >> 5], __float_as_uint(p) & 0x7FFFFFFFu);
    }
    wave_lds_sync();
    // per block: the scale sP (NaN for a NaN block) and the code multiplier 2^-es (0 for a NaN
    // or flushed block: its codes 0; XDT: es + 1024 and the flush flag, round_code at run time)
    // (p_block's rule, mxa_finish.hpp, written out: see there)
    for (int bk = ph; bk < ntb; bk += 4) {
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
      const uint32_t e = bm[ix[t] >> 5];
      // (float32: a NaN block's codes do not matter, its sP is NaN)
      const int code = XDT ? p_code_word(v[t], e, sdt) : (int)p_code_bits_f32<W4>(v[t], __uint_as_float(e));
      ptile[pr * vst + (on[t] ? ix[t] : pad)] = (int8_t)code;
    }
    wave_lds_sync();

    // ---- 2. P.V on int8 MFMA, key block outer -----------------------------------------------
    // lane maps (checked on hardware by mxa_selftest_mfma): A[m][k], m = lane % 16,
    // k = 8 (lane / 16) + 0..7; B[k][n], n = lane % 16, the same k; C[m][n] in c[i],
    // m = 4 (lane / 16) + i, n = lane % 16.  A = the P code rows, B = V^T: the head's codes
    // are [ntb][D][32], so the operand of (block b, columns 16 u ..) is one contiguous 512-B run
    float acc[NDT][4];
#pragma unroll
    for (int u = 0; u < NDT; ++u) acc[u][0] = acc[u][1] = acc[u][2] = acc[u][3] = 0.0f;
    if (r0 + kFin16 * a.waves < r_end) load_ix(r0 + kFin16 * a.waves);
    for (int b = 0; b < ntb; ++b) {
      int64_t bn[NDT];
      if (b + 2 < ntb) load_v(b + 2, bn);  // two blocks ahead
      const int64_t av = *reinterpret_cast<const int64_t*>(ptile + ln * vst + 32 * b + 8 * kg);
      const float4 s4 = *reinterpret_cast<const float4*>(sP + b * kFin16 + 4 * kg);
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
    if constexpr (XO) {
      // ---- 3'. the 16 x D block -> MX codes of blocks h NB .. of each output row (what
      // rows_prep makes of the (B, N, C) output for the proj Linear: finish_kernel's XO) ------
      wave_lds_sync();  // every lane's MFMA reads of the code tile are done
      float* ot = reinterpret_cast<float*>(wb);
      const int ost = D + 1;
#pragma unroll
      for (int u = 0; u < NDT; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (16 * u + ln < D) ot[(4 * kg + i) * ost + 16 * u + ln] = round_bfloat(acc[u][i], a.bfloat, kRoundNearest, 1);
      wave_lds_sync();
      const RowsPrepArgs ro = xo_rows_args(a.xo_codes, a.xo_exps, a.H * D, a.H * nbd, a.flush_p, a.bfloat);
      const int row = (lane & 31) >> 1, sub = lane & 1, rr = r0 + row;
      const int64_t orow = (int64_t)b_ * a.N + (rr < r_end ? rr : r0);
#pragma unroll
      for (int bp = 0; bp < NB; bp += 2) {
        const int bl = bp + (lane >> 5), blc = min(bl, NB - 1);
        float xv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) xv[j] = ot[row * ost + 32 * blc + 16 * sub + j];
        xo_block(ro, orow, h_ * nbd + blc, sub, h_ * D + 32 * blc + 16 * sub, xv, rr < r_end && bl < NB);
      }
      wave_lds_sync();
      // the area back to a clear code tile and zero block maxima (sP is rewritten per tile)
      for (int i = lane; i < (int)(L.per_wave / 16); i += 64) reinterpret_cast<uint4*>(wb)[i] = make_uint4(0, 0, 0, 0);
      wave_lds_sync();
      continue;
    }
    // ---- 3. output rows (64-B segments per row); clear the written code positions ---------
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
    wave_lds_sync();  // every lane's MFMA reads of the tile are done
#pragma unroll
    for (int t = 0; t < KS; ++t) ptile[pr * vst + (on[t] ? ix[t] : pad)] = 0;
    for (int bk = ph; bk < ntb; bk += 4) bm[bk] = 0u;
    wave_lds_sync();
  }
}

}  // namespace mxa
