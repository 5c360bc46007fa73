// Selection kernels: approximate scores + exact-order top-k.
//
// Per workgroup (one head, a chunk of its query rows): the head's score tables are
// staged in LDS once (sel_lds / sel_stage):
//   ex_pred        sign words + block exponents
//   MXINT4 / EXION / partial_*   approximator codes + block scales
//   true_ex        power-of-two codes + zero indicators + block exponents
//   ELSA           hash words + the (D+1)-entry cosine table
//   approx off     MXINT8 codes + exponents (the true scores are ranked)
// then per row (sel_scores): the scores (exact fp64 block epilogue where needed: the
// scores are exact sums of integer * 2^e), bias added in fp32 as the caller
// does; torch's CPU topk index order; the k kept indices (the op's int64 idx, which the
// finishing kernel reads too, or a 16-bit workspace copy: kept_put), and the prune-mask
// words when asked for.
//   select_kernel<..., uint32_t>  rows of <= 256 keys whose scores pack into 32-bit
//                     elements (mxa_topk_grp.hpp GEl), then
//   select_kernel<..., uint64_t>  the rows that do not (fb_only), and every row of the true
//                     scores, ELSA and rows over 256 keys
// k_top == 0: scores only (mxa_approx_scores).
// Callers replaced: the approximator + torch.topk of
//   workloads/deit/scripts/main.py:101-123, workloads/DiT/models.py:168-194,
//   workloads/PixArt/models/MX_transformer_block.py:656-678, :805-825.
#pragma once
#include <type_traits>
#include "mxa_dot.hpp"
#include "mxa_rows2.hpp"
#include "mxa_topk_grp.hpp"
#include "mxa_tail.hpp"
#include "mxa_topk_wave.hpp"

namespace mxa {

constexpr int kSelRows = 32;   // query rows per workgroup (a multiple of 4 * waves)
// packed-pass workgroup flags per 64-bit-pass workgroup: few, so that a call whose rows mostly
// do not pack still spreads the 64-bit pass over the chip (64 per workgroup ran arbitrary float32
// rows through ops.topk at half the rate of the 64-bit pass alone: 1.60 vs 0.80 ms, round 6)
constexpr int kFbItems = 4;
// waves per SIMD the 64-bit pass is compiled for (rows <= 256 keys; 6 / 8 measured slower at
// PixArt's rows: spills, profiles/r06_ab_tail.txt)
constexpr int kSelOcc = 4;
// ... and the packed pass, with the tail (DeiT: 6 measured slower, spills) and without it
// (k > 33, DiT: 4 removes its spills and measured slower) -- profiles/r06_ab_tail.txt
constexpr int kSelPOcc = 5;
constexpr int kSelPOccNT = 5;
constexpr int kSelShortT = 224;
// waves per workgroup: 2 for rows of <= 224 keys on a large grid (DeiT-base: 0.97 ->
// 0.93 ms), else 4 (DiT: 1.44 vs 1.56 ms with 2; PixArt's 128 heads: 0.069 vs 0.10 ms)
// -- measured, tools/bench_cmp.sh
inline int sel_waves_for(int T, int64_t BH, int N) {
  return T <= kSelShortT && BH * ((N + kSelRows - 1) / kSelRows) >= 8192 ? 2 : 4;
}

// LDS layout of the score tables (then the per-row top-k areas)
struct SelLds {
  size_t cd, ex, sg, z, cs, kf, rows;
};
// ex_pred for nbd <= 2: one record per key over the ex and sg areas (the same bytes: 8 nbd per
// key), which the key loop reads with one LDS load -- the key's nbd sign words, then per block
// the float bits of 2^ek, (ek + 127) << 23, or for a block exponent outside [kExpFastLo,
// kExpFastHi] (or NaN) a NaN that carries it (expred_rec_word); with 16 flag words kf: bit i of
// kf[g] = key g + 16 i has such a block, i.e. its score needs the exact slow path (sel_scores,
// expred_score_rec).  For nbd >= 3 int16 exponents and sign words in two tables,
// which keeps DiT's workgroups per CU.
constexpr int kExpFastLo = -50, kExpFastHi = 61;
__host__ __device__ inline SelLds sel_lds(int mode, int T, int D, int kst, int nbd) {
  SelLds L;
  size_t o = 0;
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  const bool codes = mode == kModeTrue || mode == kModeOpExp || mode == kModeOpMul || mode == kModeTrueEx;
  L.cd = o;
  if (codes) o += al((size_t)T * kst);
  L.ex = o;
  if (mode != kModeElsa) o += al((size_t)T * nbd * (mode == kModeExSign && nbd <= 2 ? 4 : 2));
  L.sg = o;
  if (mode == kModeExSign || mode == kModeElsa) o += al((size_t)T * nbd * 4);
  L.z = o;
  if (mode == kModeTrueEx) o += al((size_t)T * kst);
  L.cs = o;
  if (mode == kModeElsa) o += al((size_t)(D + 1) * 4);
  L.kf = o;
  if (mode == kModeExSign) o += 16 * 4;
  L.rows = o;
  return L;
}

// ex_pred score of one key: sum_b m_b 2^(eq_b + ek_b), m_b = n_b - 2 popc(sq_b ^ sk_b)
// (|m_b| <= 32).  When the block exponents span <= 23 bits and the smallest is >= -100,
// the sum shifted to the smallest exponent is an exact int32, so one conversion (round
// to nearest even) and an exact scaling give the correctly rounded float; otherwise
// (and for NaN blocks) the exact fp64 sum.  Both equal fl32 of the exact sum.
template <int NBD, typename KE>
__device__ __forceinline__ float expred_score(const uint32_t* sq, const int* eq, const KE* kex, const uint32_t* ksg,
                                              int D) {
  int m[NBD], e[NBD];
  bool nan = false;
  int emin = 1 << 20, emax = -(1 << 20);
#pragma unroll
  for (int b = 0; b < NBD; ++b) {
    const int ek = exp_from16((int16_t)kex[b]);
    nan = nan || ek == kExpNaN || eq[b] == kExpNaN;
    e[b] = eq[b] + ek;
    m[b] = min(32, D - 32 * b) - 2 * (int)__popc(sq[b] ^ ksg[b]);
    emin = min(emin, e[b]);
    emax = max(emax, e[b]);
  }
  if (nan) return __uint_as_float(0x7FC00000u);
  if (emax - emin <= 23 && emin >= -100) {
    int sum = 0;
#pragma unroll
    for (int b = 0; b < NBD; ++b) sum += m[b] << (e[b] - emin);
    return ldexpf((float)sum, emin);
  }
  double acc = 0.0;
#pragma unroll
  for (int b = 0; b < NBD; ++b) acc += (double)m[b] * pow2d(e[b]);
  return (float)acc;
}
// The exponent word of a key record (sel_lds: nbd <= 2) for the raw block exponent ek: the float
// bits of 2^ek inside the fast range; outside it a NaN whose payload holds ek in bits 8..22 (15
// bits: ex_pred's exponents are float exponents, far inside; -16384 stands for the NaN block's
// INT16_MIN) and whose low byte is 0 -- whatever the key loop computes from it is a NaN or an
// infinity with a zero low byte, which leaves the row's packing test alone.
__device__ __forceinline__ uint32_t expred_rec_word(int ek) {
  if (ek >= kExpFastLo && ek <= kExpFastHi) return (uint32_t)(ek + 127) << 23;
  return 0x7F800000u | (((uint32_t)(ek == kExpNaN16 ? -16384 : ek) & 0x7FFFu) << 8);
}
__device__ __forceinline__ int16_t expred_rec_exp(uint32_t w) {
  if (w < 0x7F800000u) return (int16_t)((int)(w >> 23) - 127);
  const int s = (int)(w << 9) >> 17;  // bits 8..22, sign-extended
  return s == -16384 ? kExpNaN16 : (int16_t)s;
}
// ... of the key whose record is rec
template <int NBD>
__device__ __forceinline__ float expred_score_rec(const uint32_t* sq, const int* eq, const uint32_t* rec, int D) {
  int16_t ke[NBD];
#pragma unroll
  for (int b = 0; b < NBD; ++b) ke[b] = expred_rec_exp(rec[NBD + b]);
  return expred_score<NBD>(sq, eq, ke, rec, D);
}

// MX dot product of a query row (codes in registers, two uint4 per 32-block, block
// exponents qe) with key row krow of the LDS code table: exact block sums by v_dot4,
// block scale 2^(qe+ke) (MUL = 0) or qe*ke/4096 (EXION, MUL = 1), fp64 accumulation
template <int MUL, int NBMAX = kMaxNB>
__device__ __forceinline__ double g_dot(const uint4* qv, const int* qe, int nbd, const int8_t* krow,
                                        const int16_t* kexp, bool& nan) {
  double acc = 0.0;
#pragma unroll
  for (int b = 0; b < NBMAX; ++b) {
    if (b < nbd) {
      const uint4 x0 = *reinterpret_cast<const uint4*>(krow + 32 * b);
      const uint4 x1 = *reinterpret_cast<const uint4*>(krow + 32 * b + 16);
      const int I = dot32(qv[2 * b], qv[2 * b + 1], x0, x1);
      const int e = exp_from16(kexp[b]);
      if (e == kExpNaN || qe[b] == kExpNaN) nan = true;
      else if (MUL) acc += (double)I * (double)(qe[b] * e) * (1.0 / 4096.0);
      else acc += (double)I * pow2d(qe[b] + e);
    }
  }
  return acc;
}

// true_ex: a = c * 2^e + z per element (c the power-of-two code, 0 for a zero MX
// element; z = 1 for a zero element), so per block
//   sum aQ aK = 2^(eq+ek) <cq,ck> + 2^eq <cq,zk> + 2^ek <zq,ck> + <zq,zk>   (exact in fp64)
__device__ __forceinline__ double g_dot_trueex(const uint4* qv, const uint4* qz, const int* qe, int nbd,
                                               const int8_t* krow, const int8_t* kzrow, const int16_t* kexp,
                                               bool& nan) {
  double acc = 0.0;
#pragma unroll
  for (int b = 0; b < kMaxNB; ++b) {
    if (b < nbd) {
      const uint4 k0 = *reinterpret_cast<const uint4*>(krow + 32 * b);
      const uint4 k1 = *reinterpret_cast<const uint4*>(krow + 32 * b + 16);
      const uint4 z0 = *reinterpret_cast<const uint4*>(kzrow + 32 * b);
      const uint4 z1 = *reinterpret_cast<const uint4*>(kzrow + 32 * b + 16);
      const int I1 = dot32(qv[2 * b], qv[2 * b + 1], k0, k1);
      const int I2 = dot32(qv[2 * b], qv[2 * b + 1], z0, z1);
      const int I3 = dot32(qz[2 * b], qz[2 * b + 1], k0, k1);
      const int I4 = dot32(qz[2 * b], qz[2 * b + 1], z0, z1);
      const int e = exp_from16(kexp[b]);
      if (e == kExpNaN || qe[b] == kExpNaN) {
        nan = true;
      } else {
        acc += (double)I1 * pow2d(qe[b] + e);
        acc += (double)I2 * pow2d(qe[b]);
        acc += (double)I3 * pow2d(e);
        acc += (double)I4;
      }
    }
  }
  return acc;
}

// ELSA cosine table entry h: cos(clamp(fl32(fl32(pi/D) * h) - 0.127f, 0)) correctly
// rounded (funcs/elsa_approximation.py:138-143; the caller may pass torch's values)
__device__ __forceinline__ float elsa_cos_entry(int D, int h) {
  const float est = (float)(3.141592653589793 / (double)D) * (float)h;
  const float cor = fmaxf(est - 0.127f, 0.0f);
  return (float)cos((double)cor);
}

// ---- the head's score tables in LDS (sel_lds) -------------------------------------
struct SelTabs {
  int8_t* tcd;    // key codes
  int16_t* tex;   // key exponents
  uint32_t* trec; // ex_pred, nbd <= 2: the key records (SelLds), in place of tex and tsg
  uint32_t* kf;   // ... and the keys outside the fast path's exponent range
  uint32_t* tsg;  // sign / hash words
  int8_t* tz;     // true_ex zero indicators
  float* tcs;     // ELSA cosine table
};
template <int MODE>
__device__ __forceinline__ SelTabs sel_stage(const Rows2Args& a, unsigned char* smem, const SelLds& L, int bh) {
  constexpr bool kOp = MODE == kModeOpExp || MODE == kModeOpMul;
  SelTabs t;
  t.tcd = reinterpret_cast<int8_t*>(smem + L.cd);
  t.tex = reinterpret_cast<int16_t*>(smem + L.ex);
  t.tsg = reinterpret_cast<uint32_t*>(smem + L.sg);
  t.tz = reinterpret_cast<int8_t*>(smem + L.z);
  t.tcs = reinterpret_cast<float*>(smem + L.cs);
  t.trec = reinterpret_cast<uint32_t*>(__builtin_assume_aligned(smem + L.ex, 16));
  t.kf = reinterpret_cast<uint32_t*>(smem + L.kf);
  const int T = a.T, D = a.D, nbd = a.nbd, kst = a.kst;
  if (MODE == kModeExSign && nbd <= 2) {  // (the range flags serve the nbd <= 2 key loop)
    if (threadIdx.x < 16) t.kf[threadIdx.x] = 0u;
    __syncthreads();
  }
  const int64_t kb = (int64_t)bh * T;
  if constexpr (MODE == kModeTrue || kOp || MODE == kModeTrueEx) {
    const int8_t* src = MODE == kModeTrue ? a.kc : a.kop;
    const int cpr = a.dpad / 16;
    for (int i = threadIdx.x; i < T * cpr; i += blockDim.x) {
      const int j = i / cpr, c = i - j * cpr;
      *reinterpret_cast<uint4*>(t.tcd + (size_t)j * kst + 16 * c) =
          *reinterpret_cast<const uint4*>(src + (kb + j) * a.dpad + 16 * c);
      if (MODE == kModeTrueEx)
        *reinterpret_cast<uint4*>(t.tz + (size_t)j * kst + 16 * c) =
            *reinterpret_cast<const uint4*>(a.kz + (kb + j) * a.dpad + 16 * c);
    }
  }
  {
    const int16_t* esrc = MODE == kModeTrue ? a.ksT : a.ksA;
    for (int i = threadIdx.x; i < T * nbd; i += blockDim.x) {
      if (MODE == kModeExSign && nbd <= 2) {
        const int ek = esrc[kb * nbd + i];  // raw (NaN: INT16_MIN, outside the range)
        const int j = nbd == 2 ? i >> 1 : i, b = i - j * nbd;  // (no division: nbd is 1 or 2)
        t.trec[2 * nbd * j + b] = a.ksg[kb * nbd + i];
        t.trec[2 * nbd * j + nbd + b] = expred_rec_word(ek);
        if (ek < kExpFastLo || ek > kExpFastHi) atomicOr(t.kf + (j & 15), 1u << (j >> 4));
        continue;
      }
      if (MODE != kModeElsa) t.tex[i] = esrc[kb * nbd + i];
      if (MODE == kModeExSign || MODE == kModeElsa) t.tsg[i] = a.ksg[kb * nbd + i];
    }
    if (MODE == kModeElsa)
      for (int h = threadIdx.x; h <= D; h += blockDim.x) t.tcs[h] = a.elsa_cos ? a.elsa_cos[h] : elsa_cos_entry(D, h);
  }
  __syncthreads();
  return t;
}

// ---- the approximate (or true) scores of query row r: keys j0, j0 + js, ... -------------
// sink(j, v, key, fast): v the score as the caller ranks it (score dtype, + bias), key its order
// key, fast (std::true_type) when v came from the fast ex_pred loop (finite, never -0)
// pred_out / true_out are written here.
template <int MODE, typename Sink>
__device__ __forceinline__ void sel_scores(const Rows2Args& a, const SelTabs& t, int bh, int r, int j0, int js,
                                           Sink&& sink) {
  const int T = a.T, D = a.D, nbd = a.nbd, kst = a.kst;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const int64_t kb = (int64_t)bh * T;
  const int64_t grow = (int64_t)bh * a.N + r;
  const int64_t brow = a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)r * a.bs2 : -1;
  // scores in the score dtype: the approximator GEMM's (or the true matmul's) output
  // rounded to it, then + bias (MX_transformer_block.py:821-822): `true_scores += bias` in place,
  // rounded again to the score dtype; `pred = pred + bias` out of place, which torch promotes to
  // float32 for a float32 bias (a 16-bit autocast pred: no second rounding, the ranking is of
  // float32 values; a float32 score dtype rounds to itself either way)
  const int sum_dt = MODE != kModeTrue && a.in_dt == kF32 ? (int)kF32 : a.s_dt;
  auto emit = [&](int j, float v) {
    v = round_dt(v, a.s_dt);
    if (brow >= 0) v = round_dt(v + load_dt(a.bias, brow + (int64_t)j * a.bs3, a.in_dt), sum_dt);
    if (MODE == kModeTrue) {
      if (a.true_out) a.true_out[grow * T + j] = v;
    } else if (a.pred_out) {
      a.pred_out[grow * T + j] = v;
    }
    sink(j, v, order_key(v), std::false_type{});
  };
  if constexpr (MODE == kModeExSign) {
    // pred = sum_b 2^(eq_b + ek_b) (n_b - 2 popc(sq_b ^ sk_b))   (exact)
    uint32_t sq[kMaxNB];
    int eq[kMaxNB];
#pragma unroll
    for (int b = 0; b < kMaxNB; ++b) {
      sq[b] = b < nbd ? a.qsg[grow * nbd + b] : 0u;
      eq[b] = b < nbd ? exp_from16(a.qsA[grow * nbd + b]) : 0;
    }
    auto keys = [&](auto nbd_c) {  // the key loop for a compile-time block count
      constexpr int NBD = decltype(nbd_c)::value;
      // (an odd D: the fast loop below halves the block lengths)
      if (brow >= 0 || a.s_dt != kF32 || js != 16 || (NBD <= 2 && (D & 1))) {
        if constexpr (NBD <= 2)
          for (int j = j0; j < T; j += js)
            emit(j, expred_score_rec<NBD>(sq, eq, t.trec + 2 * NBD * j, D));
        else
          for (int j = j0; j < T; j += js) emit(j, expred_score<NBD>(sq, eq, t.tex + j * NBD, t.tsg + j * NBD, D));
        return;
      }
      if constexpr (NBD >= 3) {
        // the bias-free key loop on raw int16 exponents (NaN = INT16_MIN drives the smallest
        // exponent below -100): a fast-path value (finite, never -0) takes the
        // three-instruction key.  (The branch-free loop below measured slower at DiT's three
        // blocks: its extra live values spill.)
        int eqr[NBD], nbk[NBD];
#pragma unroll
        for (int b = 0; b < NBD; ++b) {
          eqr[b] = eq[b] == kExpNaN ? (int)kExpNaN16 : eq[b];
          nbk[b] = min(32, D - 32 * b);
        }
        float* prow = a.pred_out ? a.pred_out + grow * T : nullptr;
        for (int j = j0; j < T; j += js) {
          const int16_t* kex = t.tex + j * NBD;
          const uint32_t* ksg = t.tsg + j * NBD;
          int e[NBD], m[NBD];
#pragma unroll
          for (int b = 0; b < NBD; ++b) {
            e[b] = eqr[b] + (int)kex[b];
            m[b] = nbk[b] - 2 * (int)__popc(sq[b] ^ ksg[b]);
          }
          int emin = e[0], emax = e[0];
#pragma unroll
          for (int b = 1; b < NBD; ++b) {
            emin = min(emin, e[b]);
            emax = max(emax, e[b]);
          }
          float v;
          uint32_t key;
          if (emax - emin <= 23 && emin >= -100) {
            int sum = 0;
#pragma unroll
            for (int b = 0; b < NBD; ++b) sum += m[b] << (e[b] - emin);
            v = ldexpf((float)sum, emin);
            key = order_key_fast(v);
          } else {
            v = expred_score<NBD>(sq, eq, kex, ksg, D);
            key = order_key(v);
          }
          if (prow) prow[j] = v;
          sink(j, v, key, std::false_type{});
        }
        return;
      }
      // No bias, float32 scores: every lane runs the same ceil(T / 16) keys (the last trip
      // peeled: keys >= T are dropped), with no branch in the loop.  When every block
      // exponent of the row and of the key lies in [kExpFastLo, kExpFastHi], the block
      // terms m_b 2^(eq_b + ek_b) are exact floats (|m_b| <= 32, 2^-100 <= 2^e <= 2^122), formed
      // as products: with h_b = m_b / 2 = popc(~sq_b ^ sk_b) + n_b / 2 - 32 (one v_bcnt with its
      // accumulate operand; the words' bits from n_b up are equal, so they count 32 - n_b) and
      // t_b = 2^ek_b (the key's record) * 2^(eq_b + 1) (once per row), a normal power of two,
      //   x0 = (float)h0 * t0 (exact),  v = fmaf((float)h1, t1, x0):
      // one rounding of the exact two-term sum = fl32(exact sum), a zero sum +0 (the conversion
      // never yields -0) (NBD <= 2).  Keys outside (range flags kf; their records hold a NaN for
      // 2^ek) are redone afterwards by the exact expred_score, under a wave-uniform branch.  A
      // fast value is finite and never -0, so its order key takes two instructions and its
      // packing test is the low byte of its bits.  pred_out is null in the attention calls: the
      // loop is compiled with and without its store, chosen once per row.
      bool row_fast = true;
      uint32_t sqn[NBD];
      int hc[NBD];
      float q2[NBD];
#pragma unroll
      for (int b = 0; b < NBD; ++b) {
        row_fast = row_fast && eq[b] >= kExpFastLo && eq[b] <= kExpFastHi;  // (NaN: kExpNaN)
        sqn[b] = ~sq[b];
        hc[b] = min(32, D - 32 * b) / 2 - 32;
      }
#pragma unroll
      for (int b = 0; b < NBD; ++b) q2[b] = row_fast ? __uint_as_float((uint32_t)(eq[b] + 128) << 23) : 0.0f;
      const int nt = (T + 15) >> 4;
      uint32_t redo = row_fast ? t.kf[j0 & 15] : lowbits(nt);  // per trip i: key j0 + 16 i
      // (the lane's first key as a value of this row: the loop's addresses are formed here, not
      // once per kernel and kept -- spilled -- across every row group: 28 B of scratch more)
      int jl = j0;
      asm volatile("" : "+v"(jl));
      auto loop = [&](auto pred_c) {
        constexpr bool PRED = decltype(pred_c)::value;
        float* prow = PRED ? a.pred_out + grow * T : nullptr;
        auto one = [&](int i, auto last_c) {
          constexpr bool LAST = decltype(last_c)::value;
          const int j = jl + 16 * i;
          uint32_t w[2 * NBD];
          if constexpr (NBD == 2) {
            const uint4 x = *reinterpret_cast<const uint4*>(t.trec + 4 * j);
            w[0] = x.x, w[1] = x.y, w[2] = x.z, w[3] = x.w;
          } else {
            const uint2 x = *reinterpret_cast<const uint2*>(t.trec + 2 * j);
            w[0] = x.x, w[1] = x.y;
          }
          float v = (float)((int)__popc(sqn[0] ^ w[0]) + hc[0]) * (__uint_as_float(w[NBD]) * q2[0]);
          if constexpr (NBD == 2)
            v = __builtin_fmaf((float)((int)__popc(sqn[1] ^ w[1]) + hc[1]), __uint_as_float(w[3]) * q2[1], v);
          const uint32_t key = order_key_fast(v);
          if (!LAST || j < T) {
            if constexpr (PRED) prow[j] = v;
            sink(j, v, key, std::true_type{});
          }
        };
        // (in pairs: one step of the record and mirror addresses per two keys)
        int i = 0;
#pragma unroll 1
        for (; i + 2 < nt; i += 2) {
          one(i, std::false_type{});
          one(i + 1, std::false_type{});
        }
        if (i + 1 < nt) one(i, std::false_type{});
        one(nt - 1, std::true_type{});
      };
      if (a.pred_out) loop(std::true_type{});
      else loop(std::false_type{});
      if (__builtin_amdgcn_ballot_w64(redo != 0u) != 0) {  // rare: the exact path for those keys
        float* prow = a.pred_out ? a.pred_out + grow * T : nullptr;
        while (redo) {
          const int i = __ffs((int)redo) - 1;
          redo &= redo - 1u;
          const int j = j0 + 16 * i;
          if (j < T) {
            const float v = expred_score_rec<NBD>(sq, eq, t.trec + 2 * NBD * j, D);
            if (prow) prow[j] = v;
            sink(j, v, order_key(v), std::false_type{});
          }
        }
      }
    };
    switch (nbd) {
      case 1: keys(std::integral_constant<int, 1>{}); break;
      case 2: keys(std::integral_constant<int, 2>{}); break;
      case 3: keys(std::integral_constant<int, 3>{}); break;
      default: keys(std::integral_constant<int, 4>{}); break;
    }
  } else if constexpr (MODE == kModeElsa) {
    // approx = ||MX_K[row r]|| * cos(clamp(pi/D * hamming - 0.127, 0))
    // (elsa_approximation.py:124-143; the key norm of row r, the reference's broadcast)
    uint32_t hq[kMaxNB];
#pragma unroll
    for (int b = 0; b < kMaxNB; ++b) hq[b] = b < nbd ? a.qsg[grow * nbd + b] : 0u;
    const float nrm = a.knorm[kb + r];
    for (int j = j0; j < T; j += js) {
      int h = 0;
#pragma unroll
      for (int b = 0; b < kMaxNB; ++b)
        if (b < nbd) h += (int)__popc(hq[b] ^ t.tsg[j * nbd + b]);
      emit(j, nrm * t.tcs[h]);
    }
  } else {
    const int8_t* qsrc = (MODE == kModeTrue ? a.qc : a.qop) + grow * a.dpad;
    const int16_t* qesrc = (MODE == kModeTrue ? a.qsT : a.qsA) + grow * nbd;
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
    for (int j = j0; j < T; j += js) {
      bool nan = false;
      double acc;
      if constexpr (MODE == kModeTrueEx)
        acc = g_dot_trueex(qv, qz, qe, nbd, t.tcd + (size_t)j * kst, t.tz + (size_t)j * kst, t.tex + j * nbd, nan);
      else
        acc = g_dot<MODE == kModeOpMul>(qv, qe, nbd, t.tcd + (size_t)j * kst, t.tex + j * nbd, nan);
      float v = nan ? __uint_as_float(0x7FC00000u) : (float)acc;
      // true = quantize_elemwise(fl32(QK^T)) * scale   (matmul.py:88-91, caller)
      if (MODE == kModeTrue) v = round_bfloat(round_dt(v, a.s_dt), a.bfloat, kRoundNearest, 1, a.s_dt) * a.scale;
      emit(j, v);
    }
  }
}

// prune mask words of one row from its kept indices (zeros.scatter_(-1, idx, 1) as bits):
// idx_at(p) for p = p0, p0 + ps, ... < k; mw is a per-row LDS scratch of ntw words; out[row * ntw +
// w] the row's words (the array's base and the row's number, the index formed at the store: with
// the row's pointer formed by the caller the packed select_kernel measured 0.3-0.5 % slower)
template <typename IdxAt>
__device__ __forceinline__ void sel_mask_words(uint32_t* out, int64_t row, int ntw, lu32* mw, bool valid, int p0, int ps, int k,
                                               IdxAt&& idx_at) {
  for (int w = p0; w < ntw; w += ps) mw[w] = 0u;
  wave_lds_sync();
  if (valid)
    for (int p = p0; p < k; p += ps) {
      const uint32_t ix = idx_at(p);
      atomicOr((uint32_t*)(mw + (ix >> 5)), 1u << (ix & 31));
    }
  wave_lds_sync();
  if (valid)
    for (int w = p0; w < ntw; w += ps) out[row * ntw + w] = mw[w];
}

// ---- four rows per wave (mxa_topk_grp.hpp): the row-group body behind the staged scores ----
// Lane gl of row gi has filled its share of g.A; bad != 0 on a lane that met a score which does
// not pack.  Shared by the fused selection (sel_rows4) and the standalone top-k (topk_rows16),
// which differ in where the elements come from and in Out: put_first(v) writes the row's first
// kept index (-1: left for the 64-bit pass; 0: handed to the tail, so that pass leaves the row
// alone), put(p, ix) the p-th kept index (and whatever goes with it).
//   El = uint32_t (packed): a row whose scores do not all leave the key's low byte free is left
//   for the 64-bit pass.
//   TW > 0 (packed): a row whose remaining work fits a TW-position prefix goes to the one-lane
//   tail (mxa_tail.hpp): its state and prefix are written to its record, tail_rec[row] (the
//   tail reads [0, tail_rec_len)); a row that `exists` and is finished here or left gets its
//   record cleared.
//   mask_out (nullable): the prune-mask words, ceil(n / 32) per row.
// tail_rec and mask_out come as the arrays' bases with the row's number: the row's own pointers,
// formed ahead of grp_topk, stayed live across it (topk_grp_kernel: up to 16 VGPRs more).
// Returns (per lane) whether this lane's row was left for the 64-bit pass.
template <int NP, typename El, int QM, int TW, typename Out>
__device__ __forceinline__ bool grp_rows4_finish(const GrpRow<El>& g, int n, int k, bool valid, bool exists, uint32_t bad,
                                                 int gi, int gl, uint32_t* tail_rec, uint32_t* mask_out, int64_t row,
                                                 Out out) {
  bool left = false;
  if constexpr (sizeof(El) == 4) {  // this row's 16 lanes: any score that does not pack
    const uint64_t bw = __builtin_amdgcn_ballot_w64(bad != 0u);
    if (valid && ((bw >> (16 * gi)) & 0xFFFFull) != 0) {
      if (gl == 0) out.put_first(-1);
      valid = false;
      left = true;
    }
  }
  wave_lds_sync();
  GrpHand hand{0u, false};
  grp_topk<NP, El, QM, TW>(g, n, k, valid, gl, &hand);
  if (TW > 0 && hand.on) {  // the row's state and prefix to the tail kernel
    uint32_t* rec = tail_rec + row * tail_rec_words(TW);
    if (gl == 0) {
      rec[0] = hand.state | kTailPending;
      out.put_first(0);
    }
    for (int p = gl; p < TW; p += 16) rec[4 + p] = (uint32_t)g.A[p];
    valid = false;
  } else if (TW > 0 && exists) {  // finished here, or left for the 64-bit pass: not the tail's
    if (gl == 0) tail_rec[row * tail_rec_words(TW)] = 0u;
  }
  if (valid)
    for (int p = gl; p < k; p += 16) out.put(p, GEl<El>::idx(g.A[p]));
  if (mask_out) {
    const int ntw = (n + 31) / 32;
    sel_mask_words(mask_out, row, ntw, g.stk, valid, gl, 16, k, [&](int p) { return GEl<El>::idx(g.A[p]); });
  }
  wave_lds_sync();
  return left;
}

// the fused selection's kept indices of row grow: kept_put
struct SelKeptOut {
  const Rows2Args& a;
  int64_t grow;
  int k;
  __device__ void put_first(int v) const { kept_put(a, grow * k, v); }
  __device__ void put(int p, uint32_t ix) const { kept_put(a, grow * k + p, (int)ix); }
};

// rows rq + (lane >> 4) of head bh; g0 = the wave's per-row areas (grp_row_bytes each).
// El = uint64_t: any row (a.fb_only: only the rows the packed pass left, kept_get(row * k) < 0).
// El = uint32_t, TW: grp_rows4_finish (the records a.tail_rec, the indices through kept_put).
// Returns (per lane) whether this lane's row was left for the 64-bit pass.
template <int NP, int MODE, typename El, int QM, int TW = 0>
__device__ __forceinline__ bool sel_rows4(const Rows2Args& a, const SelTabs& t, unsigned char* g0, int bh, int rq,
                                          int r_end, int lane) {
  constexpr bool kPacked = sizeof(El) == 4;
  const int gi = lane >> 4, gl = lane & 15;
  const int T = a.T, k = a.k_top;
  const int npa = grp_alloc(T);
  const GrpRow<El> g = carve_grp<El>(g0 + (size_t)gi * grp_row_bytes(npa, NP, sizeof(El)), npa, NP);
  const int r = rq + gi;
  bool valid = r < r_end;
  const int64_t grow = (int64_t)bh * a.N + (valid ? r : rq);
  if (!kPacked && a.fb_only && valid) valid = kept_get(a, grow * k) < 0;
  uint32_t bad = 0u, badf = 0u;
  if (valid) {
    if constexpr (kPacked)
      sel_scores<MODE>(a, t, bh, r, gl, 16, [&](int j, float v, uint32_t key, auto fast_c) {
        if constexpr (decltype(fast_c)::value) badf |= __float_as_uint(v);  // finite: the low byte
        else bad |= q_bad_bits(v);
        g.A[j] = qelem(key, (uint32_t)j);
      });
    else
      sel_scores<MODE>(a, t, bh, r, gl, 16, [&](int j, float, uint32_t key, auto) { g.A[j] = pack_ki(key, (uint32_t)j); });
  }
  bad |= badf & 0xFFu;
  if (k <= 0) return false;  // scores only
  return grp_rows4_finish<NP, El, QM, TW>(g, T, k, valid, r < r_end, bad, gi, gl, a.tail_rec, a.mask_out, grow,
                                          SelKeptOut{a, grow, k});
}

// One workgroup's work item: head bh, query-row chunk y (rows y * rows_per_wg ...).
// Returns (on every thread) whether a packed row of the chunk was left for the 64-bit pass.
template <int NP, int MODE, int kSelWaves, typename El, int QM, int TW>
__device__ __forceinline__ bool select_item(const Rows2Args& a, unsigned char* smem, int bh, int y) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = y * a.rows_per_wg, r_end = min(a.N, r0 + a.rows_per_wg);
  const SelLds L = sel_lds(MODE, a.T, a.D, a.kst, a.nbd);
  const SelTabs t = sel_stage<MODE>(a, smem, L, bh);
  unsigned char* g0 = smem + L.rows + (size_t)4 * wave * grp_row_bytes(grp_alloc(a.T), NP, sizeof(El));
  // (packed) whether a row this thread's wave handled was left for the 64-bit pass: tracked
  // per thread, not read back from idx -- other waves' kept_put(-1) need not be visible yet
  bool left = false;
  for (int rq = r0 + 4 * wave; rq < r_end; rq += 4 * kSelWaves) {
    if (sizeof(El) == 8 && a.fb_only) {  // the rows of this group that are left
      const int r = min(rq + (lane >> 4), r_end - 1);
      if (__builtin_amdgcn_ballot_w64(rq + (lane >> 4) < r_end && kept_get(a, ((int64_t)bh * a.N + r) * a.k_top) < 0) == 0)
        continue;
    }
    left |= sel_rows4<NP, MODE, El, QM, TW>(a, t, g0, bh, rq, r_end, lane);
  }
  return __syncthreads_or(left ? 1 : 0) != 0;
}

// The 64-bit pass's walk over the packed pass's workgroup flags (fb_only): workgroup wg takes
// flags [kFbItems wg, kFbItems (wg + 1)) of the n_items and calls item(i) on every thread for
// each flagged i, in order.  (Whether a barrier follows an item is the caller's business.)
template <typename Item>
__device__ __forceinline__ void fb_items(const uint32_t* flags, int64_t n_items, unsigned wg, Item&& item) {
  __shared__ uint64_t sbits;
  const int64_t i0 = (int64_t)wg * kFbItems;
  if (threadIdx.x < kFbItems) {
    const bool f = i0 + threadIdx.x < n_items && flags[i0 + threadIdx.x] != 0u;
    const uint64_t bits = __builtin_amdgcn_ballot_w64(f);
    if (threadIdx.x == 0) sbits = bits;
  }
  __syncthreads();
  uint64_t bits = sbits;
  while (bits) {
    const int i = __ffsll((long long)bits) - 1;
    bits &= bits - 1;
    item(i0 + i);
  }
}

// Selection kernel, four query rows per wave.  El = uint64_t: rows of up to 512 keys,
// every approximator.  El = uint32_t: the packed pass (rows of <= 256 keys; half the LDS
// per row, so more resident waves); each workgroup flags (a.fb_flags[bh * gy + y]) whether
// it left rows for the 64-bit pass, which then runs with fb_only: one workgroup per kFbItems
// flags, taking the flagged items one after another (fb_items; a call without such rows costs
// a small grid that exits at once).
template <int NP, int MODE, int kSelWaves, typename El = uint64_t, int QM = 0, int TW = 0>
__global__ __launch_bounds__(64 * kSelWaves) __attribute__((amdgpu_waves_per_eu(sizeof(El) == 4 ? (TW > 0 ? kSelPOcc : kSelPOccNT) : NP <= 256 ? kSelOcc : 2, 8))) void select_kernel(Rows2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (sizeof(El) == 8 && a.fb_only) {
    const int gy = a.fb_gy;
    fb_items(a.fb_flags, (int64_t)a.B * a.H * gy, blockIdx.x, [&](int64_t item) {
      select_item<NP, MODE, kSelWaves, El, QM, TW>(a, smem, (int)(item / gy), (int)(item % gy));
      __syncthreads();  // the next item re-stages the tables
    });
    return;
  }
  const bool left = select_item<NP, MODE, kSelWaves, El, QM, TW>(a, smem, blockIdx.x, blockIdx.y);
  if (sizeof(El) == 4 && a.fb_flags && threadIdx.x == 0) a.fb_flags[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = left ? 1u : 0u;
}

// ---- standalone top-k over rows of a float matrix (mxa_topk) ------------------
struct GrpTopkArgs {
  const void* vals;  // dtype dt
  int64_t rows, ld;
  int n, k;
  int64_t* out_idx;
  void* out_vals;  // dtype dt
  uint32_t* out_mask;
  int dt;
};

// the standalone top-k's workspace path (mxa_topk_ws): the packed pass's tail records and
// per-workgroup flags
struct TopkWs {
  uint32_t* tail_rec;  // [rows][tail_rec_words(TW)] (TW > 0)
  uint32_t* fb_flags;  // per packed workgroup: rows left for the 64-bit pass
  int64_t n_wg;        // packed workgroups (fb pass: flags to read)
  int fb_only;         // 64-bit pass over the flagged workgroups' rows with out_idx[row * k] < 0
};

// the standalone top-k's outputs of one row: its indices, and the values gathered at them
struct TopkRowOut {
  const GrpTopkArgs& a;
  int64_t row, src;  // src: the row's first value in a.vals
  __device__ void put_first(int v) const { a.out_idx[row * a.k] = v; }
  __device__ void put(int p, uint32_t ix) const {
    a.out_idx[row * a.k + p] = (int64_t)ix;
    if (a.out_vals) store_dt(a.out_vals, row * a.k + p, load_dt(a.vals, src + ix, a.dt), a.dt);
  }
};

// sixteen rows (four per wave) from row0: El = uint64_t any row (fb: only rows whose first
// index is -1); El = uint32_t, TW: grp_rows4_finish (the records w.tail_rec; the tail rebuilds
// the values from the elements, so a NaN or a -0 also leaves a row to the 64-bit pass).
// Returns (on every thread) whether a row was left.
template <int NP, typename El, int QM, int TW>
__device__ __forceinline__ bool topk_rows16(const GrpTopkArgs& a, const TopkWs& w, unsigned char* smem, int64_t row0,
                                            bool fb) {
  constexpr bool kPacked = sizeof(El) == 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gi = lane >> 4, gl = lane & 15;
  const int64_t row = row0 + 4 * wave + gi;
  bool valid = row < a.rows;
  if (fb && valid) valid = a.out_idx[row * a.k] < 0;
  const int npa = grp_alloc(a.n);
  const GrpRow<El> g = carve_grp<El>(smem + (size_t)(4 * wave + gi) * grp_row_bytes(npa, NP, sizeof(El)), npa, NP);
  const int64_t src = (valid ? row : 0) * a.ld;
  uint32_t bad = 0u;
  // the row's values, 256 (64-bit elements: 128) at a time: every load of a chunk issued before
  // the first is used (one load at a time left each wave waiting out a memory round trip per 16
  // values)
  constexpr int kChunk = NP < (kPacked ? 256 : 128) ? NP : (kPacked ? 256 : 128);
  for (int c0 = 0; c0 < NP; c0 += kChunk) {
    float vv[kChunk / 16];
#pragma unroll
    for (int t = 0; t < kChunk / 16; ++t) {
      const int j = c0 + gl + 16 * t;
      vv[t] = valid && j < a.n ? load_dt(a.vals, src + j, a.dt) : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < kChunk / 16; ++t) {
      const int j = c0 + gl + 16 * t;
      if (!valid || j >= a.n) continue;
      const float v = vv[t];
      if constexpr (kPacked) {
        bad |= q_bad_bits(v);
        if (a.out_vals) bad |= q_val_bad(v);  // the tail rebuilds the values from the elements
        g.A[j] = qelem(order_key(v), (uint32_t)j);
      } else {
        g.A[j] = pack_ki(order_key(v), (uint32_t)j);
      }
    }
  }
  const bool left = grp_rows4_finish<NP, El, QM, TW>(g, a.n, a.k, valid, row < a.rows, bad, gi, gl, w.tail_rec, a.out_mask,
                                                     row, TopkRowOut{a, row, src});
  return __syncthreads_or(left ? 1 : 0) != 0;
}

// El = uint64_t: every row (w.fb_only: one workgroup per kFbItems flags of the packed pass, taking
// the flagged workgroups' left rows); El = uint32_t: the packed pass, flagging per workgroup
template <int NP, typename El = uint64_t, int QM = 0, int TW = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sizeof(El) == 4 ? 5 : NP <= 256 ? 4 : 2, 8))) void topk_grp_kernel(GrpTopkArgs a, TopkWs w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (sizeof(El) == 8 && w.fb_only) {  // (no barrier of its own: topk_rows16 ends in one)
    fb_items(w.fb_flags, w.n_wg, blockIdx.x, [&](int64_t item) { topk_rows16<NP, El, QM, TW>(a, w, smem, item * 16, true); });
    return;
  }
  const bool left = topk_rows16<NP, El, QM, TW>(a, w, smem, (int64_t)blockIdx.x * 16, false);
  if (sizeof(El) == 4 && threadIdx.x == 0) w.fb_flags[blockIdx.x] = left ? 1u : 0u;
}

// one wave per row (mxa_topk_wave.hpp): waves of a 256-thread workgroup take rows
// 4 blockIdx.x + wave
template <int NP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NP <= 256 ? 8 : NP <= 512 ? 4 : 2, 8))) void topk_wave_kernel(GrpTopkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = (int)(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= a.rows) return;
  const WRow g = carve_wrow(smem + (size_t)wave * wrow_bytes(a.n), a.n);
  const int64_t src = row * a.ld;
  for (int j = (int)lane; j < a.n; j += 64) g.A[j] = pack_ki(order_key(load_dt(a.vals, src + j, a.dt)), (uint32_t)j);
  wave_lds_sync();
  wave_topk<NP / 64>(g, a.n, a.k);
  for (int p = (int)lane; p < a.k; p += 64) {
    const uint32_t ix = (uint32_t)g.A[p];
    a.out_idx[row * a.k + p] = (int64_t)ix;
    if (a.out_vals) store_dt(a.out_vals, row * a.k + p, load_dt(a.vals, src + ix, a.dt), a.dt);
  }
  if (a.out_mask) {
    const int ntw = (a.n + 31) / 32;
    sel_mask_words(a.out_mask, row, ntw, (lu32*)g.SL, true, (int)lane, 64, a.k, [&](int p) { return (uint32_t)g.A[p]; });
  }
}

}  // namespace mxa
