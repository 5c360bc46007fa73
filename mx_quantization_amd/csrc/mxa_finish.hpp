// Finishing kernel of the top-k path: for every query row and its k kept keys
// (select_kernel's indices), the true scores, softmax, MX(P) along keys and P.V,
// with P.V on int8 MFMA.  This is the 32-ROW kernel, for the calls the two 16-row kernels
// do not take (mxa_launch.hpp finish_choice): k > 64 with rows of more than 256 keys
// (below that mxa_finish_qk.hpp scores every key on MFMA), and k > 32 when the output
// goes to the proj Linear as MX codes (XO); k <= 64 (k <= 32 with XO) is
// mxa_finish16.hpp's.  The rules the three kernels share -- the true-score roundings,
// the MX(P) block rule, the corrected divide, the query-row load, the K-table staging,
// the proj-code epilogue -- are stated below, ahead of the kernel.
//
// Per workgroup (one head, or a chunk of its query rows when there are few heads):
// the head's K codes + exponents and V^T codes + exponents are staged in LDS once.
// Per wave, tiles of 32 query rows:
//   1. eight passes of four rows, one 16-lane DPP row per query row (the layout of
//      select_kernel): lane gl takes kept slots gl, gl+16, ...; the kept key's true
//      score fl32(exact sum) * scale (+ bias) by v_dot4 over the LDS codes with an
//      exact fp64 block epilogue; softmax over the kept scores (DPP
//      row reductions); P MX-quantized along keys (block maxima by LDS atomic max)
//      into the tile's dense code rows in LDS (zero elsewhere), block scales as
//      floats (NaN for a NaN block);
//   2. P.V for the tile: per 32 output columns and per 32-key MX block ONE
//      v_mfma_i32_32x32x32_i8 (K = 32 = one block, so each block keeps its exact
//      int32 sum), epilogue acc += C * (sP[row][b] * sV[b][d]) in fp32 (P.V is a
//      tolerance-only product);
//   3. the tile's output rows are written as 128-B row segments and its code rows
//      are cleared for the next tile.
// Reference: microxscaling/mx/matmul.py:68-76 (MX P.V), callers
// workloads/deit/scripts/main.py:124-152, workloads/DiT/models.py:195-225,
// workloads/PixArt/models/MX_transformer_block.py:679-717, :826-859.
#pragma once
#include "mxa_prep.hpp"
#include "mxa_dot.hpp"

namespace mxa {

constexpr int kFinTile = 32;  // query rows per MFMA tile (one wave)

typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v4i_ __attribute__((ext_vector_type(4)));

// LDS layout: tables, then per wave the P code tile [32][vst], the P block scales
// sP [ntb][32] (float), the block maxima bm [4][16] (u32, one DPP row each)
struct FinLds {
  size_t kc, ke, vt, ve, waves, per_wave, sp, bm, ot, total;
};
// xo: + the 32 x 32 fp32 output block being MX-quantized for the proj Linear
__host__ __device__ inline FinLds fin_lds(int T, int D, int kst, int nbd, int vst, int ntb, int waves, bool xo = false) {
  FinLds L;
  size_t o = 0;
  auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
  L.kc = o;
  o += al((size_t)T * kst);
  L.ke = o;
  o += al((size_t)T * nbd * 2);
  L.vt = o;
  o += al((size_t)D * vst);
  L.ve = o;
  o += al((size_t)ntb * D * 2);
  L.waves = o;
  L.sp = al((size_t)kFinTile * vst);
  L.bm = L.sp + al((size_t)ntb * kFinTile * 4);
  L.ot = L.bm + 4 * 16 * 4;  // block maxima: 16 per row of a pass
  L.per_wave = L.ot + (xo ? kFinTile * 33 * 4 : 0);
  L.total = o + (size_t)waves * L.per_wave;
  return L;
}

// exact 2^e as float (subnormal below -126, 0 below -149); NaN for the NaN exponent
__device__ __forceinline__ float scale_f(int e) {
  return e == kExpNaN ? __uint_as_float(0x7FC00000u) : (e < -149 ? 0.0f : pow2f(e));
}

// ---- the rules the three finishing kernels share -------------------------------------
// The per-element rules take the fields of Rows2Args they need by value: with a reference
// to the kernel's argument struct the register allocation of several instantiations
// changes (tools/kinfo.py against the kernels with the same code written out; DESIGN.md
// §4, "The finishing kernels as one family").
// true = quantize_elemwise(fl32(QK^T)) * scale from the exact block sum acc: the matmul's
// output in the score dtype, then * scale.  kRound = false: plain float32 scores (float32
// inputs and scores, bfloat 0 or 32), the roundings compiled away
template <bool kRound>
__device__ __forceinline__ float true_score(float acc, float scale, int bfloat, int sdt) {
  if (!kRound) return acc * scale;
  const float t = round_bfloat(round_dt(acc, sdt), bfloat, kRoundNearest, 1, sdt);
  return round_dt(t * scale, sdt);
}
// ... + bias (element off of Rows2Args::bias, of the input dtype)
__device__ __forceinline__ float true_score_bias(float t, const void* bias, int64_t off, int idt, int sdt) {
  return round_dt(t + load_dt(bias, off, idt), sdt);
}

// p = v / sum from y = RN(1 / sum), correctly rounded without a division per element
// (Markstein: q = RN(v y), r = v - q sum exact by fma, RN(q + r y) = RN(v / sum); v in
// [0, 1], sum in [1, T]: no overflow, and subnormal p only where the block is negligible)
__device__ __forceinline__ float div_by_sum(float v, float sum, float rs) {
  const float q0 = v * rs;
  return __builtin_fmaf(__builtin_fmaf(-q0, sum, v), rs, q0);
}

// MX(P) along keys, one 32-key block from the bits of its largest |p|: the scale exponent
// es (kExpNaN for a NaN block), the subnormal-flush flag and the block scale of the int8
// codes sP = 2^(es - 6) (NaN for a NaN block).  finish_qk_kernel, which holds the block in
// registers, calls it; the two gather kernels, which read the maximum from LDS and store sP
// there, write the same three lines out: routed through here, finish16_kernel's per-block
// loop no longer looks to the compiler as if its store of sP depended on the load of the
// maximum, it is vectorized by two and every instantiation needs 9 to 16 more VGPRs, and
// finish_kernel<2, 4, false, true> spills two more SGPRs
struct PBlock {
  int es;
  bool flush;
  float sP;
};
// (unit: the code unit is 2^(es - unit): 6 for MXINT8 codes, 2 for MXINT4 ones)
__device__ __forceinline__ PBlock p_block(uint32_t maxbits, int flush_p, int sdt, int unit = 6) {
  int e_raw;
  const int es = scale_exponent_dt(maxbits, 127, sdt, &e_raw);
  const bool fl = flush_p && !(e_raw != kExpNaN && e_raw > -127);
  return {es, fl, scale_f(es == kExpNaN ? kExpNaN : es - unit)};
}
// the gather kernels pass a block to the lanes that code its elements as one LDS word: es +
// 1024 (0 = a NaN block: no codes), the flush flag in bit 16.  The code of p from that
// word, the dtype roundings at run time (a flushed block codes 0s)
__device__ __forceinline__ int p_code_word(float p, uint32_t e, int sdt) {
  if (!(e & 0xFFFFu)) return 0;
  return (int)round_code((e & 0x10000u) ? p * 0.0f : p, (int)(e & 0xFFFFu) - 1024, 8, kRoundNearest, sdt);
}
// float32 scores: round_code for p >= 0, finite, from the block's code multiplier mult =
// 2^-es (0 for a flushed block): floor(p 2^-es 64 + 0.5), <= 127, as a float
__device__ __forceinline__ float p_code_f32(float p, float mult) {
  const float y = (p * mult) * 64.0f;
  return fminf(floorf(y + 0.5f), 127.0f);
}
// the same for MXINT4 P (mxa_attention_bits at width 4): floor(p 2^-es 4 + 0.5), <= 7, with the
// block scale sP = 2^(es - 2); the block rule (es, flush) does not depend on the width
__device__ __forceinline__ float p_code4_f32(float p, float mult) {
  const float y = (p * mult) * 4.0f;
  return fminf(floorf(y + 0.5f), 7.0f);
}
// W4 ? the MXINT4 rule : the MXINT8 rule, and the exponent of a code unit below es
template <bool W4>
__device__ __forceinline__ float p_code_bits_f32(float p, float mult) {
  return W4 ? p_code4_f32(p, mult) : p_code_f32(p, mult);
}
template <bool W4>
constexpr int kPUnit = W4 ? 2 : 6;

// a query row's codes (two 16-byte halves per 32-block) and block exponents
template <int NB>
__device__ __forceinline__ void load_query_row(const Rows2Args& a, int64_t grow, uint4* qv, int* qe) {
  const int8_t* qsrc = a.qc + grow * a.dpad;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    qv[2 * b] = *reinterpret_cast<const uint4*>(qsrc + 32 * b);
    qv[2 * b + 1] = *reinterpret_cast<const uint4*>(qsrc + 32 * b + 16);
    qe[b] = exp_from16(a.qsT[grow * NB + b]);
  }
}

// the head's K codes (row stride kst) and block exponents into LDS, by the whole workgroup
template <int NB>
__device__ __forceinline__ void stage_k_table(const Rows2Args& a, int64_t kb, int8_t* tkc, int16_t* tke) {
  const int cpr = a.dpad / 16;
  for (int i = threadIdx.x; i < a.T * cpr; i += blockDim.x) {
    const int j = i / cpr, c = i - j * cpr;
    *reinterpret_cast<uint4*>(tkc + (size_t)j * a.kst + 16 * c) =
        *reinterpret_cast<const uint4*>(a.kc + (kb + j) * a.dpad + 16 * c);
  }
  for (int i = threadIdx.x; i < a.T * NB; i += blockDim.x) tke[i] = a.ksT[kb * NB + i];
}

// XO: the (B, N, C) output rows as the proj Linear's MX input codes (Rows2Args::xo_codes /
// xo_exps; C = H D, nb = H NB blocks per row): what rows_prep makes of the rows, in the MX
// GEMM's A layout ...
__device__ __forceinline__ RowsPrepArgs xo_rows_args(int8_t* codes, int16_t* exps, int C, int nb, int flush, int bfloat) {
  RowsPrepArgs ro{};
  ro.codes = codes; ro.sT = exps;
  ro.dpad = C; ro.nb = nb; ro.D = C;
  ro.op_kind = MXA_OP_MXINT8; ro.flush = flush; ro.bfloat = bfloat; ro.dt = kF32;
  ro.mfma_rows = 1;  // the MX GEMM's A layout
  return ro;
}
// ... and the 16 values xv of 32-block blk of output row orow (half sub, column c0) into
// them.  Two consecutive lanes per block; every lane calls it (on: its row and block exist)
__device__ __forceinline__ void xo_block(const RowsPrepArgs& ro, int64_t orow, int blk, int sub, int c0, float* xv, bool on) {
  if (rows_prep_plain(ro)) rows_prep_block_plain<kF32>(ro, orow, blk, sub, c0, xv, on);
  else rows_prep_block(ro, orow, blk, sub, c0, xv, on);
}

// ---- the 32-row kernel ------------------------------------------------------------------
// NB: 32-blocks per head dim (nbd); KS: kept slots per lane: eight passes of four rows
// per tile, one 16-lane DPP row per query row (k <= 16 KS).
// XDT: float16 / bfloat16 inputs or scores (include/mxa.h dtype / score_dtype): the
// dtype roundings at run time; XDT = false compiles them away (the float32 path).
// XO: the output goes to the proj Linear as MX codes along C (Rows2Args::xo_codes;
// float32, D % 32 == 0: every 32-column P.V tile is one MX block of the output row)
template <int NB, int KS, bool XDT, bool XO = false>
__global__ __launch_bounds__(512) void finish_kernel(Rows2Args a) {
  const int sdt = XDT ? a.s_dt : (int)kF32, idt = XDT ? a.in_dt : (int)kF32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gi = lane >> 4, gl = lane & 15;
  const int bh = blockIdx.x;
  const int T = a.T, D = a.D, kst = a.kst, vst = a.vst, ntb = a.ntb, k = a.k_top;
  constexpr int nbd = NB;
  const int b_ = bh / a.H, h_ = bh % a.H;
  const FinLds L = fin_lds(T, D, kst, nbd, vst, ntb, a.waves, XO);
  int8_t* tkc = reinterpret_cast<int8_t*>(smem + L.kc);
  int16_t* tke = reinterpret_cast<int16_t*>(smem + L.ke);
  int8_t* tvt = reinterpret_cast<int8_t*>(smem + L.vt);
  int16_t* tve = reinterpret_cast<int16_t*>(smem + L.ve);
  unsigned char* wb = smem + L.waves + (size_t)wave * L.per_wave;
  int8_t* ptile = reinterpret_cast<int8_t*>(wb);
  float* sP = reinterpret_cast<float*>(wb + L.sp);
  // block maxima of the P row being quantized: 16 words per row (T <= 512)
  uint32_t* bm = reinterpret_cast<uint32_t*>(wb + L.bm) + 16 * gi;

  // ---- stage the head's K and V tables; clear the code tile -----------------------
  const int64_t kb = (int64_t)bh * T;
  {
    stage_k_table<NB>(a, kb, tkc, tke);
    // V^T codes, token-block-major in HBM ([ntb][D][32] per head: contiguous 2-KB runs)
    const int8_t* vsrc = a.vt + (int64_t)bh * D * a.tpad;
    for (int i = threadIdx.x; i < a.ntb * D * 2; i += blockDim.x) {
      const int half = i & 1, dd = (i >> 1) % D, tb = (i >> 1) / D;
      *reinterpret_cast<uint4*>(tvt + (size_t)dd * vst + 32 * tb + 16 * half) =
          *reinterpret_cast<const uint4*>(vsrc + ((int64_t)tb * D + dd) * 32 + 16 * half);
    }
    const int16_t* vssrc = a.vs + (int64_t)bh * ntb * D;
    for (int i = threadIdx.x; i < ntb * D; i += blockDim.x) tve[i] = vssrc[i];
    for (int i = lane; i < kFinTile * vst / 16; i += 64) reinterpret_cast<uint4*>(ptile)[i] = make_uint4(0, 0, 0, 0);
    bm[gl] = 0u;
  }
  __syncthreads();

  const int r_beg = (int)blockIdx.y * a.rows_per_wg, r_end = min(a.N, r_beg + a.rows_per_wg);

  // a pass's global inputs (the row's query codes / exponents and kept indices),
  // loaded one pass ahead so that their latency hides behind the previous pass
  struct PassIn {
    uint4 qv[2 * NB];
    int qe[NB];
    int ix[KS];
  };
  auto load_pass = [&](int r0, int pass, PassIn& in) {
    const int r = r0 + 4 * pass + gi;
    const bool valid = r < r_end;
    const int64_t grow = (int64_t)bh * a.N + (valid ? r : r_beg);
    load_query_row<NB>(a, grow, in.qv, in.qe);
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const int s = gl + 16 * t;
      in.ix[t] = valid && s < k ? kept_get(a, grow * k + s) : -1;
    }
  };
  PassIn nxt;
  if (r_beg + kFinTile * wave < r_end) load_pass(r_beg + kFinTile * wave, 0, nxt);
  for (int r0 = r_beg + kFinTile * wave; r0 < r_end; r0 += kFinTile * a.waves) {
    // ---- 1. kept scores, softmax, MX(P) into the code tile: four rows per pass ----
    for (int pass = 0; pass < kFinTile / 4; ++pass) {
      const PassIn cur = nxt;
      if (pass + 1 < kFinTile / 4) load_pass(r0, pass + 1, nxt);
      else if (r0 + kFinTile * a.waves < r_end) load_pass(r0 + kFinTile * a.waves, 0, nxt);
      const int tr = 4 * pass + gi;  // row within the tile
      const int r = r0 + tr;
      const bool valid = r < r_end;
      const int64_t grow = (int64_t)bh * a.N + (valid ? r : r0);
      const int64_t brow = a.bias ? b_ * a.bs0 + h_ * a.bs1 + (int64_t)(valid ? r : r0) * a.bs2 : -1;
      auto true_of = [&](int j) -> float {  // the true score of key j (+ bias)
        const float acc = true_dot<NB>(cur.qv, cur.qe, tkc + (size_t)j * kst, tke + j * nbd);
        const float t = true_score<true>(acc, a.scale, a.bfloat, sdt);
        return brow >= 0 ? true_score_bias(t, a.bias, brow + (int64_t)j * a.bs3, idt, sdt) : t;
      };
      if (a.true_out && valid)  // debug output: every key's true score
        for (int j = gl; j < T; j += 16) a.true_out[grow * T + j] = true_of(j);

      int ix[KS];
      float v[KS];
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        ix[t] = cur.ix[t];
        v[t] = ix[t] >= 0 ? true_of(ix[t]) : -INFINITY;
        mx = fmaxf(mx, v[t]);
      }
      mx = __uint_as_float(row16_reduce(__float_as_uint(mx), [](uint32_t x, uint32_t y) {
        return __float_as_uint(fmaxf(__uint_as_float(x), __uint_as_float(y)));
      }));
      float sum = 0.0f;
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        v[t] = ix[t] >= 0 ? expf(v[t] - mx) : 0.0f;
        sum += v[t];
      }
      sum = __uint_as_float(row16_reduce(__float_as_uint(sum), [](uint32_t x, uint32_t y) {
        return __float_as_uint(__uint_as_float(x) + __uint_as_float(y));
      }));
      // zeros.scatter_(idx, softmax) -> MXINT8 along keys (block maxima by atomic max)
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        if (ix[t] >= 0) {
          v[t] = round_dt(round_bfloat(v[t] / sum, a.bfloat, kRoundNearest, 1, sdt), sdt);
          atomicMax(&bm[ix[t] >> 5], __float_as_uint(v[t]) & 0x7FFFFFFFu);
        }
      }
      wave_lds_sync();
      if (gl < ntb) {  // block gl: its scale and its word for the lanes that code it
        // (p_block's rule written out, see there; then the block's word for p_code_word)
        int e_raw;
        const int es = scale_exponent_dt(bm[gl], 127, sdt, &e_raw);
        const bool fl = a.flush_p && !(e_raw != kExpNaN && e_raw > -127);
        sP[gl * kFinTile + tr] = scale_f(es == kExpNaN ? kExpNaN : es - 6);
        bm[gl] = (es == kExpNaN ? 0u : (uint32_t)(es + 1024)) | (fl ? 0x10000u : 0u);
      }
      wave_lds_sync();
#pragma unroll
      for (int t = 0; t < KS; ++t)
        if (ix[t] >= 0) ptile[tr * vst + ix[t]] = (int8_t)p_code_word(v[t], bm[ix[t] >> 5], sdt);
      wave_lds_sync();
      bm[gl] = 0u;
    }
    wave_lds_sync();

    // ---- 2. P.V on int8 MFMA: one v_mfma_i32_32x32x32_i8 per (32 columns, key block) ----
    // lane maps (checked on hardware by mxa_selftest_mfma32): A[m][k], m = lane % 32,
    // k = 16 (lane / 32) + 0..15; B[k][n], n = lane % 32, the same k; C[m][n] in c[i],
    // m = 8 (i / 4) + 4 (lane / 32) + i % 4, n = lane % 32
    const int m0 = 4 * (lane >> 5), ln = lane & 31, kh = 16 * (lane >> 5);
    for (int dt = 0; dt < D; dt += 32) {
      const int d = min(dt + ln, D - 1);
      float acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
      for (int b = 0; b < ntb; ++b) {
        const v4i_ av = *reinterpret_cast<const v4i_*>(ptile + ln * vst + 32 * b + kh);
        const v4i_ bv = *reinterpret_cast<const v4i_*>(tvt + (size_t)d * vst + 32 * b + kh);
        const v16i zero = {};
        const v16i c = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, zero, 0, 0, 0);
        const float sv = scale_f(exp_from16(tve[b * D + d]));
        const float* sp = sP + b * kFinTile;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 s4 = *reinterpret_cast<const float4*>(sp + 8 * q + m0);
          acc[4 * q + 0] = fmaf((float)c[4 * q + 0], s4.x * sv, acc[4 * q + 0]);
          acc[4 * q + 1] = fmaf((float)c[4 * q + 1], s4.y * sv, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf((float)c[4 * q + 2], s4.z * sv, acc[4 * q + 2]);
          acc[4 * q + 3] = fmaf((float)c[4 * q + 3], s4.w * sv, acc[4 * q + 3]);
        }
      }
      if constexpr (XO) {
        // ---- 3'. the 32 x 32 block -> MX codes of block (h D + dt) / 32 of each output
        // row (what rows_prep makes of the (B, N, C) output for the proj Linear) -------
        float* ot = reinterpret_cast<float*>(wb + L.ot);
#pragma unroll
        for (int i = 0; i < 16; ++i)
          ot[(8 * (i >> 2) + m0 + (i & 3)) * 33 + ln] = round_bfloat(acc[i], a.bfloat, kRoundNearest, 1);
        wave_lds_sync();
        const int row = lane >> 1, sub = lane & 1, r = r0 + row;
        float xv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) xv[j] = ot[row * 33 + 16 * sub + j];
        const int64_t orow = (int64_t)b_ * a.N + (r < r_end ? r : r0);
        const RowsPrepArgs ro = xo_rows_args(a.xo_codes, a.xo_exps, a.H * D, a.H * nbd, a.flush_p, a.bfloat);
        xo_block(ro, orow, h_ * nbd + dt / 32, sub, h_ * D + dt + 16 * sub, xv, r < r_end);
        wave_lds_sync();
        continue;
      }
      // ---- 3. output rows (128-B segments per row) --------------------------------
      if (dt + ln < D) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int r = r0 + 8 * (i >> 2) + m0 + (i & 3);
          if (r < r_end)
            store_dt(a.out, b_ * a.os0 + h_ * a.os1 + (int64_t)r * a.os2 + dt + ln,
                     round_bfloat(round_dt(acc[i], sdt), a.bfloat, kRoundNearest, 1, sdt), sdt);
        }
      }
    }
    wave_lds_sync();
    for (int i = lane; i < kFinTile * vst / 16; i += 64) reinterpret_cast<uint4*>(ptile)[i] = make_uint4(0, 0, 0, 0);
    wave_lds_sync();
  }
}

}  // namespace mxa
