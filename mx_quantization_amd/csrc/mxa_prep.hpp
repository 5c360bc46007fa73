// Per-block bodies of the attention operand builders: one 32-element block of a row
// (rows_prep_block, rows_prep_block_plain) and one 32-row block of a column
// (cols_prep_column).  Their callers, and what each knows about the storage dtype:
//   mxa_quant.hip   rows_prep_kernel, cols_prep_kernel, attn_prep_kernel: the dtype is a
//                   template parameter of the loads and a run-time value (a.dt) here
//   mxa_proj.hpp    the fused projections' tile epilogue: float32, stated at compile time on
//                   the PLAIN path (DT), a.dt on the general one
//   mxa_finish.hpp  xo_block, the finishing kernels' proj-code epilogue: as mxa_proj.hpp
#pragma once
#include <type_traits>
#include "mxa_kernels.hpp"

namespace mxa {

__device__ __forceinline__ int exion_m(int raw) {
  // two_step_leading_ones on an integer code (funcs/exponent_based_prediction.py:110-127):
  //   l1 = floor(log2|raw|), t = max(raw - 2^l1, 0) (signed!), l2 = floor(log2 t),
  //   approx = sign(raw) * e * (2^l1 + 2^l2) / 64   (2^-126 terms vanish in fp32)
  if (raw == 0) return 0;
  if (raw < 0) return -(1 << (31 - __clz(-raw)));
  const int p1 = 1 << (31 - __clz(raw));
  const int t = raw - p1;
  return p1 + (t > 0 ? (1 << (31 - __clz(t))) : 0);
}

// exponent of the MX-quantized block (funcs/exponent_based_prediction.py:35-36):
// floor(log2(max |MX|)), unclamped, in the dtype; MX max = maxc * 2^(es-6) (a value of the
// dtype: exact in float32 / bfloat16, and in float16 for es >= -18), maxc the largest |code|
// (unit: the code unit is 2^(es - unit) -- 6 for MXINT8, 2 for MXINT4)
__device__ __forceinline__ int mx_block_exponent(int maxc, int es, bool nan, int dt, int unit = 6) {
  if (nan) return kExpNaN;
  if (maxc == 0) return -126;
  return floor_log2_dt(__float_as_uint(round_dt((float)maxc * pow2f(es - unit), dt)), dt);
}

// ---------------------------------------------------------------------------
// attention operand builder for rows quantized along the last axis (Q, K): two
// consecutive lanes per 32-element block, lane `sub` holding the sixteen elements from
// column c0 = 32 blk + 16 sub.  Both lanes of a pair must call the bodies (DPP).
// ---------------------------------------------------------------------------
// the value of the pair's other lane
__device__ __forceinline__ uint32_t pair_swap(uint32_t v) { return dpp_u32<0xB1>(v); }  // quad_perm [1,0,3,2]

// the block's largest |code| and its packed sign word, bit (16 sub + j) = (code < 0): the
// exp-sign operand of ex_pred (codes beyond D are 0, i.e. positive)
struct RowCodes {
  int maxc;
  uint32_t signs;
};
__device__ __forceinline__ RowCodes row_block_codes(const int code[16], int sub) {
  int maxc = 0;
  uint32_t sw = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    maxc = max(maxc, abs(code[j]));
    sw |= (code[j] < 0 ? 1u : 0u) << (16 * sub + j);
  }
  return {(int)max((uint32_t)maxc, pair_swap((uint32_t)maxc)), sw | pair_swap(sw)};
}
// where the sixteen codes of lane `sub` go: row-major (row * dpad + c0), or with a.mfma_rows
// the MX GEMM's MFMA-ready A layout -- per 32-row block and K-block, 64 lanes x 16 B, lane
// (row & 31) + 32 sub holding elements 16 sub .. 16 sub + 15
__device__ __forceinline__ int64_t mfma_base(const RowsPrepArgs& a, int64_t row, int blk, int sub, int c0) {
  if (a.mfma_rows) return (((row >> 5) * a.nb + blk) * 64 + (row & 31) + 32 * sub) * 16;
  return row * a.dpad + c0;
}
// the per-block words (lane sub == 0 of a valid block): the code unit's exponent, the
// approximator scale and the sign word.  (The exponents as values: with the BlkScale passed in
// here, finish16_kernel<2, 5, false, true, true> spills two more VGPRs.)
__device__ __forceinline__ void store_block_words(const RowsPrepArgs& a, int64_t row, int blk, int sT, int sA,
                                                  uint32_t signs) {
  if (a.sT) a.sT[row * a.nb + blk] = exp_to16(sT);
  if (a.sA) a.sA[row * a.nb + blk] = exp_to16(sA);
  if (a.signs) a.signs[row * a.nb + blk] = signs;
}

// One 32-element block of a row: MXINT8 codes, block exponent, approximator operand, zero
// indicators and sign word into the RowsPrepArgs outputs (row `row`, block `blk`), for every
// setting of the arguments.  Shared with the plain body: blk_scale, row_block_codes,
// mfma_base, store_block_words.  Written out here, because as shared helpers they cost the
// general-argument projection kernels SGPR spills (qkv_proj_kernel<2..4, false> 196 -> 350
// with all of them): the rounding + maximum loop, and the packing of codes, operand and zero
// indicators word by word.
// MB: the element width.  8: MXINT8.  4: MXINT4 -- codes in [-7, 7] in the same int8 containers,
// code unit 2^(es - 2), and every approximator operand derived from those codes, as the
// reference's exponent_approximation does at a_elem_format = "int4" (its MX_Q / MX_K are MXINT4
// then: funcs/exponent_based_prediction.py:18-31): a value that rounds to the int4 code 0 has
// the sign "+", EXION's raw integer MX / 2^eA * 64 is code << (es - eA + 4) (at most 112), and
// the MXINT8 kind (partial_*'s MX side) is the int4 code itself
template <int MB = 8>
__device__ __forceinline__ void rows_prep_block(const RowsPrepArgs& a, int64_t row, int blk, int sub, int c0,
                                                float xv[16], bool valid) {
  static_assert(MB == 8 || MB == 4, "MXINT8 or MXINT4");
  constexpr int U = MB - 2;  // the code unit is 2^(es - U)
  uint32_t mb = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    xv[j] = round_bfloat(xv[j], a.bfloat, kRoundNearest, 1, a.dt);
    const uint32_t ub = __float_as_uint(xv[j]) & 0x7FFFFFFFu;
    mb = ub > mb ? ub : mb;
  }
  mb = max(mb, pair_swap(mb));
  const BlkScale s = blk_scale(mb, 127, a.dt, a.flush);
  const int es = s.es;
  const bool nanblk = s.nan;
  if (s.flush) {
#pragma unroll
    for (int j = 0; j < 16; ++j) xv[j] = xv[j] * 0.0f;
  }
  int code[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) code[j] = nanblk ? 0 : (int)round_code(xv[j], es, MB, kRoundNearest, a.dt);
  const int maxc = row_block_codes(code, sub).maxc;
  const int eA = mx_block_exponent(maxc, es, nanblk, a.dt, U);
  int op[16];
  int sA;
  switch (a.op_kind) {
    case MXA_OP_SIGN:
#pragma unroll
      for (int j = 0; j < 16; ++j) op[j] = (c0 + j < a.D) ? (code[j] < 0 ? -1 : 1) : 0;
      sA = eA;
      break;
    case MXA_OP_MXINT4:
#pragma unroll
      for (int j = 0; j < 16; ++j) op[j] = nanblk ? 0 : (int)round_code(xv[j], es, 4, kRoundNearest, a.dt);
      sA = nanblk ? kExpNaN : es - 2;
      break;
    case MXA_OP_EXION: {
      const int sh = nanblk ? 0 : es - eA + (6 - U);  // MX / 2^eA * 64 = code * 2^(es-eA+6-U), an integer < 128
#pragma unroll
      for (int j = 0; j < 16; ++j) op[j] = nanblk ? 0 : exion_m(code[j] << sh);
      sA = eA;
      break;
    }
    case MXA_OP_TRUE_EX:
      // exponent_based_sign_leading_ones (examples/deit/exponent_based_prediction.py:163-178):
      // (mx < 0 ? -1 : 1) * 2^floor(log2|mx|), zeros -> +1.  Nonzero elements as the
      // power-of-two code sign * 2^floor(log2|code|) in units of 2^(es-U); zeros in zind
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int ac = code[j] < 0 ? -code[j] : code[j];
        const int p2 = ac ? 1 << (31 - __clz(ac)) : 0;
        op[j] = code[j] < 0 ? -p2 : p2;
      }
      // a NaN block's MX values are NaN, and get_true_exponents maps them like zeros
      // (mask |x| > 0 is false: exponent 0, value +1; examples :98-110): codes 0, zind 1
      sA = nanblk ? 0 : es - U;
      break;
    default:  // MXA_OP_MXINT8 (the MX codes themselves, at either width)
#pragma unroll
      for (int j = 0; j < 16; ++j) op[j] = code[j];
      sA = nanblk ? kExpNaN : es - U;
      break;
  }
  if (valid) {
    const int64_t base = mfma_base(a, row, blk, sub, c0);
    uint32_t pc[4], po[4], pz[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      pc[w] = po[w] = pz[w] = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pc[w] |= (uint32_t)(code[4 * w + j] & 0xFF) << (8 * j);
        po[w] |= (uint32_t)(op[4 * w + j] & 0xFF) << (8 * j);
        pz[w] |= (c0 + 4 * w + j < a.D && code[4 * w + j] == 0 ? 1u : 0u) << (8 * j);
      }
    }
    if (a.codes) *reinterpret_cast<uint4*>(a.codes + base) = make_uint4(pc[0], pc[1], pc[2], pc[3]);
    if (a.op) *reinterpret_cast<uint4*>(a.op + base) = make_uint4(po[0], po[1], po[2], po[3]);
    if (a.zind) *reinterpret_cast<uint4*>(a.zind + base) = make_uint4(pz[0], pz[1], pz[2], pz[3]);
  }
  // the sign word is asked for only here (the unused half of each call compiles away): formed
  // before the operand switch it stays live across it, which costs the prep kernels 15 VGPRs
  // and with them a wave per SIMD
  const uint32_t sw = row_block_codes(code, sub).signs;
  if (valid && sub == 0) store_block_words(a, row, blk, nanblk ? kExpNaN : es - U, sA, sw);
}

// rows_prep_block for the plain case -- no bfloat rounding, no subnormal flush, no
// true_ex zero indicators, approximator operand the sign (ex_pred) or the MXINT8 code --
// with the int8 code path of q8_code: the same outputs in about a third of the VALU
// (the prep launch is VALU-bound next to its HBM stream otherwise).  A body of its own: the
// benchmark's prep, projection and finishing kernels run this instruction stream.  It has no
// flush, so its block rule is scale_exponent_dt alone, and it keeps its own float32 form of the
// block exponent: through blk_scale or mx_block_exponent the general-argument
// cross_proj_kernel<1, false, 1> gains 4 bytes of scratch and 14 SGPR spills.
__device__ __forceinline__ bool rows_prep_plain(const RowsPrepArgs& a) {
  return (a.bfloat == 0 || a.bfloat == 32) && !a.flush && !a.zind &&
         (a.op_kind == MXA_OP_MXINT8 || (a.op_kind == MXA_OP_SIGN && !a.op));
}
// DT >= 0: the storage dtype known at compile time (the fused projection and the finishing
// kernels' epilogue: float32)
template <int DT = -1>
__device__ __forceinline__ void rows_prep_block_plain(const RowsPrepArgs& a, int64_t row, int blk, int sub, int c0,
                                                      const float xv[16], bool valid) {
  const int dt = DT >= 0 ? DT : a.dt;
  uint32_t mb = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) mb = max(mb, __float_as_uint(xv[j]) & 0x7FFFFFFFu);
  mb = max(mb, pair_swap(mb));
  int e_raw;
  const int es = scale_exponent_dt(mb, 127, dt, &e_raw);
  const bool nanblk = es == kExpNaN;
  int code[16];
  auto quant = [&](auto tiny) {
    const float sc = q8_scale(es);
#pragma unroll
    for (int j = 0; j < 16; ++j) code[j] = q8_code<decltype(tiny)::value>(xv[j], sc, dt);
  };
  if (nanblk) {
#pragma unroll
    for (int j = 0; j < 16; ++j) code[j] = 0;
  } else if (es >= -121) {
    quant(std::false_type{});
  } else {
    quant(std::true_type{});
  }
  const RowCodes rc = row_block_codes(code, sub);
  const int maxc = rc.maxc;
  if (valid) {
    uint32_t pc[4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
      pc[w] = (uint32_t)(code[4 * w] & 0xFF) | (uint32_t)(code[4 * w + 1] & 0xFF) << 8 |
              (uint32_t)(code[4 * w + 2] & 0xFF) << 16 | (uint32_t)code[4 * w + 3] << 24;
    const int64_t base = mfma_base(a, row, blk, sub, c0);
    const uint4 v = make_uint4(pc[0], pc[1], pc[2], pc[3]);
    if (a.codes) *reinterpret_cast<uint4*>(a.codes + base) = v;
    if (a.op) *reinterpret_cast<uint4*>(a.op + base) = v;  // MXA_OP_MXINT8 (SIGN has none)
    if (sub == 0) {
      // float32: floor(log2(maxc * 2^(es-6))) = floor(log2 maxc) + es - 6 exactly (maxc <= 127);
      // the other dtypes round log2 to the dtype (what mx_block_exponent states)
      int eA = nanblk ? kExpNaN : (maxc == 0 ? -126 : 31 - __clz(maxc) + es - 6);
      if (dt != kF32 && !nanblk && maxc != 0)
        eA = floor_log2_dt(__float_as_uint(round_dt((float)maxc * pow2f(es - 6), dt)), dt);
      const int sT = nanblk ? kExpNaN : es - 6;
      store_block_words(a, row, blk, sT, a.op_kind == MXA_OP_SIGN ? eA : sT, rc.signs);
    }
  }
}

// The plain case at 4 bits (rows_prep_block<4> with no bfloat rounding, no flush, no zero
// indicators; operand the sign, or the MXINT4 code under either of its kinds), float32 rows:
// the kernel trace of the PixArt shapes had the general body at 21.8 us against the plain 8-bit
// one's 16.4 (profiles/r10_attn4_bench.txt).  A body of its own, so that rows_prep_block_plain
// and the kernels that inline it stay what they are.  The code: x * 2^(2 - es) is exact and
// equals (x * 2^-es) * 4 (for es < -125, where 2^(2 - es) is no float, 2^-es and then * 4),
// floor(|y| + 1/2) clipped to 7, the sign copied back (-0 converts to 0).  The block exponent:
// floor(log2(maxc * 2^(es - 2))) = floor(log2 maxc) + es - 2 exactly (maxc <= 7).
__device__ __forceinline__ bool rows_prep_plain4(const RowsPrepArgs& a) {
  return (a.bfloat == 0 || a.bfloat == 32) && !a.flush && !a.zind &&
         (a.op_kind == MXA_OP_MXINT8 || a.op_kind == MXA_OP_MXINT4 || (a.op_kind == MXA_OP_SIGN && !a.op));
}
__device__ __forceinline__ void rows_prep_block_plain4(const RowsPrepArgs& a, int64_t row, int blk, int sub, int c0,
                                                       const float xv[16], bool valid) {
  uint32_t mb = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) mb = max(mb, __float_as_uint(xv[j]) & 0x7FFFFFFFu);
  mb = max(mb, pair_swap(mb));
  int e_raw;
  const int es = scale_exponent(mb, 127, &e_raw);
  const bool nanblk = es == kExpNaN;
  int code[16];
  auto quant = [&](auto tiny) {
    const float sc = pow2f(decltype(tiny)::value ? -es : 2 - es);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float y = xv[j] * sc;
      if (decltype(tiny)::value) y = y * 4.0f;
      code[j] = (int)__builtin_copysignf(fminf(floorf(fabsf(y) + 0.5f), 7.0f), y);
    }
  };
  if (nanblk) {
#pragma unroll
    for (int j = 0; j < 16; ++j) code[j] = 0;
  } else if (es >= -125) {
    quant(std::false_type{});
  } else {
    quant(std::true_type{});
  }
  const RowCodes rc = row_block_codes(code, sub);
  if (valid) {
    uint32_t pc[4];
#pragma unroll
    for (int w = 0; w < 4; ++w)
      pc[w] = (uint32_t)(code[4 * w] & 0xFF) | (uint32_t)(code[4 * w + 1] & 0xFF) << 8 |
              (uint32_t)(code[4 * w + 2] & 0xFF) << 16 | (uint32_t)code[4 * w + 3] << 24;
    const int64_t base = mfma_base(a, row, blk, sub, c0);
    const uint4 v = make_uint4(pc[0], pc[1], pc[2], pc[3]);
    if (a.codes) *reinterpret_cast<uint4*>(a.codes + base) = v;
    if (a.op) *reinterpret_cast<uint4*>(a.op + base) = v;  // the MXINT4 code (SIGN has none)
    if (sub == 0) {
      const int eA = nanblk ? kExpNaN : (rc.maxc == 0 ? -126 : 31 - __clz(rc.maxc) + es - 2);
      const int sT = nanblk ? kExpNaN : es - 2;
      store_block_words(a, row, blk, sT, a.op_kind == MXA_OP_SIGN ? eA : sT, rc.signs);
    }
  }
}

// ---------------------------------------------------------------------------
// operand builder for matrices quantized along the row axis (V, and in2 of
// mx.matmul): blocks of 32 rows per column; output transposed [col][row] codes.
// ---------------------------------------------------------------------------
// One 32-row block of one column (m = matrix, blk, column c) from its 32 values
// (already bfloat-rounded, zero beyond the matrix): codes into the transposed
// [m][C][rpad] table, the exponent into [m][nb][C].  PLAIN: MXINT8, no flush (the
// caller checked), DT >= 0 the storage dtype known at compile time.
template <bool PLAIN = false, int DT = -1>
__device__ __forceinline__ void cols_prep_column(const ColsPrepArgs& a, int64_t m, int blk, int c, const float xv[32],
                                                 uint32_t mx) {
  const int r0 = blk * 32;
  const int dt = DT >= 0 ? DT : a.dt;
  const BlkScale s = blk_scale(mx, 127, dt, PLAIN ? 0 : a.flush);
  const int es = s.es;
  const bool nanblk = s.nan, flush = s.flush;
  const int mbits = PLAIN ? 8 : a.mbits;
  uint32_t w[8];
  if (PLAIN && nanblk) {
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = 0u;
  } else if (!flush && !nanblk && mbits == 8) {  // the plain MXINT8 case: q8_code
    const float sc = q8_scale(es);
    auto quant = [&](auto tiny) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        int cd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cd[j] = q8_code<decltype(tiny)::value>(xv[q * 4 + j], sc, dt);
        w[q] = (uint32_t)(cd[0] & 0xFF) | (uint32_t)(cd[1] & 0xFF) << 8 | (uint32_t)(cd[2] & 0xFF) << 16 |
               (uint32_t)cd[3] << 24;
      }
    };
    if (es >= -121) quant(std::false_type{});
    else quant(std::true_type{});
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      uint32_t acc = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = xv[q * 4 + j];
        if (flush) v = v * 0.0f;
        const int cd = nanblk ? 0 : (int)round_code(v, es, mbits, kRoundNearest, dt);
        acc |= (uint32_t)(cd & 0xFF) << (8 * j);
      }
      w[q] = acc;
    }
  }
  int8_t* dst = a.tb_major ? a.codes_t + ((m * a.nb + blk) * a.C + c) * 32 : a.codes_t + (m * a.C + c) * a.rpad + r0;
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[0] = make_uint4(w[0], w[1], w[2], w[3]);
  d4[1] = make_uint4(w[4], w[5], w[6], w[7]);
  a.scale[(m * a.nb + blk) * a.C + c] = exp_to16(nanblk ? kExpNaN : es - (mbits - 2));
}

}  // namespace mxa
