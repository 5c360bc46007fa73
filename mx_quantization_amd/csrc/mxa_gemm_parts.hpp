// What the three MX GEMM kernels share -- gemm_tile and mx_gemm_dig_kernel (mxa_gemm.hpp),
// proj_block (mxa_proj.hpp): the rules that must stay in lock-step with the reference, one
// definition each.
#pragma once
#include "mxa_proj_args.hpp"

namespace mxa {

typedef int v16i __attribute__((ext_vector_type(16)));  // (as mxa_finish.hpp)
typedef int v4i_ __attribute__((ext_vector_type(4)));

// wave max / min of ints within +-2^20 (block exponents, their sums), as biased uint32
__device__ __forceinline__ int wave_max_e(int v) { return (int)wave_max_u32((uint32_t)(v + (1 << 20))) - (1 << 20); }
__device__ __forceinline__ int wave_min_e(int v) { return (int)wave_min_u32((uint32_t)(v + (1 << 20))) - (1 << 20); }

// are the 32 codes of a block (its two 16-B halves) all zero?
__device__ __forceinline__ bool codes32_zero(const uint4& lo16, const uint4& hi16) {
  return ((lo16.x | lo16.y | lo16.z | lo16.w) | (hi16.x | hi16.y | hi16.z | hi16.w)) == 0u;
}

// The mx.Linear output rule, microxscaling/mx/linear.py:83-101 (not the PLAIN kernels:
// bfloat 0 / 32 and no autocast leave o + bias):
//   out = bf(round_dt(fl32(sum), autocast))   F.linear returns the autocast dtype, and
//                                             quantize_elemwise_op rounds in that dtype
//   out = bf(out + bf(bias))                  the float32 bias promotes back to float32
// sum: the fp32 rounding of the exact product; bb: the already rounded bias bf(bias).
__device__ __forceinline__ float linear_out(float sum, float bb, bool has_bias, int bfloat, int autocast) {
  float o = round_bfloat(round_dt(sum, autocast), bfloat, kRoundNearest, 1, autocast);
  if (has_bias) o = round_bfloat(o + bb, bfloat, kRoundNearest, 1);
  return o;
}

// 16 codes times 2^s (0 <= s <= kDigitSpread) as two signed base-256 digits:
// c * 2^s = d0 + 256 d1, d0 in [-128, 127], |d1| <= 127
__device__ __forceinline__ void fold_digits16(const uint4& v, int s, uint4& d0, uint4& d1) {
  const uint32_t in[4] = {v.x, v.y, v.z, v.w};
  uint32_t o0[4], o1[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t p0 = 0, p1 = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int c = (int)(int8_t)(in[w] >> (8 * b));
      const int f = c << s;
      const int lo = (int)(int8_t)f;
      p0 |= ((uint32_t)lo & 0xFFu) << (8 * b);
      p1 |= ((uint32_t)((f - lo) >> 8) & 0xFFu) << (8 * b);
    }
    o0[w] = p0;
    o1[w] = p1;
  }
  d0 = make_uint4(o0[0], o0[1], o0[2], o0[3]);
  d1 = make_uint4(o1[0], o1[1], o1[2], o1[3]);
}

// The K loop over exponent-folded digits: both operands' codes times 2^(block exponent -
// the row's / column's smallest) as two signed base-256 digits (fold_digits16), so every
// block's scale is already in the operands: the four digit products accumulate in the
// MFMA's own int32 accumulators over all K-blocks (lo x lo; lo x hi + hi x lo; hi x hi:
// |sum| <= 2 nbk 32 128^2 < 2^31) with no VALU per block.
// wdig(kb, digit): the lane's 16 B of the weight's digit chunk of K-block kb, loaded four
// blocks ahead (slot = block mod 4, reloaded right after its use); a_lo / a_hi: the lane's
// 16 B of the rows' low / high digits of block 0 in LDS, astep bytes from block to block.
struct DigitSums {
  v16i c0, c1, c2;  // lo x lo; lo x hi + hi x lo; hi x hi
};
template <class WDig>
__device__ __forceinline__ DigitSums digit_k_loop(WDig&& wdig, const int8_t* a_lo, const int8_t* a_hi, int astep, int nbk) {
  v16i c0 = {}, c1 = {}, c2 = {};
  const int last = nbk - 1;
  auto cl = [&](int kb) { return min(kb, last); };
  v4i_ L0 = wdig(0, 0), H0 = wdig(0, 1), L1 = wdig(cl(1), 0), H1 = wdig(cl(1), 1);
  v4i_ L2 = wdig(cl(2), 0), H2 = wdig(cl(2), 1), L3 = wdig(cl(3), 0), H3 = wdig(cl(3), 1);
  auto step = [&](int kb, v4i_& Ls, v4i_& Hs) {
    const v4i_ al = *reinterpret_cast<const v4i_*>(a_lo + astep * kb);
    const v4i_ ah = *reinterpret_cast<const v4i_*>(a_hi + astep * kb);
    c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, Ls, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(al, Hs, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, Hs, c2, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(ah, Ls, c1, 0, 0, 0);
    Ls = wdig(cl(kb + 4), 0);
    Hs = wdig(cl(kb + 4), 1);
    __builtin_amdgcn_sched_barrier(0);  // reload each slot right after its use
  };
  int kb = 0;
  for (; kb + 4 <= nbk; kb += 4) {
    step(kb, L0, H0);
    step(kb + 1, L1, H1);
    step(kb + 2, L2, H2);
    step(kb + 3, L3, H3);
  }
  if (kb < nbk) step(kb, L0, H0);
  if (kb + 1 < nbk) step(kb + 1, L1, H1);
  if (kb + 2 < nbk) step(kb + 2, L2, H2);
  return {c0, c1, c2};
}
// the digit sums' value c0 + 2^8 c1 + 2^16 c2 (exact in fp64) times 2^e, rounded once
__device__ __forceinline__ float digits_to_f32(int c0, int c1, int c2, int e) {
  return (float)ldexp((double)c0 + 256.0 * (double)c1 + 65536.0 * (double)c2, e);
}

// ---- MXINT4: one digit ---------------------------------------------------------------
// 16 int4 codes (|c| <= 7) times 2^s (0 <= s <= kDigit4Spread): |c * 2^s| <= 112, one signed
// int8 each
__device__ __forceinline__ uint4 fold_digit16(const uint4& v, int s) {
  const uint32_t in[4] = {v.x, v.y, v.z, v.w};
  uint32_t o[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    uint32_t p = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) p |= ((uint32_t)((int)(int8_t)(in[w] >> (8 * b)) << s) & 0xFFu) << (8 * b);
    o[w] = p;
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// digit_k_loop for one-digit operands: one MFMA per K-block into one accumulator (|sum| <=
// nbk 32 112^2 < 2^31 for nbk <= 5,349).  wdig(kb): the lane's 16 B of the weight's digit
// chunk of K-block kb, loaded four blocks ahead as above; a_d: the lane's 16 B of the rows'
// digits of block 0 in LDS, astep bytes from block to block.
template <class WDig>
__device__ __forceinline__ v16i digit4_k_loop(WDig&& wdig, const int8_t* a_d, int astep, int nbk) {
  v16i c = {};
  const int last = nbk - 1;
  auto cl = [&](int kb) { return min(kb, last); };
  v4i_ W0 = wdig(0), W1 = wdig(cl(1)), W2 = wdig(cl(2)), W3 = wdig(cl(3));
  auto step = [&](int kb, v4i_& Ws) {
    const v4i_ ad = *reinterpret_cast<const v4i_*>(a_d + astep * kb);
    c = __builtin_amdgcn_mfma_i32_32x32x32_i8(ad, Ws, c, 0, 0, 0);
    Ws = wdig(cl(kb + 4));
    __builtin_amdgcn_sched_barrier(0);  // reload each slot right after its use
  };
  int kb = 0;
  for (; kb + 4 <= nbk; kb += 4) {
    step(kb, W0);
    step(kb + 1, W1);
    step(kb + 2, W2);
    step(kb + 3, W3);
  }
  if (kb < nbk) step(kb, W0);
  if (kb + 1 < nbk) step(kb + 1, W1);
  if (kb + 2 < nbk) step(kb + 2, W2);
  return c;
}

}  // namespace mxa
