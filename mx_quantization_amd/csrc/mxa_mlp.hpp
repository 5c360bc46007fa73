// fc1 of the fused MLP (include/mxa.h mxa_mlp): mx_gemm_dig_kernel's body (mxa_gemm.hpp
// gemm_dig_block: the digit K loop, the per-block gate, the fp64 block sums) with another
// epilogue.  Where the Linear stores a wave's 32 x 32 fp32 tile, this one takes the tile
// after linear_out, applies the activation (mxa_act.hpp) and quantizes every row's 32
// values -- one MX block of fc2's input row, hidden block cb -- with rows_prep's own block
// body (xo_block, as the finishing kernels do for the proj Linear): the 1-KB chunk (row
// block, hidden block) of fc2's MFMA-ready A operand and the 32 block exponents.  The fp32
// hidden matrix never reaches HBM (pre_out / act_out: the tests' copies of it).
//   * hidden columns >= hidden_features (the last block): value 0 -- no part in the block
//     maximum, code 0 -- as rows_prep loads them;
//   * rows beyond `rows` of the last row block: not written, as rows_prep leaves them;
//   * a NaN row or weight column: NaN values, so the block's exponent is the NaN marker.
// LDS: per wave an 8 x 33 float staging tile behind gemm_dig_lds(nbk) (the transposition from
// the MFMA's column-per-lane tile to the quantizer's two lanes per row, eight rows at a time:
// a 32-row tile per wave would cost a resident workgroup per CU at both workload shapes).
#pragma once
#include "mxa_act.hpp"
#include "mxa_finish.hpp"
#include "mxa_gemm.hpp"

namespace mxa {

constexpr size_t kMlpStageBytes = 4 * 8 * 33 * 4;  // four waves' staging tiles
// gemm_dig_lds(nbk).total + kMlpStageBytes <= 160 KB for every K the digit kernel takes; at the
// workloads' 24 and 36 K-blocks three and two workgroups per CU, as mx_gemm_dig_kernel has
constexpr int kMlpNbkMax = kGemmDigNbkMax;
static_assert((size_t)kMlpNbkMax * 2048 + 400 + kMlpStageBytes <= 160 * 1024, "LDS");
// MXINT4 weights (the one-digit body, 1 KB per K-block): the same bytes at twice the K
constexpr int kMlp4NbkMax = kGemmDig4NbkMax;
static_assert((size_t)kMlp4NbkMax * 1024 + 400 + kMlpStageBytes <= 160 * 1024, "LDS");

// B4: fc2's input codes are MXINT4 (the block body's op / sA outputs: codes in [-7, 7], es - 2)
template <bool PLAIN, bool B4 = false>
struct MlpEpi {
  int8_t* codes;   // fc2's A operand, MFMA-ready: [ceil(rows / 32)][nbh][64 lanes][16 B]
  int16_t* exps;   // [rows][nbh] exponent of a code unit
  float* pre_out;  // optional (rows, hidden) fc1 output
  float* act_out;  // optional (rows, hidden) activation output
  int nbh;         // ceil(hidden / 32)
  int act, flush;  // MXA_ACT_*; fc2's input rule (flush_subnormals; bfloat: GemmArgs::bfloat)
  // (PLAIN: GemmArgs::bfloat 0 / 32 -- fc1's epilogue is o + bias)

  template <class V>
  __device__ __forceinline__ void operator()(const GemmArgs& a, int cb, int m0g, int rows, const int* rn,
                                             unsigned char* ext, V&& value) const {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ln = lane & 31, m0 = 4 * (lane >> 5);
    const int n = 32 * cb + ln, nc = min(n, a.Nc - 1);
    const bool nv = n < a.Nc;
    const bool cnan = a.bpn[nc] != 0;
    const float bb = a.bias ? (PLAIN ? a.bias[nc] : round_bfloat(a.bias[nc], a.bfloat, kRoundNearest, 1)) : 0.0f;
    float* ot = reinterpret_cast<float*>(ext) + wave * (8 * 33);
    const int row = lane >> 1, sub = lane & 1;
    float xv[16];
    // eight rows at a time (the lane's elements 4 p .. 4 p + 3: rows 8 p + m0 + 0..3); the 16
    // lanes whose row is one of them pick up their 16 values
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * p + r, m = 8 * p + m0 + r;
        float g = 0.0f;
        if (m < rows && nv) {
          float o = (cnan || rn[m]) ? __uint_as_float(0x7FC00000u) : value(i, m);
          if constexpr (PLAIN) o = a.bias ? o + bb : o;
          else o = linear_out(o, bb, a.bias != nullptr, a.bfloat, 0);
          g = mlp_act(o, act);
          const int64_t off = (int64_t)(m0g + m) * a.Nc + n;
          if (pre_out) pre_out[off] = o;
          if (act_out) act_out[off] = g;
        }
        ot[(m0 + r) * 33 + ln] = g;
      }
      wave_lds_sync();
      if ((lane >> 4) == p) {
#pragma unroll
        for (int j = 0; j < 16; ++j) xv[j] = ot[(row & 7) * 33 + 16 * sub + j];
      }
      wave_lds_sync();
    }
    RowsPrepArgs ro = xo_rows_args(codes, exps, a.Nc, nbh, flush, a.bfloat);
    if constexpr (B4) {
      ro.op_kind = MXA_OP_MXINT4;
      ro.codes = nullptr; ro.sT = nullptr; ro.op = codes; ro.sA = exps;
    }
    xo_block(ro, m0g + (row < rows ? row : 0), cb, sub, 32 * cb + 16 * sub, xv, row < rows);
  }
};

template <bool PLAIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) void mx_mlp_fc1_kernel(GemmArgs a, MlpEpi<PLAIN> e) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  gemm_dig_block<PLAIN>(a, e, smem);
}
// MXINT4 weights and rows: the one-digit body, fc2's codes written as MXINT4
template <bool PLAIN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) void mx_mlp_fc1_4_kernel(GemmArgs a, MlpEpi<PLAIN, true> e) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  gemm_dig_block<PLAIN, MlpEpi<PLAIN, true>, 1>(a, e, smem);
}

// the activation alone, elementwise (the fallback's act_out: the tests' copy)
__global__ __launch_bounds__(256) void mlp_act_kernel(const float* __restrict__ pre, float* __restrict__ out, int64_t n, int act) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) out[t] = mlp_act(pre[t], act);
}

}  // namespace mxa
