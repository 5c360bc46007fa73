// The MLP's activation between fc1 and fc2 (include/mxa.h MXA_ACT_*): nn.GELU in float32, as
// the patched blocks run it on the fc1 mx.Linear's output (workloads/DiT/models.py:286-287,
// timm's Mlp in workloads/deit/models_v2.py:55).  One definition for the fused fc1 epilogue
// (mxa_mlp.hpp) and the row quantizer's load (rows_prep_act_kernel), so the two paths give
// the same bits.  Built with -ffp-contract=off: every operation below rounds on its own, in
// the order written; erff / tanhf are the device math library's (no fast-math variants).
//   MXA_ACT_GELU       0.5 h (1 + erf(h / sqrt 2))
//   MXA_ACT_GELU_TANH  0.5 h (1 + tanh(sqrt(2 / pi) (h + 0.044715 h^3)))   (torch's tanh form)
// NaN gives NaN.  The result for h = +-inf is not pinned (here -inf gives inf * 0 = NaN in
// the last product; torch's own CPU kernel returns NaN for gelu(+inf) in the erf form).
#pragma once
#include "mxa_common.hpp"

namespace mxa {

constexpr int kActNone = 0;  // RowsPrepArgs::act: 0 none, else 1 + MXA_ACT_*

__device__ __forceinline__ float gelu_erf(float h) {
  return 0.5f * h * (1.0f + erff(h * 0.70710678118654752440f));
}
__device__ __forceinline__ float gelu_tanh(float h) {
  const float inner = 0.79788456080286535588f * (h + 0.044715f * (h * h * h));
  return 0.5f * h * (1.0f + tanhf(inner));
}
// act: MXA_ACT_GELU or MXA_ACT_GELU_TANH (the entry point checked it)
__device__ __forceinline__ float mlp_act(float h, int act) { return act == MXA_ACT_GELU_TANH ? gelu_tanh(h) : gelu_erf(h); }

}  // namespace mxa
