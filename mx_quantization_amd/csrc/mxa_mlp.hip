// The MLP entry point of include/mxa.h (mxa_mlp): fc1 -> GELU -> fc2, the hidden matrix kept
// as fc2's MX input codes.  fc1 on the digit kernel's body with the quantizing epilogue
// (mxa_mlp.hpp); an fc1 the digit kernel does not take runs as mxa_linear into an fp32
// workspace and is quantized by rows_prep with the activation applied on load
// (RowsPrepArgs::act) -- the same GELU, the same block quantizer, the same bits.
#include "mxa_launch.hpp"
#include "mxa_mlp.hpp"

namespace mxa {

// does fc1 run on the digit kernel's body?  The weight's digits cover the output columns
// (one group, or groups of a multiple of 32 columns: linear_gemm_args) and the K-blocks fit
// the LDS next to the staging tiles.  A weight whose header this process has not seen yet
// counts as not: the fallback's workspace covers both paths.
static bool mlp_fc1_fused(const void* w1, int in_f, int hidden) {
  LinearWeightHeader h{};
  if (!w1 || !linear_weight_known_header(w1, &h) || h.out_f != hidden || h.in_f != in_f) return false;
  return (h.gw == hidden || h.gw % 32 == 0) && (in_f + 31) / 32 <= (h.elem_bits == 4 ? kMlp4NbkMax : kMlpNbkMax);
}

// the workspace: x and the hidden matrix as MX rows the way mxa_linear lays its input out
// (MFMA-ready codes, then exponents), then the unfused fallback's fp32 hidden matrix
struct MlpLayout { MxRows x, h; float* hf; };
static MlpLayout mlp_layout(Carver& ws, int64_t rows, int in_f, int hidden, bool fused) {
  MlpLayout L{};
  L.x = carve_mx_rows(ws, rows, in_f, true);
  L.h = carve_mx_rows(ws, rows, hidden, true);
  L.hf = ws.take<float>(fused ? 0 : rows * hidden);
  return L;
}

template <bool PLAIN>
static int launch_mlp_fc1(const GemmArgs& ga, const MlpEpi<PLAIN>& e, bool bits4, hipStream_t stream) {
  const MlpEpi<PLAIN, true> e4{e.codes, e.exps, e.pre_out, e.act_out, e.nbh, e.act, e.flush};
  const size_t lds = gemm_dig_lds(ga.nbk, bits4 ? 1 : 2).total + kMlpStageBytes;
  const void* k = bits4 ? reinterpret_cast<const void*>(&mx_mlp_fc1_4_kernel<PLAIN>)
                           : reinterpret_cast<const void*>(&mx_mlp_fc1_kernel<PLAIN>);
  if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return MXA_ERR_LAUNCH;
  const dim3 grid((unsigned)((ga.M + 31) / 32));
  if (bits4) hipLaunchKernelGGL(mx_mlp_fc1_4_kernel<PLAIN>, grid, dim3(256), lds, stream, ga, e4);
  else hipLaunchKernelGGL(mx_mlp_fc1_kernel<PLAIN>, grid, dim3(256), lds, stream, ga, e);
  return launch_status();
}

}  // namespace mxa

using namespace mxa;

extern "C" int64_t mxa_mlp_workspace_bytes(int64_t rows, int32_t in_features, const void* w1, int32_t hidden_features,
                                           int32_t out_features) {
  if (rows <= 0 || in_features <= 0 || hidden_features <= 0 || out_features <= 0 || rows > INT32_MAX) return -1;
  Carver ws;
  mlp_layout(ws, rows, in_features, hidden_features, mlp_fc1_fused(w1, in_features, hidden_features));
  return ws.off;
}

extern "C" int mxa_mlp(const float* x, int64_t rows, int32_t in_features, int64_t x_row_stride, const void* w1,
                       int32_t hidden_features, const float* b1, int32_t act, const void* w2, int32_t out_features,
                       const float* b2, float* y, int64_t y_row_stride, float* pre_out, float* act_out,
                       int32_t flush_subnormals, int32_t bfloat, void* workspace, int64_t workspace_bytes,
                       hipStream_t stream) {
  if (!x || !w1 || !w2 || !y || rows <= 0 || rows > INT32_MAX || in_features <= 0 || hidden_features <= 0 ||
      out_features <= 0 || x_row_stride < in_features || y_row_stride < out_features)
    return MXA_ERR_ARG;
  if (act != MXA_ACT_GELU && act != MXA_ACT_GELU_TANH) return MXA_ERR_ARG;
  if (!valid_bfloat(bfloat)) return MXA_ERR_ARG;
  int bits = 0, bits2 = 0;  // the weights' element width (their headers'): one for the whole chain
  if (!linear_weight_verify_any_group(w1, hidden_features, in_features, flush_subnormals, bfloat, stream, &bits) ||
      !linear_weight_verify_any_group(w2, out_features, hidden_features, flush_subnormals, bfloat, stream, &bits2) ||
      bits != bits2)
    return MXA_ERR_ARG;
  const bool fused = mlp_fc1_fused(w1, in_features, hidden_features);
  const int64_t need = mxa_mlp_workspace_bytes(rows, in_features, w1, hidden_features, out_features);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) return MXA_ERR_WORKSPACE;
  // (a Linear the tile kernel would refuse is refused whichever kernel would run it: launch_gemm_shape)
  if ((rows + 63) / 64 > 65535) return MXA_ERR_UNSUPPORTED;

  Carver ws(workspace);
  const MlpLayout L = mlp_layout(ws, rows, in_features, hidden_features, fused);
  int8_t *xc = L.x.codes, *hc = L.h.codes;
  int16_t *xe = L.x.exps, *he = L.h.exps;
  float* hf = L.hf;  // the unfused fallback's fp32 hidden matrix

  const RowsPrepArgs rx = flat_rows_prep(x, rows, in_features, x_row_stride, flush_subnormals, bfloat, xc, xe, 1, bits);
  int rc = launch_rows_prep(rx, stream);
  if (rc) return rc;
  if (fused) {
    const GemmArgs ga = linear_gemm_args(xc, xe, rows, in_features, w1, hidden_features, b1, nullptr, hidden_features,
                                         bfloat, 0, true);
    if (!ga.bpd) return MXA_ERR_ARG;  // (mlp_fc1_fused read the same header)
    const int nbh = (hidden_features + 31) / 32;
    if (bfloat == 0 || bfloat == 32)
      rc = launch_mlp_fc1<true>(ga, MlpEpi<true>{hc, he, pre_out, act_out, nbh, act, flush_subnormals}, bits == 4, stream);
    else
      rc = launch_mlp_fc1<false>(ga, MlpEpi<false>{hc, he, pre_out, act_out, nbh, act, flush_subnormals}, bits == 4, stream);
    if (rc) return rc;
  } else {
    rc = launch_linear_codes(xc, xe, rows, in_features, w1, hidden_features, b1, hf, hidden_features, bfloat, 0, stream,
                             true);
    if (rc) return rc;
    const int64_t n = rows * hidden_features;
    if (pre_out && hipMemcpyAsync(pre_out, hf, (size_t)n * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess)
      return MXA_ERR_LAUNCH;
    if (act_out) {
      hipLaunchKernelGGL(mlp_act_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 65536)), dim3(256), 0, stream,
                         hf, act_out, n, act);
      if (launch_status() != MXA_OK) return MXA_ERR_LAUNCH;
    }
    RowsPrepArgs rh = flat_rows_prep(hf, rows, hidden_features, hidden_features, flush_subnormals, bfloat, hc, he, 1, bits);
    rh.act = 1 + act;
    rc = launch_rows_prep(rh, stream);
    if (rc) return rc;
  }
  return launch_linear_codes(hc, he, rows, hidden_features, w2, out_features, b2, y, y_row_stride, bfloat, 0, stream,
                             true);
}
