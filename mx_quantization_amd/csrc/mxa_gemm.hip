// Launches of the block-scaled MX GEMM (mxa_gemm.hpp) and the mx.Linear entry point of
// include/mxa.h (mxa_linear: x -> MX codes along in_features -> GEMM with a prepared weight).
#include <algorithm>

#include "mxa_gemm.hpp"
#include "mxa_launch.hpp"

namespace mxa {

int gemm_smax(int nbk) {
  int s = -1;
  while ((int64_t)nbk * 516128 * ((int64_t)1 << (s + 1)) < ((int64_t)1 << 31)) ++s;
  return s;
}

// The launch on one tile shape (mxa_gemm.hpp GemmShape<SH>); ga.smax is set.  A prepared
// weight's digit kernel launches from here too, behind the shape's refusal tests: a Linear
// the tile kernel would refuse is refused whichever kernel would run it.
template <bool PLAIN, int SH>
static int launch_gemm_shape(const GemmArgs& ga, int64_t batch, hipStream_t stream, bool bits4) {
  using S = GemmShape<SH>;
  const size_t lds = gemm_lds(ga.nbk, SH).total;
  const int64_t gx = (ga.Nc + S::CW - 1) / S::CW, gy = (ga.M + S::RW - 1) / S::RW;
  if (lds > 160 * 1024 || gy > 65535) return MXA_ERR_UNSUPPORTED;
  if (ga.bpd && batch == 1 && ga.nbk <= (bits4 ? kGemmDig4NbkMax : kGemmDigNbkMax)) {
    // a prepared weight: the exponent-folded digits, every row block in the one launch (a
    // block the digits cannot take sums its K-blocks in fp64 in the same workgroup); an
    // MXINT4 weight (its header's width) on the one-digit kernel
    const size_t dl = gemm_dig_lds(ga.nbk, bits4 ? 1 : 2).total;
    const void* dk = bits4 ? reinterpret_cast<const void*>(&mx_gemm_dig4_kernel<PLAIN>)
                              : reinterpret_cast<const void*>(&mx_gemm_dig_kernel<PLAIN>);
    if (hipFuncSetAttribute(dk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dl) != hipSuccess) return MXA_ERR_LAUNCH;
    const dim3 grid((unsigned)((ga.M + 31) / 32));
    if (bits4) hipLaunchKernelGGL(mx_gemm_dig4_kernel<PLAIN>, grid, dim3(256), dl, stream, ga);
    else hipLaunchKernelGGL(mx_gemm_dig_kernel<PLAIN>, grid, dim3(256), dl, stream, ga);
    return launch_status();
  }
  const void* gk = reinterpret_cast<const void*>(&mx_gemm_kernel<PLAIN, SH>);
  if (hipFuncSetAttribute(gk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return MXA_ERR_LAUNCH;
  // grid.z <= 65535: larger batches in slices; a wave whose spreads the int32 sums cannot
  // take sums its blocks in fp64 itself (gemm_tile's run_f64): one launch per slice
  const int64_t esz = (ga.linear || ga.dt == kF32) ? 4 : 2;
  for (int64_t b0 = 0; b0 < batch; b0 += 65535) {
    GemmArgs gs = ga;
    gs.a += b0 * ga.a_bat; gs.ae += b0 * ga.ae_bat; gs.b += b0 * ga.b_bat; gs.be += b0 * ga.be_bat;
    gs.c = static_cast<unsigned char*>(ga.c) + b0 * ga.c_bat * esz;
    const int64_t nb = std::min<int64_t>(65535, batch - b0);
    hipLaunchKernelGGL((mx_gemm_kernel<PLAIN, SH>), dim3((unsigned)gx, (unsigned)gy, (unsigned)nb), dim3(256), lds, stream, gs);
    if (launch_status() != MXA_OK) return MXA_ERR_LAUNCH;
  }
  return MXA_OK;
}

// the tile shape: products of <= 64 columns on 128 x 64 tiles; float32 products of 65..256
// contiguous columns on 32-row strips of whole rows (the strip stages float32 rows: only the
// PLAIN instantiation has it); else 64 x 128
template <bool PLAIN>
static int launch_gemm_p(const GemmArgs& ga0, int64_t batch, hipStream_t stream, bool bits4) {
  GemmArgs ga = ga0;
  ga.smax = gemm_smax(ga.nbk);
  if (ga.Nc <= GemmShape<kGemmTall>::CW) return launch_gemm_shape<PLAIN, kGemmTall>(ga, batch, stream, bits4);
  if constexpr (PLAIN)
    if (ga.Nc <= GemmShape<kGemmWide>::CW && ga.ldc == ga.Nc) return launch_gemm_shape<true, kGemmWide>(ga, batch, stream, bits4);
  return launch_gemm_shape<PLAIN, kGemmSquare>(ga, batch, stream, bits4);
}

int launch_gemm(const GemmArgs& ga, int64_t batch, hipStream_t stream, bool bits4) {
  if (ga.M <= 0 || ga.Nc <= 0 || ga.nbk <= 0 || batch <= 0) return MXA_ERR_ARG;
  const bool plain = (ga.bfloat == 0 || ga.bfloat == 32) && (ga.linear ? ga.autocast == 0 : ga.dt == kF32);
  return plain ? launch_gemm_p<true>(ga, batch, stream, bits4) : launch_gemm_p<false>(ga, batch, stream, bits4);
}

// The GemmArgs of an mx.Linear on MX rows (rows_prep layout: codes [rows][Cpad] or MFMA-ready,
// exponents [rows][nbk]) with a prepared weight (its row-major codes / exponents; its
// MFMA-ready codes and digits where its column blocks are the output columns)
GemmArgs linear_gemm_args(const int8_t* xc, const int16_t* xs, int64_t rows, int in_f, const void* wq, int out_f,
                          const float* bias, float* out, int64_t out_row_stride, int bfloat, int autocast, bool x_mfma,
                          bool* bits4) {
  const LinearLayout W = linear_layout(out_f, in_f, out_f);  // raw regions do not depend on gw
  const unsigned char* wb = static_cast<const unsigned char*>(wq);
  GemmArgs g{};
  g.a = xc; g.ae = xs; g.lda = W.Cpad; g.a_mfma = x_mfma ? 1 : 0;
  g.b = reinterpret_cast<const int8_t*>(wb + W.rawc); g.ldb = W.Cpad;
  g.be = reinterpret_cast<const int16_t*>(wb + W.rawe); g.be_n = W.nbk; g.be_k = 1;
  g.M = (int)rows; g.Nc = out_f; g.nbk = W.nbk;
  // the MFMA-ready codes when the buffer's column blocks are the output columns (one group,
  // or groups of a multiple of 32 columns): its header's group width decides
  LinearWeightHeader h{};
  const bool known = linear_weight_known_header(wq, &h);
  if (bits4) *bits4 = known && h.elem_bits == 4;
  if (known && (h.gw == out_f || h.gw % 32 == 0)) {
    const LinearLayout P = linear_layout(out_f, in_f, h.gw, h.elem_bits);
    g.bpk = reinterpret_cast<const int8_t*>(wb + P.pk);
    g.b_nb32 = P.G * P.NB32;
    g.bpd = reinterpret_cast<const int8_t*>(wb + P.pd);
    g.bps = reinterpret_cast<const int16_t*>(wb + P.ps);
    g.bpn = reinterpret_cast<const int16_t*>(wb + P.pn);
    g.bgs = reinterpret_cast<const int16_t*>(wb + P.gs);
    g.bG = P.G;
  }
  g.linear = 1; g.dt = kF32; g.bfloat = bfloat; g.autocast = autocast; g.bias = bias;
  g.c = out; g.ldc = out_row_stride;
  return g;
}

// GEMM of MX rows with a prepared Linear weight: out = mx.Linear epilogue
int launch_linear_codes(const int8_t* xc, const int16_t* xs, int64_t rows, int in_f, const void* wq, int out_f,
                        const float* bias, float* out, int64_t out_row_stride, int bfloat, int autocast,
                        hipStream_t stream, bool x_mfma) {
  if (rows > ((int64_t)1 << 31) - 1) return MXA_ERR_UNSUPPORTED;
  bool bits4 = false;
  const GemmArgs ga =
      linear_gemm_args(xc, xs, rows, in_f, wq, out_f, bias, out, out_row_stride, bfloat, autocast, x_mfma, &bits4);
  return launch_gemm(ga, 1, stream, bits4);
}

}  // namespace mxa

using namespace mxa;

extern "C" int64_t mxa_linear_workspace_bytes(int64_t rows, int32_t in_features, int32_t out_features) {
  if (rows <= 0 || in_features <= 0 || out_features <= 0 || rows > INT32_MAX) return -1;
  Carver ws;
  carve_mx_rows(ws, rows, in_features, true);  // x as MFMA-ready codes + exponents: the whole workspace
  return ws.off;
}

extern "C" int mxa_linear(const float* x, int64_t rows, int32_t in_features, int64_t x_row_stride, const void* wq,
                          int32_t out_features, const float* bias, float* out, int64_t out_row_stride,
                          int32_t flush_subnormals, int32_t bfloat, int32_t autocast_dtype, void* workspace,
                          int64_t workspace_bytes, hipStream_t stream) {
  if (!x || !wq || !out || rows <= 0 || in_features <= 0 || out_features <= 0 || x_row_stride < in_features ||
      out_row_stride < out_features)
    return MXA_ERR_ARG;
  if (!valid_bfloat(bfloat)) return MXA_ERR_ARG;
  if (autocast_dtype != 0 && autocast_dtype != MXA_DT_F16 && autocast_dtype != MXA_DT_BF16) return MXA_ERR_ARG;
  int bits = 0;  // the weight's element width (its header's): x is quantized at the same
  if (!linear_weight_verify_any_group(wq, out_features, in_features, flush_subnormals, bfloat, stream, &bits))
    return MXA_ERR_ARG;
  const int64_t need = mxa_linear_workspace_bytes(rows, in_features, out_features);
  if (!workspace || workspace_bytes < need || !aligned16(workspace)) return MXA_ERR_WORKSPACE;
  Carver ws(workspace);
  const MxRows xr = carve_mx_rows(ws, rows, in_features, true);
  int rc = launch_rows_prep(
      flat_rows_prep(x, rows, in_features, x_row_stride, flush_subnormals, bfloat, xr.codes, xr.exps, 1, bits), stream);
  if (rc) return rc;
  return launch_linear_codes(xr.codes, xr.exps, rows, in_features, wq, out_features, bias, out, out_row_stride, bfloat,
                             autocast_dtype, stream, true);
}
