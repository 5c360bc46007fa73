// The fused qkv projection's launches (mxa_proj.hpp) and the Linear weight preparation
// entry points of include/mxa.h.
#include <algorithm>
#include <mutex>
#include <unordered_map>

#include "mxa_proj_launch.hpp"

namespace mxa {

// one thread per (padded column, K-block): the MFMA-ready codes and the exponents
__global__ __launch_bounds__(256) void linear_pack_kernel(const int8_t* rawc, const int16_t* rawe, int out_f, int gw,
                                                          int NB32, int nbk, int Cpad, int64_t pcols, int8_t* pk,
                                                          int16_t* pe) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pcols * nbk) return;
  const int64_t pc = t / nbk;
  const int kb = (int)(t - pc * nbk);
  const int64_t blkc = pc / 32;  // group * NB32 + cb
  const int n = (int)(pc - blkc * 32);
  const int64_t g = blkc / NB32;
  const int cb = (int)(blkc - g * NB32);
  const int gc = 32 * cb + n;
  const bool real = gc < gw;
  const int64_t col = g * gw + gc;
  uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
  int16_t e = 0;
  if (real) {
    lo = *reinterpret_cast<const uint4*>(rawc + col * Cpad + 32 * kb);
    hi = *reinterpret_cast<const uint4*>(rawc + col * Cpad + 32 * kb + 16);
    e = rawe[col * nbk + kb];
  }
  int8_t* dst = pk + ((blkc * nbk + kb) * 64) * 16;
  *reinterpret_cast<uint4*>(dst + n * 16) = lo;
  *reinterpret_cast<uint4*>(dst + (n + 32) * 16) = hi;
  pe[pc * nbk + kb] = e;
}

// per padded column: smallest finite block exponent and the spread, the NaN flag
__global__ __launch_bounds__(256) void linear_stats_kernel(const int16_t* pe, int64_t pcols, int nbk, int16_t* ps,
                                                           int16_t* pn) {
  const int64_t pc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pc >= pcols) return;
  int lo = 1 << 20, hi = -(1 << 20), nan = 0;
  for (int kb = 0; kb < nbk; ++kb) {
    const int e = exp_from16(pe[pc * nbk + kb]);
    if (e != kExpNaN) {
      lo = min(lo, e);
      hi = max(hi, e);
    } else {
      nan = 1;
    }
  }
  if (lo > hi) lo = hi = 0;
  ps[2 * pc] = (int16_t)lo;
  ps[2 * pc + 1] = (int16_t)(hi - lo);
  pn[pc] = (int16_t)nan;
}

// one thread per (padded column, K-block): the exponent-folded digits of the MFMA-ready
// codes (the column's two 16-B halves sit at lanes n and n + 32 of the block's 1-KB chunk)
__global__ __launch_bounds__(256) void linear_digits_kernel(const int8_t* pk, const int16_t* pe, const int16_t* ps,
                                                            int nbk, int64_t pcols, int8_t* pd) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pcols * nbk) return;
  const int64_t pc = t / nbk;
  const int kb = (int)(t - pc * nbk);
  const int64_t blkc = pc / 32;
  const int n = (int)(pc - blkc * 32);
  const int e = exp_from16(pe[pc * nbk + kb]);
  const int sp = ps[2 * pc + 1];
  const int s = e == kExpNaN ? 0 : e - ps[2 * pc];
  const bool ok = sp <= kDigitSpread;
  const int8_t* src = pk + ((blkc * nbk + kb) * 64) * 16;
  int8_t* dst = pd + ((blkc * nbk + kb) * 128) * 16;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    if (ok) fold_digits16(*reinterpret_cast<const uint4*>(src + (n + 32 * h) * 16), s, d0, d1);
    *reinterpret_cast<uint4*>(dst + (n + 32 * h) * 16) = d0;
    *reinterpret_cast<uint4*>(dst + (64 + n + 32 * h) * 16) = d1;
  }
}

// the same for an MXINT4 weight: one plane, [blkc][kb][lane][16 B] (mxa_gemm_parts.hpp fold_digit16)
__global__ __launch_bounds__(256) void linear_digit4_kernel(const int8_t* pk, const int16_t* pe, const int16_t* ps,
                                                            int nbk, int64_t pcols, int8_t* pd) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pcols * nbk) return;
  const int64_t pc = t / nbk;
  const int kb = (int)(t - pc * nbk);
  const int64_t blkc = pc / 32;
  const int n = (int)(pc - blkc * 32);
  const int e = exp_from16(pe[pc * nbk + kb]);
  const int s = e == kExpNaN ? 0 : e - ps[2 * pc];
  const bool ok = ps[2 * pc + 1] <= kDigit4Spread;
  const int64_t chunk = ((blkc * nbk + kb) * 64) * 16;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint4 v = *reinterpret_cast<const uint4*>(pk + chunk + (n + 32 * h) * 16);
    *reinterpret_cast<uint4*>(pd + chunk + (n + 32 * h) * 16) = ok ? fold_digit16(v, s) : make_uint4(0, 0, 0, 0);
  }
}

// per group of gw real columns: smallest column exponent, largest column spread
__global__ __launch_bounds__(64) void linear_group_stats_kernel(const int16_t* ps, int G, int NB32, int gw, int16_t* gs) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int lo = 1 << 20, sp = 0;
  for (int gc = 0; gc < gw; ++gc) {
    const int64_t pc = ((int64_t)g * NB32 + gc / 32) * 32 + gc % 32;
    lo = min(lo, (int)ps[2 * pc]);
    sp = max(sp, (int)ps[2 * pc + 1]);
  }
  gs[2 * g] = (int16_t)lo;
  gs[2 * g + 1] = (int16_t)sp;
}

// ---- fused qkv projection (mxa_proj.hpp) ------------------------------------------
// the operands' settings leave only the plain rounding (qkv_proj_kernel<NBD, true>)
static bool proj_plain(const ProjArgs& pa) {
  auto plain_bf = [](int bf) { return bf == 0 || bf == 32; };
  auto plain_rows = [&](const RowsPrepArgs& r) {
    return plain_bf(r.bfloat) && !r.flush && !r.zind && r.dt == kF32 &&
           (r.op_kind == MXA_OP_MXINT8 || (r.op_kind == MXA_OP_SIGN && !r.op));
  };
  return plain_bf(pa.bfloat) && pa.autocast == 0 && plain_rows(pa.rq) && plain_rows(pa.rk) && pa.cv.mbits == 8 &&
         !pa.cv.flush && plain_bf(pa.cv.bfloat) && pa.cv.dt == kF32;
}

template <int NBD, bool PLAIN>
static int launch_proj_nbd(const ProjArgs& pa, int part, hipStream_t stream) {
  switch (part) {
    case kPartQ: return launch_proj_kernel<cross_proj_kernel<NBD, PLAIN, kPartQ>, kPartQ, NBD>(pa, stream);
    case kPartKV: return launch_proj_kernel<cross_proj_kernel<NBD, PLAIN, kPartKV>, kPartKV, NBD>(pa, stream);
    default: return launch_proj_kernel<qkv_proj_kernel<NBD, PLAIN>, kPartQKV, NBD>(pa, stream);
  }
}

template <bool PLAIN>
static int launch_proj_p(const ProjArgs& pa, int part, hipStream_t stream) {
  switch ((pa.D + 31) / 32) {
    case 1: return launch_proj_nbd<1, PLAIN>(pa, part, stream);
    case 2: return launch_proj_nbd<2, PLAIN>(pa, part, stream);
    case 3: return launch_proj_nbd<3, PLAIN>(pa, part, stream);
    default: return launch_proj_nbd<4, PLAIN>(pa, part, stream);
  }
}

int launch_proj(const ProjArgs& pa, hipStream_t stream, int part) {
  return proj_plain(pa) ? launch_proj_p<true>(pa, part, stream) : launch_proj_p<false>(pa, part, stream);
}

__global__ void linear_header_kernel(LinearWeightHeader* h, LinearWeightHeader v) {
  if (threadIdx.x == 0) *h = v;
}

// prepared buffers whose header is known to the host (pointer -> header)
static std::mutex g_wmu;
static std::unordered_map<const void*, LinearWeightHeader> g_weights;

static void linear_weight_note(const void* wq, const LinearWeightHeader& h) {
  std::lock_guard<std::mutex> g(g_wmu);
  g_weights[wq] = h;
}

bool linear_weight_known_header(const void* wq, LinearWeightHeader* h) {
  std::lock_guard<std::mutex> g(g_wmu);
  auto it = g_weights.find(wq);
  if (it == g_weights.end()) return false;
  *h = it->second;
  return true;
}

// a buffer prepared elsewhere (another process, or copied): its header read from the device
// (a synchronisation: not under stream capture); the caller notes it once it has checked it
static bool linear_weight_fetch_header(const void* wq, hipStream_t stream, LinearWeightHeader* h) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
  if (hipMemcpyAsync(h, wq, sizeof(*h), hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
  return hipStreamSynchronize(stream) == hipSuccess;
}

// (a note that does not match may be that of a buffer since freed whose address this one has
// taken -- a framework's caching allocator hands addresses out again: the device's copy decides)
bool linear_weight_verify(const void* wq, const LinearWeightHeader& want, hipStream_t stream) {
  LinearWeightHeader h{};
  if (linear_weight_known_header(wq, &h) && h == want) return true;
  if (!linear_weight_fetch_header(wq, stream, &h) || !(h == want)) return false;
  linear_weight_note(wq, h);
  return true;
}

bool linear_weight_verify_any_group(const void* wq, int out_f, int in_f, int flush, int bfloat, hipStream_t stream,
                                    int* elem_bits) {
  LinearWeightHeader h{};
  auto fits = [&](const LinearWeightHeader& x) {
    return x == linear_weight_header(out_f, in_f, x.gw, flush, bfloat, elem_bits ? x.elem_bits : 0);
  };
  if (!(linear_weight_known_header(wq, &h) && fits(h))) {  // unknown, or a stale note (linear_weight_verify)
    if (!linear_weight_fetch_header(wq, stream, &h)) return false;
    if (h.magic != kLinearWeightMagic || h.gw <= 0 || h.out_f % h.gw || (h.elem_bits != 0 && h.elem_bits != 4))
      return false;
    if (!fits(h)) return false;
    linear_weight_note(wq, h);
  }
  if (elem_bits) *elem_bits = elem_bits ? h.elem_bits : 0;
  return true;
}

LinearWeightHeader linear_weight_header(int out_f, int in_f, int gw, int flush, int bfloat, int elem_bits) {
  LinearWeightHeader h{};
  h.magic = kLinearWeightMagic; h.version = 3;
  h.out_f = out_f; h.in_f = in_f; h.gw = gw; h.flush = flush ? 1 : 0; h.bfloat = bfloat; h.elem_bits = elem_bits;
  return h;
}

}  // namespace mxa

using namespace mxa;

static bool weight_shape_ok(int out_f, int in_f, int gw, int elem_bits) {
  return out_f > 0 && in_f > 0 && gw > 0 && out_f % gw == 0 && (elem_bits == 8 || elem_bits == 4);
}

extern "C" int64_t mxa_linear_weight_bytes_bits(int32_t out_features, int32_t in_features, int32_t group_width,
                                                int32_t elem_bits) {
  if (!weight_shape_ok(out_features, in_features, group_width, elem_bits)) return -1;
  return linear_layout(out_features, in_features, group_width, elem_bits == 4 ? 4 : 0).total;
}

extern "C" int64_t mxa_linear_weight_bytes(int32_t out_features, int32_t in_features, int32_t group_width) {
  return mxa_linear_weight_bytes_bits(out_features, in_features, group_width, 8);
}

extern "C" int mxa_linear_weight_prep_bits(const float* w, int32_t out_features, int32_t in_features,
                                           int32_t group_width, int32_t flush_subnormals, int32_t bfloat,
                                           int32_t elem_bits, void* wq, hipStream_t stream) {
  if (!w || !wq || !weight_shape_ok(out_features, in_features, group_width, elem_bits)) return MXA_ERR_ARG;
  if (!valid_bfloat(bfloat)) return MXA_ERR_ARG;
  if (!aligned16(wq)) return MXA_ERR_ARG;
  const int hbits = elem_bits == 4 ? 4 : 0;  // the header's field: an MXINT8 buffer keeps 0
  const LinearLayout W = linear_layout(out_features, in_features, group_width, hbits);
  unsigned char* wb = static_cast<unsigned char*>(wq);
  // (4 bits: rows_prep's MXINT4 operand -- codes in [-7, 7], exponents es - 2 -- into the raw regions)
  const RowsPrepArgs rw = flat_rows_prep(w, out_features, in_features, in_features,
                                         flush_subnormals, bfloat, reinterpret_cast<int8_t*>(wb + W.rawc),
                                         reinterpret_cast<int16_t*>(wb + W.rawe), 0, hbits);
  int rc = launch_rows_prep(rw, stream);
  if (rc) return rc;
  const int8_t* rawc = reinterpret_cast<const int8_t*>(wb + W.rawc);
  const int16_t* rawe = reinterpret_cast<const int16_t*>(wb + W.rawe);
  const int64_t pcols = (int64_t)W.G * W.NB32 * 32;
  hipLaunchKernelGGL(linear_pack_kernel, dim3((unsigned)((pcols * W.nbk + 255) / 256)), dim3(256), 0, stream,
                     rawc, rawe, out_features, group_width, W.NB32, W.nbk, W.Cpad, pcols,
                     reinterpret_cast<int8_t*>(wb + W.pk), reinterpret_cast<int16_t*>(wb + W.pe));
  if (launch_status() != MXA_OK) return MXA_ERR_LAUNCH;
  hipLaunchKernelGGL(linear_stats_kernel, dim3((unsigned)((pcols + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<const int16_t*>(wb + W.pe), pcols, W.nbk, reinterpret_cast<int16_t*>(wb + W.ps),
                     reinterpret_cast<int16_t*>(wb + W.pn));
  const dim3 dgrid((unsigned)((pcols * W.nbk + 255) / 256));
  if (hbits == 4)
    hipLaunchKernelGGL(linear_digit4_kernel, dgrid, dim3(256), 0, stream, reinterpret_cast<const int8_t*>(wb + W.pk),
                       reinterpret_cast<const int16_t*>(wb + W.pe), reinterpret_cast<const int16_t*>(wb + W.ps), W.nbk,
                       pcols, reinterpret_cast<int8_t*>(wb + W.pd));
  else
    hipLaunchKernelGGL(linear_digits_kernel, dgrid, dim3(256), 0, stream, reinterpret_cast<const int8_t*>(wb + W.pk),
                       reinterpret_cast<const int16_t*>(wb + W.pe), reinterpret_cast<const int16_t*>(wb + W.ps), W.nbk,
                       pcols, reinterpret_cast<int8_t*>(wb + W.pd));
  hipLaunchKernelGGL(linear_group_stats_kernel, dim3((unsigned)((W.G + 63) / 64)), dim3(64), 0, stream,
                     reinterpret_cast<const int16_t*>(wb + W.ps), W.G, W.NB32, group_width,
                     reinterpret_cast<int16_t*>(wb + W.gs));
  const LinearWeightHeader h =
      linear_weight_header(out_features, in_features, group_width, flush_subnormals, bfloat, hbits);
  hipLaunchKernelGGL(linear_header_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<LinearWeightHeader*>(wb + W.hdr),
                     h);
  if (launch_status() != MXA_OK) return MXA_ERR_LAUNCH;
  linear_weight_note(wq, h);
  return MXA_OK;
}

extern "C" int mxa_linear_weight_prep(const float* w, int32_t out_features, int32_t in_features, int32_t group_width,
                                      int32_t flush_subnormals, int32_t bfloat, void* wq, hipStream_t stream) {
  return mxa_linear_weight_prep_bits(w, out_features, in_features, group_width, flush_subnormals, bfloat, 8, wq, stream);
}
