// Row-kernel launches: the finishing kernel of the top-k path (mxa_finish.hpp) and the
// dense (top_k=False) branch: the MFMA finishing kernel with every key kept
// (mxa_finish_qk.hpp, T <= 256), else the row kernel (mxa_rows2.hpp).
#include "mxa_finish.hpp"
#include "mxa_launch.hpp"

// Compiled five times (build_native.py, MXA_FIN_PART): part 0 the dispatch (launch_rows) and
// the dense row kernel, parts 1..4 the 32-row finishing kernel for NB = 1..4 blocks per head
// dim (launch_finish32_p<NB>), so that the instantiations build in parallel.
#ifndef MXA_FIN_PART
#define MXA_FIN_PART 0
#endif

namespace mxa {

#if MXA_FIN_PART == 0

// ---- the dense row kernel (mxa_rows2.hpp) ------------------------------------------
static size_t rows2_total(const Rows2Args& ra, int W) {
  return rows2_lds(ra.T, ra.D, ra.kst, ra.nbd, ra.vst, ra.ntb, ra.tpad, W).total;
}
// waves per workgroup: the size (8 or 16) that keeps the most waves resident per CU
// (LDS-limited workgroups x waves, capped by the kernel's 7-waves-per-SIMD register use)
static int rows2_waves(const Rows2Args& ra) {
  auto resident = [&](int w) {
    const size_t t = rows2_total(ra, w);
    return t > 160 * 1024 ? 0 : std::min((int)(160 * 1024 / t) * w, 28);
  };
  const int r8 = resident(8), r16 = resident(16);
  if (r8 > 0 || r16 > 0) return r16 > r8 ? 16 : 8;
  return rows2_total(ra, 4) <= 160 * 1024 ? 4 : 0;
}

template <int S>
static int launch_dense_s(const Rows2Args& ra0, int BH, hipStream_t stream, bool plan) {
  Rows2Args ra = ra0;
  ra.waves = rows2_waves(ra);
  if (ra.waves <= 0) return MXA_ERR_UNSUPPORTED;
  if (plan) return MXA_OK;
  const size_t lds = rows2_total(ra, ra.waves);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&dense_rows_kernel<S>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return MXA_ERR_LAUNCH;
  // few heads: split each head's rows over grid.y so that the launch still has ~4
  // workgroups per CU
  const int chunks = std::max(1, std::min((ra.N + ra.waves - 1) / ra.waves, 1024 / std::max(BH, 1)));
  ra.rows_per_wg = (ra.N + chunks - 1) / chunks;
  const unsigned gy = (unsigned)((ra.N + ra.rows_per_wg - 1) / ra.rows_per_wg);
  hipLaunchKernelGGL(dense_rows_kernel<S>, dim3((unsigned)BH, gy), dim3(64 * ra.waves), lds, stream, ra);
  return launch_status();
}

#endif  // MXA_FIN_PART == 0

// ---- finishing kernel (mxa_finish.hpp): 32-row MFMA tiles, one per wave ------------
// (wave cap 12: the kernel's register use is not looked up)
static int finish_plan(const Rows2Args& ra, int BH, int* waves, int* rows_per_wg) {
  const bool xo = ra.xo_codes != nullptr;
  auto lds = [&](int w) { return fin_lds(ra.T, ra.D, ra.kst, ra.nbd, ra.vst, ra.ntb, w, xo).total; };
  return finish_tile_plan(kFinTile, ra.N, BH, lds, 12, waves, rows_per_wg);
}
template <int NB, int KS, bool XDT, bool XO = false>
static int launch_finish_xdt(const Rows2Args& ra0, int BH, hipStream_t stream) {
  Rows2Args ra = ra0;
  int rc = finish_plan(ra, BH, &ra.waves, &ra.rows_per_wg);
  if (rc) return rc;
  const size_t lds = fin_lds(ra.T, ra.D, ra.kst, ra.nbd, ra.vst, ra.ntb, ra.waves, XO).total;
  return launch_finish_tiles<&finish_kernel<NB, KS, XDT, XO>>(ra, BH, lds, stream);
}
template <int NB, int KS>
static int launch_finish_ks(const Rows2Args& ra, int BH, hipStream_t stream) {
  if (ra.xo_codes) {  // output MX codes for the proj Linear: float32, D % 32 == 0
    if (ra.s_dt != kF32 || ra.in_dt != kF32 || ra.D % 32) return MXA_ERR_UNSUPPORTED;
    return launch_finish_xdt<NB, KS, false, true>(ra, BH, stream);
  }
  if constexpr (KS >= 8) {
    if (ra.s_dt != kF32 || ra.in_dt != kF32) return launch_finish_xdt<NB, KS, true>(ra, BH, stream);
    return launch_finish_xdt<NB, KS, false>(ra, BH, stream);
  }
  return MXA_ERR_UNSUPPORTED;  // k <= 64 without xo: the 16-row kernel
}
template <int NB>
static int launch_finish_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  // k <= 64 (k <= 32 with the proj's codes) is the 16-row kernel's (mxa_fin16.hip)
  if (ra.k_top <= (ra.xo_codes ? 32 : 64)) return MXA_ERR_UNSUPPORTED;
  const int ks = (ra.k_top + 15) / 16;  // slots per lane: 16 lanes per row
  if (ks <= 4) return launch_finish_ks<NB, 4>(ra, BH, stream);
  if (ks <= 8) return launch_finish_ks<NB, 8>(ra, BH, stream);
  if (ks <= 16) return launch_finish_ks<NB, 16>(ra, BH, stream);
  return launch_finish_ks<NB, 32>(ra, BH, stream);
}
#if MXA_FIN_PART > 0
#define MXA_FIN_FN2(i) launch_finish32_p##i
#define MXA_FIN_FN(i) MXA_FIN_FN2(i)
int MXA_FIN_FN(MXA_FIN_PART)(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  if (plan) {
    int w, r;
    return finish_plan(ra, BH, &w, &r);
  }
  return launch_finish_nb<MXA_FIN_PART>(ra, BH, stream);
}
#else
static int launch_finish(const Rows2Args& ra, int BH, hipStream_t stream, bool plan, int elem_bits) {
  const int kind = rows_kernel_kind(true, ra.k_top, ra.T, ra.nbd, ra.xo_codes != nullptr);
  const bool xdt = ra.s_dt != kF32 || ra.in_dt != kF32;
  if (elem_bits == 4) {  // MXINT4 P: the 16-row kernel (short and LONG) and the MFMA kernel, float32
    if (xdt || ra.xo_codes) return MXA_ERR_UNSUPPORTED;
    if (kind == MXA_FIN_MFMA) return launch_finish_qk_x0w4(ra, BH, stream, plan);
    if (kind != MXA_FIN_GATHER16) return MXA_ERR_UNSUPPORTED;
    return long_rows(ra.T) ? launch_finish16_l0w4(ra, BH, stream, plan) : launch_finish16_x0w4(ra, BH, stream, plan);
  }
  if (kind == MXA_FIN_MFMA) return xdt ? launch_finish_qk_x1(ra, BH, stream, plan) : launch_finish_qk_x0(ra, BH, stream, plan);
  // k <= 64 (DeiT's 20 / 30, PixArt's 20): 16-row tiles, four lanes per row (also with the
  // proj's MX input codes for k <= 32); larger k with T > 256: the 32-row kernel.
  // (rows over 512 keys, float32 only: its LONG instantiations, which stage no K table)
  if (kind == MXA_FIN_GATHER16 && long_rows(ra.T) && !xdt) return launch_finish16_l0(ra, BH, stream, plan);
  if (kind == MXA_FIN_GATHER16) return xdt ? launch_finish16_x1(ra, BH, stream, plan) : launch_finish16_x0(ra, BH, stream, plan);
  switch (ra.nbd) {
    case 1: return launch_finish32_p1(ra, BH, stream, plan);
    case 2: return launch_finish32_p2(ra, BH, stream, plan);
    case 3: return launch_finish32_p3(ra, BH, stream, plan);
    default: return launch_finish32_p4(ra, BH, stream, plan);
  }
}

// the row kernel of the path: the finishing kernel (top-k) or the dense kernel
int launch_rows(const Rows2Args& ra, bool topk, bool true_mode, int S, int BH, hipStream_t stream, bool plan,
                int elem_bits, bool full) {
  // mxa_attention_full on rows over 512 keys, the dense branch or k > 64: the tiled MFMA kernel
  // (mxa_finish_qk_long.hpp), which reads the selection's prune-mask words or keeps every key
  if (finish_qk_long_wanted(full, topk, ra.k_top, ra.T)) {
    Rows2Args rl = ra;
    if (topk && true_mode) rl.true_out = nullptr;  // (the selection kernel wrote them)
    if (!topk) {
      rl.dense = 1;
      rl.mask_out = nullptr;
    }
    return elem_bits == 4 ? launch_finish_qk_long_w4(rl, BH, stream, plan) : launch_finish_qk_long_w8(rl, BH, stream, plan);
  }
  if (topk) {
    // the selection kernel already wrote the true scores when it ranked them
    Rows2Args rf = ra;
    if (true_mode) rf.true_out = nullptr;
    return launch_finish(rf, BH, stream, plan, elem_bits);
  }
  // the dense branch: the MFMA finishing kernel with every key kept (T <= 256: a row's scores
  // in registers); longer rows: the v_dot4 row kernel
  if (rows_kernel_kind(false, 0, ra.T, ra.nbd, false) == MXA_FIN_DENSE_MFMA) {
    Rows2Args rd = ra;
    rd.dense = 1;
    rd.mask_out = nullptr;
    if (elem_bits == 4) return launch_finish_qk_x0w4(rd, BH, stream, plan);  // (refuses float16 / bfloat16)
    if (rd.s_dt != kF32 || rd.in_dt != kF32) return launch_finish_qk_x1(rd, BH, stream, plan);
    return launch_finish_qk_x0(rd, BH, stream, plan);
  }
  if (elem_bits == 4) return MXA_ERR_UNSUPPORTED;  // dense_rows_kernel: MXINT8 P only
  switch (S) {
    case 1: return launch_dense_s<1>(ra, BH, stream, plan);
    case 2: return launch_dense_s<2>(ra, BH, stream, plan);
    case 4: return launch_dense_s<4>(ra, BH, stream, plan);
    default: return launch_dense_s<8>(ra, BH, stream, plan);
  }
}
#endif  // MXA_FIN_PART


}  // namespace mxa
