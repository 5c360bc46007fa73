// Row-kernel launches.  launch_rows switches once on the kind finish_choice (mxa_launch.hpp)
// gives for the call and hands over to that kernel's launcher: the MFMA finishing kernels
// (mxa_fin_qk.hip, mxa_fin_qkl.hip), the 16-row gather kernel (mxa_fin16.hip), and the two
// launched from this file: the 32-row gather kernel (mxa_finish.hpp) and the dense branch's
// v_dot4 row kernel (mxa_rows2.hpp).
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
// the row kernel of the path: the one switch over finish_choice's kind (mxa_launch.hpp)
int launch_rows(const Rows2Args& ra0, const FinFacts& f, bool true_mode, int S, int BH, hipStream_t stream, bool plan) {
  const FinChoice c = finish_choice(f);
  if (c.status) return c.status;
  Rows2Args ra = ra0;
  if (f.topk && true_mode) ra.true_out = nullptr;  // the selection kernel already wrote the true scores
  if (c.kind == MXA_FIN_DENSE_MFMA || c.kind == MXA_FIN_DENSE_MFMA_LONG) {  // every key kept: no mask words
    ra.dense = 1;
    ra.mask_out = nullptr;
  }
  // the plan pass runs before the workspace is bound: the gather kernels' LDS plans read only whether the
  // proj's code pointer is set, never the pointer
  static int8_t plan_xo;
  if (plan && f.xo) ra.xo_codes = &plan_xo;
  const bool w4 = f.bits == 4;  // (finish_choice: float32 then)
  switch (c.kind) {
    case MXA_FIN_MFMA_LONG:
    case MXA_FIN_DENSE_MFMA_LONG:
      return w4 ? launch_finish_qk_long_w4(ra, BH, stream, plan) : launch_finish_qk_long_w8(ra, BH, stream, plan);
    case MXA_FIN_MFMA:
    case MXA_FIN_DENSE_MFMA:
      if (w4) return launch_finish_qk_x0w4(ra, BH, stream, plan);
      return f.xdt ? launch_finish_qk_x1(ra, BH, stream, plan) : launch_finish_qk_x0(ra, BH, stream, plan);
    case MXA_FIN_GATHER16:  // (rows over 512 keys: the LONG instantiations, which stage no K table)
      if (long_rows(ra.T) && f.xo) return launch_finish16_l0xo(ra, BH, stream, plan);  // (finish_choice: MXINT8, k <= 32)
      if (long_rows(ra.T)) return w4 ? launch_finish16_l0w4(ra, BH, stream, plan) : launch_finish16_l0(ra, BH, stream, plan);
      if (w4) return launch_finish16_x0w4(ra, BH, stream, plan);
      return f.xdt ? launch_finish16_x1(ra, BH, stream, plan) : launch_finish16_x0(ra, BH, stream, plan);
    case MXA_FIN_GATHER32:
      switch (ra.nbd) {
        case 1: return launch_finish32_p1(ra, BH, stream, plan);
        case 2: return launch_finish32_p2(ra, BH, stream, plan);
        case 3: return launch_finish32_p3(ra, BH, stream, plan);
        default: return launch_finish32_p4(ra, BH, stream, plan);
      }
    default:  // MXA_FIN_DENSE_ROWS
      switch (S) {
        case 1: return launch_dense_s<1>(ra, BH, stream, plan);
        case 2: return launch_dense_s<2>(ra, BH, stream, plan);
        case 4: return launch_dense_s<4>(ra, BH, stream, plan);
        default: return launch_dense_s<8>(ra, BH, stream, plan);
      }
  }
}
#endif  // MXA_FIN_PART


}  // namespace mxa
