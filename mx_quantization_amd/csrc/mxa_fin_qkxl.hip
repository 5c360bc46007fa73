// Launches of the chunked tiled MFMA finishing kernel for dense rows of 1,025 .. 4,096 keys
// (mxa_finish_qk_xl.hpp).  Compiled twice (build_native.py): MXA_FQXL_W4=0 the MXINT8-P
// instantiations (launch_finish_qk_xl_w8), MXA_FQXL_W4=1 the MXINT4-P ones
// (launch_finish_qk_xl_w4), so that the two build in parallel.  A third compilation, MXA_FQXL_XDT=1
// (MXINT8 P), holds the float16 / bfloat16 instantiations (launch_finish_qk_xl_x1: mxa_attention_dt).
// MXA_FQXL_MASK=1 (with either MXA_FQXL_W4): the masked float32 instantiations of the top-k branch with
// k_top > 64 (launch_finish_qk_xl_m8 / _m4: mxa_attention_nth), two more units; MXA_FQXL_MASK=1 with
// MXA_FQXL_XDT=1 the masked float16 / bfloat16 ones (launch_finish_qk_xl_mx: mxa_attention_nth_dt, k_top > 256).
#include "mxa_finish_qk_xl.hpp"
#include "mxa_launch.hpp"

#ifndef MXA_FQXL_W4
#define MXA_FQXL_W4 0
#endif
#ifndef MXA_FQXL_XDT
#define MXA_FQXL_XDT 0
#endif
#ifndef MXA_FQXL_MASK
#define MXA_FQXL_MASK 0
#endif
#if MXA_FQXL_MASK && MXA_FQXL_XDT
#define MXA_FQXL_FN launch_finish_qk_xl_mx
#elif MXA_FQXL_MASK && MXA_FQXL_W4
#define MXA_FQXL_FN launch_finish_qk_xl_m4
#elif MXA_FQXL_MASK
#define MXA_FQXL_FN launch_finish_qk_xl_m8
#elif MXA_FQXL_XDT
#define MXA_FQXL_FN launch_finish_qk_xl_x1
#elif MXA_FQXL_W4
#define MXA_FQXL_FN launch_finish_qk_xl_w4
#else
#define MXA_FQXL_FN launch_finish_qk_xl_w8
#endif

namespace mxa {

constexpr bool kFqxlW4 = MXA_FQXL_W4 != 0;
constexpr bool kFqxlXdt = MXA_FQXL_XDT != 0;
constexpr bool kFqxlMask = MXA_FQXL_MASK != 0;
static_assert(!(kFqxlW4 && kFqxlXdt), "MXINT4 P: float32 only");

// One instantiation planned by finish_mfma_plan from its own registers (lds: one chunk's tables, fql_lds, whatever T
// and the number of waves are), then launched.  The kernel's barriers need whole tiles of whole waves: 1 .. 8 waves,
// a workgroup's rows a multiple of the tile.  finish_tile_plan gives nothing else; the test is a guard on that
template <auto Kernel>
static int launch_finish_qk_xl(Rows2Args ra, size_t lds, int BH, hipStream_t stream) {
  const int rc = finish_mfma_plan(ra, kFqRows, lds, BH, kernel_waves_per_simd<Kernel>(), &ra.waves, &ra.rows_per_wg);
  if (rc) return rc;
  if (ra.waves < 1 || ra.waves > 8 || ra.rows_per_wg <= 0 || ra.rows_per_wg % kFqRows) return MXA_ERR_LAUNCH;
  return launch_finish_tiles<Kernel>(ra, BH, lds, stream);
}
template <int NB>
static int launch_finish_qk_xl_nb(const Rows2Args& ra, int BH, hipStream_t stream) {
  if (ra.dpad != 32 * NB) return MXA_ERR_ARG;
  const size_t lds = fql_lds(NB, ra.D).total;
  constexpr int NBX = NB + (kFqxlXdt ? kFqDtNB : 0) + (kFqxlMask ? kFqXlMaskNB : 0);
  if (finish_mfma_extra(ra)) return launch_finish_qk_xl<&finish_qk_xl_kernel<NBX, kFqxlW4, true>>(ra, lds, BH, stream);
  return launch_finish_qk_xl<&finish_qk_xl_kernel<NBX, kFqxlW4, false>>(ra, lds, BH, stream);
}

int MXA_FQXL_FN(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  // (launch_rows chooses the unit by the call's dtypes; the plan pass runs before they are bound)
  // (the masked units: the top-k branch, whose mask words the selection wrote -- bound after the plan pass)
  if ((!kFqxlXdt && (ra.s_dt != kF32 || ra.in_dt != kF32)) || ra.xo_codes || (ra.dense != 0) == kFqxlMask) return MXA_ERR_UNSUPPORTED;
  if (kFqxlMask && !plan && !ra.mask_out) return MXA_ERR_ARG;
  if (!xl_rows(ra.T) || ra.T > kXlRowsT || ra.ntb != (ra.T + 31) / 32 || ra.tpad != 32 * ra.ntb || ra.nbd < 1 || ra.nbd > 4 ||
      ra.D > 32 * ra.nbd)
    return MXA_ERR_UNSUPPORTED;
  if (plan) {
    int w, r;
    return finish_mfma_plan(ra, kFqRows, fql_lds(ra.nbd, ra.D).total, BH, 2, &w, &r);
  }
  return dispatch_nbd(ra.nbd, [&](auto nb) { return launch_finish_qk_xl_nb<decltype(nb)::value>(ra, BH, stream); });
}

}  // namespace mxa
