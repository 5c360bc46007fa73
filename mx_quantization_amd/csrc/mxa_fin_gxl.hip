// Launches of the LDS-slot gather kernel (mxa_finish_gather_xl.hpp: rows of 1,025 .. 4,096 keys, 65 <= k <= 256,
// float16 / bfloat16 tensors or scores, MXINT8 P: mxa_attention_nth_dt).  One unit, four instantiations (NB).
#include "mxa_finish_gather_xl.hpp"
#include "mxa_launch.hpp"

namespace mxa {

static_assert(kGxlMaxK <= kGxlSlots, "finish_choice sends no k past the slot table");

int launch_finish_gather_xl(const Rows2Args& ra, int BH, hipStream_t stream, bool plan) {
  // the slot table holds kGxlSlots keys of 15 bits a row; the chunk walk needs whole 32-key blocks of a row of
  // 1,025 .. 4,096 keys.  (The plan pass runs before the dtypes are bound.)
  if (!xl_rows(ra.T) || ra.T > kXlRowsT || ra.k_top < 1 || ra.k_top > kGxlSlots || ra.k_top > ra.T || ra.xo_codes ||
      ra.ntb != (ra.T + 31) / 32 || ra.tpad != 32 * ra.ntb || ra.nbd < 1 || ra.nbd > 4 || ra.D > 32 * ra.nbd || ra.dpad != 32 * ra.nbd)
    return MXA_ERR_UNSUPPORTED;
  auto lds = [&](int w) { return gxl_lds(ra.D, ra.ntb, w).total; };  // of a workgroup of w waves
  if (plan) {
    int w, r;
    return finish_tile_plan(kFin16, ra.N, BH, lds, finish_wave_cap(2), &w, &r);
  }
  if (ra.s_dt != kF16 && ra.s_dt != kBF16) return MXA_ERR_UNSUPPORTED;  // a slot's value has 16 bits
  return dispatch_nbd(ra.nbd, [&](auto nb) { return launch_finish_waves<&finish_gather_xl_kernel<decltype(nb)::value>>(ra, kFin16, lds, BH, stream); });
}

}  // namespace mxa
