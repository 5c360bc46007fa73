// The fused projections' MXINT4 launches (W4A4: qkv_proj4_kernel, cross_proj4_kernel of
// mxa_proj.hpp), in a translation unit of their own so that they compile beside mxa_proj.hip.
// General rounding only: one instantiation per (NBD, part).
#include "mxa_proj_launch.hpp"

namespace mxa {

template <int NBD>
static int launch_proj4_nbd(const ProjArgs& pa, int part, hipStream_t stream) {
  switch (part) {
    case kPartQ: return launch_proj_kernel<cross_proj4_kernel<NBD, kPartQ>, kPartQ, NBD, 4>(pa, stream);
    case kPartKV: return launch_proj_kernel<cross_proj4_kernel<NBD, kPartKV>, kPartKV, NBD, 4>(pa, stream);
    default: return launch_proj_kernel<qkv_proj4_kernel<NBD>, kPartQKV, NBD, 4>(pa, stream);
  }
}

int launch_proj4(const ProjArgs& pa, hipStream_t stream, int part) {
  return dispatch_nbd((pa.D + 31) / 32, [&](auto nb) { return launch_proj4_nbd<decltype(nb)::value>(pa, part, stream); });
}

}  // namespace mxa
