// Resident workgroups per CU of the fused projection kernels at the PixArt width (C = 1152, D = 72:
// NBD 3), as launch_proj_kernel asks for them: hipOccupancyMaxActiveBlocksPerMultiprocessor with the
// kernel's threads and its proj_lds bytes, for the Q, KV and QKV passes at MXINT8 (general rounding)
// and MXINT4.  Prints one line per kernel, with the registers the runtime reports.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I include -I mx_quantization_amd/csrc \
//         tools/micro/proj_occupancy.hip -o tools/micro/proj_occupancy && tools/micro/proj_occupancy
#include <cstdio>

#include "mxa_proj.hpp"

using namespace mxa;

template <auto Kernel>
static void report(const char* name, int parts, int bits) {
  const int C = 1152, D = 72, nbk = C / 32, threads = 64 * parts * 3;
  const size_t lds = proj_lds(C, nbk, D, parts, bits).total;
  const void* kern = reinterpret_cast<const void*>(Kernel);
  int n = -1;
  hipFuncAttributes fa{};
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, threads, lds) != hipSuccess ||
      hipFuncGetAttributes(&fa, kern) != hipSuccess) {
    std::printf("%-28s query failed\n", name);
    return;
  }
  std::printf("%-28s threads %3d  lds %6zu B  regs %3d  workgroups per CU %d\n", name, threads, lds, fa.numRegs, n);
}

int main() {
  report<cross_proj_kernel<3, false, kPartQ>>("cross_proj_kernel<3,0,Q>", 1, 8);
  report<cross_proj_kernel<3, false, kPartKV>>("cross_proj_kernel<3,0,KV>", 2, 8);
  report<qkv_proj_kernel<3, false>>("qkv_proj_kernel<3,0>", 3, 8);
  report<cross_proj_kernel<3, true, kPartQ>>("cross_proj_kernel<3,1,Q>", 1, 8);
  report<cross_proj_kernel<3, true, kPartKV>>("cross_proj_kernel<3,1,KV>", 2, 8);
  report<qkv_proj_kernel<3, true>>("qkv_proj_kernel<3,1>", 3, 8);
  report<cross_proj4_kernel<3, kPartQ>>("cross_proj4_kernel<3,Q>", 1, 4);
  report<cross_proj4_kernel<3, kPartKV>>("cross_proj4_kernel<3,KV>", 2, 4);
  report<qkv_proj4_kernel<3>>("qkv_proj4_kernel<3>", 3, 4);
  return 0;
}
