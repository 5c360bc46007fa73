// The launch of one projection kernel instantiation (mxa_proj.hpp), shared by the translation
// units that hold them: mxa_proj.hip (MXINT8) and mxa_proj4.hip (MXINT4).
#pragma once
#include <map>
#include <mutex>
#include <utility>

#include "mxa_launch.hpp"
#include "mxa_proj.hpp"

namespace mxa {

// Kernel: qkv_proj_kernel<NBD, PLAIN> (PART kPartQKV) or cross_proj_kernel<NBD, PLAIN, PART>; MB 4:
// qkv_proj4_kernel<NBD> or cross_proj4_kernel<NBD, PART> (one x code tile in LDS)
template <auto Kernel, int PART, int NBD, int MB = 8>
static int launch_proj_kernel(const ProjArgs& pa, hipStream_t stream) {
  constexpr int kParts = ProjParts<PART>::kParts, kThreads = 64 * kParts * NBD;
  const size_t lds = proj_lds(pa.Cpad, pa.nbk, pa.D, kParts, MB).total;
  if (lds > 160 * 1024) return MXA_ERR_UNSUPPORTED;
  const void* kern = reinterpret_cast<const void*>(Kernel);
  if (hipFuncSetAttribute(kern,
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return MXA_ERR_LAUNCH;
  // head groups: a workgroup loops over hpg heads after staging its x tile once; the
  // group count minimises (rounds of resident workgroups) x (heads + ~1/4 head of x
  // staging) -- with all heads per workgroup DeiT-base's 1,792 workgroups ran 3.5
  // rounds of 512 resident ones, the last half empty
  // resident workgroups per CU and the CU count, per (device, LDS size), queried once
  int dev = 0;
  (void)hipGetDevice(&dev);
  int per_cu = 1, cus = 256;
  {
    static std::mutex mu;
    static std::map<std::pair<int, size_t>, std::pair<int, int>> cache;  // per instantiation
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({dev, lds});
    if (it == cache.end()) {
      int n = 0, c = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, kThreads, lds) != hipSuccess || n < 1) n = 1;
      if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c < 1) c = 256;
      it = cache.emplace(std::make_pair(dev, lds), std::make_pair(n, c)).first;
    }
    per_cu = it->second.first;
    cus = it->second.second;
  }
  ProjArgs p = pa;
  const int64_t wg0 = (int64_t)((pa.N + 31) / 32) * pa.B, slots = (int64_t)per_cu * cus;
  int best_g = 1;
  double best = 1e300;
  for (int g = 1; g <= pa.H; ++g) {
    const int hpg = (pa.H + g - 1) / g;
    if (g > 1 && (pa.H + hpg - 1) / hpg != g) continue;  // same hpg as a smaller g
    const double cost = (double)((wg0 * g + slots - 1) / slots) * (hpg + 0.25);
    if (cost < best - 1e-9) {
      best = cost;
      best_g = g;
    }
  }
  p.hpg = (pa.H + best_g - 1) / best_g;
  const int ng = (pa.H + p.hpg - 1) / p.hpg;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)((pa.N + 31) / 32), (unsigned)pa.B, (unsigned)ng), dim3(kThreads), lds,
                     stream, p);
  return launch_status();
}

}  // namespace mxa
