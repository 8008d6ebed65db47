// conv_launch.h — the launch front end of the network's persistent convolution kernels (nn_conv.hip: k_conv3x3, k_conv3x3_dma,
// k_conv_pair32, k_conv_first_pair; nn_conv_deep.hip: k_conv3x3_deep, k_conv3x3_deep16, k_conv3x3_deep_ls, k_conv3x3_kloop64).
// Host side only; the counterpart of the per-object feature kernels is object_launch.h.
//
// Every such kernel takes one argument struct with `ntiles` and loops over the tiles itself: the grid is 8 XCDs x `nslots`
// workgroups, never more than the tiles need.  A site states how many workgroups an XCD holds (the kernel's resident workgroups
// per CU x 32 CUs) as `cap`; the caps stay with the sites, they follow from each kernel's LDS and registers.  The working sets
// are dynamic LDS, so hipFuncAttributeMaxDynamicSharedMemorySize is raised once per process and kernel, at the kernel's own
// first launch.
#pragma once
#include "common.h"
#include <limits.h>
#include <stdlib.h>

#ifdef __HIPCC__
namespace {

// integer value of an environment variable, `fallback` when it is not set
inline int env_int(const char* name, int fallback) {
  const char* e = getenv(name);
  return e ? atoi(e) : fallback;
}

// Tile counts of a ConvArgs launch from the kernel's Cfg (TW x TH output tiles).  PACK: images narrower than the 224-pixel
// tile row lie G = 224 / W side by side in one tile row.
template <class Cfg, bool PACK, class Args>
int conv_tiles(Args& a) {
  a.G = PACK ? 224 / a.W : 1;
  a.tiles_x = PACK ? 224 / Cfg::TW : (a.W + Cfg::TW - 1) / Cfg::TW;
  a.tiles_y = (a.H + Cfg::TH - 1) / Cfg::TH;
  const long long nt = (long long)(a.N / a.G) * a.tiles_x * a.tiles_y;
  ARG_CHECK(nt < INT_MAX, "conv3x3: too many tiles");
  a.ntiles = (int)nt;
  return ALIBY_OK;
}

// One persistent launch: 8 XCDs x at most `cap` slots of THREADS threads with `lds_bytes` of dynamic LDS.
template <auto Kernel, int THREADS, class Args>
int launch(Args& a, int lds_bytes, int cap, hipStream_t stream) {
  static bool attr_done = false;
  if (!attr_done) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    attr_done = true;
  }
  const int per_xcd = (a.ntiles + 7) / 8;
  const int nslots = per_xcd < cap ? per_xcd : cap;
  hipLaunchKernelGGL(Kernel, dim3(8 * nslots), dim3(THREADS), lds_bytes, stream, a);
  KERNEL_CHECK();
  return ALIBY_OK;
}

}  // namespace
#endif  // __HIPCC__
