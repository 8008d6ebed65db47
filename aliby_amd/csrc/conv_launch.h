// conv_launch.h — the launch front end of the network's persistent convolution kernels (nn_conv.hip: k_conv3x3, k_conv3x3_dma,
// k_conv_pair32, k_conv_first_pair; nn_conv_deep.hip: k_conv3x3_deep, k_conv3x3_deep16, k_conv3x3_deep_ls, k_conv3x3_kloop64).
// The counterpart of the per-object feature kernels is object_launch.h; the device-side sibling, with the bf16 / MFMA primitives
// these kernels share, is conv_mfma.h.
//
// Every such kernel takes one argument struct with `ntiles` and `order` and loops over the tiles itself (tile_walk, the one
// device function here): the grid is 8 XCDs x `nslots` workgroups, never more than the tiles need.  A site states how many
// workgroups an XCD holds (the kernel's resident workgroups per CU x 32 CUs) as `cap`; the caps stay with the sites, they follow
// from each kernel's LDS and registers.  The working sets are dynamic LDS, so hipFuncAttributeMaxDynamicSharedMemorySize is
// raised once per process and kernel, at the kernel's own first launch.
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

// The tiles of this workgroup.  Workgroup b lives on XCD b % 8 and is slot b / 8 of it; XCD x owns the contiguous eighth
// [x * per_xcd, (x + 1) * per_xcd) of the tile list, so that neighbouring tiles (shared halos) meet in the same L2, and its
// slots share the eighth with a stride of nslots.  order 0 walks the eighth upwards; order 1 walks the mirror image, from its
// last tile down: the same tiles per XCD and the same count per slot, so the only difference is WHEN a tile runs.  A launch
// that walks against its producer starts on the part of the tensor that the producer wrote last, which is the part the
// Infinity Cache still holds.  The k-th tile of the workgroup, k < count, is first + k * step.
struct TileWalk {
  int first, step, count;
};
__device__ __forceinline__ TileWalk tile_walk(int ntiles, int order) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = gridDim.x >> 3;
  const int per_xcd = (ntiles + 7) >> 3;
  const int lo = xcd * per_xcd, hi = min(ntiles, lo + per_xcd);
  TileWalk w;
  w.count = lo + slot < hi ? (hi - lo - slot + nslots - 1) / nslots : 0;
  w.first = order ? hi - 1 - slot : lo + slot;
  w.step = order ? -nslots : nslots;
  return w;
}

// The direction of the next persistent launch on `ctx`: pinned, or (the default) opposite to the previous one.  A launch with
// phase stamps switched on (the debug-trace entry points) walks upwards: the stamps are those of workgroup 0's first tiles.
inline int next_order(aliby_ctx* ctx, bool traced) {
  if (traced || ctx->conv_order == ALIBY_CONV_ASCENDING) return 0;
  if (ctx->conv_order == ALIBY_CONV_DESCENDING) return 1;
  return (int)(ctx->conv_launches++ & 1u);
}

// One persistent launch: 8 XCDs x at most `cap` slots of THREADS threads with `lds_bytes` of dynamic LDS.
template <auto Kernel, int THREADS, class Args>
int launch(aliby_ctx* ctx, Args& a, int lds_bytes, int cap, hipStream_t stream) {
  a.order = next_order(ctx, a.trace != nullptr);
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
