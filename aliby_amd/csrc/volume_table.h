// volume_table.h — the object table of volume labels [F, Z, Y, X]: voxel count and bounding box per (stack, label), one read of
// the labels.  Shared by the per-object volume kernels that start from it (feat_coloc3d.hip, feat_texture3d.hip).  A lane walks
// 16 voxels of a row and flushes once per run of equal labels; integer atomics only, so the table is exact whatever the order.
#pragma once
#include "common.h"

#ifdef __HIPCC__
namespace {

// labels [F, Z, Y, X]; offsets[f] = first row of stack f; row = offsets[f] + label - 1; bmin / bmax [row][z, y, x]
__global__ __launch_bounds__(256) void k_c3_table(const uint16_t* __restrict__ labels, int F, int Z, int Y, int X, const int* __restrict__ offsets,
                                                  unsigned* __restrict__ count, unsigned* __restrict__ bmin, unsigned* __restrict__ bmax) {
  const size_t vol = (size_t)Z * Y * X;
  const int segs = (X + 15) / 16;
  const size_t total = (size_t)F * Z * Y * segs;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int sg = (int)(i % segs);
    size_t rest = i / segs;
    const unsigned y = (unsigned)(rest % Y);
    rest /= Y;
    const unsigned z = (unsigned)(rest % Z);
    const int f = (int)(rest / Z);
    const uint16_t* lb = labels + (size_t)f * vol + ((size_t)z * Y + y) * X;
    const int x0 = sg * 16, x1 = min(X, x0 + 16);
    const int base = offsets[f], nrows = offsets[f + 1] - base;
    unsigned cur = 0;
    int xs = x0;
    for (int x = x0; x <= x1; ++x) {
      const unsigned L = x < x1 ? lb[x] : 0xffffffffu;  // (the sentinel closes the last run)
      if (L == cur) continue;
      if (cur && (int)cur <= nrows) {
        const size_t row = (size_t)(base + cur - 1);
        atomicAdd(&count[row], (unsigned)(x - xs));
        atomicMin(&bmin[row * 3 + 0], z); atomicMin(&bmin[row * 3 + 1], y); atomicMin(&bmin[row * 3 + 2], (unsigned)xs);
        atomicMax(&bmax[row * 3 + 0], z); atomicMax(&bmax[row * 3 + 1], y); atomicMax(&bmax[row * 3 + 2], (unsigned)(x - 1));
      }
      cur = L;
      xs = x;
    }
  }
}

// table = [count n][bmin 3n][bmax 3n] (7 n words of device memory), offsets_dev [F + 1]: clears the table and fills it on `s`
inline int volume_table_launch(const uint16_t* labels, int F, int Z, int Y, int X, const int* offsets_dev, int n, unsigned* table, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(table, 0, sizeof(unsigned) * (size_t)n, s));
  HIP_TRY(hipMemsetAsync(table + n, 0xFF, sizeof(unsigned) * (size_t)n * 3, s));
  HIP_TRY(hipMemsetAsync(table + (size_t)n * 4, 0, sizeof(unsigned) * (size_t)n * 3, s));
  const size_t total = (size_t)F * Z * Y * ((X + 15) / 16);
  const unsigned grid = (unsigned)((total + 255) / 256 < 32768 ? (total + 255) / 256 : 32768);
  hipLaunchKernelGGL(k_c3_table, dim3(grid), dim3(256), 0, s, labels, F, Z, Y, X, offsets_dev, table, table + n, table + (size_t)n * 4);
  KERNEL_CHECK();
  return ALIBY_OK;
}

}  // namespace
#endif  // __HIPCC__
