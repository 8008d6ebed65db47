// volume_table.h — the front end of the per-object kernels on volume labels [F, Z, Y, X] (feat_coloc3d.hip, feat_texture3d.hip,
// feat_intensity3d_detail.hip; feat_neighbors3d.hip and feat_relate3d.hip take the table and the plan):
// the object table (k_volume_table: voxel count and bounding box per (stack, label), one read of the labels), the host's plan
// around it (volume_plan), the arguments and the prologue every such kernel opens with, and the launch of a <dtype, GLOBAL> kernel.
// (The index decode of k_volume_table and the entries' shape check are volume_pass.h, shared with the whole-stack kernels.)
#pragma once
#include <algorithm>
#include <memory>
#include <new>
#include "volume_pass.h"

#ifdef __HIPCC__
#define VOLUME_GLOBAL_BLOCKS 256             // workgroups of the global-scratch form, at most
#define VOLUME_GLOBAL_BYTES (1ull << 30)     // ceiling of their working sets, all workgroups together

namespace {

// labels [F, Z, Y, X]; offsets[f] = first row of stack f; row = offsets[f] + label - 1; bmin / bmax [row][z, y, x].  A lane walks
// 16 voxels of a row and flushes once per run of equal labels; integer atomics only, so the table is exact whatever the order.
__global__ __launch_bounds__(256) void k_volume_table(const uint16_t* __restrict__ labels, int F, int Z, int Y, int X, const int* __restrict__ offsets,
                                                      unsigned* __restrict__ count, unsigned* __restrict__ bmin, unsigned* __restrict__ bmax) {
  const size_t vol = (size_t)Z * Y * X;
  const int segs = (X + 15) / 16;
  const size_t total = (size_t)F * Z * Y * segs;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const StackIndex g = stack_index(i, Z, Y, segs);
    const unsigned z = (unsigned)g.z, y = (unsigned)g.y;
    const uint16_t* lb = labels + (size_t)g.f * vol + ((size_t)z * Y + y) * X;
    const int x0 = g.x * 16, x1 = min(X, x0 + 16);
    const int base = offsets[g.f], nrows = offsets[g.f + 1] - base;
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
  const size_t blocks = ((size_t)F * Z * Y * ((X + 15) / 16) + 255) / 256;
  hipLaunchKernelGGL(k_volume_table, dim3((unsigned)(blocks < 32768 ? blocks : 32768)), dim3(256), 0, s, labels, F, Z, Y, X, offsets_dev, table, table + n, table + (size_t)n * 4);
  KERNEL_CHECK();
  return ALIBY_OK;
}

// What every per-object kernel is handed.  The LDS form (GLOBAL = false) walks all n rows and skips those of the other form; the
// global-scratch form walks items[0 .. n_items).
struct VolumeArgs {
  const uint16_t* labels;
  int F, Z, Y, X;
  const int* offsets;     // [F+1]
  const unsigned* count;  // [n]
  const unsigned* bmin;   // [n][z, y, x]
  const unsigned* bmax;   // inclusive
  const int* items;       // GLOBAL: rows of the objects above the LDS budget
  int n_items;            // GLOBAL: how many; else the number of rows
};

// (The helpers take the fields they read: a reference to the by-value kernel argument costs k_coloc3d registers.)
template <bool GLOBAL>
__device__ __forceinline__ int volume_row(const int* items, int it) { return GLOBAL ? items[it] : it; }

// the stack of a row: offsets[f] <= row < offsets[f + 1]; its label there is row - offsets[f] + 1
__device__ __forceinline__ int volume_stack_of(const int* offsets, int F, int row) {
  int f = 0, fhi = F;
  while (fhi - f > 1) { const int mid = (f + fhi) >> 1; if (offsets[mid] <= row) f = mid; else fhi = mid; }
  return f;
}

// the bounding box of a row with voxels; voxel i of it in raster order (z, y, x) as an index into the stack
struct VolumeBox {
  unsigned z0, y0, x0, d, h, w, nbox;  // (a stack holds at most 2^30 voxels)
  __device__ __forceinline__ size_t index(unsigned i, int Y, int X) const {
    const unsigned x = i % w, r = i / w;
    return ((size_t)(z0 + r / h) * Y + (y0 + r % h)) * X + (x0 + x);
  }
};
__device__ __forceinline__ VolumeBox volume_box(const unsigned* bmin, const unsigned* bmax, int row) {
  VolumeBox b;
  b.z0 = bmin[(size_t)row * 3]; b.y0 = bmin[(size_t)row * 3 + 1]; b.x0 = bmin[(size_t)row * 3 + 2];
  b.d = bmax[(size_t)row * 3] - b.z0 + 1; b.h = bmax[(size_t)row * 3 + 1] - b.y0 + 1; b.w = bmax[(size_t)row * 3 + 2] - b.x0 + 1;
  b.nbox = b.d * b.h * b.w;
  return b;
}

// The gather of the kernels that keep an object's voxel LIST (feat_coloc3d.hip, feat_intensity3d_detail.hip): the voxels of label L
// inside its box in raster order (z, y, x), by order-preserving compaction, PER_LANE consecutive voxels of the box per lane and round.
// visit(pos, i, idx) once per voxel of the object: pos = its rank in the list, i = its index in the box, idx = its index in the
// stack.  Returns the number of voxels to every lane.  All BLOCK lanes call it; wsum = LDS int[BLOCK / 64]; a barrier
// lies before the first visit, none after the last.  The lane of a voxel depends on the object's own box only.
template <int BLOCK, int PER_LANE, class Visit>
__device__ __forceinline__ int volume_gather(const uint16_t* lab, uint16_t L, const VolumeBox& box, int Y, int X, int* wsum, Visit visit) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int base = 0;
  for (unsigned i0 = 0; i0 < box.nbox; i0 += BLOCK * PER_LANE) {
    size_t idx[PER_LANE];
    unsigned in = 0;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      const unsigned i = i0 + (unsigned)tid * PER_LANE + k;
      idx[k] = 0;
      if (i < box.nbox) {
        idx[k] = box.index(i, Y, X);
        if (lab[idx[k]] == L) in |= 1u << k;
      }
    }
    const int c = __popc(in);
    int incl = c;  // inclusive scan of the lanes' counts inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    __syncthreads();
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < BLOCK / 64; ++i) { const int s = wsum[i]; if (i < wid) off += s; tot += s; }
    int pos = base + off + incl - c;
    base += tot;
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
      if (!(in & (1u << k))) continue;
      visit(pos, i0 + (unsigned)tid * PER_LANE + k, idx[k]);
      ++pos;
    }
  }
  return base;
}

struct VolumePlan {
  VolumeArgs args;          // labels, shape, table, offsets and items on the device; n_items = n (the LDS form's)
  int* d_extra;             // the family's extra words on the device
  int n, n_big, grid_big;   // rows; rows of the global-scratch form; its workgroups (x per_block_mult)
  size_t need;              // bytes of one of its workgroups' working set
  unsigned char* gscratch;  // grid_big * per_block_mult * need bytes
  std::unique_ptr<unsigned[]> host;  // the table as read back and the item list: lives as long as the plan, whatever the exit
};

// bytes of a plan's head in the context's scratch: the table, the offsets, the extra words and the item list, 256-byte aligned
inline size_t volume_plan_head_bytes(int n, int F, size_t extra_words) {
  return (((size_t)n * 7 + (size_t)(F + 1) + extra_words + (size_t)n) * 4 + 255) & ~(size_t)255;
}

// size_of_row(count, bmin[3], bmax[3]) = what a row is measured by against lds_limit; bytes_for(largest such measure above the
// limit) = one workgroup's bytes in global scratch; per_block_mult = workgroups per grid column.  Scratch, from byte `base` (a
// multiple of 256) on: [count n][bmin 3n][bmax 3n][offsets F+1][extra][items n], then (256-byte aligned) the global-scratch form's
// working sets.  Needs offsets_host[F] > 0.  base: a call that needs the tables of two label stacks (feat_relate3d.hip) places the
// second plan behind the first one's volume_plan_head_bytes; it sizes the scratch for both BEFORE the first plan (a block that
// grows moves, and only the plan that grows it puts its own table back) and asks for an lds_limit no row exceeds.
template <class SizeOf, class BytesFor>
int volume_plan(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host, const int32_t* extra_host,
                size_t extra_words, size_t lds_limit, SizeOf size_of_row, BytesFor bytes_for, size_t per_block_mult, hipStream_t s, VolumePlan* p,
                const char* who, size_t base = 0) {
  const int n = offsets_host[F];
  const size_t tab_words = (size_t)n * 7, off_bytes = sizeof(int) * (size_t)(F + 1);
  const size_t head_bytes = volume_plan_head_bytes(n, F, extra_words);
  int rc = aliby_ensure_scratch(ctx, base + head_bytes);
  if (rc) return rc;
  unsigned* table = (unsigned*)((unsigned char*)ctx->scratch + base);
  HIP_TRY(hipMemcpyAsync(table + tab_words, offsets_host, off_bytes, hipMemcpyHostToDevice, s));
  rc = volume_table_launch(labels, F, Z, Y, X, (const int*)(table + tab_words), n, table, s);
  if (rc) return rc;
  // the table is read back: the host needs the rows above the LDS budget, and the largest
  p->host.reset(new (std::nothrow) unsigned[tab_words + (size_t)n]);
  if (!p->host) { aliby_set_error("%s: out of host memory", who); return ALIBY_ERR_INVALID; }
  unsigned* table_host = p->host.get();
  int* items_host = (int*)(table_host + tab_words);
  hipError_t e = hipMemcpyAsync(table_host, table, sizeof(unsigned) * tab_words, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && aliby_wait_stream(s) != ALIBY_OK) e = hipErrorUnknown;
  if (e != hipSuccess) { aliby_set_error("%s: reading the object table back failed: %s", who, hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  size_t max_big = 0;
  p->n_big = 0;
  for (int i = 0; i < n; ++i) {
    const size_t size = size_of_row(table_host[i], table_host + n + 3 * (size_t)i, table_host + 4 * (size_t)n + 3 * (size_t)i);
    if (size > lds_limit) { items_host[p->n_big++] = i; max_big = size > max_big ? size : max_big; }
  }
  p->need = 0, p->grid_big = 0;
  if (p->n_big) {
    p->need = bytes_for(max_big);
    const size_t fit = VOLUME_GLOBAL_BYTES / p->need / per_block_mult;
    p->grid_big = (int)std::min<size_t>({fit > 0 ? fit : 1, VOLUME_GLOBAL_BLOCKS, (size_t)p->n_big});
    void* before = ctx->scratch;
    rc = aliby_ensure_scratch(ctx, base + head_bytes + p->need * (size_t)p->grid_big * per_block_mult);
    if (rc) return rc;
    if (ctx->scratch != before) {  // the block moved: put the table and the offsets back
      table = (unsigned*)((unsigned char*)ctx->scratch + base);
      e = hipMemcpyAsync(table, table_host, sizeof(unsigned) * tab_words, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(table + tab_words, offsets_host, off_bytes, hipMemcpyHostToDevice, s);
    }
  }
  int* d_off = (int*)(table + tab_words);
  p->d_extra = d_off + (F + 1);
  int* d_items = p->d_extra + extra_words;
  if (e == hipSuccess && extra_words) e = hipMemcpyAsync(p->d_extra, extra_host, sizeof(int) * extra_words, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && p->n_big) e = hipMemcpyAsync(d_items, items_host, sizeof(int) * (size_t)p->n_big, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { aliby_set_error("%s: upload failed: %s", who, hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  p->n = n;
  p->gscratch = (unsigned char*)ctx->scratch + base + head_bytes;
  p->args = VolumeArgs{labels, F, Z, Y, X, d_off, table, table + n, table + (size_t)n * 4, d_items, n};
  return ALIBY_OK;
}

// one launch of a per-object kernel, k_u16 / k_f32 = its two pixel types at one GLOBAL; lds = dynamic LDS bytes (0: none)
template <class Args>
hipError_t volume_launch(int dtype, void (*k_u16)(Args), void (*k_f32)(Args), const Args& a, dim3 grid, unsigned block, size_t lds, hipStream_t s) {
  void (*k)(Args) = dtype == ALIBY_U16 ? k_u16 : k_f32;
  if (lds) {
    const hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, grid, dim3(block), lds, s, a);
  return hipGetLastError();
}

}  // namespace
#endif  // __HIPCC__
