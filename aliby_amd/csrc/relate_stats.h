// relate_stats.h — what the 2-D `relate` kernels (feat_relate.hip) and the volume kernels (feat_relate3d.hip) share: the per-workgroup
// counters (one int per label of the OTHER set, in LDS or in a slab of the context's scratch), the absent row, the write of a row's
// parent with the children atomic, the write of the five columns, and the layout of a side's workspace.  Centres are [rows, DIM] in
// axis order (z,) y, x, NaN = absent (neighbors_stats.h).  Definitions: the headers of the two .hip files, where the walks over an
// object's box and over its parent's outline stay (a tile's box is a table row with max_h x max_w known to the host, a stack's a
// VolumeBox; the finish kernels give a row a wave and a workgroup).  The run folding in front of the counters' atomics and the argmax
// loop over them are a dozen lines that each overlap kernel spells out: moved into functions here they changed the 2-D kernel's
// instruction stream (24 + 11 more instructions and one more SGPR in both forms), which nothing measured argues to be neutral; with
// them in place the 2-D kernels compile to the instructions they had (two zero-initialised register pairs trade names).
#pragma once
#include "common.h"
#include "neighbors_stats.h"

#ifdef __HIPCC__

// bytes of one workgroup's counters for a set whose largest tile or stack has max_count labels (label 0 has a slot: no index shift)
static inline size_t relate_counter_bytes(int max_count) { return (((size_t)max_count + 1) * sizeof(int) + 15) & ~(size_t)15; }

extern __shared__ __align__(16) int relate_lds[];

// the counters of this workgroup: named LDS in the LDS form (no flat pointer), a slab of the context's scratch in the global one
template <bool GLOBAL>
struct RelateCounts {
  int* g;
  __device__ __forceinline__ void zero(int k) const {
    if constexpr (GLOBAL) g[k] = 0;
    else relate_lds[k] = 0;
  }
  __device__ __forceinline__ void add(int k, int n) const {
    if constexpr (GLOBAL) atomicAdd(&g[k], n);
    else atomicAdd(&relate_lds[k], n);
  }
  // (global form: the adds were made in L2, so the read goes there too)
  __device__ __forceinline__ int get(int k) const {
    if constexpr (GLOBAL) return __hip_atomic_load(&g[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return relate_lds[k];
  }
};

// a row without pixels: the `neighbors` family's NaN centre (how the finish kernels and the other direction know it), no parent
template <int DIM>
__device__ __forceinline__ void relate_absent(double* centres, int* parent, int* overlap, int oi) {
  neighbors_absent_centre<DIM>(centres + DIM * (size_t)oi);
  parent[oi] = 0;
  overlap[oi] = 0;
}

// The parent of a present row, on one thread: top = the largest counter (0: no parent), p = the smallest label that reaches it, and
// one integer atomicAdd on the parent's children counter.  row0 = the first row of the other set's tile or stack; p <= nt <= its rows, so the counter lies inside the other table.
__device__ __forceinline__ void relate_parent_write(int* parent, int* overlap, int* children_other, int oi, int row0, int top, int p) {
  const bool has = top > 0;
  parent[oi] = has ? p : 0;
  overlap[oi] = has ? top : 0;
  if (has) atomicAdd(&children_other[row0 + p - 1], 1);
}

// the five columns of a row: Parent, ParentOverlap, Children count, Distance_Centroid, Distance_Minimum (NaN without a parent)
__device__ __forceinline__ void relate_row_write(double* out, int p, int overlap, int children, double d_centre, double d_min) {
  out[0] = (double)p;
  out[1] = (double)overlap;
  out[2] = (double)children;
  out[3] = d_centre;
  out[4] = d_min;
}

// The workspace of one side: centres [n, DIM] float64, then parent, overlap and children [n] int32 each, rounded up to 8 bytes (the
// next side starts with float64).
struct RelateSide {
  double* centres;
  int *parent, *overlap, *children;
};
template <int DIM>
static inline size_t relate_side_bytes(int n) { return ((size_t)n * (DIM * sizeof(double) + 3 * sizeof(int)) + 7) & ~(size_t)7; }
template <int DIM>
static inline RelateSide relate_side(unsigned char* base, int n) {
  RelateSide s;
  s.centres = reinterpret_cast<double*>(base);
  s.parent = reinterpret_cast<int*>(base + (size_t)n * DIM * sizeof(double));
  s.overlap = s.parent + n;
  s.children = s.overlap + n;
  return s;
}

#endif  // __HIPCC__
