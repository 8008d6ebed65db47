// neighbors_stats.h — what the 2-D `neighbors` kernels (feat_neighbors.hip) and the volume kernels (feat_neighbors3d.hip) share:
// the label bitmap of the scan kernels and their last step (columns 0-1, the centre), the best-two record, and the whole closest-two
// kernel (columns 2-6), templated on the number of axes.  Centres are [rows, DIM] in axis order (z,) y, x, and every sum over the axes
// is a left fold in that order: a stack of one plane (dz = 0) gets the 2-D family's bits in columns 0-5.  Definitions: the headers of
// the two .hip files, where the scan loops stay (their offsets, caps and workgroup sizes differ on purpose).
#pragma once
#include "common.h"

#ifdef __HIPCC__

#define NEIGHBORS_CLOSEST_BLOCK 256  // k_neighbors_closest: one wave per row

// LDS bytes of the bitmap for stacks of at most max_count labels (<= 8 KiB: labels are uint16)
static inline size_t neighbors_bitmap_bytes(int max_count) { return (((size_t)(max_count >> 5) + 1) * sizeof(unsigned int) + 15) & ~(size_t)15; }

// The workgroup size of a scan kernel: BLOCK where the kernel fixes it, blockDim.x (BLOCK = 0) where the launch picks it.
template <int BLOCK>
__device__ __forceinline__ auto neighbors_block() {
  if constexpr (BLOCK > 0) return BLOCK;
  else return (unsigned int)blockDim.x;
}

// The dynamic LDS of a scan kernel (neighbors_bitmap_bytes): one bit per label 1..nt of the scanned object's stack.  All threads of
// the workgroup call clear() and popcount().  (The array is named here, not passed in: a pointer member would be a flat one.)
extern __shared__ __align__(16) unsigned int neighbors_bitmap[];
template <int BLOCK>
struct NeighborsBitmap {
  int nt;  // labels with a bit; a label above it can only come from a wrong count: it has no bit and is not counted
  __device__ __forceinline__ void clear() const {
    for (int k = threadIdx.x; k < (nt >> 5) + 1; k += neighbors_block<BLOCK>()) neighbors_bitmap[k] = 0u;
    __syncthreads();
  }
  // in_s: the offset lies in S.  Two filters: the last label this thread set, a test of the bit (a stale read: a redundant atomic)
  __device__ __forceinline__ void mark(bool in_s, int v, int& last_set) const {
    if (in_s && v <= nt && v != last_set) {
      const unsigned int bit = 1u << (v & 31);
      if (!(reinterpret_cast<volatile unsigned int*>(neighbors_bitmap)[v >> 5] & bit)) atomicOr(&neighbors_bitmap[v >> 5], bit);
      last_set = v;
    }
  }
  __device__ __forceinline__ int popcount() const {  // this thread's share, after a barrier
    int cnt = 0;
    for (int k = threadIdx.x; k < (nt >> 5) + 1; k += neighbors_block<BLOCK>()) cnt += __popc(neighbors_bitmap[k]);
    return cnt;
  }
};

// a row without pixels: NaN in columns 0-1 and in the centre, which is how k_neighbors_closest knows it (and how the kernels of
// feat_relate.hip know an absent object of either set)
template <int DIM>
__device__ __forceinline__ void neighbors_absent_centre(double* ctr) {
  for (int k = DIM; k-- > 0;) ctr[k] = NAN;
}
template <int DIM>
__device__ __forceinline__ void neighbors_absent(double* out, double* ctr) {
  neighbors_absent_centre<DIM>(ctr);
  out[0] = out[1] = NAN;
}

// A centre coordinate: the exact 64-bit coordinate sum over the pixel count, one float64 division.  (feat_relate.hip takes its centres
// from here too.)
__device__ __forceinline__ double neighbors_centre(long long s, int n) { return (double)s / (double)n; }

// The outline predicate of the 2-D family as a function of one pixel: (y, x) of the tile `lab` [Y,X] holds L; it is on L's outline
// when it lies on the first or last row or column of the frame or has an 8-neighbour of another value (0 included).
// k_neighbors_scan finds the same thing inside its walk over the offsets of T, which contain the 3 x 3 square; the kernels that walk
// no offsets (feat_relate.hip: the minimum distance to a parent's outline, the tertiary image) call this.
__device__ __forceinline__ bool neighbors_outline(const unsigned short* lab, int Y, int X, int y, int x, int L) {
  if (y == 0 || y == Y - 1 || x == 0 || x == X - 1) return true;
  const unsigned short* r = lab + (size_t)y * X + x;
  return r[-X - 1] != L || r[-X] != L || r[-X + 1] != L || r[-1] != L || r[1] != L || r[X - 1] != L || r[X] != L || r[X + 1] != L;
}

// The end of a scan kernel, on thread 0 after the block reductions: cnt bits set, n pixels of the object, `outline` of them on its
// outline, `touching` of those in contact, s... = the coordinate sums in axis order.  Columns 0-1 and the centre.
template <typename... Sum>
__device__ __forceinline__ void neighbors_scan_write(double* out, double* ctr, int cnt, int n, int outline, int touching, Sum... s) {
  if (n == 0) return neighbors_absent<sizeof...(Sum)>(out, ctr);  // (a row whose area the labels do not bear out: absent)
  out[0] = (double)cnt;
  out[1] = (double)touching / (double)outline * 100.0;
  ((*ctr++ = neighbors_centre(s, n)), ...);
}

// The two best (key, label) candidates under the order "lower key, then lower label": a total order on distinct labels, so the
// merged result does not depend on which lane saw which row.  INFINITY / INT_MAX: no candidate.
struct NeighborsBest2 {
  double k1 = INFINITY, k2 = INFINITY;
  int l1 = INT_MAX, l2 = INT_MAX;
  static __device__ __forceinline__ bool less(double ka, int la, double kb, int lb) { return ka < kb || (ka == kb && la < lb); }
  __device__ __forceinline__ void insert(double key, int l) {
    if (less(key, l, k1, l1)) {
      k2 = k1; l2 = l1; k1 = key; l1 = l;
    } else if (less(key, l, k2, l2)) {
      k2 = key; l2 = l;
    }
  }
  __device__ __forceinline__ void wave_merge() {  // the lanes of a group hold the best two of the group's rows; groups double
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
      const double p1 = __shfl_xor(k1, m, WAVE), p2 = __shfl_xor(k2, m, WAVE);
      const int q1 = __shfl_xor(l1, m, WAVE), q2 = __shfl_xor(l2, m, WAVE);
      if (less(p1, q1, k1, l1)) {
        const bool mine = less(k1, l1, p2, q2);
        k2 = mine ? k1 : p2; l2 = mine ? l1 : q2;
        k1 = p1; l1 = q1;
      } else if (less(p1, q1, k2, l2)) {
        k2 = p1; l2 = q1;
      }
    }
  }
};

// a . b over the axes, folded from the left: (z z + y y) + x x
template <int DIM>
__device__ __forceinline__ double neighbors_dot(const double (&a)[DIM], const double (&b)[DIM]) {
  double s = a[0] * b[0];
  for (int k = 1; k < DIM; ++k) s = s + a[k] * b[k];
  return s;
}

// |v1 x v2|: the scalar cross product in the plane; in space the components on the axes (z, y, x), of which a stack of one plane leaves
// wz alone.  (fabs(w) and sqrt(w w) can differ in the last bit: column 6 is the one column the two families share only approximately.)
__device__ __forceinline__ double neighbors_cross(const double (&a)[2], const double (&b)[2]) { return fabs(a[1] * b[0] - a[0] * b[1]); }
__device__ __forceinline__ double neighbors_cross(const double (&a)[3], const double (&b)[3]) {
  const double wz = a[2] * b[1] - a[1] * b[2], wy = a[0] * b[2] - a[2] * b[0], wx = a[1] * b[0] - a[0] * b[1];
  return sqrt((wx * wx + wy * wy) + wz * wz);
}

// Columns 2-6, after the scan kernel on the same stream: one wave per row; the lanes stride over the centres of the row's own stack.
// Args supplies rows() and stack_rows(row, lo, hi): the rows [lo, hi) of the stack of `row` (row lo + l - 1 is label l), or false.
template <int DIM, typename Args>
__global__ __launch_bounds__(NEIGHBORS_CLOSEST_BLOCK) void k_neighbors_closest(Args a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int row = blockIdx.x * (NEIGHBORS_CLOSEST_BLOCK / WAVE) + threadIdx.x / WAVE;  // wave-uniform
  if (row >= a.rows()) return;
  double* out = a.out + (size_t)row * a.ld + a.col0 + 2;
  double c[DIM], p[DIM], v1[DIM], v2[DIM];
  for (int k = 0; k < DIM; ++k) c[k] = a.centres[DIM * (size_t)row + k];
  int lo, hi;
  if (c[0] != c[0] || !a.stack_rows(row, lo, hi)) {  // absent (the scan kernel wrote a NaN centre)
    if (lane < 5) out[lane] = NAN;
    return;
  }
  NeighborsBest2 best;
  for (int j = lo + lane; j < hi; j += WAVE) {
    if (j == row) continue;
    for (int k = 0; k < DIM; ++k) p[k] = a.centres[DIM * (size_t)j + k];
    if (p[0] != p[0]) continue;
    for (int k = 0; k < DIM; ++k) p[k] = p[k] - c[k];
    best.insert(neighbors_dot<DIM>(p, p), j - lo + 1);
  }
  best.wave_merge();
  if (lane != 0) return;
  const bool has1 = best.l1 != INT_MAX, has2 = best.l2 != INT_MAX;
  out[0] = has1 ? (double)best.l1 : 0.0;
  out[1] = has1 ? sqrt(best.k1) : 0.0;
  out[2] = has2 ? (double)best.l2 : 0.0;
  out[3] = has2 ? sqrt(best.k2) : 0.0;
  double angle = 0.0;
  if (has2) {
    const double *c1 = a.centres + DIM * (size_t)(lo + best.l1 - 1), *c2 = a.centres + DIM * (size_t)(lo + best.l2 - 1);
    for (int k = 0; k < DIM; ++k) { v1[k] = c1[k] - c[k]; v2[k] = c2[k] - c[k]; }
    angle = (best.k1 == 0.0 || best.k2 == 0.0) ? (double)NAN : atan2(neighbors_cross(v1, v2), neighbors_dot<DIM>(v1, v2)) * (180.0 / M_PI);
  }
  out[4] = angle;
}

template <int DIM, typename Args>
static inline void neighbors_closest_launch(const Args& a, int rows, hipStream_t s) {
  const int per_block = NEIGHBORS_CLOSEST_BLOCK / WAVE;
  hipLaunchKernelGGL((k_neighbors_closest<DIM, Args>), dim3((rows + per_block - 1) / per_block), dim3(NEIGHBORS_CLOSEST_BLOCK), 0, s, a);
}

#endif  // __HIPCC__
