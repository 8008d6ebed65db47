// feat_coloc3d.hip — colocalisation of channel pairs inside the objects of volume labels [F, Z, Y, X]: the multi-channel family
// of BASELINE config 5 (feat_intensity3d.hip and feat_sizeshape3d.hip are the single-channel ones).  An EXTENSION like them:
// CellProfiler's MeasureColocalization is defined on the list of an object's pixels, so it means the same on voxels; parity with
// cp_measure is unpinned.  Eight columns per (object, pair), the 2-D family's: Pearson, Slope, Manders_1/2, RWC_1/2, Costes_1/2
// (definitions: the header of feat_coloc.hip; the arithmetic itself is coloc_stats.h, shared with the 2-D per-pair kernel).
//
// Two passes; the first, the split of the rows between the two forms of the second and the kernel's prologue are volume_table.h,
// shared with feat_texture3d.hip.
//   1. k_volume_table: voxel count and bounding box per (stack, label), one read of the labels.
//   2. k_coloc3d: one workgroup of 256 lanes per (object, pair).  The object's voxels of both channels are gathered from its
//      bounding box in raster order (z, y, x) by order-preserving compaction (volume_gather, volume_table.h) into two float lists,
//      then each list is copied, sorted (bitonic) and reduced to its distinct values in place: the dense rank of a value is its index
//      among them (binary search), so no rank is ever stored, in LDS or in HBM.  16 bytes per voxel: lists up to C3_LDS_VOXELS live in LDS (128 KiB),
//      longer ones in global scratch (template parameter GLOBAL, same code).
// Reproducibility: the workgroup size is fixed and the lane of a voxel, the sort and every reduction tree depend on the object's
// own voxel list only, never on the other objects of the launch, the batch or which of the two forms ran: results are bitwise
// independent of all three (the 2-D kernels size their workgroup by the launch's largest object and are not).
#include "common.h"
#include "coloc_stats.h"
#include "volume_table.h"

typedef unsigned short u16;

#define C3_BLOCK 256
#define C3_LDS_VOXELS 8192  // power of two (the sort pads to one): 4 lists x 4 bytes x 8192 = 128 KiB of the CU's 160
#define C3_PER_LANE 4       // voxels of the bounding box per lane and compaction round
#define C3_MAX_PAIRS 64

namespace {

struct C3Args {
  VolumeArgs v;
  const void* pixels;  // [F,C,Z,Y,X]
  int C;
  const int* pairs;         // [n_pairs][2]
  int cap;                  // GLOBAL: power of two >= the largest voxel count; else C3_LDS_VOXELS
  unsigned char* gscratch;  // GLOBAL: gridDim.x * gridDim.y lists of cap * 16 bytes
  double* out;
  int ld, col0, pair_stride;
  int col_pearson, col_manders, col_rwc, col_costes;  // inside a pair's block of columns, -1 = not requested
  double thr, scale_max;
};

// sorted[0 .. n) ascending -> its distinct values in sorted[0 .. m), m returned to every lane.  In place: a value moves to a
// position at or below its own, and a round's reads (own and left neighbour) come before its writes (the barriers of
// block_compact_slot lie between); the one element a later round reads from an earlier round's range, the last, can only have
// been rewritten with itself.
__device__ __forceinline__ int distinct_in_place(float* sorted, int n, int* wsum) {
  int m = 0;
  for (int i0 = 0; i0 < n; i0 += C3_BLOCK) {
    const int i = i0 + (int)threadIdx.x;
    bool first = false;
    float v = 0.f;
    if (i < n) { v = sorted[i]; first = i == 0 || sorted[i - 1] != v; }
    const int pos = block_compact_slot(first, m, wsum);
    if (first) sorted[pos] = v;
  }
  __syncthreads();
  return m;
}

// dense ranks by lookup: the rank of a value is its index among the object's distinct values of that channel
struct SortedRanks {
  const float* fv;
  const float* sv;
  const float* d1;
  const float* d2;
  int m1, m2;
  static __device__ __forceinline__ int index_of(const float* d, int m, float v) {
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (d[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
  }
  __device__ __forceinline__ double R() const { return (double)max(m1, m2); }  // largest rank (m - 1) + 1
  __device__ __forceinline__ long long diff(int j) const { return llabs((long long)index_of(d1, m1, fv[j]) - (long long)index_of(d2, m2, sv[j])); }
};

template <typename T, bool GLOBAL>
__global__ __launch_bounds__(C3_BLOCK) void k_coloc3d(C3Args a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double vec[4 * 8];
  __shared__ float red_f[8];
  __shared__ int red_i[8];
  __shared__ int wsum[4];
  const int cap = GLOBAL ? a.cap : C3_LDS_VOXELS;
  unsigned char* ws = GLOBAL ? (a.gscratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)cap * 16) : lds_raw;
  float* fv = reinterpret_cast<float*>(ws);
  float* sv = fv + cap;
  float* d1 = sv + cap;
  float* d2 = d1 + cap;
  const int tid = threadIdx.x;
  const int ch0 = a.pairs[2 * blockIdx.y], ch1 = a.pairs[2 * blockIdx.y + 1];
  const size_t vol = (size_t)a.v.Z * a.v.Y * a.v.X;

  for (int it = blockIdx.x; it < a.v.n_items; it += gridDim.x) {
    const int row = volume_row<GLOBAL>(a.v.items, it);
    const unsigned cnt = a.v.count[row];
    if (GLOBAL ? cnt > (unsigned)cap : cnt > (unsigned)C3_LDS_VOXELS) continue;  // (the other form's object; uniform)
    double* out = a.out + (size_t)row * a.ld + a.col0 + (size_t)blockIdx.y * a.pair_stride;
    if (cnt == 0) {  // a label without voxels
      if (tid == 0) {
        if (a.col_pearson >= 0) { out[a.col_pearson] = NAN; out[a.col_pearson + 1] = NAN; }
        if (a.col_manders >= 0) { out[a.col_manders] = NAN; out[a.col_manders + 1] = NAN; }
        if (a.col_rwc >= 0) { out[a.col_rwc] = NAN; out[a.col_rwc + 1] = NAN; }
        if (a.col_costes >= 0) { out[a.col_costes] = NAN; out[a.col_costes + 1] = NAN; }
      }
      continue;
    }
    const int f = volume_stack_of(a.v.offsets, a.v.F, row);
    const u16 L = (u16)(row - a.v.offsets[f] + 1);
    const u16* lab = a.v.labels + (size_t)f * vol;
    const T* p0 = reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + ch0) * vol;
    const T* p1 = reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + ch1) * vol;
    const VolumeBox box = volume_box(a.v.bmin, a.v.bmax, row);

    // ---- gather (raster order): C3_PER_LANE consecutive voxels of the box per lane and round (volume_gather) -------------
    __syncthreads();  // the previous object's lists are done with
    const int base = volume_gather<C3_BLOCK, C3_PER_LANE>(lab, L, box, a.v.Y, a.v.X, wsum, [&](int pos, unsigned, size_t idx) {
      if (pos < cap) { fv[pos] = px_load<T>(p0, idx); sv[pos] = px_load<T>(p1, idx); }  // (pos < count <= cap: a guard, not a path)
    });
    __syncthreads();
    const int N = min(base, cap);

    // ---- RWC: the distinct values of each channel, sorted -----------------------------------------------------------------
    int m1 = 0, m2 = 0;
    if (a.col_rwc >= 0) {
      const int n2 = next_pow2(N);
      for (int i = tid; i < n2; i += C3_BLOCK) { d1[i] = i < N ? fv[i] : INFINITY; d2[i] = i < N ? sv[i] : INFINITY; }
      block_bitonic_sort(d1, n2);
      block_bitonic_sort(d2, n2);
      m1 = distinct_in_place(d1, N, wsum);
      m2 = distinct_in_place(d2, N, wsum);
    }
    coloc_block_stats(fv, sv, N, out, a.col_pearson, a.col_manders, a.col_rwc, a.col_costes, a.thr, a.scale_max,
                      SortedRanks{fv, sv, d1, d2, m1, m2}, vec, red_f, red_i);
    __syncthreads();
  }
}

}  // namespace

extern "C" int aliby_coloc3d_lds_voxels(void) { return C3_LDS_VOXELS; }

extern "C" int aliby_features_coloc3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y, int X,
                                      const int32_t* pairs_host, int n_pairs, const int32_t* offsets_host, double* out, int ld, int col0,
                                      int pair_stride, int col_pearson, int col_manders, int col_rwc, int col_costes, double thr_percent,
                                      double costes_scale_max, void* stream) {
  ARG_CHECK(ctx && labels && pixels && pairs_host && offsets_host && out, "coloc3d: null argument");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "coloc3d: dtype must be ALIBY_U16 or ALIBY_F32");
  if (!volume_shape_ok("coloc3d", F, Z, Y, X, offsets_host, 1ull << 30)) return ALIBY_ERR_INVALID;
  ARG_CHECK(C > 0, "coloc3d: bad shape");
  ARG_CHECK(n_pairs > 0 && n_pairs <= C3_MAX_PAIRS, "coloc3d: between 1 and 64 channel pairs per call");
  for (int p = 0; p < n_pairs; ++p) {
    ARG_CHECK(pairs_host[2 * p] >= 0 && pairs_host[2 * p] < C && pairs_host[2 * p + 1] >= 0 && pairs_host[2 * p + 1] < C,
              "coloc3d: channel out of range");
    ARG_CHECK(pairs_host[2 * p] != pairs_host[2 * p + 1], "coloc3d: a pair needs two different channels");
  }
  const int cols[4] = {col_pearson, col_manders, col_rwc, col_costes};
  for (int k = 0; k < 4; ++k) ARG_CHECK(cols[k] < 0 || cols[k] + 2 <= pair_stride, "coloc3d: a metric's columns exceed the pair's block");
  ARG_CHECK(col0 >= 0 && pair_stride >= 0 && (long long)col0 + (long long)n_pairs * pair_stride <= ld, "coloc3d: bad output stride");
  ARG_CHECK(costes_scale_max > 0.0 && costes_scale_max < 1e300 && thr_percent == thr_percent, "coloc3d: bad thr / scale_max");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);

  // a row is measured by its voxel count; a workgroup of the global-scratch form holds four lists of the next power of two (the
  // sort pads to one) of the largest count, and there is one per (grid column, pair); the pairs travel as the plan's extra words
  VolumePlan plan;
  const int rc = volume_plan(
      ctx, labels, F, Z, Y, X, offsets_host, pairs_host, 2 * (size_t)n_pairs, C3_LDS_VOXELS,
      [](unsigned count, const unsigned*, const unsigned*) { return (size_t)count; },
      [](size_t max_count) { size_t cap = C3_LDS_VOXELS; while (cap < max_count) cap <<= 1; return cap * 16; }, (size_t)n_pairs, s, &plan, "coloc3d");
  if (rc) return rc;

  C3Args a;
  a.v = plan.args; a.pixels = pixels; a.C = C; a.pairs = plan.d_extra; a.out = out; a.ld = ld; a.col0 = col0;
  a.pair_stride = pair_stride; a.col_pearson = col_pearson; a.col_manders = col_manders; a.col_rwc = col_rwc; a.col_costes = col_costes;
  a.thr = thr_percent; a.scale_max = costes_scale_max;
  hipError_t e = hipSuccess;
  if (plan.n_big < n) {  // rows within the LDS budget, absent labels included; not launched when every row is of the other form
    a.cap = C3_LDS_VOXELS; a.gscratch = nullptr;
    e = volume_launch(dtype, k_coloc3d<u16, false>, k_coloc3d<float, false>, a, dim3(n, n_pairs), C3_BLOCK, (size_t)C3_LDS_VOXELS * 16, s);
  }
  if (e == hipSuccess && plan.n_big) {
    a.v.n_items = plan.n_big; a.cap = (int)(plan.need / 16); a.gscratch = plan.gscratch;
    e = volume_launch(dtype, k_coloc3d<u16, true>, k_coloc3d<float, true>, a, dim3(plan.grid_big, n_pairs), C3_BLOCK, 0, s);
  }
  if (e != hipSuccess) { aliby_set_error("coloc3d: kernel launch failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  // the table, offsets and pairs live in ctx scratch: they must be consumed before the host reuses it
  return aliby_wait_stream(s);
}
