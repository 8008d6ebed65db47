// feat_coloc3d.hip — colocalisation of channel pairs inside the objects of volume labels [F, Z, Y, X]: the multi-channel family
// of BASELINE config 5 (feat_intensity3d.hip and feat_sizeshape3d.hip are the single-channel ones).  An EXTENSION like them:
// CellProfiler's MeasureColocalization is defined on the list of an object's pixels, so it means the same on voxels; parity with
// cp_measure is unpinned.  Eight columns per (object, pair), the 2-D family's: Pearson, Slope, Manders_1/2, RWC_1/2, Costes_1/2
// (definitions: the header of feat_coloc.hip; the arithmetic itself is coloc_stats.h, shared with the 2-D per-pair kernel).
//
// Two passes.
//   1. k_c3_table (volume_table.h): voxel count and bounding box per (stack, label), one read of the labels.  A lane walks 16 voxels of a row and
//      flushes once per run of equal labels; integer atomics only, so the table is exact whatever the order.
//   2. k_coloc3d: one workgroup of 256 lanes per (object, pair).  The object's voxels of both channels are gathered from its
//      bounding box in raster order (z, y, x) by order-preserving compaction into two float lists, then each list is copied,
//      sorted (bitonic) and reduced to its distinct values in place: the dense rank of a value is its index among them (binary
//      search), so no rank is ever stored, in LDS or in HBM.  16 bytes per voxel: lists up to C3_LDS_VOXELS live in LDS (128 KiB),
//      longer ones in global scratch (template parameter GLOBAL, same code).
// Reproducibility: the workgroup size is fixed and the lane of a voxel, the sort and every reduction tree depend on the object's
// own voxel list only, never on the other objects of the launch, the batch or which of the two forms ran: results are bitwise
// independent of all three (the 2-D kernels size their workgroup by the launch's largest object and are not).
#include "common.h"
#include "coloc_stats.h"
#include "volume_table.h"  // k_c3_table, shared with feat_texture3d.hip

typedef unsigned short u16;

#define C3_BLOCK 256
#define C3_LDS_VOXELS 8192  // power of two (the sort pads to one): 4 lists x 4 bytes x 8192 = 128 KiB of the CU's 160
#define C3_PER_LANE 4       // voxels of the bounding box per lane and compaction round
#define C3_MAX_PAIRS 64
#define C3_GLOBAL_BLOCKS 256
#define C3_GLOBAL_BYTES (1ull << 30)  // ceiling of the global-scratch form's lists, all workgroups together

namespace {

struct C3Args {
  const u16* labels;
  const void* pixels;  // [F,C,Z,Y,X]
  int F, C, Z, Y, X;
  const int* offsets;       // [F+1]
  const unsigned* count;    // [n]
  const unsigned* bmin;     // [n][z, y, x]
  const unsigned* bmax;     // inclusive
  const int* pairs;         // [n_pairs][2]
  const int* items;         // GLOBAL: rows of the objects above the LDS budget
  int n_items;              // GLOBAL: how many; else the number of rows
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
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ch0 = a.pairs[2 * blockIdx.y], ch1 = a.pairs[2 * blockIdx.y + 1];
  const size_t vol = (size_t)a.Z * a.Y * a.X;

  for (int it = blockIdx.x; it < a.n_items; it += gridDim.x) {
    const int row = GLOBAL ? a.items[it] : it;
    const unsigned cnt = a.count[row];
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
    int f = 0, fhi = a.F;  // the stack of this row: offsets[f] <= row < offsets[f + 1]
    while (fhi - f > 1) { const int mid = (f + fhi) >> 1; if (a.offsets[mid] <= row) f = mid; else fhi = mid; }
    const u16 L = (u16)(row - a.offsets[f] + 1);
    const u16* lab = a.labels + (size_t)f * vol;
    const T* p0 = reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + ch0) * vol;
    const T* p1 = reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + ch1) * vol;
    const unsigned z0 = a.bmin[(size_t)row * 3], y0 = a.bmin[(size_t)row * 3 + 1], x0 = a.bmin[(size_t)row * 3 + 2];
    const unsigned h = a.bmax[(size_t)row * 3 + 1] - y0 + 1, w = a.bmax[(size_t)row * 3 + 2] - x0 + 1;
    const unsigned nbox = (a.bmax[(size_t)row * 3] - z0 + 1) * h * w;  // (a stack holds at most 2^30 voxels)

    // ---- gather (raster order): C3_PER_LANE consecutive voxels of the box per lane and round -----------------------------
    __syncthreads();  // the previous object's lists are done with
    int base = 0;
    for (unsigned i0 = 0; i0 < nbox; i0 += C3_BLOCK * C3_PER_LANE) {
      size_t idx[C3_PER_LANE];
      unsigned in = 0;
#pragma unroll
      for (int k = 0; k < C3_PER_LANE; ++k) {
        const unsigned i = i0 + (unsigned)tid * C3_PER_LANE + k;
        idx[k] = 0;
        if (i < nbox) {
          const unsigned x = i % w, r = i / w;
          idx[k] = ((size_t)(z0 + r / h) * a.Y + (y0 + r % h)) * a.X + (x0 + x);
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
      for (int i = 0; i < C3_BLOCK / 64; ++i) { const int s = wsum[i]; if (i < wid) off += s; tot += s; }
      int pos = base + off + incl - c;
      base += tot;
#pragma unroll
      for (int k = 0; k < C3_PER_LANE; ++k) {
        if (!(in & (1u << k))) continue;
        if (pos < cap) { fv[pos] = px_load<T>(p0, idx[k]); sv[pos] = px_load<T>(p1, idx[k]); }  // (pos < count <= cap: a guard, not a path)
        ++pos;
      }
    }
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

template <typename T, bool GLOBAL>
void launch_coloc3d(const C3Args& a, dim3 grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((k_coloc3d<T, GLOBAL>), grid, dim3(C3_BLOCK), lds, s, a);
}

}  // namespace

extern "C" int aliby_coloc3d_lds_voxels(void) { return C3_LDS_VOXELS; }

extern "C" int aliby_features_coloc3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y, int X,
                                      const int32_t* pairs_host, int n_pairs, const int32_t* offsets_host, double* out, int ld, int col0,
                                      int pair_stride, int col_pearson, int col_manders, int col_rwc, int col_costes, double thr_percent,
                                      double costes_scale_max, void* stream) {
  ARG_CHECK(ctx && labels && pixels && pairs_host && offsets_host && out, "coloc3d: null argument");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "coloc3d: dtype must be ALIBY_U16 or ALIBY_F32");
  ARG_CHECK(F > 0 && C > 0 && Z > 0 && Y > 0 && X > 0, "coloc3d: bad shape");
  ARG_CHECK(X <= 65536 && Y <= 65536 && Z <= 65536 && (size_t)Z * Y * X <= (1ull << 30), "coloc3d: stack too large");
  ARG_CHECK(n_pairs > 0 && n_pairs <= C3_MAX_PAIRS, "coloc3d: between 1 and 64 channel pairs per call");
  for (int p = 0; p < n_pairs; ++p) {
    ARG_CHECK(pairs_host[2 * p] >= 0 && pairs_host[2 * p] < C && pairs_host[2 * p + 1] >= 0 && pairs_host[2 * p + 1] < C,
              "coloc3d: channel out of range");
    ARG_CHECK(pairs_host[2 * p] != pairs_host[2 * p + 1], "coloc3d: a pair needs two different channels");
  }
  const int cols[4] = {col_pearson, col_manders, col_rwc, col_costes};
  for (int k = 0; k < 4; ++k) ARG_CHECK(cols[k] < 0 || cols[k] + 2 <= pair_stride, "coloc3d: a metric's columns exceed the pair's block");
  ARG_CHECK(offsets_host[0] == 0 && col0 >= 0 && pair_stride >= 0 && (long long)col0 + (long long)n_pairs * pair_stride <= ld,
            "coloc3d: bad offsets / output stride");
  for (int f = 0; f < F; ++f) ARG_CHECK(offsets_host[f + 1] >= offsets_host[f] && offsets_host[f + 1] - offsets_host[f] <= 65535, "coloc3d: bad offsets");
  ARG_CHECK(costes_scale_max > 0.0 && costes_scale_max < 1e300 && thr_percent == thr_percent, "coloc3d: bad thr / scale_max");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);

  // scratch: [count n][bmin 3n][bmax 3n][offsets F+1][pairs 2 n_pairs][items n], then (16-byte aligned) the lists of the
  // global-scratch form.  The table is read back: the host needs the largest count and the rows above the LDS budget.
  const size_t tab_words = (size_t)n * 7, head_words = tab_words + (size_t)(F + 1) + 2 * (size_t)n_pairs + (size_t)n;
  const size_t head_bytes = (head_words * 4 + 255) & ~(size_t)255;
  int rc = aliby_ensure_scratch(ctx, head_bytes);
  if (rc) return rc;
  unsigned* count = (unsigned*)ctx->scratch;
  int* d_off = (int*)(count + tab_words);
  HIP_TRY(hipMemcpyAsync(d_off, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
  rc = volume_table_launch(labels, F, Z, Y, X, d_off, n, count, s);
  if (rc) return rc;
  unsigned* table_host = (unsigned*)malloc(sizeof(unsigned) * tab_words + sizeof(int) * (size_t)n);
  if (!table_host) { aliby_set_error("coloc3d: out of host memory"); return ALIBY_ERR_INVALID; }
  int* items_host = (int*)(table_host + tab_words);
  hipError_t e = hipMemcpyAsync(table_host, count, sizeof(unsigned) * tab_words, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && aliby_wait_stream(s) != ALIBY_OK) e = hipErrorUnknown;
  if (e != hipSuccess) { free(table_host); aliby_set_error("coloc3d: reading the object table back failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  unsigned max_count = 0;
  int n_big = 0;
  for (int i = 0; i < n; ++i) {
    max_count = table_host[i] > max_count ? table_host[i] : max_count;
    if (table_host[i] > C3_LDS_VOXELS) items_host[n_big++] = i;
  }
  size_t need = 0;  // bytes of one global-scratch list set
  int g = 0;
  if (n_big) {
    size_t cap = C3_LDS_VOXELS;
    while (cap < max_count) cap <<= 1;
    need = cap * 16;
    size_t blocks = C3_GLOBAL_BYTES / need / (size_t)n_pairs;
    if (blocks < 1) blocks = 1;
    g = (int)(blocks < C3_GLOBAL_BLOCKS ? blocks : C3_GLOBAL_BLOCKS);
    if (g > n_big) g = n_big;
    void* before = ctx->scratch;
    rc = aliby_ensure_scratch(ctx, head_bytes + need * (size_t)g * (size_t)n_pairs);
    if (rc) { free(table_host); return rc; }
    if (ctx->scratch != before) {  // the block moved: put the table and the offsets back
      count = (unsigned*)ctx->scratch;
      d_off = (int*)(count + tab_words);
      e = hipMemcpyAsync(count, table_host, sizeof(unsigned) * tab_words, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s);
    }
  }
  int* d_pairs = d_off + (F + 1);
  int* d_items = d_pairs + 2 * n_pairs;
  if (e == hipSuccess) e = hipMemcpyAsync(d_pairs, pairs_host, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && n_big) e = hipMemcpyAsync(d_items, items_host, sizeof(int) * (size_t)n_big, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { free(table_host); aliby_set_error("coloc3d: upload failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }

  C3Args a;
  a.labels = labels; a.pixels = pixels; a.F = F; a.C = C; a.Z = Z; a.Y = Y; a.X = X; a.offsets = d_off; a.count = count;
  a.bmin = count + n; a.bmax = count + (size_t)n * 4; a.pairs = d_pairs; a.items = d_items; a.out = out; a.ld = ld; a.col0 = col0;
  a.pair_stride = pair_stride; a.col_pearson = col_pearson; a.col_manders = col_manders; a.col_rwc = col_rwc; a.col_costes = col_costes;
  a.thr = thr_percent; a.scale_max = costes_scale_max;
  if (n_big < n) {  // rows within the LDS budget, absent labels included
    a.n_items = n; a.cap = C3_LDS_VOXELS; a.gscratch = nullptr;
    const size_t lds = (size_t)C3_LDS_VOXELS * 16;
    const void* fn = dtype == ALIBY_U16 ? (const void*)k_coloc3d<u16, false> : (const void*)k_coloc3d<float, false>;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) {
      if (dtype == ALIBY_U16) launch_coloc3d<u16, false>(a, dim3(n, n_pairs), lds, s);
      else launch_coloc3d<float, false>(a, dim3(n, n_pairs), lds, s);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess && n_big) {
    a.n_items = n_big; a.cap = (int)(need / 16); a.gscratch = (unsigned char*)ctx->scratch + head_bytes;
    if (dtype == ALIBY_U16) launch_coloc3d<u16, true>(a, dim3(g, n_pairs), 0, s);
    else launch_coloc3d<float, true>(a, dim3(g, n_pairs), 0, s);
    e = hipGetLastError();
  }
  free(table_host);
  if (e != hipSuccess) { aliby_set_error("coloc3d: kernel launch failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  // the table, offsets and pairs live in ctx scratch: they must be consumed before the host reuses it
  { const int rcw = aliby_wait_stream(s); if (rcw) return rcw; }
  return ALIBY_OK;
}
