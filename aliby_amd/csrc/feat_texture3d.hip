// feat_texture3d.hip — Haralick texture of the objects of volume labels [F, Z, Y, X], one channel per call: the texture family of
// BASELINE config 5 (feat_intensity3d.hip, feat_sizeshape3d.hip and feat_coloc3d.hip are the other three).  An EXTENSION like them:
// cp_measure's `texture` takes a 3-D (masks, pixels) pair as it is and mahotas' haralick then walks 13 directions instead of 4;
// neither is vendored, parity is unpinned.  Restated (the 2-D definitions: the header of feat_texture.hip):
//   grey level = uint16 >> 8 or rint(255 f) clipped, rescaled to gray_levels (grey_of, haralick_stats.h);
//   per object: the bounding box in (z, y, x) with every voxel that is not the object's set to 0; for each direction d the
//   symmetric co-occurrence matrix of the voxel pairs (p, p + scale d) inside the box, pairs touching grey level 0 dropped,
//   matrix side = largest grey level of the crop + 1; the 13 statistics of haralick_stats.h.  A direction without a pair gives
//   13 NaN, a label without voxels a row of NaN.  Voxel spacing is not used (CellProfiler's 3-D texture ignores it).
// Directions as offsets on the array axes (z, y, x), column block d of the 13 x 13 output columns.  This is mahotas' _3d_deltas
// AS RECALLED, not as read: the matrix is symmetrised, so any 13 directions covering one half of the 26 neighbours give the same
// 13 x 13 numbers, only the block index of a direction rests on the recall (DESIGN.md "unpinned").  T3_DIRS below is the only
// place the kernel knows the order:
//   (1,0,0) (1,1,0) (0,1,0) (1,-1,0) (0,0,1) (1,0,1) (0,1,1) (1,1,1) (1,-1,1) (1,0,-1) (0,1,-1) (1,1,-1) (1,-1,-1)
//
// Two passes.
//   1. k_c3_table (volume_table.h): voxel count and bounding box per (stack, label), one read of the labels.
//   2. k_texture3d: one workgroup of 256 lanes per object.  The byte crop of the box is built once; the present grey levels are
//      renumbered 0 .. K-1 through a 256-bit presence mask; per direction the K (K + 1) / 2 cells of the symmetric matrix are
//      counted with integer atomics on 32-bit counters (a volume object has tens of thousands of pairs per direction: the 2-D
//      kernel's 16-bit counters overflow and its key sort does not scale), the cells go through haralick_cell into the integer
//      marginals and haralick_marginal_sums / haralick_finish write the 13 numbers.  Crop (T3_LDS_VOXELS bytes) and counters (T3_MAX_CELLS x 4 bytes, every
//      K up to 255) live in LDS together: 152.5 KiB (157.3 with the marginals) of the CU's 160, so ONE workgroup per CU.  Boxes beyond T3_LDS_VOXELS take
//      the same code with both in global scratch (template parameter GLOBAL).
// Reproducibility: the counts are exact integers, the workgroup size is fixed, and every floating-point reduction walks the cells
// and the marginals in an order that depends on the object's own K and levels only: rows are bitwise independent of the run, the
// batch, the other objects of the launch and of which of the two forms ran.
#include "common.h"
#include "haralick_stats.h"
#include "volume_table.h"

typedef unsigned short u16;

#define T3_BLOCK 256
#define T3_NDIR 13
#define T3_LDS_VOXELS 24576                // bytes of the crop in LDS = voxels of the largest bounding box of the LDS form
#define T3_MAX_CELLS (255 * 256 / 2 + 256)  // K (K + 1) / 2 at K = 255, rounded up to 32896: 128.5 KiB of counters
#define T3_GLOBAL_BLOCKS 256
#define T3_GLOBAL_BYTES (1ull << 30)  // ceiling of the global-scratch form's crops and counters, all workgroups together

namespace {

__device__ const int T3_DIRS[T3_NDIR][3] = {{1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {1, -1, 0}, {0, 0, 1}, {1, 0, 1}, {0, 1, 1},
                                            {1, 1, 1}, {1, -1, 1}, {1, 0, -1}, {0, 1, -1}, {1, 1, -1}, {1, -1, -1}};

struct T3Args {
  const u16* labels;
  const void* pixels;  // [F,C,Z,Y,X]
  int F, C, Z, Y, X, channel;
  const int* offsets;       // [F+1]
  const unsigned* count;    // [n]
  const unsigned* bmin;     // [n][z, y, x]
  const unsigned* bmax;     // inclusive
  const int* items;         // GLOBAL: rows of the objects whose box is above the LDS budget
  int n_items;              // GLOBAL: how many; else the number of rows
  unsigned cap;             // GLOBAL: bytes of a crop (multiple of 16) >= the largest box; else T3_LDS_VOXELS
  unsigned char* gscratch;  // GLOBAL: gridDim.x x (cap + 4 T3_MAX_CELLS) bytes
  int scale, gray_levels;
  double* out;
  int ld, col0;
};

template <typename T, bool GLOBAL>
__global__ __launch_bounds__(T3_BLOCK) void k_texture3d(T3Args a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ int hx[256];      // p_x counts
  __shared__ int hplus[512];   // p_{x+y} counts
  __shared__ int hminus[256];  // p_{x-y} counts
  __shared__ double vec[4 * 8];
  __shared__ int red_i[8];
  __shared__ unsigned int bits[8];   // presence of the grey levels 1..255 in the object
  __shared__ unsigned char rk[256];  // grey level -> rank among the present levels
  __shared__ unsigned char lev[256]; // rank -> grey level

  const unsigned cap = GLOBAL ? a.cap : (unsigned)T3_LDS_VOXELS;
  unsigned char* g = GLOBAL ? (a.gscratch + (size_t)blockIdx.x * ((size_t)cap + 4 * (size_t)T3_MAX_CELLS)) : lds_raw;
  unsigned int* cells = reinterpret_cast<unsigned int*>(g + cap);
  const int tid = threadIdx.x;
  const size_t vol = (size_t)a.Z * a.Y * a.X;

  for (int it = blockIdx.x; it < a.n_items; it += gridDim.x) {
    const int row = GLOBAL ? a.items[it] : it;
    double* out = a.out + (size_t)row * a.ld + a.col0;
    if (a.count[row] == 0) {  // a label without voxels
      for (int k = tid; k < T3_NDIR * TX_NSTAT; k += T3_BLOCK) out[k] = NAN;
      continue;
    }
    const unsigned z0 = a.bmin[(size_t)row * 3], y0 = a.bmin[(size_t)row * 3 + 1], x0 = a.bmin[(size_t)row * 3 + 2];
    const int dd = (int)(a.bmax[(size_t)row * 3] - z0 + 1), h = (int)(a.bmax[(size_t)row * 3 + 1] - y0 + 1), w = (int)(a.bmax[(size_t)row * 3 + 2] - x0 + 1);
    const unsigned nbox = (unsigned)dd * (unsigned)h * (unsigned)w;  // (a stack holds at most 2^30 voxels)
    if (GLOBAL ? nbox > cap : nbox > (unsigned)T3_LDS_VOXELS) continue;  // (the other form's object; uniform)
    int f = 0, fhi = a.F;  // the stack of this row: offsets[f] <= row < offsets[f + 1]
    while (fhi - f > 1) { const int mid = (f + fhi) >> 1; if (a.offsets[mid] <= row) f = mid; else fhi = mid; }
    const u16 L = (u16)(row - a.offsets[f] + 1);
    const u16* lab = a.labels + (size_t)f * vol;
    const T* px = reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + a.channel) * vol;

    // ---- byte crop of the box, raster order (z, y, x); four voxels' loads are issued together ----------------------------
    __syncthreads();  // the previous object's crop and marginals are done with
    int gmax = 0;
    for (unsigned i0 = tid; i0 < nbox; i0 += 4 * T3_BLOCK) {
      u16 lb[4];
      T pv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned i = min(i0 + (unsigned)u * T3_BLOCK, nbox - 1);
        const unsigned x = i % (unsigned)w, r = i / (unsigned)w;
        const size_t idx = ((size_t)(z0 + r / (unsigned)h) * a.Y + (y0 + r % (unsigned)h)) * a.X + (x0 + x);
        lb[u] = lab[idx];
        pv[u] = px[idx];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const unsigned i = i0 + (unsigned)u * T3_BLOCK;
        if (i >= nbox) break;
        const int q = lb[u] == L ? grey_of(pv[u], a.gray_levels, 8) : 0;
        g[i] = (unsigned char)q;
        gmax = max(gmax, q);
      }
    }
    const int maxv = block_max_i32(gmax, red_i) + 1;  // side of mahotas' matrix: max grey level + 1
    __syncthreads();
    // ---- present grey levels -> ranks
    if (tid < 8) bits[tid] = 0;
    __syncthreads();
    for (unsigned i = tid; i < nbox; i += T3_BLOCK) {
      const int q = g[i];
      if (q > 0) atomicOr(&bits[q >> 5], 1u << (q & 31));
    }
    __syncthreads();
    int K = 0;
    for (int w8 = 0; w8 < 8; ++w8) K += __popc(bits[w8]);
    for (int q = tid; q < 256; q += T3_BLOCK) {
      if ((bits[q >> 5] >> (q & 31)) & 1u) {
        int r = __popc(bits[q >> 5] & ((1u << (q & 31)) - 1u));
        for (int w8 = 0; w8 < (q >> 5); ++w8) r += __popc(bits[w8]);
        rk[q] = (unsigned char)r;
        lev[r] = (unsigned char)q;
      }
    }
    __syncthreads();
    if (K == 0) {  // grey level 0 throughout: no direction has a pair
      for (int k = tid; k < T3_NDIR * TX_NSTAT; k += T3_BLOCK) out[k] = NAN;
      continue;
    }
    const int minlev = lev[0], maxlev = lev[K - 1];
    const int ncell = K * (K + 1) / 2;  // <= T3_MAX_CELLS (K <= 255: level 0 is never present)

    for (int d = 0; d < T3_NDIR; ++d) {
      const int dz = T3_DIRS[d][0] * a.scale, dy = T3_DIRS[d][1] * a.scale, dx = T3_DIRS[d][2] * a.scale;
      double* fo = out + d * TX_NSTAT;
      // only the occupied ranges of the marginals are ever touched: [minlev, maxlev], [0, maxlev-minlev], [2 minlev, 2 maxlev]
      for (int k = tid; k <= maxlev - minlev; k += T3_BLOCK) { hx[minlev + k] = 0; hminus[k] = 0; }
      for (int k = 2 * minlev + tid; k <= 2 * maxlev; k += T3_BLOCK) hplus[k] = 0;
      for (int k = tid; k < ncell; k += T3_BLOCK) cells[k] = 0;
      __syncthreads();
      // ---- the cells: one integer atomic per voxel pair ------------------------------------------------------------------
      int mine = 0;
      if (dz < dd) {  // (else no pair fits the box: dz >= 0 in every direction)
        for (unsigned i = tid; i < nbox; i += T3_BLOCK) {
          const int va = g[i];
          if (va == 0) continue;
          const unsigned r = i / (unsigned)w;
          const int x2 = (int)(i % (unsigned)w) + dx, y2 = (int)(r % (unsigned)h) + dy, z2 = (int)(r / (unsigned)h) + dz;
          if (x2 < 0 || x2 >= w || y2 < 0 || y2 >= h || z2 >= dd) continue;
          const int vb = g[((unsigned)z2 * (unsigned)h + (unsigned)y2) * (unsigned)w + (unsigned)x2];
          if (vb == 0) continue;
          const int ra = rk[va], rb = rk[vb];
          const int hi = max(ra, rb);
          atomicAdd(&cells[hi * (hi + 1) / 2 + min(ra, rb)], 1u);
          ++mine;
        }
      }
      const int NP = block_sum_i32(mine, red_i);  // ordered voxel pairs (< 2^30); T = 2 NP entries in the symmetric matrix
      __syncthreads();
      if (NP == 0) {
        // mahotas raises ValueError on an empty matrix; CellProfiler records NaN
        for (int k = tid; k < TX_NSTAT; k += T3_BLOCK) fo[k] = NAN;
        __syncthreads();
        continue;
      }
      const double Tt = 2.0 * (double)NP;
      const double logT = log2_int(2 * NP);

      double acc[3] = {0, 0, 0};
      for (int idx = tid; idx < ncell; idx += T3_BLOCK) {
        const int c = (int)cells[idx];
        if (!c) continue;
        const int rh = haralick_tri_row(idx);
        haralick_cell(c, lev[idx - rh * (rh + 1) / 2], lev[rh], Tt, logT, hx, hplus, hminus, acc);
      }
      HaralickSums hs;
      haralick_marginal_sums(hs, acc, hx, hplus, hminus, minlev, maxlev, maxv, Tt, logT, vec);
      double hxy = 0;  // HXY1: second pass over the cells now that p_x is complete
      for (int idx = tid; idx < ncell; idx += T3_BLOCK) {
        const int c = (int)cells[idx];
        if (!c) continue;
        const int rh = haralick_tri_row(idx);
        hxy += haralick_hxy1_term(c, lev[idx - rh * (rh + 1) / 2], lev[rh], hx, Tt, logT);
      }
      haralick_finish(fo, hs, hxy, maxv, vec);
      __syncthreads();
    }
  }
}

template <typename T, bool GLOBAL>
void launch_texture3d(const T3Args& a, int grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((k_texture3d<T, GLOBAL>), dim3(grid), dim3(T3_BLOCK), lds, s, a);
}

}  // namespace

extern "C" int aliby_texture3d_lds_voxels(void) { return T3_LDS_VOXELS; }

extern "C" int aliby_features_texture3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y, int X,
                                        int channel, const int32_t* offsets_host, int scale, int gray_levels, double* out, int ld, int col0,
                                        void* stream) {
  ARG_CHECK(ctx && labels && pixels && offsets_host && out, "texture3d: null argument");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "texture3d: dtype must be ALIBY_U16 or ALIBY_F32");
  ARG_CHECK(F > 0 && C > 0 && Z > 0 && Y > 0 && X > 0, "texture3d: bad shape");
  ARG_CHECK(X <= 65536 && Y <= 65536 && Z <= 65536 && (size_t)Z * Y * X <= (1ull << 30), "texture3d: stack too large");
  ARG_CHECK(channel >= 0 && channel < C, "texture3d: channel out of range");
  ARG_CHECK(scale >= 1 && gray_levels >= 2 && gray_levels <= 256, "texture3d: scale >= 1 and 2 <= gray_levels <= 256");
  ARG_CHECK(offsets_host[0] == 0 && col0 >= 0 && (long long)col0 + T3_NDIR * TX_NSTAT <= ld, "texture3d: bad offsets / output stride");
  for (int f = 0; f < F; ++f) ARG_CHECK(offsets_host[f + 1] >= offsets_host[f] && offsets_host[f + 1] - offsets_host[f] <= 65535, "texture3d: bad offsets");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);
  { const int rcl = haralick_log2_table_ready(ctx, s); if (rcl) return rcl; }

  // scratch: [count n][bmin 3n][bmax 3n][offsets F+1][items n], then (256-byte aligned) the crops and counters of the
  // global-scratch form.  The table is read back: the host needs the rows whose box is above the LDS budget, and the largest.
  const size_t tab_words = (size_t)n * 7, head_words = tab_words + (size_t)(F + 1) + (size_t)n;
  const size_t head_bytes = (head_words * 4 + 255) & ~(size_t)255;
  int rc = aliby_ensure_scratch(ctx, head_bytes);
  if (rc) return rc;
  unsigned* count = (unsigned*)ctx->scratch;
  int* d_off = (int*)(count + tab_words);
  HIP_TRY(hipMemcpyAsync(d_off, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
  rc = volume_table_launch(labels, F, Z, Y, X, d_off, n, count, s);
  if (rc) return rc;
  unsigned* table_host = (unsigned*)malloc(sizeof(unsigned) * tab_words + sizeof(int) * (size_t)n);
  if (!table_host) { aliby_set_error("texture3d: out of host memory"); return ALIBY_ERR_INVALID; }
  int* items_host = (int*)(table_host + tab_words);
  hipError_t e = hipMemcpyAsync(table_host, count, sizeof(unsigned) * tab_words, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && aliby_wait_stream(s) != ALIBY_OK) e = hipErrorUnknown;
  if (e != hipSuccess) { free(table_host); aliby_set_error("texture3d: reading the object table back failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  const unsigned* bmin = table_host + n;
  const unsigned* bmax = table_host + (size_t)n * 4;
  size_t max_box = 0;
  int n_big = 0;
  for (int i = 0; i < n; ++i) {
    if (!table_host[i]) continue;
    const size_t box = (size_t)(bmax[3 * i] - bmin[3 * i] + 1) * (bmax[3 * i + 1] - bmin[3 * i + 1] + 1) * (bmax[3 * i + 2] - bmin[3 * i + 2] + 1);
    if (box > T3_LDS_VOXELS) { items_host[n_big++] = i; max_box = box > max_box ? box : max_box; }
  }
  size_t need = 0;  // bytes of one workgroup's crop and counters in global scratch
  int g = 0;
  if (n_big) {
    const size_t cap = (max_box + 15) & ~(size_t)15;
    need = cap + 4 * (size_t)T3_MAX_CELLS;
    size_t blocks = T3_GLOBAL_BYTES / need;
    if (blocks < 1) blocks = 1;
    g = (int)(blocks < T3_GLOBAL_BLOCKS ? blocks : T3_GLOBAL_BLOCKS);
    if (g > n_big) g = n_big;
    void* before = ctx->scratch;
    rc = aliby_ensure_scratch(ctx, head_bytes + need * (size_t)g);
    if (rc) { free(table_host); return rc; }
    if (ctx->scratch != before) {  // the block moved: put the table and the offsets back
      count = (unsigned*)ctx->scratch;
      d_off = (int*)(count + tab_words);
      e = hipMemcpyAsync(count, table_host, sizeof(unsigned) * tab_words, hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s);
    }
  }
  int* d_items = d_off + (F + 1);
  if (e == hipSuccess && n_big) e = hipMemcpyAsync(d_items, items_host, sizeof(int) * (size_t)n_big, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) { free(table_host); aliby_set_error("texture3d: upload failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }

  T3Args a;
  a.labels = labels; a.pixels = pixels; a.F = F; a.C = C; a.Z = Z; a.Y = Y; a.X = X; a.channel = channel; a.offsets = d_off; a.count = count;
  a.bmin = count + n; a.bmax = count + (size_t)n * 4; a.items = d_items; a.scale = scale; a.gray_levels = gray_levels; a.out = out; a.ld = ld;
  a.col0 = col0;
  {  // rows within the LDS budget, absent labels included (a row of the other form is skipped by its workgroup at once)
    a.n_items = n; a.cap = T3_LDS_VOXELS; a.gscratch = nullptr;
    const size_t lds = (size_t)T3_LDS_VOXELS + 4 * (size_t)T3_MAX_CELLS;
    const void* fn = dtype == ALIBY_U16 ? (const void*)k_texture3d<u16, false> : (const void*)k_texture3d<float, false>;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) {
      if (dtype == ALIBY_U16) launch_texture3d<u16, false>(a, n, lds, s);
      else launch_texture3d<float, false>(a, n, lds, s);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess && n_big) {
    a.n_items = n_big; a.cap = (unsigned)(need - 4 * (size_t)T3_MAX_CELLS); a.gscratch = (unsigned char*)ctx->scratch + head_bytes;
    if (dtype == ALIBY_U16) launch_texture3d<u16, true>(a, g, 0, s);
    else launch_texture3d<float, true>(a, g, 0, s);
    e = hipGetLastError();
  }
  free(table_host);
  if (e != hipSuccess) { aliby_set_error("texture3d: kernel launch failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  // the table and the offsets live in ctx scratch: they must be consumed before the host reuses it
  { const int rcw = aliby_wait_stream(s); if (rcw) return rcw; }
  return ALIBY_OK;
}
