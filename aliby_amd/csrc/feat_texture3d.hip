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
// Two passes; the first, the split of the rows between the two forms of the second and the kernel's prologue are volume_table.h,
// shared with feat_coloc3d.hip.
//   1. k_volume_table: voxel count and bounding box per (stack, label), one read of the labels.
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

namespace {

__device__ const int T3_DIRS[T3_NDIR][3] = {{1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {1, -1, 0}, {0, 0, 1}, {1, 0, 1}, {0, 1, 1},
                                            {1, 1, 1}, {1, -1, 1}, {1, 0, -1}, {0, 1, -1}, {1, 1, -1}, {1, -1, -1}};

struct T3Args {
  VolumeArgs v;        // (items: the rows whose box is above the LDS budget)
  const void* pixels;  // [F,C,Z,Y,X]
  int C, channel;
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
  const size_t vol = (size_t)a.v.Z * a.v.Y * a.v.X;

  for (int it = blockIdx.x; it < a.v.n_items; it += gridDim.x) {
    const int row = volume_row<GLOBAL>(a.v.items, it);
    double* out = a.out + (size_t)row * a.ld + a.col0;
    if (a.v.count[row] == 0) {  // a label without voxels
      for (int k = tid; k < T3_NDIR * TX_NSTAT; k += T3_BLOCK) out[k] = NAN;
      continue;
    }
    const VolumeBox box = volume_box(a.v.bmin, a.v.bmax, row);
    const int dd = (int)box.d, h = (int)box.h, w = (int)box.w;
    const unsigned nbox = box.nbox;
    if (GLOBAL ? nbox > cap : nbox > (unsigned)T3_LDS_VOXELS) continue;  // (the other form's object; uniform)
    const int f = volume_stack_of(a.v.offsets, a.v.F, row);
    const u16 L = (u16)(row - a.v.offsets[f] + 1);
    const u16* lab = a.v.labels + (size_t)f * vol;
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
        const size_t idx = box.index(i, a.v.Y, a.v.X);
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

}  // namespace

extern "C" int aliby_texture3d_lds_voxels(void) { return T3_LDS_VOXELS; }

extern "C" int aliby_features_texture3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y, int X,
                                        int channel, const int32_t* offsets_host, int scale, int gray_levels, double* out, int ld, int col0,
                                        void* stream) {
  ARG_CHECK(ctx && labels && pixels && offsets_host && out, "texture3d: null argument");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "texture3d: dtype must be ALIBY_U16 or ALIBY_F32");
  if (!volume_shape_ok("texture3d", F, Z, Y, X, offsets_host, 1ull << 30)) return ALIBY_ERR_INVALID;
  ARG_CHECK(C > 0 && channel >= 0 && channel < C, "texture3d: channel out of range");
  ARG_CHECK(scale >= 1 && gray_levels >= 2 && gray_levels <= 256, "texture3d: scale >= 1 and 2 <= gray_levels <= 256");
  ARG_CHECK(col0 >= 0 && (long long)col0 + T3_NDIR * TX_NSTAT <= ld, "texture3d: bad output stride");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);
  { const int rcl = haralick_log2_table_ready(ctx, s); if (rcl) return rcl; }

  // a row is measured by the volume of its box (an absent label: 0); a workgroup of the global-scratch form holds the crop of the
  // largest box, rounded up to 16 bytes, and the counters
  VolumePlan plan;
  const int rc = volume_plan(
      ctx, labels, F, Z, Y, X, offsets_host, nullptr, 0, T3_LDS_VOXELS,
      [](unsigned count, const unsigned* lo, const unsigned* hi) {
        return count ? (size_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1) : (size_t)0;
      },
      [](size_t max_box) { return ((max_box + 15) & ~(size_t)15) + 4 * (size_t)T3_MAX_CELLS; }, 1, s, &plan, "texture3d");
  if (rc) return rc;

  T3Args a;
  a.v = plan.args; a.pixels = pixels; a.C = C; a.channel = channel; a.scale = scale; a.gray_levels = gray_levels; a.out = out; a.ld = ld;
  a.col0 = col0;
  // rows within the LDS budget, absent labels included.  Launched even when every row is of the other form (coloc3d skips it then):
  // its workgroup skips such a row at once
  a.cap = T3_LDS_VOXELS; a.gscratch = nullptr;
  hipError_t e = volume_launch(dtype, k_texture3d<u16, false>, k_texture3d<float, false>, a, dim3(n), T3_BLOCK,
                               (size_t)T3_LDS_VOXELS + 4 * (size_t)T3_MAX_CELLS, s);
  if (e == hipSuccess && plan.n_big) {
    a.v.n_items = plan.n_big; a.cap = (unsigned)(plan.need - 4 * (size_t)T3_MAX_CELLS); a.gscratch = plan.gscratch;
    e = volume_launch(dtype, k_texture3d<u16, true>, k_texture3d<float, true>, a, dim3(plan.grid_big), T3_BLOCK, 0, s);
  }
  if (e != hipSuccess) { aliby_set_error("texture3d: kernel launch failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  // the table and the offsets live in ctx scratch: they must be consumed before the host reuses it
  return aliby_wait_stream(s);
}
