// feat_texture.hip — cp_measure "texture" (Haralick), one workgroup per (object, channel).
//
// Reference call site: wrap_cp_measure_features (extraction/core/functions/loaders.py:135-150) with
// fun = get_core_measurements()["texture"] (default feature list, pipe_builder.py:49-56).
// cp_measure 0.1.17 / mahotas 1.4.18 are not vendored; restated from CellProfiler's MeasureTexture
// and mahotas.features.haralick(distance=scale, ignore_zeros=True):
//   grey level = uint16 >> 8 (skimage img_as_ubyte) or rint(255 f) for [0,1] floats;
//   per object: bbox crop, non-object pixels = 0; symmetric co-occurrence at distance `scale` for the
//   directions (0,1),(1,1),(1,0),(1,-1); pairs touching grey level 0 are dropped; 13 statistics.
//
// MI355X shape: a 256x256 co-occurrence matrix does not fit LDS in any useful way and is >99% empty for
// a ~1k-pixel object, so the matrix is kept SPARSE: the (lo,hi) grey-level pair of every pixel pair is
// a 16-bit key, keys are bitonic-sorted in LDS, equal-key runs are the non-zero cells.  Objects with few
// distinct grey levels K (the common case: ~30 for a nucleus) skip the sort: levels are renumbered 0..K-1
// through a 256-bit presence mask and the K(K+1)/2 cells of the symmetric matrix are counted directly with
// integer LDS atomics (16-bit counters, two per word) in the memory the keys would have used.  Marginals
// (p_x, p_{x+y}, p_{x-y}) are integer LDS histograms, so every statistic is exact-integer counts
// divided once by the total: no atomics on floats, run-to-run deterministic.
#include "common.h"
#include "object_launch.h"
#include "haralick_stats.h"  // grey_of, the log2 table, cells -> marginals -> the 13 statistics (shared with feat_texture3d.hip)

typedef unsigned short u16;

struct TextureArgs {
  const u16* labels;
  const void* planes;
  int F, C, Y, X, channel;
  const aliby_object* tab;
  int n_obj;
  int cap_pix;   // >= max bbox area (bytes for the grey crop), multiple of 16
  int cap_keys;  // power of two >= max area
  int cap_cells; // 16-bit cell counters that fit the key area (0: dense path off, an area could overflow 16 bits)
  unsigned char* gscratch;
  int scale, gray_levels;
  int grey_shift;  // 8: uint16 pixels; 0: uint8 pixels in uint16 storage (ALIBY_U8W)
  double* out;
  int ld, col0;
};

template <typename T, bool GLOBAL>
__global__ __launch_bounds__(256) void k_texture(TextureArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ int hx[256];      // p_x counts
  __shared__ int hplus[512];   // p_{x+y} counts
  __shared__ int hminus[256];  // p_{x-y} counts
  __shared__ double vec[4 * 8];
  __shared__ int red_i[8];
  __shared__ int wsum[4];
  __shared__ unsigned int bits[8];     // presence of the grey levels 1..255 in the object
  __shared__ unsigned char rk[256];    // grey level -> rank among the present levels
  __shared__ unsigned char lev[256];   // rank -> grey level

  unsigned char* ws = GLOBAL ? (a.gscratch + (size_t)blockIdx.x * ((size_t)a.cap_pix + (size_t)a.cap_keys * 4)) : lds_raw;
  unsigned char* g = ws;
  unsigned int* keys = reinterpret_cast<unsigned int*>(ws + a.cap_pix);
  const int tid = threadIdx.x;
  const size_t plane = (size_t)a.Y * a.X;
  const int DY[4] = {0, 1, 1, 1}, DX[4] = {1, 1, 0, -1};

  for (int oi = blockIdx.x; oi < a.n_obj; oi += gridDim.x) {
    const aliby_object o = a.tab[oi];
    double* out = a.out + (size_t)oi * a.ld + a.col0;
    if (o.area <= 0) {
      for (int k = tid; k < 4 * TX_NSTAT; k += blockDim.x) out[k] = NAN;
      continue;
    }
    const u16* lab = a.labels + (size_t)o.tile * plane;
    const T* px = reinterpret_cast<const T*>(a.planes) + ((size_t)o.tile * a.C + a.channel) * plane;
    const int h = o.y1 - o.y0, w = o.x1 - o.x0, npix = h * w;
    const u16 L = (u16)o.label;

    __syncthreads();
    int gmax = 0;
    // (the loads of four pixels are issued together: one memory latency per batch, see feat_intensity.hip)
    for (int i0 = tid; i0 < npix; i0 += 4 * blockDim.x) {
      u16 lb[4];
      T pv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = min(i0 + u * (int)blockDim.x, npix - 1);
        const size_t idx = (size_t)(o.y0 + i / w) * a.X + (o.x0 + i % w);
        lb[u] = lab[idx];
        pv[u] = px[idx];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * (int)blockDim.x;
        if (i >= npix) break;
        const int q = lb[u] == L ? grey_of(pv[u], a.gray_levels, a.grey_shift) : 0;
        g[i] = (unsigned char)q;
        gmax = max(gmax, q);
      }
    }
    const int maxv = block_max_i32(gmax, red_i) + 1;  // side of mahotas' matrix: max grey level + 1
    __syncthreads();
    // ---- present grey levels -> ranks
    if (tid < 8) bits[tid] = 0;
    __syncthreads();
    for (int i = tid; i < npix; i += blockDim.x) {
      const int q = g[i];
      if (q > 0) atomicOr(&bits[q >> 5], 1u << (q & 31));
    }
    __syncthreads();
    int K = 0;
    for (int w8 = 0; w8 < 8; ++w8) K += __popc(bits[w8]);
    for (int q = tid; q < 256; q += blockDim.x) {
      if ((bits[q >> 5] >> (q & 31)) & 1u) {
        int r = __popc(bits[q >> 5] & ((1u << (q & 31)) - 1u));
        for (int w8 = 0; w8 < (q >> 5); ++w8) r += __popc(bits[w8]);
        rk[q] = (unsigned char)r;
        lev[r] = (unsigned char)q;
      }
    }
    __syncthreads();
    const int minlev = K ? lev[0] : 0, maxlev = K ? lev[K - 1] : 0;
    const int ncell = K * (K + 1) / 2;
    const bool dense = !GLOBAL && ncell > 0 && ncell <= a.cap_cells;
    unsigned int* cells = keys;  // two 16-bit counters per word

    for (int d = 0; d < 4; ++d) {
      const int dy = DY[d] * a.scale, dx = DX[d] * a.scale;
      double* fo = out + d * TX_NSTAT;
      // only the occupied ranges of the marginals are ever touched: [minlev, maxlev], [0, maxlev-minlev], [2 minlev, 2 maxlev]
      for (int k = tid; k <= maxlev - minlev; k += blockDim.x) { hx[minlev + k] = 0; hminus[k] = 0; }
      for (int k = 2 * minlev + tid; k <= 2 * maxlev; k += blockDim.x) hplus[k] = 0;
      int NP;
      if (dense) {
        // ---- direct counting of the K(K+1)/2 cells --------------------------------------------------
        for (int k = tid; k < (ncell + 1) / 2; k += blockDim.x) cells[k] = 0;
        __syncthreads();
        int mine = 0;
        for (int i = tid; i < npix; i += blockDim.x) {
          const int r = i / w, c = i % w, r2 = r + dy, c2 = c + dx;
          if (r2 >= 0 && r2 < h && c2 >= 0 && c2 < w) {
            const int va = g[i], vb = g[r2 * w + c2];
            if (va > 0 && vb > 0) {
              const int ra = rk[va], rb = rk[vb];
              const int hi = max(ra, rb), idx = hi * (hi + 1) / 2 + min(ra, rb);
              atomicAdd(&cells[idx >> 1], (idx & 1) ? 65536u : 1u);
              ++mine;
            }
          }
        }
        NP = block_sum_i32(mine, red_i);
        __syncthreads();
      } else {
        // ---- pair keys (order-preserving compaction is unnecessary: keys get sorted) ----------
        int base = 0;
        for (int i0 = 0; i0 < npix; i0 += blockDim.x) {
          const int i = i0 + tid;
          bool ok = false;
          unsigned int key = 0;
          if (i < npix) {
            const int r = i / w, c = i % w, r2 = r + dy, c2 = c + dx;
            if (r2 >= 0 && r2 < h && c2 >= 0 && c2 < w) {
              const int va = g[i], vb = g[r2 * w + c2];
              if (va > 0 && vb > 0) {
                ok = true;
                key = (unsigned)(min(va, vb) << 8) | (unsigned)max(va, vb);
              }
            }
          }
          const int pos = block_compact_slot(ok, base, wsum);
          if (ok) keys[pos] = key;
        }
        __syncthreads();
        NP = base;  // ordered pixel pairs; T = 2*NP entries in the symmetric matrix
      }
      if (NP == 0) {
        // mahotas raises ValueError on an empty matrix; CellProfiler records NaN
        for (int k = tid; k < TX_NSTAT; k += blockDim.x) fo[k] = NAN;
        __syncthreads();
        continue;
      }
      const double Tt = 2.0 * (double)NP;
      const double logT = log2_int(2 * NP);
      if (!dense) {
        const int n2 = next_pow2(NP);
        for (int i = NP + tid; i < n2; i += blockDim.x) keys[i] = 0xFFFFFFFFu;
        block_bitonic_sort(keys, n2);
      }

      // ---- non-zero cells -> integer marginals + cell sums ------------------------------------------
      double acc[3] = {0, 0, 0};  // sum p^2 (as counts^2), sum i*j*count, sum p*log2(p)
      auto cell1 = [&](int c, int lo, int hi) { haralick_cell(c, lo, hi, Tt, logT, hx, hplus, hminus, acc); };
      auto dense_cell = [&](int idx, int& c, int& lo, int& hi) {  // triangular index -> (count, levels)
        c = (int)((cells[idx >> 1] >> (16 * (idx & 1))) & 0xffffu);
        const int rh = haralick_tri_row(idx);
        lo = lev[idx - rh * (rh + 1) / 2];
        hi = lev[rh];
      };
      if (dense) {
        for (int idx = tid; idx < ncell; idx += blockDim.x) {
          int c, lo, hi;
          dense_cell(idx, c, lo, hi);
          if (c) cell1(c, lo, hi);
        }
      } else {
        for (int i = tid; i < NP; i += blockDim.x) {
          const unsigned int key = keys[i];
          if (i > 0 && keys[i - 1] == key) continue;
          int lo_ = i + 1, hi_ = NP;
          while (lo_ < hi_) { const int mid = (lo_ + hi_) >> 1; if (keys[mid] == key) lo_ = mid + 1; else hi_ = mid; }
          cell1(lo_ - i, (int)(key >> 8), (int)(key & 255u));
        }
      }
      HaralickSums hs;
      haralick_marginal_sums(hs, acc, hx, hplus, hminus, minlev, maxlev, maxv, Tt, logT, vec);

      // HXY1 = -sum_ij p_ij log2(px_i py_j): second pass over the cells now that p_x is complete
      double hxy = 0;
      if (dense) {
        for (int idx = tid; idx < ncell; idx += blockDim.x) {
          int c, lo, hi;
          dense_cell(idx, c, lo, hi);
          if (c) hxy += haralick_hxy1_term(c, lo, hi, hx, Tt, logT);
        }
      } else {
        for (int i = tid; i < NP; i += blockDim.x) {
          const unsigned int key = keys[i];
          if (i > 0 && keys[i - 1] == key) continue;
          int lo_ = i + 1, hi_ = NP;
          while (lo_ < hi_) { const int mid = (lo_ + hi_) >> 1; if (keys[mid] == key) lo_ = mid + 1; else hi_ = mid; }
          const int c = lo_ - i;
          const int lo = (int)(key >> 8), hi = (int)(key & 255u);
          hxy += haralick_hxy1_term(c, lo, hi, hx, Tt, logT);
        }
      }
      haralick_finish(fo, hs, hxy, maxv, vec);
      __syncthreads();
    }
  }
}

extern "C" int aliby_features_texture(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype,
                                      int F, int C, int Y, int X, int channel,
                                      const aliby_object* table_dev, int n_obj, int max_h, int max_w,
                                      int max_area, int scale, int gray_levels, double* out, int ld,
                                      int col0, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  if (n_obj == 0) return ALIBY_OK;
  ARG_CHECK(labels && planes && table_dev && out, "NULL argument");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32 || dtype == ALIBY_U8W, "dtype must be ALIBY_U16, ALIBY_U8W or ALIBY_F32");
  ARG_CHECK(channel >= 0 && channel < C, "channel out of range");
  ARG_CHECK(F > 0 && Y > 0 && X > 0 && max_h >= 0 && max_w >= 0 && max_area >= 0, "bad shape");
  ARG_CHECK(scale >= 1 && gray_levels >= 2 && gray_levels <= 256, "scale >= 1 and 2 <= gray_levels <= 256");
  ARG_CHECK(col0 >= 0 && col0 + 4 * TX_NSTAT <= ld, "columns exceed row stride");
  TextureArgs a;
  a.labels = labels; a.planes = planes; a.F = F; a.C = C; a.Y = Y; a.X = X; a.channel = channel;
  a.tab = table_dev; a.n_obj = n_obj; a.scale = scale; a.gray_levels = gray_levels;
  a.out = out; a.ld = ld; a.col0 = col0;
  a.grey_shift = dtype == ALIBY_U8W ? 0 : 8;
  if (dtype == ALIBY_U8W) dtype = ALIBY_U16;
  a.cap_pix = (int)(((size_t)max_h * max_w + 15) & ~(size_t)15);
  const int ck = aliby_pow2_at_least(max_area, 2048);  // >= 4096 16-bit cells for the direct-counting path (K <= 90 distinct grey levels)
  a.cap_keys = ck;
  a.cap_cells = max_area < 65536 ? 2 * ck : 0;
  const size_t need = (size_t)a.cap_pix + (size_t)ck * 4;
  hipStream_t s = as_stream(stream);
  { const int rc = haralick_log2_table_ready(ctx, s); if (rc) return rc; }
  return object_launch(ctx, object_kernel(dtype, k_texture<u16, false>, k_texture<float, false>),
                       object_kernel(dtype, k_texture<u16, true>, k_texture<float, true>), a, n_obj, need, 96 * 1024,
                       (long long)max_h * max_w, s);
}
