// dynamics.hip — Cellpose post-network dynamics: (dY, dX, cellprob) -> label images, (dZ, dY, dX, cellprob) -> label volumes.
//
// Reference call site: `model.eval(...)` at src/aliby/segment/dispatch.py:208-215 (cellpose 4.0.6,
// uv.lock:130-131 — not vendored, weights not obtainable; PARITY UNPINNED against Cellpose itself).
// Restated from the published algorithm (cellpose.dynamics.compute_masks):
//   follow_flows            200 Euler steps p += bilinear(dP/5)(p), torch grid_sample index mapping
//                           (align_corners=False, zero padding), float32, positions clamped;
//   get_masks               end-point histogram padded by 20, seeds = 5x5 maxima with > 10 points,
//                           seed masks grown 5 x (3x3 dilation AND bin > 2) inside an 11x11 window,
//                           overlaps resolved by (points, raster position) priority, pixel label =
//                           seed owning its end-point bin, masks > max_size_fraction of the image
//                           dropped, labels renumbered in order of first raster appearance;
//   remove_bad_flow_masks   heat diffusion from each mask's centre (2 x max extent iterations, 9-point
//                           mean restricted to the mask), flows = normalised central differences,
//                           masks with mean squared error vs dP/5 above flow_threshold dropped;
//   fill_holes_and_remove_small_masks  masks < min_size dropped, holes filled, labels 1..n.
// The CPU restatement (oracle/cellpose_restated.py) writes the same float32/float64 operations in the
// same order, so label images are compared bit-for-bit.
//
// Volumes (cellpose's do_3D: `segment(pixels, do_3D=True)` -> `model.eval(..., do_3D=True, z_axis=1)`, dispatch.py:193-198,
// 208-215), restated by tests/cellpose3d_ref.py in the same float32 operations and order:
//   follow      niter Euler steps p = clamp(p + trilinear(dP * fg / 5 * 2/(L-1))(p), -1, 1) in grid_sample's normalised
//               coordinates (align_corners=False, zero padding; taps tnw..bse, weights (wx*wy)*wz, summed from 0 in tap order);
//   seeds       end-point histogram (padded by 20 in cellpose; end points never leave the volume, so the margin is always empty
//               and the histogram here is unpadded, out-of-range reads being empty), maxima of 5x5x5 with > 10 points;
//   growth      5 x (3x3x3 dilation AND bin > 2) in an 11x11x11 window per seed, overlaps resolved by (points, raster position);
//   labels      voxel = seed owning its end cell, masks above max_size_fraction of the volume dropped, first-appearance ids;
//   fill        masks below min_size dropped, 3-D holes (6-connected background, inside the bounding box) filled, ids 1..n.
// No flow-error QC: cellpose documents flow_threshold as "not used for 3D".
//
// Kernel shapes: per-pixel kernels are HBM/L2-bound streaming passes (flow following is an L2-resident
// gather loop); everything per mask runs as one workgroup per object with its bbox staged in LDS.
// Images and volumes share every stage that does not depend on how a frame is indexed: the foreground compaction, the label
// assignment, the first-appearance ranking, the final ids and the hole fill.
#include "common.h"
#include <type_traits>
#include <vector>

typedef unsigned short u16;
typedef unsigned long long u64;

#define RPAD 20
#define LABELS_PER_VOL 65536  // rows of the volume object table per volume (row = label - 1)

// F frames: images [F,Y,X] or volumes [F,Z,Y,X].  The shared stages index a frame's pixels (voxels) and the cells of its
// end-point histogram linearly.
struct DynShape {
  int F, Y, X, YP, XP;  // images: YP = Y + 2*RPAD, XP = X + 2*RPAD (the padded end-point histogram)
  size_t P, PP;         // pixels per frame, end-point histogram cells per frame (volumes: unpadded, PP = P)
  int Z;                // planes per volume (images: 1)
};

// ---------------------------------------------------------------------------------------------
// 0. one pass over (dP, cellprob): the normalised, masked flow field im = ((mask ? dP : 0) / 5) * (2 / (size-1)) and the
//    compacted list of foreground pixels (cellprob > thr).  Only ~10-35 % of the pixels are foreground and each follows 200
//    dependent steps, so everything after this pass that is per followed pixel (end point, temporary label) lives in arrays
//    indexed by the list position j, not by the pixel.  Wave-aggregated append, one global atomic per 4096 pixels; the order
//    of the list inside a chunk is raster order, the order of the chunks is irrelevant (every consumer is order-free).
// ---------------------------------------------------------------------------------------------
#define FG_CHUNK 4096  // pixels per workgroup pass
struct FlowScale {
  float c[3];  // 2 / (L - 1) per flow component, in dP's component order
};

template <int NC>  // flow components: 2 (dY, dX) or 3 (dZ, dY, dX)
__global__ __launch_bounds__(256) void k_prep_compact(const float* __restrict__ dP, const float* __restrict__ prob, float thr,
                                                      DynShape s, FlowScale sc, float* __restrict__ im,
                                                      int* __restrict__ list, int* __restrict__ count, int reverse) {
  __shared__ int red_i[8];
  __shared__ int wsum[4];
  __shared__ int s_base;
  const size_t total = (size_t)s.F * s.P;
  const size_t nchunks = (total + FG_CHUNK - 1) / FG_CHUNK;
  // (reverse: a test hook, ALIBY_DEBUG_FG_REVERSE=1 — chunks reserve their list space in descending raster order, the order the
  // scheduler only produces now and then; everything downstream must not care)
  for (size_t ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const size_t c0 = (reverse ? nchunks - 1 - ci : ci) * FG_CHUNK;
    unsigned fgmask = 0;
#pragma unroll
    for (int k = 0; k < FG_CHUNK / 256; ++k) {
      const size_t i = c0 + (size_t)k * 256 + threadIdx.x;
      if (i >= total) continue;
      const bool m = prob[i] > thr;
      fgmask |= (unsigned)m << k;
      const size_t f = i / s.P, p = i % s.P;
#pragma unroll
      for (int d = 0; d < NC; ++d) {
        float v = dP[(f * NC + d) * s.P + p];
        v = m ? v : 0.0f;
        v = v / 5.0f;
        im[(f * NC + d) * s.P + p] = v * sc.c[d];
      }
    }
    const int tot = block_sum_i32(__popc(fgmask), red_i);
    if (tot == 0) continue;  // block-uniform
    if (threadIdx.x == 0) s_base = atomicAdd(count, tot);
    __syncthreads();
    int base = s_base;
#pragma unroll
    for (int k = 0; k < FG_CHUNK / 256; ++k) {
      const bool fg = (fgmask >> k) & 1u;
      const int pos = block_compact_slot(fg, base, wsum);
      if (fg) list[pos] = (int)(c0 + (size_t)k * 256 + threadIdx.x);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// 1. flow following + end-point histogram
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float tap(const float* __restrict__ f, int yy, int xx, int H, int W) {
  return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? f[(size_t)yy * W + xx] : 0.0f;
}

__global__ __launch_bounds__(256) void k_follow(const float* __restrict__ im, const int* __restrict__ list,
                                                const int* __restrict__ count, DynShape s, int niter,
                                                int* __restrict__ ptc, int* __restrict__ h1, u64* __restrict__ M1,
                                                float* __restrict__ pfinal) {
  const int total = *count;
  const int H = s.Y, W = s.X;
  const float sx = (float)(W - 1), sy = (float)(H - 1), Wf = (float)W, Hf = (float)H;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += gridDim.x * blockDim.x) {
    const size_t i = (size_t)list[j];
    const size_t f = i / s.P, p = i % s.P;
    const float* imy = im + (f * 2 + 0) * s.P;
    const float* imx = im + (f * 2 + 1) * s.P;
    const int y = (int)(p / W), x = (int)(p % W);
    float px = (float)x / sx * 2.0f - 1.0f;
    float py = (float)y / sy * 2.0f - 1.0f;
    // The eight taps of the bilinear sample are kept in registers and re-read only when the point enters another
    // pixel cell: points reach their sink within a few dozen steps and then jitter inside one cell, so most of the
    // 200 steps issue no loads at all (the kernel is bound by the gather address rate otherwise).
    int cell_x = INT_MIN, cell_y = INT_MIN;
    float xnw = 0.f, xne = 0.f, xsw = 0.f, xse = 0.f, ynw = 0.f, yne = 0.f, ysw = 0.f, yse = 0.f;
    for (int t = 0; t < niter; ++t) {
      const float ix = ((px + 1.0f) * Wf - 1.0f) / 2.0f;
      const float iy = ((py + 1.0f) * Hf - 1.0f) / 2.0f;
      const float x0 = floorf(ix), y0 = floorf(iy);
      const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
      const float wnw = (x1 - ix) * (y1 - iy);
      const float wne = (ix - x0) * (y1 - iy);
      const float wsw = (x1 - ix) * (iy - y0);
      const float wse = (ix - x0) * (iy - y0);
      const int x0i = (int)x0, y0i = (int)y0;
      if (x0i != cell_x || y0i != cell_y) {
        const int x1i = (int)x1, y1i = (int)y1;
        xnw = tap(imx, y0i, x0i, H, W); xne = tap(imx, y0i, x1i, H, W); xsw = tap(imx, y1i, x0i, H, W); xse = tap(imx, y1i, x1i, H, W);
        ynw = tap(imy, y0i, x0i, H, W); yne = tap(imy, y0i, x1i, H, W); ysw = tap(imy, y1i, x0i, H, W); yse = tap(imy, y1i, x1i, H, W);
        cell_x = x0i; cell_y = y0i;
      }
      float dx = 0.0f + xnw * wnw;
      dx = dx + xne * wne;
      dx = dx + xsw * wsw;
      dx = dx + xse * wse;
      float dy = 0.0f + ynw * wnw;
      dy = dy + yne * wne;
      dy = dy + ysw * wsw;
      dy = dy + yse * wse;
      const float npx = fminf(fmaxf(px + dx, -1.0f), 1.0f);
      const float npy = fminf(fmaxf(py + dy, -1.0f), 1.0f);
      // A step is a function of the position alone: once a step leaves (px, py) as it was, every later step does too.  Points
      // reach their sink within a few dozen steps (the increments fall below half an ulp of the position), so when no lane of
      // the wave — neighbouring pixels, mostly of one mask — moved, the remaining iterations are skipped: same bits, fewer steps.
      const bool moved = npx != px || npy != py;
      px = npx;
      py = npy;
      if (__ballot(moved) == 0ull) break;
    }
    const float fx = (px + 1.0f) * 0.5f * sx;
    const float fy = (py + 1.0f) * 0.5f * sy;
    if (pfinal) { pfinal[(f * 2 + 0) * s.P + p] = fy; pfinal[(f * 2 + 1) * s.P + p] = fx; }
    float qy = fmaxf(fy + (float)RPAD, 0.0f), qx = fmaxf(fx + (float)RPAD, 0.0f);
    qy = fminf(qy, (float)(H + RPAD - 1));
    qx = fminf(qx, (float)(W + RPAD - 1));
    const int cell = (int)qy * s.XP + (int)qx;
    ptc[j] = cell;  // (indexed by the list position)
    atomicAdd(&h1[f * s.PP + cell], 1);
    // the seed-ownership map is only ever looked up at end-point cells: they are cleared here, by whoever ends there, instead of
    // by a memset of 8 bytes per padded pixel (k_grow's atomicMax runs in a later launch; cells never looked up may hold anything)
    M1[f * s.PP + cell] = 0ull;
  }
}

struct Taps3 { float v[8]; };

__device__ __forceinline__ float tap3(const float* __restrict__ f, int zz, int yy, int xx, const DynShape& s) {
  return (zz >= 0 && zz < s.Z && yy >= 0 && yy < s.Y && xx >= 0 && xx < s.X) ? f[((size_t)zz * s.Y + yy) * s.X + xx] : 0.0f;
}

__device__ __forceinline__ void load_taps(const float* __restrict__ f, int z0, int y0, int x0, const DynShape& s, Taps3& t) {
  // PyTorch's order: tnw, tne, tsw, tse, bnw, bne, bsw, bse (t/b = z0/z1, n/s = y0/y1, w/e = x0/x1)
  t.v[0] = tap3(f, z0, y0, x0, s);
  t.v[1] = tap3(f, z0, y0, x0 + 1, s);
  t.v[2] = tap3(f, z0, y0 + 1, x0, s);
  t.v[3] = tap3(f, z0, y0 + 1, x0 + 1, s);
  t.v[4] = tap3(f, z0 + 1, y0, x0, s);
  t.v[5] = tap3(f, z0 + 1, y0, x0 + 1, s);
  t.v[6] = tap3(f, z0 + 1, y0 + 1, x0, s);
  t.v[7] = tap3(f, z0 + 1, y0 + 1, x0 + 1, s);
}

__device__ __forceinline__ float interp8(const Taps3& t, const float* w) {
  float acc = 0.0f + t.v[0] * w[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) acc = acc + t.v[k] * w[k];
  return acc;
}

// one atomic per wave where every lane ends in the same cell (neighbouring voxels of one mask mostly do)
__device__ __forceinline__ void wave_count(int* h, unsigned long long key) {
  const int lane = threadIdx.x & (WAVE - 1);
  const unsigned long long active = __ballot(1);
  const int lead = __ffsll((long long)active) - 1;
  const unsigned long long k = __shfl(key, lead, WAVE);
  const unsigned long long same = __ballot(key == k);
  if (same == active) {
    if (lane == lead) atomicAdd(&h[k], (int)__popcll(active));
  } else {
    atomicAdd(&h[key], 1);
  }
}

__global__ __launch_bounds__(256) void k3_follow(const float* __restrict__ im, const int* __restrict__ list,
                                                 const int* __restrict__ count, DynShape s, int niter, int* __restrict__ ptc,
                                                 int* __restrict__ h1, u64* __restrict__ M1, float* __restrict__ pfinal) {
  const int total = *count;
  const float sz = (float)(s.Z - 1), sy = (float)(s.Y - 1), sx = (float)(s.X - 1);
  const float Zf = (float)s.Z, Yf = (float)s.Y, Xf = (float)s.X;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += gridDim.x * blockDim.x) {
    const size_t i = (size_t)list[j];
    const size_t f = i / s.P, p = i % s.P;
    const float* imz = im + (f * 3 + 0) * s.P;
    const float* imy = im + (f * 3 + 1) * s.P;
    const float* imx = im + (f * 3 + 2) * s.P;
    const int z = (int)(p / ((size_t)s.Y * s.X)), y = (int)((p / s.X) % s.Y), x = (int)(p % s.X);
    float pz = (float)z / sz * 2.0f - 1.0f;
    float py = (float)y / sy * 2.0f - 1.0f;
    float px = (float)x / sx * 2.0f - 1.0f;
    // the 8 taps of each component stay in registers until the point enters another voxel cell (as in k_follow: most of the
    // steps of a point that has reached its sink issue no loads)
    int cz = INT_MIN, cyy = INT_MIN, cxx = INT_MIN;
    Taps3 tz, ty, tx;
    for (int t = 0; t < niter; ++t) {
      const float ix = ((px + 1.0f) * Xf - 1.0f) / 2.0f;
      const float iy = ((py + 1.0f) * Yf - 1.0f) / 2.0f;
      const float iz = ((pz + 1.0f) * Zf - 1.0f) / 2.0f;
      const float x0 = floorf(ix), y0 = floorf(iy), z0 = floorf(iz);
      const float x1 = x0 + 1.0f, y1 = y0 + 1.0f, z1 = z0 + 1.0f;
      const float wxw = x1 - ix, wxe = ix - x0, wyn = y1 - iy, wys = iy - y0, wzt = z1 - iz, wzb = iz - z0;
      float w[8];
      w[0] = (wxw * wyn) * wzt;
      w[1] = (wxe * wyn) * wzt;
      w[2] = (wxw * wys) * wzt;
      w[3] = (wxe * wys) * wzt;
      w[4] = (wxw * wyn) * wzb;
      w[5] = (wxe * wyn) * wzb;
      w[6] = (wxw * wys) * wzb;
      w[7] = (wxe * wys) * wzb;
      const int x0i = (int)x0, y0i = (int)y0, z0i = (int)z0;
      if (x0i != cxx || y0i != cyy || z0i != cz) {
        load_taps(imz, z0i, y0i, x0i, s, tz);
        load_taps(imy, z0i, y0i, x0i, s, ty);
        load_taps(imx, z0i, y0i, x0i, s, tx);
        cz = z0i; cyy = y0i; cxx = x0i;
      }
      const float dz = interp8(tz, w), dy = interp8(ty, w), dx = interp8(tx, w);
      const float npz = fminf(fmaxf(pz + dz, -1.0f), 1.0f);
      const float npy = fminf(fmaxf(py + dy, -1.0f), 1.0f);
      const float npx = fminf(fmaxf(px + dx, -1.0f), 1.0f);
      // a step is a function of the position alone: once no lane of the wave moved, no later step moves it (same bits)
      const bool moved = npz != pz || npy != py || npx != px;
      pz = npz;
      py = npy;
      px = npx;
      if (__ballot(moved) == 0ull) break;
    }
    const float fz = (pz + 1.0f) * 0.5f * sz;
    const float fy = (py + 1.0f) * 0.5f * sy;
    const float fx = (px + 1.0f) * 0.5f * sx;
    if (pfinal) {
      pfinal[(f * 3 + 0) * s.P + p] = fz;
      pfinal[(f * 3 + 1) * s.P + p] = fy;
      pfinal[(f * 3 + 2) * s.P + p] = fx;
    }
    // cellpose's cell of the padded histogram, trunc(clamp(end + 20, 0, L + 19)), shifted back by the pad
    const int qz = (int)fminf(fmaxf(fz + (float)RPAD, 0.0f), (float)(s.Z + RPAD - 1)) - RPAD;
    const int qy = (int)fminf(fmaxf(fy + (float)RPAD, 0.0f), (float)(s.Y + RPAD - 1)) - RPAD;
    const int qx = (int)fminf(fmaxf(fx + (float)RPAD, 0.0f), (float)(s.X + RPAD - 1)) - RPAD;
    // (end points lie in [0, L-1], so the cell is inside the volume; clamped again so that no write can leave it)
    const int cell = (min(max(qz, 0), s.Z - 1) * s.Y + min(max(qy, 0), s.Y - 1)) * s.X + min(max(qx, 0), s.X - 1);
    ptc[j] = cell;
    wave_count(h1, (unsigned long long)(f * s.PP + cell));
    M1[f * s.PP + cell] = 0ull;  // (the owner map is only looked up at end cells: cleared by whoever ends there)
  }
}

// ---------------------------------------------------------------------------------------------
// 2. seeds (5x5 / 5x5x5 maxima with > 10 points) and their grown masks
// ---------------------------------------------------------------------------------------------
// Per-frame seed lists (65536 slots each; a frame with more seeds than uint16 labels overflows later anyway and is reported).
// (Round 3 tried finding the seeds from the end points of the foreground list instead of this scan of the padded histogram:
// 7 M scattered 4-byte gathers fetched more bytes than the scan streams, 0.52 ms against 0.22 ms.)
// The image and volume forms stay apart: the image histogram is padded (no bounds per tap, 121-cell windows on one wave), the
// volume histogram is not (every axis bounded, 1331-cell windows on four waves).
#define H_MASK 0x7fffffff
#define SEEDS_PER_FRAME 65536
__global__ void k_seeds(const int* __restrict__ h1, DynShape s, int* __restrict__ seed_list, int* __restrict__ seed_count) {
  const size_t total = (size_t)s.F * s.PP;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int h = h1[i];
    if (h <= 10) continue;
    const size_t f = i / s.PP;
    const int cell = (int)(i % s.PP), r = cell / s.XP, c = cell % s.XP;
    const int* hf = h1 + f * s.PP;
    bool ismax = true;
    for (int dr = -2; dr <= 2 && ismax; ++dr)
      for (int dc = -2; dc <= 2; ++dc) {
        const int rr = r + dr, cc = c + dc;
        if (rr < 0 || rr >= s.YP || cc < 0 || cc >= s.XP) continue;
        if (hf[rr * s.XP + cc] > h) { ismax = false; break; }
      }
    if (!ismax) continue;
    const int k = atomicAdd(&seed_count[f], 1);
    if (k < SEEDS_PER_FRAME) seed_list[f * SEEDS_PER_FRAME + k] = cell;
  }
}

// one wave per seed: 11x11 window, 5 x (3x3 dilation AND h>2); owner = max (points, cell) priority
__global__ __launch_bounds__(64) void k_grow(const int* __restrict__ h1, DynShape s, const int* __restrict__ seed_list,
                                             const int* __restrict__ seed_count, u64* __restrict__ M1, int* __restrict__ cnt,
                                             int* __restrict__ firstpos, int* __restrict__ newid) {
  __shared__ unsigned char ok[121], cur[121], nxt[121];
  const int f = blockIdx.y;
  const int n = min(seed_count[f], SEEDS_PER_FRAME);
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const int cell = seed_list[(size_t)f * SEEDS_PER_FRAME + k];
    const int r0 = cell / s.XP, c0 = cell % s.XP;
    const int* hf = h1 + (size_t)f * s.PP;
    // the words of this seed's temporary label (its cell + 1): pixel count, first raster position, final id — touched only
    // at seed cells, so they are initialised here instead of by three memsets of 4 bytes per padded pixel
    if (threadIdx.x == 0) {
      cnt[(size_t)f * s.PP + cell] = 0;
      firstpos[(size_t)f * s.PP + cell] = INT_MAX;
      newid[(size_t)f * s.PP + cell] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 121; i += 64) {
      const int rr = r0 - 5 + i / 11, cc = c0 - 5 + i % 11;
      const bool in = rr >= 0 && rr < s.YP && cc >= 0 && cc < s.XP;
      ok[i] = (in && (hf[rr * s.XP + cc] & H_MASK) > 2) ? 1 : 0;
      cur[i] = (i == 60) ? 1 : 0;
    }
    __syncthreads();
    for (int it = 0; it < 5; ++it) {
      for (int i = threadIdx.x; i < 121; i += 64) {
        const int r = i / 11, c = i % 11;
        unsigned char v = 0;
        for (int dr = -1; dr <= 1; ++dr)
          for (int dc = -1; dc <= 1; ++dc) {
            const int rr = r + dr, cc = c + dc;
            if (rr >= 0 && rr < 11 && cc >= 0 && cc < 11) v |= cur[rr * 11 + cc];
          }
        nxt[i] = v & ok[i];
      }
      __syncthreads();
      for (int i = threadIdx.x; i < 121; i += 64) cur[i] = nxt[i];
      __syncthreads();
    }
    const u64 prio = ((u64)(unsigned)(hf[cell] & H_MASK) << 32) | (u64)(unsigned)cell;
    for (int i = threadIdx.x; i < 121; i += 64) {
      if (!cur[i]) continue;
      const int rr = r0 - 5 + i / 11, cc = c0 - 5 + i % 11;
      atomicMax(&M1[(size_t)f * s.PP + rr * s.XP + cc], prio + 1ull);  // +1: 0 means "no seed"
    }
  }
}

__global__ void k3_seeds(const int* __restrict__ h1, DynShape s, int* __restrict__ seed_list, int* __restrict__ seed_count) {
  const size_t total = (size_t)s.F * s.P;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int h = h1[i];
    if (h <= 10) continue;
    const size_t f = i / s.P;
    const int cell = (int)(i % s.P);
    const int z = cell / (s.Y * s.X), y = (cell / s.X) % s.Y, x = cell % s.X;
    const int* hf = h1 + f * s.P;
    bool ismax = true;
    for (int dz = -2; dz <= 2 && ismax; ++dz) {
      const int zz = z + dz;
      if (zz < 0 || zz >= s.Z) continue;
      for (int dy = -2; dy <= 2 && ismax; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= s.Y) continue;
        for (int dx = -2; dx <= 2; ++dx) {
          const int xx = x + dx;
          if (xx < 0 || xx >= s.X) continue;
          if (hf[((size_t)zz * s.Y + yy) * s.X + xx] > h) { ismax = false; break; }
        }
      }
    }
    if (!ismax) continue;
    const int k = atomicAdd(&seed_count[f], 1);
    if (k < SEEDS_PER_FRAME) seed_list[f * SEEDS_PER_FRAME + k] = cell;  // (the count goes on: the host reports the overflow)
  }
}

#define W3 11
#define W3N (W3 * W3 * W3)
__global__ __launch_bounds__(256) void k3_grow(const int* __restrict__ h1, DynShape s, const int* __restrict__ seed_list,
                                               const int* __restrict__ seed_count, u64* __restrict__ M1, int* __restrict__ cnt,
                                               int* __restrict__ firstpos, int* __restrict__ newid) {
  __shared__ unsigned char ok[W3N], cur[W3N], nxt[W3N];
  const int f = blockIdx.y;
  const int n = min(seed_count[f], SEEDS_PER_FRAME);
  const int* hf = h1 + (size_t)f * s.P;
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const int cell = seed_list[(size_t)f * SEEDS_PER_FRAME + k];
    const int z0 = cell / (s.Y * s.X), y0 = (cell / s.X) % s.Y, x0 = cell % s.X;
    if (threadIdx.x == 0) {  // this seed's words (temporary label = cell + 1)
      cnt[(size_t)f * s.P + cell] = 0;
      firstpos[(size_t)f * s.P + cell] = INT_MAX;
      newid[(size_t)f * s.P + cell] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < W3N; i += blockDim.x) {
      const int zz = z0 - 5 + i / (W3 * W3), yy = y0 - 5 + (i / W3) % W3, xx = x0 - 5 + i % W3;
      const bool in = zz >= 0 && zz < s.Z && yy >= 0 && yy < s.Y && xx >= 0 && xx < s.X;
      ok[i] = (in && hf[((size_t)zz * s.Y + yy) * s.X + xx] > 2) ? 1 : 0;  // (outside: cellpose's empty padding)
      cur[i] = (i == W3N / 2) ? 1 : 0;
    }
    __syncthreads();
    for (int it = 0; it < 5; ++it) {
      for (int i = threadIdx.x; i < W3N; i += blockDim.x) {
        const int a = i / (W3 * W3), b = (i / W3) % W3, c = i % W3;
        unsigned char v = 0;
        for (int da = -1; da <= 1; ++da)
          for (int db = -1; db <= 1; ++db)
            for (int dc = -1; dc <= 1; ++dc) {
              const int aa = a + da, bb = b + db, cc = c + dc;
              if (aa >= 0 && aa < W3 && bb >= 0 && bb < W3 && cc >= 0 && cc < W3) v |= cur[(aa * W3 + bb) * W3 + cc];
            }
        nxt[i] = v & ok[i];
      }
      __syncthreads();
      for (int i = threadIdx.x; i < W3N; i += blockDim.x) cur[i] = nxt[i];
      __syncthreads();
    }
    const u64 prio = ((u64)(unsigned)hf[cell] << 32) | (u64)(unsigned)cell;
    for (int i = threadIdx.x; i < W3N; i += blockDim.x) {
      if (!cur[i]) continue;  // (a set cell passed `ok`, so it lies inside the volume)
      const int zz = z0 - 5 + i / (W3 * W3), yy = y0 - 5 + (i / W3) % W3, xx = x0 - 5 + i % W3;
      atomicMax(&M1[(size_t)f * s.P + ((size_t)zz * s.Y + yy) * s.X + xx], prio + 1ull);  // +1: 0 means "no seed"
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// 3. pixel labels (temporary id = owning seed's cell + 1), sizes, first raster positions, first-appearance renumbering
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_assign(const int* __restrict__ list, const int* __restrict__ count, const int* __restrict__ ptc,
                                                const u64* __restrict__ M1, DynShape s, unsigned int* __restrict__ labc,
                                                int* __restrict__ cnt, int* __restrict__ firstpos) {
  const int total = *count;
  const int rounds = (total + (int)(gridDim.x * blockDim.x) - 1) / (int)(gridDim.x * blockDim.x);
  for (int it = 0; it < rounds; ++it) {  // (every lane takes part in the ballots below)
    const int j = (it * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    const bool live = j < total;
    size_t f = 0;
    int p = 0;
    unsigned int lab = 0;
    if (live) {
      const size_t i = (size_t)list[j];
      f = i / s.P;
      p = (int)(i % s.P);
      const u64 m = M1[f * s.PP + ptc[j]];
      if (m) lab = (unsigned int)((m - 1ull) & 0xFFFFFFFFull) + 1u;
      labc[j] = lab;
    }
    // Neighbouring lanes are neighbouring foreground pixels of a row, mostly of the same mask: one atomic pair per RUN of equal
    // labels inside the wave instead of one per pixel.  Integer atomics: same result in any order.
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long key = ((unsigned long long)f << 32) | lab;
    const unsigned long long prev = __shfl_up(key, 1, WAVE);
    const int prev_p = __shfl_up(p, 1, WAVE);
    // (the list is in raster order inside a 4096-pixel chunk of k_prep_compact, and the chunks land in it in the order their
    // workgroups reserved space: where a wave straddles two chunks the position can step BACK inside a run of one label — a
    // mask that spans both — and the run's first lane no longer holds its smallest position: such a step starts a new run)
    const bool head = lab && (lane == 0 || prev != key || prev_p > p);
    const unsigned long long heads = __ballot(head || !lab) | ~__ballot(1);
    if (head) {
      const unsigned long long after = lane == 63 ? 0ull : (heads >> (lane + 1));
      const int run = after ? __ffsll((long long)after) : 64 - lane;
      atomicAdd(&cnt[f * s.PP + lab - 1], run);
      atomicMin(&firstpos[f * s.PP + lab - 1], p);  // (positions ascend inside a run: the head holds the run's first)
    }
  }
}

// New id of every kept label = 1 + the number of kept labels of its frame that appear earlier in raster order (cellpose renumbers
// in order of first appearance).  The labels are the frame's seeds (a few hundred): one thread per seed counts the others.
// T: the type cellpose compares a mask's size with max_size_fraction of the frame in — float32 for images, float64 for volumes.
template <typename T>
__global__ __launch_bounds__(256) void k_rank_ids(const int* __restrict__ seed_list, const int* __restrict__ seed_count, DynShape s,
                                                  const int* __restrict__ cnt, const int* __restrict__ firstpos, T big,
                                                  int* __restrict__ newid, int* __restrict__ ntot) {
  __shared__ int frame_pos[1024];
  __shared__ int red_i[8];
  const int f = blockIdx.x;
  const int n = min(seed_count[f], SEEDS_PER_FRAME);
  const int* sl = seed_list + (size_t)f * SEEDS_PER_FRAME;
  const size_t base = (size_t)f * s.PP;
  int kept_total = 0;
  for (int k0 = 0; k0 < n; k0 += blockDim.x) {
    const int k = k0 + threadIdx.x;
    int mine = INT_MAX, cell = 0;
    bool kept = false;
    if (k < n) {
      cell = sl[k];
      const int c = cnt[base + cell];
      kept = c > 0 && !((T)c > big);
      mine = kept ? firstpos[base + cell] : INT_MAX;
    }
    int before = 0;
    for (int q0 = 0; q0 < n; q0 += 1024) {  // the other seeds' first positions, 1024 at a time through LDS
      __syncthreads();
      for (int q = threadIdx.x; q < 1024; q += blockDim.x) {
        int v = INT_MAX;
        if (q0 + q < n) {
          const int cq = sl[q0 + q];
          const int c = cnt[base + cq];
          if (c > 0 && !((T)c > big)) v = firstpos[base + cq];
        }
        frame_pos[q] = v;
      }
      __syncthreads();
      const int m = min(1024, n - q0);
      if (kept)
        for (int q = 0; q < m; ++q) before += frame_pos[q] < mine ? 1 : 0;
    }
    if (kept) newid[base + cell] = before + 1;
    kept_total += kept ? 1 : 0;
  }
  kept_total = block_sum_i32(kept_total, red_i);
  if (threadIdx.x == 0) ntot[f] = kept_total;
}

__global__ void k_apply_ids(const int* __restrict__ list, const int* __restrict__ count, const unsigned int* __restrict__ labc,
                            const int* __restrict__ newid, DynShape s, u16* __restrict__ labels) {
  const int total = *count;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += gridDim.x * blockDim.x) {
    const unsigned int lab = labc[j];
    if (!lab) continue;  // (labels is zero-filled)
    const size_t i = (size_t)list[j];
    const int id = newid[(i / s.P) * s.PP + lab - 1];
    if (id) labels[i] = (u16)(id > 65535 ? 65535 : id);
  }
}

struct Obj3 {
  int z0, y0, x0, z1, y1, x1;  // inclusive bounds while built
  int area, pad_;
};

// labels (ids clamped to 65535: a volume with that many is reported as an overflow) and the object table [F, LABELS_PER_VOL]:
// inclusive bounding box and voxel count per label, one set of atomics per wave where all its lanes share a label
__global__ __launch_bounds__(256) void k3_apply_ids(const int* __restrict__ list, const int* __restrict__ count,
                                                    const unsigned int* __restrict__ labc, const int* __restrict__ newid, DynShape s,
                                                    u16* __restrict__ labels, Obj3* __restrict__ tab) {
  const int total = *count;
  const int rounds = (total + (int)(gridDim.x * blockDim.x) - 1) / (int)(gridDim.x * blockDim.x);
  for (int it = 0; it < rounds; ++it) {
    const int j = (it * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    int id = 0, z = 0, y = 0, x = 0;
    size_t f = 0;
    if (j < total) {
      const unsigned int lab = labc[j];
      const size_t i = (size_t)list[j];
      f = i / s.P;
      const size_t p = i % s.P;
      if (lab) {
        id = newid[f * s.PP + lab - 1];
        id = id > 65535 ? 65535 : id;
        if (id) labels[i] = (u16)id;
      }
      z = (int)(p / ((size_t)s.Y * s.X));
      y = (int)((p / s.X) % s.Y);
      x = (int)(p % s.X);
    }
    const unsigned long long key = ((unsigned long long)f << 32) | (unsigned)id;
    const unsigned long long k0 = __shfl(key, 0, WAVE);
    const bool uniform = __ballot(key == k0) == __ballot(1);
    if (uniform) {
      if (id == 0) continue;
      int zmin = z, zmax = z, ymin = y, ymax = y, xmin = x, xmax = x, a = 1;
      for (int o = WAVE / 2; o > 0; o >>= 1) {
        zmin = min(zmin, __shfl_xor(zmin, o, WAVE)); zmax = max(zmax, __shfl_xor(zmax, o, WAVE));
        ymin = min(ymin, __shfl_xor(ymin, o, WAVE)); ymax = max(ymax, __shfl_xor(ymax, o, WAVE));
        xmin = min(xmin, __shfl_xor(xmin, o, WAVE)); xmax = max(xmax, __shfl_xor(xmax, o, WAVE));
        a += __shfl_xor(a, o, WAVE);
      }
      if ((threadIdx.x & (WAVE - 1)) == 0) {
        Obj3* o = tab + f * LABELS_PER_VOL + (id - 1);
        atomicMin(&o->z0, zmin); atomicMax(&o->z1, zmax);
        atomicMin(&o->y0, ymin); atomicMax(&o->y1, ymax);
        atomicMin(&o->x0, xmin); atomicMax(&o->x1, xmax);
        atomicAdd(&o->area, a);
      }
    } else if (id) {
      Obj3* o = tab + f * LABELS_PER_VOL + (id - 1);
      atomicMin(&o->z0, z); atomicMax(&o->z1, z);
      atomicMin(&o->y0, y); atomicMax(&o->y1, y);
      atomicMin(&o->x0, x); atomicMax(&o->x1, x);
      atomicAdd(&o->area, 1);
    }
  }
}
// (the uniform branch assumes a full wave: the grid is a multiple of 64 lanes and lanes past the list end carry key (0, 0), so a
// wave that straddles the end is never uniform unless every lane is background)

__global__ void k3_init_table(Obj3* __restrict__ tab, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    Obj3 o;
    o.z0 = o.y0 = o.x0 = INT_MAX;
    o.z1 = o.y1 = o.x1 = -1;
    o.area = 0;
    o.pad_ = 0;
    tab[i] = o;
  }
}

// ---------------------------------------------------------------------------------------------
// 4. flow QC (images): heat diffusion per mask, flow error, removal
// ---------------------------------------------------------------------------------------------
struct QcArgs {
  const u16* labels;
  const float* dP;  // [F,2,Y,X] network-scale flows
  int F, Y, X;
  const aliby_object* tab;
  int n_obj;
  const int* niter_tile;  // [F]
  size_t cap_cells;       // >= (max_h+2)*(max_w+2)
  unsigned char* gscratch;
  double* Tg;             // [F,Y,X]
};

template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_diffuse(QcArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_d[8];
  __shared__ int red_i[8];
  __shared__ long long red_l[8];
  unsigned char* ws = GLOBAL ? (a.gscratch + (size_t)blockIdx.x * a.cap_cells * 17) : lds_raw;
  double* T0 = reinterpret_cast<double*>(ws);
  double* T1 = T0 + a.cap_cells;
  unsigned char* mk = reinterpret_cast<unsigned char*>(T1 + a.cap_cells);
  const int tid = threadIdx.x;
  const size_t plane = (size_t)a.Y * a.X;
  for (int oi = blockIdx.x; oi < a.n_obj; oi += gridDim.x) {
    const aliby_object o = a.tab[oi];
    if (o.area <= 0) continue;
    const u16* lab = a.labels + (size_t)o.tile * plane;
    const int h = o.y1 - o.y0, w = o.x1 - o.x0, ph = h + 2, pw = w + 2;
    const u16 L = (u16)o.label;
    __syncthreads();
    long long sy = 0, sx = 0;
    for (int i = tid; i < ph * pw; i += blockDim.x) {
      const int r = i / pw - 1, c = i % pw - 1;
      unsigned char m = 0;
      if (r >= 0 && r < h && c >= 0 && c < w && lab[(size_t)(o.y0 + r) * a.X + o.x0 + c] == L) { m = 1; sy += r; sx += c; }
      mk[i] = m;
      T0[i] = 0.0;
      T1[i] = 0.0;
    }
    const long long SY = block_sum_i64(sy, red_l), SX = block_sum_i64(sx, red_l);
    const double ymed = (double)SY / (double)o.area, xmed = (double)SX / (double)o.area;
    // mask pixel closest to the centre of mass; first in raster order on ties
    double best = INFINITY;
    int bi = INT_MAX;
    for (int i = tid; i < h * w; i += blockDim.x) {
      const int r = i / w, c = i % w;
      if (!mk[(r + 1) * pw + c + 1]) continue;
      const double dx = (double)c - xmed, dy = (double)r - ymed;
      const double d = dx * dx + dy * dy;
      if (d < best) { best = d; bi = i; }
    }
    const double BEST = -block_max_f64(-best, red_d);
    const int CI = block_min_i32(best == BEST ? bi : INT_MAX, red_i);
    const int cidx = (CI / w + 1) * pw + (CI % w) + 1;
    const int niter = a.niter_tile[o.tile];
    double* src = T0;
    double* dst = T1;
    // One heat source at the centre, niter sweeps of the 9-point mean.  T is zero outside the mask for the whole
    // run (only mask pixels are ever written), so the reference's "neighbour * mask" products add exactly the
    // neighbour's value or +0.0 and are dropped; the order of the nine additions is the reference's.  A lane
    // walks down one column strip with the 3x3 window rolling through registers: 3 LDS reads per pixel, not 9
    // (+9 mask bytes).  The "+1 at the centre" of sweep it+1 is applied by the lane that writes the centre in
    // sweep it, which leaves one barrier per sweep.
    const int ngrp = max(1, (int)blockDim.x / max(w, 1));      // row groups working side by side
    const int rows_per = (h + ngrp - 1) / ngrp;
    const int grp = tid / max(w, 1), col0 = tid - grp * w;
    __syncthreads();
    if (tid == 0 && niter > 0) src[cidx] += 1.0;
    for (int it = 0; it < niter; ++it) {
      __syncthreads();
      const bool more = it + 1 < niter;
      if (grp < ngrp) {
        const int r0 = grp * rows_per, r1 = min(h, r0 + rows_per);
        for (int c = col0; c < w; c += (ngrp == 1 ? (int)blockDim.x : w)) {
          if (r0 >= r1) break;
          int q = (r0 + 1) * pw + c + 1;
          double a0 = src[q - pw - 1], a1 = src[q - pw], a2 = src[q - pw + 1];
          double b0 = src[q - 1], b1 = src[q], b2 = src[q + 1];
          for (int r = r0; r < r1; ++r, q += pw) {
            const double c0 = src[q + pw - 1], c1 = src[q + pw], c2 = src[q + pw + 1];
            if (mk[q]) {
              double acc = 0.0;
              acc = acc + b1;
              acc = acc + a1;
              acc = acc + c1;
              acc = acc + b0;
              acc = acc + b2;
              acc = acc + a0;
              acc = acc + a2;
              acc = acc + c0;
              acc = acc + c2;
              // acc / 9.0, correctly rounded, as multiply + two FMAs instead of the ~15-instruction fp64 division
              // sequence (Markstein: q0 = RN(a*c), r = a - 9*q0 exact, RN(q0 + r*c) = RN(a/9) for c = RN(1/9);
              // checked against the division on 2e9 random doubles)
              const double q0 = acc * (1.0 / 9.0);
              double v = fma(fma(-9.0, q0, acc), 1.0 / 9.0, q0);
              if (more && q == cidx) v += 1.0;
              dst[q] = v;
            }
            a0 = b0; a1 = b1; a2 = b2;
            b0 = c0; b1 = c1; b2 = c2;
          }
          if (ngrp > 1) break;  // one column per lane when the box is narrower than the workgroup
        }
      }
      double* t = src; src = dst; dst = t;
    }
    __syncthreads();
    double* Tt = a.Tg + (size_t)o.tile * plane;
    for (int i = tid; i < h * w; i += blockDim.x) {
      const int q = (i / w + 1) * pw + (i % w) + 1;
      if (mk[q]) Tt[(size_t)(o.y0 + i / w) * a.X + o.x0 + i % w] = src[q];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_flow_error(QcArgs a, float flow_thr, int* __restrict__ bad) {
  __shared__ double vec[4 * 2];
  const int tid = threadIdx.x;
  const size_t plane = (size_t)a.Y * a.X;
  for (int oi = blockIdx.x; oi < a.n_obj; oi += gridDim.x) {
    const aliby_object o = a.tab[oi];
    if (o.area <= 0) { if (tid == 0) bad[oi] = 1; continue; }
    const u16* lab = a.labels + (size_t)o.tile * plane;
    const double* T = a.Tg + (size_t)o.tile * plane;
    const float* dy_net = a.dP + ((size_t)o.tile * 2 + 0) * plane;
    const float* dx_net = a.dP + ((size_t)o.tile * 2 + 1) * plane;
    const int h = o.y1 - o.y0, w = o.x1 - o.x0;
    const u16 L = (u16)o.label;
    double e[2] = {0, 0};
    for (int i = tid; i < h * w; i += blockDim.x) {
      const int y = o.y0 + i / w, x = o.x0 + i % w;
      const size_t idx = (size_t)y * a.X + x;
      if (lab[idx] != L) continue;
      const double tu = (y > 0) ? T[idx - a.X] : 0.0, td = (y + 1 < a.Y) ? T[idx + a.X] : 0.0;
      const double tl = (x > 0) ? T[idx - 1] : 0.0, tr = (x + 1 < a.X) ? T[idx + 1] : 0.0;
      const double dy = td - tu, dx = tr - tl;
      const double nrm = 1e-60 + sqrt(dy * dy + dx * dx);
      const double my = dy / nrm, mx = dx / nrm;
      const double ey = my - (double)dy_net[idx] / 5.0, ex = mx - (double)dx_net[idx] / 5.0;
      e[0] += ey * ey;
      e[1] += ex * ex;
    }
    block_sum_vec_all<2>(e, vec);
    if (tid == 0) {
      const double err = e[0] / (double)o.area + e[1] / (double)o.area;
      bad[oi] = (err > (double)flow_thr) ? 1 : 0;
    }
    __syncthreads();
  }
}

// The heat map Tg is written at mask pixels and read at mask pixels and their four neighbours: zero is needed on every object's
// box grown by one pixel, not on the whole frame (8 bytes per pixel).  All boxes are cleared before any mask is written.
__global__ __launch_bounds__(256) void k_zero_boxes(const aliby_object* __restrict__ tab, int n_obj, int Y, int X, double* __restrict__ Tg) {
  const size_t plane = (size_t)Y * X;
  for (int oi = blockIdx.x; oi < n_obj; oi += gridDim.x) {
    const aliby_object o = tab[oi];
    if (o.area <= 0) continue;
    const int y0 = max(o.y0 - 1, 0), y1 = min(o.y1 + 1, Y), x0 = max(o.x0 - 1, 0), x1 = min(o.x1 + 1, X);
    const int w = x1 - x0, n = (y1 - y0) * w;
    double* T = Tg + (size_t)o.tile * plane;
    for (int i = threadIdx.x; i < n; i += blockDim.x) T[(size_t)(y0 + i / w) * X + x0 + i % w] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------
// 5. survivors -> final ids; hole filling; small-mask removal
// ---------------------------------------------------------------------------------------------
// The two object tables, read by k_final_ids (the rows of frame f, and which of them are kept) and by k_fill (the rows that
// workgroup row g walks, and their boxes with exclusive extents).
struct Box {
  int frame, label;
  int z0, y0, x0, d, h, w;
};

// images: aliby_object rows of all frames in one list (frame f's from offsets[f]), bounds exclusive above; bad[] from the flow QC
struct ImageObjects {
  const aliby_object* tab;
  const int* offsets;  // [F+1]
  const int* bad;
  int n_obj;
  __device__ size_t first(int f) const { return (size_t)offsets[f]; }
  __device__ int count(int f) const { return offsets[f + 1] - offsets[f]; }
  __device__ bool keep(size_t i, int min_size) const { return !bad[i] && tab[i].area > 0 && tab[i].area >= min_size; }
  __device__ u64 box_cells(size_t) const { return 0; }      // (the image fill is sized from the host's copy of the table)
  __device__ int fill_count(int) const { return n_obj; }    // (one grid row walks the rows of every frame)
  __device__ size_t fill_row(int, int k) const { return (size_t)k; }
  __device__ Box box(int, size_t i) const {
    const aliby_object o = tab[i];
    return Box{o.tile, o.label, 0, o.y0, o.x0, 1, o.y1 - o.y0, o.x1 - o.x0};
  }
};

// volumes: Obj3 rows [F, LABELS_PER_VOL], row k of volume f holding label k + 1, bounds inclusive
struct VolumeObjects {
  const Obj3* tab;
  const int* ntot;  // [F] labels per volume
  __device__ size_t first(int f) const { return (size_t)f * LABELS_PER_VOL; }
  __device__ int count(int f) const { return min(ntot[f], LABELS_PER_VOL - 1); }
  __device__ bool keep(size_t i, int min_size) const { return tab[i].area > 0 && tab[i].area >= min_size; }
  // the box grown by one voxel per side: the largest kept one sizes the hole fill's scratch
  __device__ u64 box_cells(size_t i) const {
    const Obj3 o = tab[i];
    return (u64)(o.z1 - o.z0 + 3) * (o.y1 - o.y0 + 3) * (o.x1 - o.x0 + 3);
  }
  __device__ int fill_count(int f) const { return count(f); }  // (grid row f walks volume f)
  __device__ size_t fill_row(int f, int k) const { return first(f) + k; }
  __device__ Box box(int f, size_t i) const {
    const Obj3 o = tab[i];
    return Box{f, (int)(i - first(f)) + 1, o.z0, o.y0, o.x0, o.z1 - o.z0 + 1, o.y1 - o.y0 + 1, o.x1 - o.x0 + 1};
  }
};

// one workgroup per frame: newlabel = rank among the kept rows (1-based); max_cells = the largest box_cells of a kept row
template <class Objects>
__global__ __launch_bounds__(1024) void k_final_ids(Objects ob, int min_size, int* __restrict__ newlabel, int* __restrict__ nfinal,
                                                    u64* __restrict__ max_cells) {
  __shared__ int part[1024];
  const int f = blockIdx.x, t = threadIdx.x;
  const size_t lo0 = ob.first(f);
  const int n = ob.count(f);
  const int per = (n + 1023) / 1024;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int c = 0;
  u64 big = 0;
  for (int i = lo; i < hi; ++i) {
    if (!ob.keep(lo0 + i, min_size)) continue;
    ++c;
    const u64 cells = ob.box_cells(lo0 + i);
    big = cells > big ? cells : big;
  }
  part[t] = c;
  if (big) atomicMax(max_cells, big);
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = (t >= o) ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - c;
  for (int i = lo; i < hi; ++i) newlabel[lo0 + i] = ob.keep(lo0 + i, min_size) ? ++run : 0;
  if (t == 1023) nfinal[f] = part[1023];
}

template <class Objects>
struct FillArgs {
  const u16* labels;  // first-appearance labels, before small-mask removal
  int Y, X;
  size_t frame;       // pixels per frame
  Objects ob;
  const int* newlabel;  // per table row (0: dropped)
  size_t cap_cells;
  unsigned char* gscratch;
  u16* out;  // zeroed; a 16-bit atomic max resolves nested holes (highest label wins)
};

// max into one half of an aligned 32-bit word (there are no 16-bit atomics): compare-and-swap until our half is >= v
__device__ __forceinline__ void atomic_max_u16(u16* addr, unsigned v) {
  unsigned int* word = reinterpret_cast<unsigned int*>(reinterpret_cast<size_t>(addr) & ~(size_t)3);
  const unsigned shift = (reinterpret_cast<size_t>(addr) & 2) ? 16u : 0u;
  unsigned int old = *word;
  while (((old >> shift) & 0xffffu) < v) {
    const unsigned int want = (old & ~(0xffffu << shift)) | (v << shift);
    const unsigned int seen = atomicCAS(word, old, want);
    if (seen == old) break;
    old = seen;
  }
}

// cell i of a box of h rows by w columns per plane -> (plane, row, column); boxes of the 4-neighbourhood have one plane
template <int NB, class I>
__device__ __forceinline__ void box_cell(I i, int h, int w, int& q, int& r, int& c) {
  c = (int)(i % w);
  if constexpr (NB == 6) {
    r = (int)((i / w) % h);
    q = (int)(i / ((I)w * h));
  } else {
    r = (int)(i / w);
    q = 0;
  }
}

// One workgroup per kept mask: its box with a one-pixel ring (state 0 unknown, 1 mask, 2 reachable from outside), flooded with
// the NB-neighbourhood (4: images, 6: volumes) until nothing changes; everything not reached is the filled mask.
template <int NB, bool GLOBAL, class Objects>
__global__ __launch_bounds__(256) void k_fill(FillArgs<Objects> a) {
  using I = typename std::conditional<NB == 6, size_t, int>::type;  // (a volume's box may pass 2^31 cells)
  constexpr int zr = NB == 6 ? 1 : 0;                                // ring planes before the box
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ int s_changed;
  unsigned char* st = GLOBAL ? (a.gscratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.cap_cells) : lds_raw;
  const int tid = threadIdx.x, g = blockIdx.y;
  const int n = a.ob.fill_count(g);
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const size_t row = a.ob.fill_row(g, k);
    const int nl = a.newlabel[row];
    if (nl == 0) continue;  // (block-uniform)
    const Box b = a.ob.box(g, row);
    const int ph = b.h + 2, pw = b.w + 2;
    const I ncell = (I)(b.d + 2 * zr) * ph * pw, nin = (I)b.d * b.h * b.w;
    if ((size_t)ncell > a.cap_cells) continue;  // (cannot happen: cap_cells is the largest kept box)
    const u16* lab = a.labels + (size_t)b.frame * a.frame;
    u16* out = a.out + (size_t)b.frame * a.frame;
    const u16 L = (u16)b.label;
    __syncthreads();
    for (I i = tid; i < ncell; i += blockDim.x) {
      int q, r, c;
      box_cell<NB>(i, ph, pw, q, r, c);
      q -= zr; r -= 1; c -= 1;
      unsigned char v;
      if (q < 0 || q >= b.d || r < 0 || r >= b.h || c < 0 || c >= b.w) v = 2;  // ring: background reachable from outside
      else v = (lab[((size_t)(b.z0 + q) * a.Y + b.y0 + r) * a.X + b.x0 + c] == L) ? 1 : 0;
      st[i] = v;
    }
    __syncthreads();
    const I sl = (I)ph * pw;
    for (I sweep = 0; sweep < ncell; ++sweep) {
      if (tid == 0) s_changed = 0;
      __syncthreads();
      int ch = 0;
      for (I i = tid; i < nin; i += blockDim.x) {
        int q, r, c;
        box_cell<NB>(i, b.h, b.w, q, r, c);
        const I kk = ((I)(q + zr) * ph + r + 1) * pw + c + 1;
        if (st[kk] != 0) continue;
        bool outside = st[kk - 1] == 2 || st[kk + 1] == 2 || st[kk - pw] == 2 || st[kk + pw] == 2;
        if constexpr (NB == 6) outside = outside || st[kk - sl] == 2 || st[kk + sl] == 2;
        if (outside) { st[kk] = 2; ch = 1; }
      }
      if (ch) s_changed = 1;
      __syncthreads();
      const int any = s_changed;
      __syncthreads();
      if (!any) break;
    }
    for (I i = tid; i < nin; i += blockDim.x) {
      int q, r, c;
      box_cell<NB>(i, b.h, b.w, q, r, c);
      const I kk = ((I)(q + zr) * ph + r + 1) * pw + c + 1;
      if (st[kk] != 2) atomic_max_u16(&out[((size_t)(b.z0 + q) * a.Y + b.y0 + r) * a.X + b.x0 + c], (unsigned)nl);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------------------------
static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// consecutive 256-byte-aligned pieces of a caller's workspace
struct Carve {
  unsigned char* p;
  template <class T>
  T* take(size_t n) {
    T* r = reinterpret_cast<T*>(p);
    p += align256(sizeof(T) * n);
    return r;
  }
};

// ALIBY_DEBUG_FG_REVERSE=1, a test hook: the compaction runs as one workgroup, which walks the chunks last to first, so that is
// their order in the list (read per call: a test switches it)
static int fg_reverse() {
  const char* e = getenv("ALIBY_DEBUG_FG_REVERSE");
  return e && atoi(e) ? 1 : 0;
}

// The hole fill's box states: in LDS up to 128 KB, else one slab of context scratch per workgroup (grid-strided over the masks)
// after the scratch's first `head` bytes.  n x groups workgroups.
template <int NB, class Objects>
static int launch_fill(aliby_ctx* ctx, FillArgs<Objects> a, int n, int groups, int lds_block, size_t head, hipStream_t s) {
  if (a.cap_cells <= 128 * 1024) {
    a.gscratch = nullptr;
    if (a.cap_cells > 32 * 1024)
      HIP_TRY(hipFuncSetAttribute((const void*)(k_fill<NB, false, Objects>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)a.cap_cells));
    hipLaunchKernelGGL((k_fill<NB, false, Objects>), dim3(n, groups), dim3(lds_block), a.cap_cells, s, a);
  } else {
    const int g = n < 256 ? n : 256;
    const int rc = aliby_ensure_scratch(ctx, head + (size_t)g * groups * a.cap_cells);
    if (rc) return rc;
    a.gscratch = (unsigned char*)ctx->scratch + head;
    hipLaunchKernelGGL((k_fill<NB, true, Objects>), dim3(g, groups), dim3(256), 0, s, a);
  }
  KERNEL_CHECK();
  return ALIBY_OK;
}

extern "C" {

size_t aliby_masks_workspace_bytes(int F, int Y, int X) {
  const size_t P = (size_t)Y * X, PP = (size_t)(Y + 2 * RPAD) * (X + 2 * RPAD);
  size_t b = 0;
  b += align256(sizeof(float) * 2 * P * F);   // im
  b += align256(sizeof(int) * P * F) * 3;     // foreground list, end-point cells, temporary labels (sized for an all-foreground frame)
  b += align256(sizeof(int) * PP * F) * 4;    // h1, cnt, firstpos, newid
  b += align256(sizeof(u64) * PP * F);        // M1
  b += align256(sizeof(u16) * P * F);         // first-appearance labels (before QC)
  b += align256(sizeof(double) * P * F);      // Tg
  b += align256(sizeof(int) * SEEDS_PER_FRAME * (size_t)F);  // seed lists
  b += align256(sizeof(aliby_object) * 65536 * (size_t)F);  // object table
  b += align256(sizeof(int) * 65536 * (size_t)F) * 2;  // bad, newlabel
  b += align256(sizeof(int) * (size_t)(5 * F + 8));    // counters
  return b;
}

int aliby_object_table(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X, const int32_t* offsets_host,
                       aliby_object* table_dev, aliby_object* table_host, void* stream);

int aliby_masks_from_flows(aliby_ctx* ctx, const float* dP, const float* cellprob, int F, int Y, int X, int niter,
                           float cellprob_threshold, float flow_threshold, int min_size, float max_size_fraction,
                           void* workspace, size_t workspace_bytes, uint16_t* labels_out, int32_t* n_labels_host,
                           float* p_final_out, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(F >= 0 && Y > 1 && X > 1, "bad shape");
  if (F == 0) return ALIBY_OK;
  ARG_CHECK(dP && cellprob && workspace && labels_out && n_labels_host, "NULL argument");
  ARG_CHECK(workspace_bytes >= aliby_masks_workspace_bytes(F, Y, X), "workspace too small (aliby_masks_workspace_bytes)");
  ARG_CHECK(niter >= 0, "niter must be >= 0");
  hipStream_t s = as_stream(stream);
  DynShape sh;
  sh.F = F; sh.Y = Y; sh.X = X; sh.YP = Y + 2 * RPAD; sh.XP = X + 2 * RPAD; sh.Z = 1;
  sh.P = (size_t)Y * X; sh.PP = (size_t)sh.YP * sh.XP;
  ARG_CHECK(sh.PP < (size_t)INT_MAX && F <= 65535, "image too large");

  Carve w{(unsigned char*)workspace};
  float* im = w.take<float>(2 * sh.P * F);
  int* fg_list = w.take<int>(sh.P * F);
  int* ptc = w.take<int>(sh.P * F);
  unsigned* labc = w.take<unsigned>(sh.P * F);
  int* h1 = w.take<int>(sh.PP * F);
  int* cnt = w.take<int>(sh.PP * F);
  int* firstpos = w.take<int>(sh.PP * F);
  int* newid = w.take<int>(sh.PP * F);
  u64* M1 = w.take<u64>(sh.PP * F);
  u16* labels_tmp = w.take<u16>(sh.P * F);
  double* Tg = w.take<double>(sh.P * F);
  int* seed_list = w.take<int>(SEEDS_PER_FRAME * (size_t)F);
  aliby_object* tab = w.take<aliby_object>(65536 * (size_t)F);
  int* bad = w.take<int>(65536 * (size_t)F);
  int* newlabel = w.take<int>(65536 * (size_t)F);
  int* counters = w.take<int>((size_t)(5 * F + 8));
  int* fg_count = counters + 1;
  int* ntot = counters + 8;          // [F]
  int* niter_tile = ntot + F;        // [F]
  int* nfinal = niter_tile + F;      // [F]
  int* seed_count = nfinal + F;      // [F]

  const size_t totP = sh.P * F, totPP = sh.PP * F;
  ARG_CHECK(totP < (size_t)INT_MAX, "batch too large for 32-bit pixel indices");
  const int gP = (int)((totP + 255) / 256 > 16384 ? 16384 : (totP + 255) / 256);

  // Memsets: the end-point histogram (read in 5x5 / 11x11 neighbourhoods: it must be zero everywhere), the two label images
  // (written at foreground pixels only) and the counters.  Everything else — the seed map M1, the per-label count / first
  // position / new id words — is initialised where it is used (k_follow, k_grow).
  HIP_TRY(hipMemsetAsync(h1, 0, sizeof(int) * totPP, s));
  HIP_TRY(hipMemsetAsync(labels_tmp, 0, sizeof(u16) * totP, s));
  HIP_TRY(hipMemsetAsync(labels_out, 0, sizeof(u16) * totP, s));
  HIP_TRY(hipMemsetAsync(counters, 0, sizeof(int) * (size_t)(5 * F + 8), s));
  const FlowScale sc{{2.0f / (float)(Y - 1), 2.0f / (float)(X - 1), 0.0f}};
  const int rev = fg_reverse();
  hipLaunchKernelGGL((k_prep_compact<2>), dim3(rev ? 1 : gP), dim3(256), 0, s, dP, cellprob, cellprob_threshold, sh, sc, im, fg_list,
                     fg_count, rev);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_follow, dim3(gP), dim3(256), 0, s, im, fg_list, fg_count, sh, niter, ptc, h1, M1, p_final_out);
  KERNEL_CHECK();
  const int gPP = (int)((totPP + 255) / 256 > 16384 ? 16384 : (totPP + 255) / 256);
  hipLaunchKernelGGL(k_seeds, dim3(gPP), dim3(256), 0, s, h1, sh, seed_list, seed_count);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_grow, dim3(256, F), dim3(64), 0, s, h1, sh, seed_list, seed_count, M1, cnt, firstpos, newid);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_assign, dim3(gP), dim3(256), 0, s, fg_list, fg_count, ptc, M1, sh, labc, cnt, firstpos);
  KERNEL_CHECK();
  const float big = (float)((double)Y * (double)X * (double)max_size_fraction);
  hipLaunchKernelGGL((k_rank_ids<float>), dim3(F), dim3(256), 0, s, seed_list, seed_count, sh, cnt, firstpos, big, newid, ntot);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_apply_ids, dim3(gP), dim3(256), 0, s, fg_list, fg_count, labc, newid, sh, labels_tmp);
  KERNEL_CHECK();
  HIP_TRY(hipMemcpyAsync(n_labels_host, ntot, sizeof(int) * F, hipMemcpyDeviceToHost, s));
  { const int rcw = aliby_wait_stream(s); if (rcw) return rcw; }
  int n_obj = 0;
  {
    std::vector<int> nseeds((size_t)F);
    HIP_TRY(hipMemcpy(nseeds.data(), seed_count, sizeof(int) * F, hipMemcpyDeviceToHost));  // (the stream is idle: just waited)
    for (int f = 0; f < F; ++f)
      if (nseeds[f] >= SEEDS_PER_FRAME - 1) {
        aliby_set_error("Segmentation produced %d seeds in one tile; uint16 cast unsafe.", nseeds[f]);
        return ALIBY_ERR_OVERFLOW;
      }
  }
  for (int f = 0; f < F; ++f) {
    if (n_labels_host[f] >= 65535) {
      aliby_set_error("Segmentation produced %d labels; uint16 cast unsafe.", n_labels_host[f]);
      return ALIBY_ERR_OVERFLOW;
    }
    n_obj += n_labels_host[f];
  }
  if (n_obj == 0) return ALIBY_OK;  // labels_out is all zero

  // ---- per-mask stages: object table, flow QC, hole fill ----------------------------------------
  std::vector<int> offsets((size_t)F + 1, 0);
  for (int f = 0; f < F; ++f) offsets[f + 1] = offsets[f] + n_labels_host[f];
  std::vector<aliby_object> tab_host((size_t)n_obj);
  int rc = aliby_object_table(ctx, labels_tmp, F, Y, X, offsets.data(), tab, tab_host.data(), stream);
  if (rc) return rc;
  int max_h = 0, max_w = 0;
  std::vector<int> nit((size_t)F);
  for (int f = 0; f < F; ++f) {
    int me = 0;
    for (int i = offsets[f]; i < offsets[f + 1]; ++i) {
      const int hh = tab_host[i].y1 - tab_host[i].y0, ww = tab_host[i].x1 - tab_host[i].x0;
      if (tab_host[i].area <= 0) continue;
      if (hh > max_h) max_h = hh;
      if (ww > max_w) max_w = ww;
      if (hh + 1 + ww + 1 > me) me = hh + 1 + ww + 1;
    }
    nit[f] = 2 * me;
  }
  HIP_TRY(hipMemcpyAsync(niter_tile, nit.data(), sizeof(int) * F, hipMemcpyHostToDevice, s));
  // offsets for k_final_ids live in ctx scratch (aliby_object_table put them there)
  const int* d_off = (const int*)ctx->scratch;
  const size_t cells = ((size_t)(max_h + 2) * (max_w + 2) + 15) & ~(size_t)15;
  const size_t head = align256(sizeof(int) * (size_t)(F + 1));  // (the offsets' bytes at the start of ctx scratch)

  if (flow_threshold > 0.0f) {
    hipLaunchKernelGGL(k_zero_boxes, dim3(n_obj < 8192 ? n_obj : 8192), dim3(256), 0, s, tab, n_obj, Y, X, Tg);
    KERNEL_CHECK();
    QcArgs q;
    q.labels = labels_tmp; q.dP = dP; q.F = F; q.Y = Y; q.X = X; q.tab = tab; q.n_obj = n_obj;
    q.niter_tile = niter_tile; q.cap_cells = cells; q.Tg = Tg;
    const size_t need = cells * 17;
    if (need <= 128 * 1024) {
      q.gscratch = nullptr;
      if (need > 32 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void*)k_diffuse<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
      // four waves per mask whatever its size: a sweep is a few dozen instructions per pixel behind one barrier, and one wave
      // walking 10+ rows per lane per sweep (the per-object default for small windows) left the SIMDs idle 70 % of the time —
      // 2.66 -> 1.8 ms for 16 k nuclei (64 / 128 / 256 threads: 5.5 / 4.8 / 4.6 ms for the whole dynamics)
      hipLaunchKernelGGL((k_diffuse<false>), dim3(n_obj), dim3(256), need, s, q);
    } else {
      // ctx scratch holds the offsets in its first bytes: put the slabs after them, and upload the offsets again (ensure_scratch
      // may reallocate)
      const int g = n_obj < 256 ? n_obj : 256;
      const int rc2 = aliby_ensure_scratch(ctx, head + (size_t)g * need);
      if (rc2) return rc2;
      HIP_TRY(hipMemcpyAsync(ctx->scratch, offsets.data(), sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
      d_off = (const int*)ctx->scratch;
      q.gscratch = (unsigned char*)ctx->scratch + head;
      hipLaunchKernelGGL((k_diffuse<true>), dim3(g), dim3(256), 0, s, q);
    }
    KERNEL_CHECK();
    hipLaunchKernelGGL(k_flow_error, dim3(n_obj), dim3(aliby_pick_block((long long)max_h * max_w)), 0, s, q, flow_threshold, bad);
    KERNEL_CHECK();
  } else {
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int) * (size_t)n_obj, s));
  }
  const ImageObjects ob{tab, d_off, bad, n_obj};
  hipLaunchKernelGGL((k_final_ids<ImageObjects>), dim3(F), dim3(1024), 0, s, ob, min_size, newlabel, nfinal, (u64*)nullptr);
  KERNEL_CHECK();
  const FillArgs<ImageObjects> fa{labels_tmp, Y, X, sh.P, ob, newlabel, cells, nullptr, labels_out};
  rc = launch_fill<4>(ctx, fa, n_obj, 1, aliby_pick_block((long long)max_h * max_w), head, s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(n_labels_host, nfinal, sizeof(int) * F, hipMemcpyDeviceToHost, s));
  { const int rcw = aliby_wait_stream(s); if (rcw) return rcw; }
  return ALIBY_OK;
}

size_t aliby_masks3d_workspace_bytes(int F, int Z, int Y, int X) {
  const size_t V = (size_t)Z * Y * X * (size_t)(F > 0 ? F : 0);
  size_t b = 0;
  b += align256(sizeof(float) * 3 * V);  // im
  b += align256(sizeof(int) * V) * 3;    // foreground list, end cells, temporary labels
  b += align256(sizeof(int) * V) * 4;    // h1, cnt, firstpos, newid
  b += align256(sizeof(u64) * V);        // M1
  b += align256(sizeof(u16) * V);        // first-appearance labels
  b += align256(sizeof(int) * SEEDS_PER_FRAME * (size_t)F);    // seed lists
  b += align256(sizeof(Obj3) * LABELS_PER_VOL * (size_t)F);   // object table
  b += align256(sizeof(int) * LABELS_PER_VOL * (size_t)F);    // new labels
  b += align256(sizeof(int) * (size_t)(4 * F + 8));           // counters
  return b;
}

int aliby_masks_from_flows_3d(aliby_ctx* ctx, const float* dP, const float* cellprob, int F, int Z, int Y, int X, int niter,
                              float cellprob_threshold, int min_size, float max_size_fraction, void* workspace,
                              size_t workspace_bytes, uint16_t* labels_out, int32_t* n_labels_host, float* p_final_out,
                              void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(F >= 0 && Z > 1 && Y > 1 && X > 1, "bad shape (Z, Y, X > 1)");
  if (F == 0) return ALIBY_OK;
  ARG_CHECK(dP && cellprob && workspace && labels_out && n_labels_host, "NULL argument");
  ARG_CHECK(workspace_bytes >= aliby_masks3d_workspace_bytes(F, Z, Y, X), "workspace too small (aliby_masks3d_workspace_bytes)");
  ARG_CHECK(niter >= 0, "niter must be >= 0");
  DynShape sh;
  sh.F = F; sh.Z = Z; sh.Y = Y; sh.X = X; sh.YP = Y; sh.XP = X;
  sh.P = sh.PP = (size_t)Z * Y * X;
  ARG_CHECK(sh.P * F < (size_t)INT_MAX, "batch too large for 32-bit voxel indices");
  hipStream_t s = as_stream(stream);

  Carve w{(unsigned char*)workspace};
  const size_t tot = sh.P * F;
  float* im = w.take<float>(3 * tot);
  int* fg_list = w.take<int>(tot);
  int* ptc = w.take<int>(tot);
  unsigned* labc = w.take<unsigned>(tot);
  int* h1 = w.take<int>(tot);
  int* cnt = w.take<int>(tot);
  int* firstpos = w.take<int>(tot);
  int* newid = w.take<int>(tot);
  u64* M1 = w.take<u64>(tot);
  u16* labels_tmp = w.take<u16>(tot);
  int* seed_list = w.take<int>(SEEDS_PER_FRAME * (size_t)F);
  Obj3* tab = w.take<Obj3>(LABELS_PER_VOL * (size_t)F);
  int* newlabel = w.take<int>(LABELS_PER_VOL * (size_t)F);
  int* counters = w.take<int>((size_t)(4 * F + 8));
  u64* max_cells = (u64*)counters;  // counters[0..1]
  int* fg_count = counters + 2;
  int* ntot = counters + 8;         // [F]
  int* seed_count = ntot + F;       // [F]
  int* nfinal = seed_count + F;     // [F]

  HIP_TRY(hipMemsetAsync(h1, 0, sizeof(int) * tot, s));
  HIP_TRY(hipMemsetAsync(labels_tmp, 0, sizeof(u16) * tot, s));
  HIP_TRY(hipMemsetAsync(labels_out, 0, sizeof(u16) * tot, s));
  HIP_TRY(hipMemsetAsync(counters, 0, sizeof(int) * (size_t)(4 * F + 8), s));
  const int gV = (int)((tot + 255) / 256 > 16384 ? 16384 : (tot + 255) / 256);
  const FlowScale sc{{2.0f / (float)(Z - 1), 2.0f / (float)(Y - 1), 2.0f / (float)(X - 1)}};
  const int rev = fg_reverse();
  hipLaunchKernelGGL((k_prep_compact<3>), dim3(rev ? 1 : gV), dim3(256), 0, s, dP, cellprob, cellprob_threshold, sh, sc, im, fg_list,
                     fg_count, rev);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_follow, dim3(gV), dim3(256), 0, s, im, fg_list, fg_count, sh, niter, ptc, h1, M1, p_final_out);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_seeds, dim3(gV), dim3(256), 0, s, h1, sh, seed_list, seed_count);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_grow, dim3(1024, F), dim3(256), 0, s, h1, sh, seed_list, seed_count, M1, cnt, firstpos, newid);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_assign, dim3(gV), dim3(256), 0, s, fg_list, fg_count, ptc, M1, sh, labc, cnt, firstpos);
  KERNEL_CHECK();
  const double big = (double)sh.P * (double)max_size_fraction;
  hipLaunchKernelGGL((k_rank_ids<double>), dim3(F), dim3(256), 0, s, seed_list, seed_count, sh, cnt, firstpos, big, newid, ntot);
  KERNEL_CHECK();
  const size_t ntab = (size_t)LABELS_PER_VOL * F;
  hipLaunchKernelGGL(k3_init_table, dim3((int)((ntab + 255) / 256)), dim3(256), 0, s, tab, ntab);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_apply_ids, dim3(gV), dim3(256), 0, s, fg_list, fg_count, labc, newid, sh, labels_tmp, tab);
  KERNEL_CHECK();
  const VolumeObjects ob{tab, ntot};
  hipLaunchKernelGGL((k_final_ids<VolumeObjects>), dim3(F), dim3(1024), 0, s, ob, min_size, newlabel, nfinal, max_cells);
  KERNEL_CHECK();
  // one download: max_cells (2 words), fg count, pad, ntot[F], seed_count[F], nfinal[F]
  std::vector<int> host((size_t)(4 * F + 8));
  HIP_TRY(hipMemcpyAsync(host.data(), counters, sizeof(int) * host.size(), hipMemcpyDeviceToHost, s));
  { const int rcw = aliby_wait_stream(s); if (rcw) return rcw; }
  u64 cells = 0;
  memcpy(&cells, host.data(), sizeof(cells));
  int max_n = 0;
  for (int f = 0; f < F; ++f) {
    const int nseed = host[8 + F + f], nlab = host[8 + f];
    if (nseed >= SEEDS_PER_FRAME - 1 || nlab >= 65535) {
      aliby_set_error("Segmentation produced %d labels (%d seeds) in one volume; uint16 cast unsafe.", nlab, nseed);
      return ALIBY_ERR_OVERFLOW;
    }
    max_n = nlab > max_n ? nlab : max_n;
  }
  for (int f = 0; f < F; ++f) n_labels_host[f] = host[8 + 2 * F + f];
  if (cells == 0) return ALIBY_OK;  // no mask kept: labels_out is all zero, the counts are 0

  // (a box beyond LDS — a 40 x 100 x 100 box is 400 k voxels — takes the global scratch: one slab per workgroup and volume)
  const FillArgs<VolumeObjects> fa{labels_tmp, Y, X, sh.P, ob, newlabel, (size_t)((cells + 15) & ~15ull), nullptr, labels_out};
  const int rc = launch_fill<6>(ctx, fa, max_n, F, 256, 0, s);
  if (rc) return rc;
  { const int rcw = aliby_wait_stream(s); if (rcw) return rcw; }
  return ALIBY_OK;
}

}  // extern "C"
