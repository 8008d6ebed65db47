// dynamics3d.hip — Cellpose's post-network dynamics for volumes (do_3D): (dZ, dY, dX, cellprob) [F,...,Z,Y,X] -> labels.
//
// Reference call site: `segment(pixels, do_3D=True)` -> `model.eval(..., do_3D=True, z_axis=1)` (src/aliby/segment/dispatch.py:
// 193-198, 208-215; cellpose 4.0.6 not vendored — PARITY UNPINNED against Cellpose itself).  Restated from the published
// algorithm (cellpose.dynamics.compute_masks with a 3-D flow field); the float32 restatement tests/cellpose3d_ref.py writes the
// same operations in the same order, so labels are compared bit for bit.
//   follow      niter Euler steps p = clamp(p + trilinear(dP * fg / 5 * 2/(L-1))(p), -1, 1) in grid_sample's normalised
//               coordinates (align_corners=False, zero padding; taps tnw..bse, weights (wx*wy)*wz, summed from 0 in tap order);
//   seeds       end-point histogram (padded by 20 in cellpose; end points never leave the volume, so the margin is always empty
//               and the histogram here is unpadded, out-of-range reads being empty), maxima of 5x5x5 with > 10 points;
//   growth      5 x (3x3x3 dilation AND bin > 2) in an 11x11x11 window per seed, overlaps resolved by (points, raster position);
//   labels      voxel = seed owning its end cell, masks above max_size_fraction of the volume dropped, first-appearance ids;
//   fill        masks below min_size dropped, 3-D holes (6-connected background, inside the bounding box) filled, ids 1..n.
// No flow-error QC: cellpose documents flow_threshold as "not used for 3D".
//
// The structure is dynamics.hip's: a compacted foreground list, end cells per list position, per-volume seed lists, growth by an
// atomic max over the seed priority, then an object table and the hole fill (LDS boxes, or grid-strided global scratch for boxes
// beyond LDS).
#include "common.h"

typedef unsigned short u16;
typedef unsigned long long u64;

#define RPAD3 20
#define SEEDS_PER_VOL 65536
#define LABELS_PER_VOL 65536
#define FG_CHUNK3 4096

struct Dyn3 {
  int F, Z, Y, X;
  size_t V;  // voxels per volume
};

struct Obj3 {
  int z0, y0, x0, z1, y1, x1;  // inclusive bounds while built
  int area, pad_;
};

// ---------------------------------------------------------------------------------------------
// 0. masked, normalised flow field im_d = ((fg ? dP_d : 0) / 5) * (2 / (L_d - 1)) and the compacted foreground list
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k3_prep_compact(const float* __restrict__ dP, const float* __restrict__ prob, float thr, Dyn3 s,
                                                       float cz, float cy, float cx, float* __restrict__ im, int* __restrict__ list,
                                                       int* __restrict__ count) {
  __shared__ int red_i[8];
  __shared__ int wsum[4];
  __shared__ int s_base;
  const size_t total = (size_t)s.F * s.V;
  const size_t nchunks = (total + FG_CHUNK3 - 1) / FG_CHUNK3;
  for (size_t ci = blockIdx.x; ci < nchunks; ci += gridDim.x) {
    const size_t c0 = ci * FG_CHUNK3;
    unsigned fgmask = 0;
#pragma unroll
    for (int k = 0; k < FG_CHUNK3 / 256; ++k) {
      const size_t i = c0 + (size_t)k * 256 + threadIdx.x;
      if (i >= total) continue;
      const bool m = prob[i] > thr;
      fgmask |= (unsigned)m << k;
      const size_t f = i / s.V, p = i % s.V;
      float vz = dP[(f * 3 + 0) * s.V + p], vy = dP[(f * 3 + 1) * s.V + p], vx = dP[(f * 3 + 2) * s.V + p];
      vz = m ? vz : 0.0f;
      vy = m ? vy : 0.0f;
      vx = m ? vx : 0.0f;
      vz = vz / 5.0f;
      vy = vy / 5.0f;
      vx = vx / 5.0f;
      im[(f * 3 + 0) * s.V + p] = vz * cz;
      im[(f * 3 + 1) * s.V + p] = vy * cy;
      im[(f * 3 + 2) * s.V + p] = vx * cx;
    }
    const int tot = block_sum_i32(__popc(fgmask), red_i);
    if (tot == 0) continue;  // block-uniform
    if (threadIdx.x == 0) s_base = atomicAdd(count, tot);
    __syncthreads();
    int base = s_base;
#pragma unroll
    for (int k = 0; k < FG_CHUNK3 / 256; ++k) {
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
struct Taps3 { float v[8]; };

__device__ __forceinline__ float tap3(const float* __restrict__ f, int zz, int yy, int xx, const Dyn3& s) {
  return (zz >= 0 && zz < s.Z && yy >= 0 && yy < s.Y && xx >= 0 && xx < s.X) ? f[((size_t)zz * s.Y + yy) * s.X + xx] : 0.0f;
}

__device__ __forceinline__ void load_taps(const float* __restrict__ f, int z0, int y0, int x0, const Dyn3& s, Taps3& t) {
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
                                                 const int* __restrict__ count, Dyn3 s, int niter, int* __restrict__ ptc,
                                                 int* __restrict__ h1, u64* __restrict__ M1, float* __restrict__ pfinal) {
  const int total = *count;
  const float sz = (float)(s.Z - 1), sy = (float)(s.Y - 1), sx = (float)(s.X - 1);
  const float Zf = (float)s.Z, Yf = (float)s.Y, Xf = (float)s.X;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += gridDim.x * blockDim.x) {
    const size_t i = (size_t)list[j];
    const size_t f = i / s.V, p = i % s.V;
    const float* imz = im + (f * 3 + 0) * s.V;
    const float* imy = im + (f * 3 + 1) * s.V;
    const float* imx = im + (f * 3 + 2) * s.V;
    const int z = (int)(p / ((size_t)s.Y * s.X)), y = (int)((p / s.X) % s.Y), x = (int)(p % s.X);
    float pz = (float)z / sz * 2.0f - 1.0f;
    float py = (float)y / sy * 2.0f - 1.0f;
    float px = (float)x / sx * 2.0f - 1.0f;
    // the 8 taps of each component stay in registers until the point enters another voxel cell (dynamics.hip: most of the
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
      pfinal[(f * 3 + 0) * s.V + p] = fz;
      pfinal[(f * 3 + 1) * s.V + p] = fy;
      pfinal[(f * 3 + 2) * s.V + p] = fx;
    }
    // cellpose's cell of the padded histogram, trunc(clamp(end + 20, 0, L + 19)), shifted back by the pad
    const int qz = (int)fminf(fmaxf(fz + (float)RPAD3, 0.0f), (float)(s.Z + RPAD3 - 1)) - RPAD3;
    const int qy = (int)fminf(fmaxf(fy + (float)RPAD3, 0.0f), (float)(s.Y + RPAD3 - 1)) - RPAD3;
    const int qx = (int)fminf(fmaxf(fx + (float)RPAD3, 0.0f), (float)(s.X + RPAD3 - 1)) - RPAD3;
    // (end points lie in [0, L-1], so the cell is inside the volume; clamped again so that no write can leave it)
    const int cell = (min(max(qz, 0), s.Z - 1) * s.Y + min(max(qy, 0), s.Y - 1)) * s.X + min(max(qx, 0), s.X - 1);
    ptc[j] = cell;
    wave_count(h1, (unsigned long long)(f * s.V + cell));
    M1[f * s.V + cell] = 0ull;  // (the owner map is only looked up at end cells: cleared by whoever ends there)
  }
}

// ---------------------------------------------------------------------------------------------
// 2. seeds: 5x5x5 maxima with > 10 points; growth in 11x11x11 windows
// ---------------------------------------------------------------------------------------------
__global__ void k3_seeds(const int* __restrict__ h1, Dyn3 s, int* __restrict__ seed_list, int* __restrict__ seed_count) {
  const size_t total = (size_t)s.F * s.V;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int h = h1[i];
    if (h <= 10) continue;
    const size_t f = i / s.V;
    const int cell = (int)(i % s.V);
    const int z = cell / (s.Y * s.X), y = (cell / s.X) % s.Y, x = cell % s.X;
    const int* hf = h1 + f * s.V;
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
    if (k < SEEDS_PER_VOL) seed_list[f * SEEDS_PER_VOL + k] = cell;  // (the count goes on: the host reports the overflow)
  }
}

#define W3 11
#define W3N (W3 * W3 * W3)
__global__ __launch_bounds__(256) void k3_grow(const int* __restrict__ h1, Dyn3 s, const int* __restrict__ seed_list,
                                               const int* __restrict__ seed_count, u64* __restrict__ M1, int* __restrict__ cnt,
                                               int* __restrict__ firstpos, int* __restrict__ newid) {
  __shared__ unsigned char ok[W3N], cur[W3N], nxt[W3N];
  const int f = blockIdx.y;
  const int n = min(seed_count[f], SEEDS_PER_VOL);
  const int* hf = h1 + (size_t)f * s.V;
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    const int cell = seed_list[(size_t)f * SEEDS_PER_VOL + k];
    const int z0 = cell / (s.Y * s.X), y0 = (cell / s.X) % s.Y, x0 = cell % s.X;
    if (threadIdx.x == 0) {  // this seed's words (temporary label = cell + 1)
      cnt[(size_t)f * s.V + cell] = 0;
      firstpos[(size_t)f * s.V + cell] = INT_MAX;
      newid[(size_t)f * s.V + cell] = 0;
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
      atomicMax(&M1[(size_t)f * s.V + ((size_t)zz * s.Y + yy) * s.X + xx], prio + 1ull);  // +1: 0 means "no seed"
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// 3. voxel labels (temporary id = owning seed's cell + 1), sizes, first raster positions, first-appearance renumbering
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k3_assign(const int* __restrict__ list, const int* __restrict__ count, const int* __restrict__ ptc,
                                                 const u64* __restrict__ M1, Dyn3 s, unsigned int* __restrict__ labc,
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
      f = i / s.V;
      p = (int)(i % s.V);
      const u64 m = M1[f * s.V + ptc[j]];
      if (m) lab = (unsigned int)((m - 1ull) & 0xFFFFFFFFull) + 1u;
      labc[j] = lab;
    }
    // one atomic pair per run of equal labels inside the wave (dynamics.hip k_assign: a step back in position starts a new run)
    const int lane = threadIdx.x & (WAVE - 1);
    const unsigned long long key = ((unsigned long long)f << 32) | lab;
    const unsigned long long prev = __shfl_up(key, 1, WAVE);
    const int prev_p = __shfl_up(p, 1, WAVE);
    const bool head = lab && (lane == 0 || prev != key || prev_p > p);
    const unsigned long long heads = __ballot(head || !lab) | ~__ballot(1);
    if (head) {
      const unsigned long long after = lane == 63 ? 0ull : (heads >> (lane + 1));
      const int run = after ? __ffsll((long long)after) : 64 - lane;
      atomicAdd(&cnt[f * s.V + lab - 1], run);
      atomicMin(&firstpos[f * s.V + lab - 1], p);
    }
  }
}

// new id of every kept label = 1 + the kept labels of its volume that appear earlier in raster order
__global__ __launch_bounds__(256) void k3_rank_ids(const int* __restrict__ seed_list, const int* __restrict__ seed_count, Dyn3 s,
                                                   const int* __restrict__ cnt, const int* __restrict__ firstpos, double big,
                                                   int* __restrict__ newid, int* __restrict__ ntot) {
  __shared__ int vol_pos[1024];
  __shared__ int red_i[8];
  const int f = blockIdx.x;
  const int n = min(seed_count[f], SEEDS_PER_VOL);
  const int* sl = seed_list + (size_t)f * SEEDS_PER_VOL;
  const size_t base = (size_t)f * s.V;
  int kept_total = 0;
  for (int k0 = 0; k0 < n; k0 += blockDim.x) {
    const int k = k0 + threadIdx.x;
    int mine = INT_MAX, cell = 0;
    bool kept = false;
    if (k < n) {
      cell = sl[k];
      const int c = cnt[base + cell];
      kept = c > 0 && !((double)c > big);
      mine = kept ? firstpos[base + cell] : INT_MAX;
    }
    int before = 0;
    for (int q0 = 0; q0 < n; q0 += 1024) {
      __syncthreads();
      for (int q = threadIdx.x; q < 1024; q += blockDim.x) {
        int v = INT_MAX;
        if (q0 + q < n) {
          const int cq = sl[q0 + q];
          const int c = cnt[base + cq];
          if (c > 0 && !((double)c > big)) v = firstpos[base + cq];
        }
        vol_pos[q] = v;
      }
      __syncthreads();
      const int m = min(1024, n - q0);
      if (kept)
        for (int q = 0; q < m; ++q) before += vol_pos[q] < mine ? 1 : 0;
    }
    if (kept) newid[base + cell] = before + 1;
    kept_total += kept ? 1 : 0;
  }
  kept_total = block_sum_i32(kept_total, red_i);
  if (threadIdx.x == 0) ntot[f] = kept_total;
}

// labels (ids clamped to 65535: a volume with that many is reported as an overflow) and the object table [F, LABELS_PER_VOL]:
// inclusive bounding box and voxel count per label, one set of atomics per wave where all its lanes share a label
__global__ __launch_bounds__(256) void k3_apply_ids(const int* __restrict__ list, const int* __restrict__ count,
                                                    const unsigned int* __restrict__ labc, const int* __restrict__ newid, Dyn3 s,
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
      f = i / s.V;
      const size_t p = i % s.V;
      if (lab) {
        id = newid[f * s.V + lab - 1];
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
// 4. small-mask removal -> final ids; the largest padded box of a kept mask
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k3_final_ids(const Obj3* __restrict__ tab, const int* __restrict__ ntot, int min_size,
                                                     int* __restrict__ newlabel, int* __restrict__ nfinal,
                                                     unsigned long long* __restrict__ max_cells) {
  __shared__ int part[1024];
  const int f = blockIdx.x, t = threadIdx.x;
  const int n = min(ntot[f], LABELS_PER_VOL - 1);
  const Obj3* tf = tab + (size_t)f * LABELS_PER_VOL;
  const int per = (n + 1023) / 1024;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int c = 0;
  unsigned long long big = 0;
  for (int i = lo; i < hi; ++i) {
    const Obj3 o = tf[i];
    const bool keep = o.area > 0 && o.area >= min_size;
    c += keep ? 1 : 0;
    if (keep) {
      const unsigned long long cells = (unsigned long long)(o.z1 - o.z0 + 3) * (o.y1 - o.y0 + 3) * (o.x1 - o.x0 + 3);
      big = cells > big ? cells : big;
    }
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
  for (int i = lo; i < hi; ++i) {
    const Obj3 o = tf[i];
    const bool keep = o.area > 0 && o.area >= min_size;
    newlabel[(size_t)f * LABELS_PER_VOL + i] = keep ? ++run : 0;
  }
  if (t == 1023) nfinal[f] = part[1023];
}

// ---------------------------------------------------------------------------------------------
// 5. hole filling: one workgroup per kept mask, its box with a one-voxel ring (state 0 unknown, 1 mask, 2 reachable from outside),
//    flooded with the 6-neighbourhood until nothing changes; everything not reached is the filled mask
// ---------------------------------------------------------------------------------------------
struct Fill3 {
  const u16* labels;  // first-appearance labels, before small-mask removal
  Dyn3 s;
  const Obj3* tab;
  const int* ntot;
  const int* newlabel;
  size_t cap_cells;
  unsigned char* gscratch;
  u16* out;  // [F,Z,Y,X], zeroed; a 16-bit atomic max resolves nested holes (highest label wins)
};

__device__ __forceinline__ void atomic_max_u16_3d(u16* addr, unsigned v) {
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

template <bool GLOBAL>
__global__ __launch_bounds__(256) void k3_fill(Fill3 a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ int s_changed;
  unsigned char* st = GLOBAL ? (a.gscratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.cap_cells) : lds_raw;
  const int tid = threadIdx.x;
  const int f = blockIdx.y;
  const int n = min(a.ntot[f], LABELS_PER_VOL - 1);
  const Dyn3 s = a.s;
  const u16* lab = a.labels + (size_t)f * s.V;
  u16* out = a.out + (size_t)f * s.V;
  for (int oi = blockIdx.x; oi < n; oi += gridDim.x) {
    const int nl = a.newlabel[(size_t)f * LABELS_PER_VOL + oi];
    if (nl == 0) continue;  // (block-uniform)
    const Obj3 o = a.tab[(size_t)f * LABELS_PER_VOL + oi];
    const int d = o.z1 - o.z0 + 1, h = o.y1 - o.y0 + 1, w = o.x1 - o.x0 + 1;
    const int pd = d + 2, ph = h + 2, pw = w + 2;
    const size_t ncell = (size_t)pd * ph * pw, nin = (size_t)d * h * w;
    if (ncell > a.cap_cells) continue;  // (cannot happen: cap_cells is the largest kept box)
    const u16 L = (u16)(oi + 1);
    __syncthreads();
    for (size_t i = tid; i < ncell; i += blockDim.x) {
      const int c = (int)(i % pw) - 1, r = (int)((i / pw) % ph) - 1, q = (int)(i / ((size_t)pw * ph)) - 1;
      unsigned char v;
      if (q < 0 || q >= d || r < 0 || r >= h || c < 0 || c >= w) v = 2;  // ring: background reachable from outside
      else v = (lab[((size_t)(o.z0 + q) * s.Y + o.y0 + r) * s.X + o.x0 + c] == L) ? 1 : 0;
      st[i] = v;
    }
    __syncthreads();
    for (size_t sweep = 0; sweep < ncell; ++sweep) {
      if (tid == 0) s_changed = 0;
      __syncthreads();
      int ch = 0;
      for (size_t i = tid; i < nin; i += blockDim.x) {
        const int c = (int)(i % w), r = (int)((i / w) % h), q = (int)(i / ((size_t)w * h));
        const size_t k = ((size_t)(q + 1) * ph + r + 1) * pw + c + 1;
        if (st[k] != 0) continue;
        const size_t sl = (size_t)ph * pw;
        if (st[k - 1] == 2 || st[k + 1] == 2 || st[k - pw] == 2 || st[k + pw] == 2 || st[k - sl] == 2 || st[k + sl] == 2) {
          st[k] = 2;
          ch = 1;
        }
      }
      if (ch) s_changed = 1;
      __syncthreads();
      const int any = s_changed;
      __syncthreads();
      if (!any) break;
    }
    for (size_t i = tid; i < nin; i += blockDim.x) {
      const int c = (int)(i % w), r = (int)((i / w) % h), q = (int)(i / ((size_t)w * h));
      const size_t k = ((size_t)(q + 1) * ph + r + 1) * pw + c + 1;
      if (st[k] != 2) atomic_max_u16_3d(&out[((size_t)(o.z0 + q) * s.Y + o.y0 + r) * s.X + o.x0 + c], (unsigned)nl);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------------
static inline size_t align256_3(size_t x) { return (x + 255) & ~(size_t)255; }

#define LDS_FILL_MAX (128 * 1024)
#define GLOBAL_FILL_GROUPS 256

extern "C" {

size_t aliby_masks3d_workspace_bytes(int F, int Z, int Y, int X) {
  const size_t V = (size_t)Z * Y * X * (size_t)(F > 0 ? F : 0);
  size_t b = 0;
  b += align256_3(sizeof(float) * 3 * V);  // im
  b += align256_3(sizeof(int) * V) * 3;    // foreground list, end cells, temporary labels
  b += align256_3(sizeof(int) * V) * 4;    // h1, cnt, firstpos, newid
  b += align256_3(sizeof(u64) * V);        // M1
  b += align256_3(sizeof(u16) * V);        // first-appearance labels
  b += align256_3(sizeof(int) * SEEDS_PER_VOL * (size_t)F);     // seed lists
  b += align256_3(sizeof(Obj3) * LABELS_PER_VOL * (size_t)F);   // object table
  b += align256_3(sizeof(int) * LABELS_PER_VOL * (size_t)F);    // new labels
  b += align256_3(sizeof(int) * (size_t)(4 * F + 8));           // counters
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
  Dyn3 sh;
  sh.F = F; sh.Z = Z; sh.Y = Y; sh.X = X;
  sh.V = (size_t)Z * Y * X;
  ARG_CHECK(sh.V * F < (size_t)INT_MAX, "batch too large for 32-bit voxel indices");
  hipStream_t s = as_stream(stream);

  unsigned char* w = (unsigned char*)workspace;
  auto take = [&](size_t bytes) { unsigned char* p = w; w += align256_3(bytes); return p; };
  const size_t tot = sh.V * F;
  float* im = (float*)take(sizeof(float) * 3 * tot);
  int* fg_list = (int*)take(sizeof(int) * tot);
  int* ptc = (int*)take(sizeof(int) * tot);
  unsigned* labc = (unsigned*)take(sizeof(int) * tot);
  int* h1 = (int*)take(sizeof(int) * tot);
  int* cnt = (int*)take(sizeof(int) * tot);
  int* firstpos = (int*)take(sizeof(int) * tot);
  int* newid = (int*)take(sizeof(int) * tot);
  u64* M1 = (u64*)take(sizeof(u64) * tot);
  u16* labels_tmp = (u16*)take(sizeof(u16) * tot);
  int* seed_list = (int*)take(sizeof(int) * SEEDS_PER_VOL * (size_t)F);
  Obj3* tab = (Obj3*)take(sizeof(Obj3) * LABELS_PER_VOL * (size_t)F);
  int* newlabel = (int*)take(sizeof(int) * LABELS_PER_VOL * (size_t)F);
  int* counters = (int*)take(sizeof(int) * (size_t)(4 * F + 8));
  unsigned long long* max_cells = (unsigned long long*)counters;  // counters[0..1]
  int* fg_count = counters + 2;
  int* ntot = counters + 8;         // [F]
  int* seed_count = ntot + F;       // [F]
  int* nfinal = seed_count + F;     // [F]

  HIP_TRY(hipMemsetAsync(h1, 0, sizeof(int) * tot, s));
  HIP_TRY(hipMemsetAsync(labels_tmp, 0, sizeof(u16) * tot, s));
  HIP_TRY(hipMemsetAsync(labels_out, 0, sizeof(u16) * tot, s));
  HIP_TRY(hipMemsetAsync(counters, 0, sizeof(int) * (size_t)(4 * F + 8), s));
  const int gV = (int)((tot + 255) / 256 > 16384 ? 16384 : (tot + 255) / 256);
  const float cz = 2.0f / (float)(Z - 1), cy = 2.0f / (float)(Y - 1), cx = 2.0f / (float)(X - 1);
  hipLaunchKernelGGL(k3_prep_compact, dim3(gV), dim3(256), 0, s, dP, cellprob, cellprob_threshold, sh, cz, cy, cx, im, fg_list,
                     fg_count);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_follow, dim3(gV), dim3(256), 0, s, im, fg_list, fg_count, sh, niter, ptc, h1, M1, p_final_out);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_seeds, dim3(gV), dim3(256), 0, s, h1, sh, seed_list, seed_count);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_grow, dim3(1024, F), dim3(256), 0, s, h1, sh, seed_list, seed_count, M1, cnt, firstpos, newid);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_assign, dim3(gV), dim3(256), 0, s, fg_list, fg_count, ptc, M1, sh, labc, cnt, firstpos);
  KERNEL_CHECK();
  const double big = (double)sh.V * (double)max_size_fraction;
  hipLaunchKernelGGL(k3_rank_ids, dim3(F), dim3(256), 0, s, seed_list, seed_count, sh, cnt, firstpos, big, newid, ntot);
  KERNEL_CHECK();
  const size_t ntab = (size_t)LABELS_PER_VOL * F;
  hipLaunchKernelGGL(k3_init_table, dim3((int)((ntab + 255) / 256)), dim3(256), 0, s, tab, ntab);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_apply_ids, dim3(gV), dim3(256), 0, s, fg_list, fg_count, labc, newid, sh, labels_tmp, tab);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k3_final_ids, dim3(F), dim3(1024), 0, s, tab, ntot, min_size, newlabel, nfinal, max_cells);
  KERNEL_CHECK();
  // one download: max_cells (2 words), fg count, pad, ntot[F], seed_count[F], nfinal[F]
  int* host = new int[4 * F + 8];
  hipError_t e = hipMemcpyAsync(host, counters, sizeof(int) * (size_t)(4 * F + 8), hipMemcpyDeviceToHost, s);
  if (e != hipSuccess) { delete[] host; HIP_TRY(e); }
  { const int rcw = aliby_wait_stream(s); if (rcw) { delete[] host; return rcw; } }
  unsigned long long cells = 0;
  memcpy(&cells, host, sizeof(cells));
  int max_n = 0;
  for (int f = 0; f < F; ++f) {
    const int nseed = host[8 + F + f], nlab = host[8 + f];
    if (nseed >= SEEDS_PER_VOL - 1 || nlab >= 65535) {
      aliby_set_error("Segmentation produced %d labels (%d seeds) in one volume; uint16 cast unsafe.", nlab, nseed);
      delete[] host;
      return ALIBY_ERR_OVERFLOW;
    }
    max_n = nlab > max_n ? nlab : max_n;
  }
  for (int f = 0; f < F; ++f) n_labels_host[f] = host[8 + 2 * F + f];
  delete[] host;
  if (cells == 0) return ALIBY_OK;  // no mask kept: labels_out is all zero, the counts are 0

  Fill3 fa;
  fa.labels = labels_tmp; fa.s = sh; fa.tab = tab; fa.ntot = ntot; fa.newlabel = newlabel; fa.out = labels_out;
  fa.cap_cells = (size_t)((cells + 15) & ~15ull);
  if (fa.cap_cells <= LDS_FILL_MAX) {
    fa.gscratch = nullptr;
    if (fa.cap_cells > 32 * 1024)
      HIP_TRY(hipFuncSetAttribute((const void*)k3_fill<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fa.cap_cells));
    hipLaunchKernelGGL((k3_fill<false>), dim3(max_n, F), dim3(256), fa.cap_cells, s, fa);
  } else {
    // boxes beyond LDS (a 40 x 100 x 100 box is 400 k voxels): one slab of global scratch per workgroup, grid-strided over masks
    const int g = max_n < GLOBAL_FILL_GROUPS ? max_n : GLOBAL_FILL_GROUPS;
    int rc = aliby_ensure_scratch(ctx, (size_t)g * F * fa.cap_cells);
    if (rc) return rc;
    fa.gscratch = (unsigned char*)ctx->scratch;
    hipLaunchKernelGGL((k3_fill<true>), dim3(g, F), dim3(256), 0, s, fa);
  }
  KERNEL_CHECK();
  { const int rcw = aliby_wait_stream(s); if (rcw) return rcw; }
  return ALIBY_OK;
}

}  // extern "C"
