// feat_granularity3d.hip — "granularity3d": the granular spectrum of feat_granularity.hip (CellProfiler MeasureGranularity) on
// labelled stacks [F, Z, Y, X], CellProfiler's volumetric branch recalled (PARITY UNPINNED; restated in tests/granularity3d_ref.py,
// defined in include/aliby_hip.h).  The structure is the 2-D file's, one dimension up; every stack is on its own:
//
//   sample (trilinear, map_coordinates order 1)  ->  background (erode, dilate with ball(element_size), reflect border, on a further
//   subsample; trilinear back; subtract; clamp at 0)
//   -> for i in 1..L:  ero = erode(ero, ball(1));  rec = reconstruct(ero under pix)  [Jacobi sweeps to the fixed point];
//                      mean_i(object) = mean over the object's voxels of rec resized to the stack (trilinear);
//                      Granularity_i = (mean_{i-1} - mean_i) * 100 / max(mean_0, eps),  mean_0 on the ORIGINAL pixels.
//
// The image mask is the whole stack (CellProfiler's default); the "objects" mask of the 2-D family is not built.  Where an axis of a
// resize's destination has length 1 its coordinate is 0 (CellProfiler's (m - 1) / (n - 1) is 0 / 0 there): the one deliberate
// departure, with which a stack of one plane is the 2-D family.  float64 throughout, no contraction (-ffp-contract=off).
//
// The per-object means take their bounding boxes from the shared volume table (volume_table.h), built in the caller's workspace:
// one wave per (stack, label) row, the lanes stride the box in raster order, fixed reduction order — a row carries the same bits
// whatever the run, the other stacks of the call and the batch.  The reconstruction reads one change flag per 16 sweeps, so the
// entry waits on its stream: a main-stream call.
#include "common.h"
#include "volume_table.h"

typedef unsigned short u16;

#define GRANULARITY3D_MAX_ELEMENT 16  // bounds the per-voxel scan of the ball (about 17 k offsets at 16); not a structural limit
#define GRANULARITY3D_MAX_LENGTH 64
#define G3_CHUNK 16                   // Jacobi sweeps between two reads of the change flag

namespace {

struct Gran3Geom {
  int F, Z, Y, X;   // stack
  int sz, sh, sw;   // subsampled
  int bz, bh, bw;   // background grid
};

// scipy.ndimage.map_coordinates(order=1, mode="constant", cval=0): linear interpolation inside [0, n-1] on every axis, 0 outside.
// z is the outermost blend: with a z fraction of 0 the result is the 2-D file's `bilinear` on plane z0 (p * 1 + q * 0 = p).
template <typename LoadF>
__device__ __forceinline__ double trilinear(LoadF load, int n0, int n1, int n2, double z, double y, double x) {
  if (!(z >= 0.0 && z <= (double)(n0 - 1) && y >= 0.0 && y <= (double)(n1 - 1) && x >= 0.0 && x <= (double)(n2 - 1))) return 0.0;
  const int z0 = (int)floor(z), y0 = (int)floor(y), x0 = (int)floor(x);
  const int z1 = min(z0 + 1, n0 - 1), y1 = min(y0 + 1, n1 - 1), x1 = min(x0 + 1, n2 - 1);
  const double fz = z - (double)z0, fy = y - (double)y0, fx = x - (double)x0;
  double p[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int zz = k ? z1 : z0;
    const double a = load(zz, y0, x0), b = load(zz, y0, x1), c = load(zz, y1, x0), d = load(zz, y1, x1);
    p[k] = (a * (1.0 - fx) + b * fx) * (1.0 - fy) + (c * (1.0 - fx) + d * fx) * fy;
  }
  return p[0] * (1.0 - fz) + p[1] * fz;
}

// element i of a [F, d, h, w] array
struct Voxel { int f, z, y, x; };
__device__ __forceinline__ Voxel voxel_of(size_t i, int d, int h, int w) {
  Voxel v;
  v.x = (int)(i % w);
  size_t r = i / w;
  v.y = (int)(r % h);
  r /= h;
  v.z = (int)(r % d);
  v.f = (int)(r / d);
  return v;
}

// The two sampling kernels take their positions as i / size, as the reference divides: i * (1 / size) can differ in the last place,
// which at the far edge decides between the voxel and 0 (size 0.7 at 61, 121 voxels, ...; the comment in feat_granularity.hip).
template <typename T>
__global__ void k_g3_sample_stack(const T* __restrict__ pixels, int C, int channel, Gran3Geom g, double size, double* __restrict__ dst) {
  const size_t total = (size_t)g.F * g.sz * g.sh * g.sw, vol = (size_t)g.Z * g.Y * g.X;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const Voxel v = voxel_of(i, g.sz, g.sh, g.sw);
    const T* p = pixels + ((size_t)v.f * C + channel) * vol;
    dst[i] = trilinear([&](int zz, int yy, int xx) { return (double)px_load<T>(p, ((size_t)zz * g.Y + yy) * g.X + xx); }, g.Z, g.Y, g.X,
                       (double)v.z / size, (double)v.y / size, (double)v.x / size);
  }
}

// generic [F,d,h,w] double -> [F,d2,h2,w2] double resample at (i, j, k) / size (order 1)
__global__ void k_g3_resample(const double* __restrict__ src, int F, int d, int h, int w, int d2, int h2, int w2, double size,
                              double* __restrict__ dst) {
  const size_t total = (size_t)F * d2 * h2 * w2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const Voxel v = voxel_of(i, d2, h2, w2);
    const double* p = src + (size_t)v.f * d * h * w;
    dst[i] = trilinear([&](int zz, int yy, int xx) { return p[((size_t)zz * h + yy) * w + xx]; }, d, h, w, (double)v.z / size,
                       (double)v.y / size, (double)v.x / size);
  }
}

// ndimage mode="reflect": d c b a | a b c d | d c b a.  The footprint may be many times longer than the axis: fold until inside.
__device__ __forceinline__ int reflect(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
  return i;
}

// the largest w >= 0 with w * w <= r, for 0 <= r <= 16^2 (exact: float sqrt is within one of it)
__device__ __forceinline__ int g3_isqrt(int r) {
  int w = (int)sqrtf((float)r);
  if (w * w > r) --w;
  if ((w + 1) * (w + 1) <= r) ++w;
  return w;
}

// grey erosion (DILATE = false) / dilation, ball(radius) footprint (dz^2 + dy^2 + dx^2 <= radius^2), reflect border.  min and max
// are exact, so the order of the scan does not matter.
template <bool DILATE>
__global__ void k_g3_morph(const double* __restrict__ src, int F, int d, int h, int w, int radius, double* __restrict__ dst) {
  const size_t total = (size_t)F * d * h * w;
  const int r2 = radius * radius;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const Voxel v = voxel_of(i, d, h, w);
    const double* p = src + (size_t)v.f * d * h * w;
    double best = DILATE ? -INFINITY : INFINITY;
    for (int dz = -radius; dz <= radius; ++dz) {
      const size_t zoff = (size_t)reflect(v.z + dz, d) * h;
      const int rz = r2 - dz * dz;
      const int wy = g3_isqrt(rz);
      for (int dy = -wy; dy <= wy; ++dy) {
        const double* line = p + (zoff + reflect(v.y + dy, h)) * w;
        const int wx = g3_isqrt(rz - dy * dy);
        for (int dx = -wx; dx <= wx; ++dx) {
          const double q = line[reflect(v.x + dx, w)];
          best = DILATE ? fmax(best, q) : fmin(best, q);
        }
      }
    }
    dst[i] = best;
  }
}

// pix = ero = max(sub - trilinear(back), 0)
__global__ void k_g3_subtract(const double* __restrict__ sub, const double* __restrict__ back, Gran3Geom g, int resized, double cz, double cy,
                              double cx, double* __restrict__ pix, double* __restrict__ ero) {
  const size_t total = (size_t)g.F * g.sz * g.sh * g.sw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    double b;
    if (resized) {
      const Voxel v = voxel_of(i, g.sz, g.sh, g.sw);
      const double* p = back + (size_t)v.f * g.bz * g.bh * g.bw;
      b = trilinear([&](int zz, int yy, int xx) { return p[((size_t)zz * g.bh + yy) * g.bw + xx]; }, g.bz, g.bh, g.bw, (double)v.z * cz,
                    (double)v.y * cy, (double)v.x * cx);
    } else {
      b = back[i];
    }
    const double q = fmax(sub[i] - b, 0.0);
    pix[i] = q;
    ero[i] = q;
  }
}

// one Jacobi sweep of the reconstruction by dilation with ball(1) (the centre and the six face neighbours), bounded by pix; voxels
// outside the stack never contribute
__global__ void k_g3_recon_sweep(const double* __restrict__ in, const double* __restrict__ pix, int F, int d, int h, int w,
                                 double* __restrict__ out, int* __restrict__ changed) {
  const size_t total = (size_t)F * d * h * w, row = (size_t)w, plane = (size_t)h * w;
  int any = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const Voxel v = voxel_of(i, d, h, w);
    double m = in[i];
    if (v.z > 0) m = fmax(m, in[i - plane]);
    if (v.z + 1 < d) m = fmax(m, in[i + plane]);
    if (v.y > 0) m = fmax(m, in[i - row]);
    if (v.y + 1 < h) m = fmax(m, in[i + row]);
    if (v.x > 0) m = fmax(m, in[i - 1]);
    if (v.x + 1 < w) m = fmax(m, in[i + 1]);
    m = fmin(m, pix[i]);
    any |= m != in[i];
    out[i] = m;
  }
  if (__any(any) && (threadIdx.x & 63) == 0) atomicOr(changed, 1);
}

struct Gran3MeanArgs {
  VolumeArgs v;        // labels, shape, offsets and the table (n_items = rows)
  Gran3Geom g;
  const void* pixels;  // STEP0: the original pixels (typed)
  int C, channel;
  const double* rec;   // STEP > 0: [F, sz, sh, sw]
  double cz, cy, cx;   // stack -> subsampled coordinates ((sz - 1) / (Z - 1), ...; 0 on an axis of length 1)
  double* prev;        // [rows] mean of the previous step (updated)
  double* start;       // [rows] max(mean_0, eps) (written by step 0)
  double* out;         // feature matrix
  int ld, col;         // column of this step
};

// one wave per row: mean over the object's voxels of the (resized) image; the lanes stride the bounding box in raster order, fixed
// reduction order.  A row without voxels gets NaN.
template <typename T, bool STEP0>
__global__ __launch_bounds__(64) void k_g3_means(Gran3MeanArgs a) {
  const int lane = threadIdx.x;
  const int Y = a.v.Y, X = a.v.X;
  const size_t vol = (size_t)a.v.Z * Y * X;
  for (int row = blockIdx.x; row < a.v.n_items; row += gridDim.x) {
    const unsigned count = a.v.count[row];
    double s = 0.0;
    if (count > 0) {
      const int f = volume_stack_of(a.v.offsets, a.v.F, row);
      const u16 L = (u16)(row - a.v.offsets[f] + 1);
      const u16* lab = a.v.labels + (size_t)f * vol;
      const VolumeBox box = volume_box(a.v.bmin, a.v.bmax, row);
      const T* px = STEP0 ? reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + a.channel) * vol : nullptr;
      const double* rec = STEP0 ? nullptr : a.rec + (size_t)f * a.g.sz * a.g.sh * a.g.sw;
      for (unsigned i = lane; i < box.nbox; i += 64) {
        const unsigned r = i / box.w;
        const int xx = (int)(box.x0 + i % box.w), yy = (int)(box.y0 + r % box.h), zz = (int)(box.z0 + r / box.h);
        const size_t idx = ((size_t)zz * Y + yy) * X + xx;
        if (lab[idx] != L) continue;
        if (STEP0) s += (double)px_load<T>(px, idx);
        else s += trilinear([&](int z2, int y2, int x2) { return rec[((size_t)z2 * a.g.sh + y2) * a.g.sw + x2]; }, a.g.sz, a.g.sh, a.g.sw,
                            (double)zz * a.cz, (double)yy * a.cy, (double)xx * a.cx);
      }
    }
    s = wave_sum(s);
    if (lane == 0) {
      const double mean = count > 0 ? s / (double)count : NAN;
      if (STEP0) {
        a.prev[row] = mean;
        a.start[row] = fmax(mean, 2.220446049250313e-16);
      } else {
        a.out[(size_t)row * a.ld + a.col] = (a.prev[row] - mean) * 100.0 / a.start[row];
        a.prev[row] = mean;
      }
    }
  }
}

inline unsigned g3_grid(size_t n) { return (unsigned)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384); }

inline int g3_sampled(int n, double size) { return size < 1 ? (int)ceil(n * size) : n; }  // numpy: mgrid[0 : n * size] has ceil(n * size) points

// the factor of a resize's coordinates, destination length n <- source length m
inline double g3_scale(int m, int n) { return n > 1 ? (double)(m - 1) / (double)(n - 1) : 0.0; }

void g3_geometry(int F, int Z, int Y, int X, double subsample_size, double image_sample_size, Gran3Geom* g) {
  g->F = F; g->Z = Z; g->Y = Y; g->X = X;
  g->sz = g3_sampled(Z, subsample_size); g->sh = g3_sampled(Y, subsample_size); g->sw = g3_sampled(X, subsample_size);
  g->bz = g3_sampled(g->sz, image_sample_size); g->bh = g3_sampled(g->sh, image_sample_size); g->bw = g3_sampled(g->sw, image_sample_size);
}

// 4 x [ns] doubles (sub -> pix, ero, two reconstruction buffers), 2 x [nb] doubles, the rows' two means, the flag, then the
// object table (7 words a row) and the offsets
size_t g3_bytes(const Gran3Geom& g, int rows) {
  const size_t ns = (size_t)g.F * g.sz * g.sh * g.sw, nb = (size_t)g.F * g.bz * g.bh * g.bw;
  return 4 * ns * 8 + 2 * nb * 8 + 2 * (size_t)rows * 8 + 256 + ((size_t)rows * 7 + (size_t)g.F + 1) * 4;
}

bool g3_sizes_ok(double subsample_size, double image_sample_size) {
  return subsample_size > 0 && subsample_size <= 1 && image_sample_size > 0 && image_sample_size <= 1;
}

}  // namespace

extern "C" size_t aliby_granularity3d_workspace_bytes(int F, int Z, int Y, int X, int rows, double subsample_size, double image_sample_size) {
  if (F <= 0 || Z <= 0 || Y <= 0 || X <= 0 || rows < 0 || !g3_sizes_ok(subsample_size, image_sample_size)) return 0;
  Gran3Geom g;
  g3_geometry(F, Z, Y, X, subsample_size, image_sample_size, &g);
  return g3_bytes(g, rows);
}

extern "C" int aliby_features_granularity3d(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y,
                                            int X, int channel, const int32_t* offsets_host, double subsample_size, double image_sample_size,
                                            int element_size, int spectrum_length, void* workspace, size_t workspace_bytes,
                                            int32_t* sweeps_host, double* out, int ld, int col0, void* stream_) {
  ARG_CHECK(ctx && labels && pixels && offsets_host && out, "granularity3d: null argument");
  if (!volume_shape_ok("granularity3d", F, Z, Y, X, offsets_host, 1ull << 30)) return ALIBY_ERR_INVALID;
  ARG_CHECK(Y > 1 && X > 1, "granularity3d: Y and X must be above 1");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "granularity3d: dtype must be ALIBY_U16 or ALIBY_F32");
  ARG_CHECK(channel >= 0 && channel < C, "granularity3d: channel out of range");
  ARG_CHECK(g3_sizes_ok(subsample_size, image_sample_size), "granularity3d: sample sizes must be in (0, 1]");
  ARG_CHECK(element_size >= 1 && element_size <= GRANULARITY3D_MAX_ELEMENT, "granularity3d: element_size must lie in 1..16");
  ARG_CHECK(spectrum_length >= 1 && spectrum_length <= GRANULARITY3D_MAX_LENGTH, "granularity3d: spectrum length must lie in 1..64");
  ARG_CHECK(col0 >= 0 && (long long)col0 + spectrum_length <= ld, "granularity3d: columns exceed row stride");
  Gran3Geom g;
  g3_geometry(F, Z, Y, X, subsample_size, image_sample_size, &g);
  ARG_CHECK(g.sh > 1 && g.sw > 1 && g.bh > 1 && g.bw > 1, "granularity3d: stack too small for these sample sizes");
  const int rows = offsets_host[F];
  if (sweeps_host) for (int k = 0; k < spectrum_length; ++k) sweeps_host[k] = 0;
  if (rows <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream_);
  const size_t ns = (size_t)F * g.sz * g.sh * g.sw, nb = (size_t)F * g.bz * g.bh * g.bw;
  ARG_CHECK(workspace != nullptr && workspace_bytes >= g3_bytes(g, rows), "workspace smaller than aliby_granularity3d_workspace_bytes()");
  ARG_CHECK(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  unsigned char* w = (unsigned char*)workspace;
  double* bufA = (double*)w;           w += ns * 8;
  double* bufB = (double*)w;           w += ns * 8;
  double* bufC = (double*)w;           w += ns * 8;
  double* bufD = (double*)w;           w += ns * 8;
  double* backA = (double*)w;          w += nb * 8;
  double* backB = (double*)w;          w += nb * 8;
  double* prev = (double*)w;           w += (size_t)rows * 8;
  double* start = (double*)w;          w += (size_t)rows * 8;
  int* flag = (int*)w;                 w += 256;
  unsigned* table = (unsigned*)w;      w += (size_t)rows * 7 * 4;
  int* offsets_dev = (int*)w;

  // 0. the object table: voxel count and bounding box of every row
  HIP_TRY(hipMemcpyAsync(offsets_dev, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
  int rc = volume_table_launch(labels, F, Z, Y, X, offsets_dev, rows, table, s);
  if (rc) return rc;
  // 1. subsample (bufA = sub)
  if (dtype == ALIBY_U16) hipLaunchKernelGGL((k_g3_sample_stack<u16>), dim3(g3_grid(ns)), dim3(256), 0, s, (const u16*)pixels, C, channel, g, subsample_size, bufA);
  else hipLaunchKernelGGL((k_g3_sample_stack<float>), dim3(g3_grid(ns)), dim3(256), 0, s, (const float*)pixels, C, channel, g, subsample_size, bufA);
  // 2. background: subsample again, erode, dilate, resize back, subtract, clamp (bufB = pix, bufC = ero)
  const bool resized = image_sample_size < 1;
  const double* back_src = bufA;
  if (resized) {
    hipLaunchKernelGGL(k_g3_resample, dim3(g3_grid(nb)), dim3(256), 0, s, bufA, F, g.sz, g.sh, g.sw, g.bz, g.bh, g.bw, image_sample_size, backA);
    back_src = backA;
  }
  double* eroded = resized ? backB : bufC;
  double* dilated = resized ? backA : bufD;
  hipLaunchKernelGGL((k_g3_morph<false>), dim3(g3_grid(nb)), dim3(256), 0, s, back_src, F, g.bz, g.bh, g.bw, element_size, eroded);
  hipLaunchKernelGGL((k_g3_morph<true>), dim3(g3_grid(nb)), dim3(256), 0, s, eroded, F, g.bz, g.bh, g.bw, element_size, dilated);
  hipLaunchKernelGGL(k_g3_subtract, dim3(g3_grid(ns)), dim3(256), 0, s, bufA, dilated, g, resized ? 1 : 0, g3_scale(g.bz, g.sz), g3_scale(g.bh, g.sh),
                     g3_scale(g.bw, g.sw), bufB, bufC);
  KERNEL_CHECK();
  double* pix = bufB;
  double* ero = bufC;
  double* spare[2] = {bufA, bufD};  // (sub is no longer needed; with image_sample_size == 1 bufD held the dilated image, consumed above)
  // 3. the objects' starting means, on the original pixels
  Gran3MeanArgs m;
  m.v = VolumeArgs{labels, F, Z, Y, X, offsets_dev, table, table + rows, table + (size_t)rows * 4, nullptr, rows};
  m.g = g; m.pixels = pixels; m.C = C; m.channel = channel; m.rec = nullptr;
  m.cz = g3_scale(g.sz, Z); m.cy = g3_scale(g.sh, Y); m.cx = g3_scale(g.sw, X);
  m.prev = prev; m.start = start; m.out = out; m.ld = ld; m.col = col0;
  const unsigned og = (unsigned)(rows < 65535 ? rows : 65535);
  if (dtype == ALIBY_U16) hipLaunchKernelGGL((k_g3_means<u16, true>), dim3(og), dim3(64), 0, s, m);
  else hipLaunchKernelGGL((k_g3_means<float, true>), dim3(og), dim3(64), 0, s, m);
  // 4. the spectrum
  // Jacobi sweeps move a value one voxel per sweep along a geodesic path, which in a serpentine corridor can be as long as half the
  // stack has voxels: that is the hard cap (reaching it without convergence is reported, never returned as a result).
  const long long max_total = (long long)g.sz * g.sh * g.sw / 2 + 64;
  for (int step = 1; step <= spectrum_length; ++step) {
    double* next = spare[0];
    hipLaunchKernelGGL((k_g3_morph<false>), dim3(g3_grid(ns)), dim3(256), 0, s, ero, F, g.sz, g.sh, g.sw, 1, next);
    spare[0] = ero;
    ero = next;
    // reconstruction: rec0 = ero (<= pix), Jacobi sweeps in chunks of 16 until a whole chunk changes nothing
    const double* cur = ero;
    double* pp[2] = {spare[0], spare[1]};
    int which = 0, sweeps = 0;
    for (;;) {
      HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), s));
      for (int k = 0; k < G3_CHUNK; ++k) {
        hipLaunchKernelGGL(k_g3_recon_sweep, dim3(g3_grid(ns)), dim3(256), 0, s, cur, pix, F, g.sz, g.sh, g.sw, pp[which], flag);
        cur = pp[which];
        which ^= 1;
      }
      sweeps += G3_CHUNK;
      int changed = 0;
      HIP_TRY(hipMemcpyAsync(&changed, flag, sizeof(int), hipMemcpyDeviceToHost, s));
      rc = aliby_wait_stream(s);
      if (rc != ALIBY_OK) return rc;
      if (!changed) break;
      if (sweeps >= max_total) {
        aliby_set_error("granularity3d: the reconstruction of spectrum step %d did not converge within %d sweeps on a %d x %d x %d stack", step,
                        sweeps, g.sz, g.sh, g.sw);
        return ALIBY_ERR_TOO_LARGE;
      }
    }
    KERNEL_CHECK();
    if (sweeps_host) sweeps_host[step - 1] = sweeps;
    m.rec = cur;
    m.col = col0 + step - 1;
    hipLaunchKernelGGL((k_g3_means<u16, false>), dim3(og), dim3(64), 0, s, m);  // (T is unused when STEP0 is false)
  }
  KERNEL_CHECK();
  return ALIBY_OK;  // (the last means kernel is still in flight on `stream`: the workspace is released in stream order, as in 2-D)
}
