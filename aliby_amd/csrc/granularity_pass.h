// granularity_pass.h — what the 2-D `granularity` family (feat_granularity.hip) and the volume family (feat_granularity3d.hip)
// share: CellProfiler's MeasureGranularity up to the per-object means, templated on the number of axes.  Everything up to those means
// is a property of the IMAGE, so one call does it once per (frame or stack, channel) and finishes every object with L + 1 mean kernels:
//
//   sample (linear, map_coordinates order 1)  ->  background (erode, dilate with disk / ball(element_size), reflect border, on a further
//   subsample; linear back; subtract; clamp at 0)
//   -> for i in 1..L:  ero = erode(ero, disk / ball(1));  rec = reconstruct(ero under pix)  [Jacobi sweeps to the fixed point];
//                      mean_i(object) = mean over the object's pixels of rec resized to the source (linear);
//                      Granularity_i = (mean_{i-1} - mean_i) * 100 / max(mean_0, eps),  mean_0 on the ORIGINAL pixels.
//
// An image is [F, d, h, w] with d = 1 in 2-D, where no kernel reads the z axis (DIM is a template argument: no run-time switch).  The
// optional image mask (2-D's "objects") is a pointer that may be null: pixels outside it count as 0 in the morphology.  float64
// throughout, no contraction (-ffp-contract=off), and every expression in one fixed order: a stack of one plane gets the 2-D family's
// bits.  The per-object means differ (2-D walks aliby_object rows, 3-D the volume table), so they stay in the two files and the driver
// reaches them through a callable; they share gran_means_write.  The reconstruction reads one change flag per GRANULARITY_CHUNK sweeps,
// so the driver waits on its stream.
#pragma once
#include "common.h"

#define GRANULARITY_CHUNK 16  // Jacobi sweeps between two reads of the change flag

namespace {

struct GranExtent { int d, h, w; };  // (z,) y, x lengths; d = 1 in 2-D

struct GranGeom {
  int F;
  GranExtent src, sub, back;  // the frames or stacks, subsampled, the background grid
};

// elements of F images; a 2-D kernel leaves d (= 1) out of the product
template <int DIM = 3>
__host__ __device__ static inline size_t gran_count(int F, GranExtent e) { return DIM == 3 ? (size_t)F * e.d * e.h * e.w : (size_t)F * e.h * e.w; }

static inline int gran_sampled(int n, double size) { return size < 1 ? (int)ceil(n * size) : n; }  // numpy: mgrid[0 : n * size] has ceil(n * size) points

// The factor of a resize's coordinates, destination length n <- source length m.  Where the destination has length 1 its coordinate is
// 0 (CellProfiler's (m - 1) / (n - 1) is 0 / 0 there): the one deliberate departure, with which a stack of one plane is the 2-D family.
static inline double gran_scale(int m, int n) { return n > 1 ? (double)(m - 1) / (double)(n - 1) : 0.0; }

static inline GranGeom gran_geometry(int F, GranExtent src, double subsample_size, double image_sample_size) {
  GranGeom g;
  g.F = F;
  g.src = src;
  g.sub = GranExtent{gran_sampled(src.d, subsample_size), gran_sampled(src.h, subsample_size), gran_sampled(src.w, subsample_size)};
  g.back = GranExtent{gran_sampled(g.sub.d, image_sample_size), gran_sampled(g.sub.h, image_sample_size), gran_sampled(g.sub.w, image_sample_size)};
  return g;
}

// The head of a workspace: 4 x [ns] doubles (sub -> pix, ero, two reconstruction buffers), 2 x [nb] doubles, the rows' two means and
// the flag.  Each entry adds its own tail behind it.
struct GranBuffers {
  double *bufA, *bufB, *bufC, *bufD, *backA, *backB, *prev, *start;
  int* flag;
  unsigned char* tail;
};

static inline size_t gran_image_bytes(const GranGeom& g, int rows) {
  return 4 * gran_count(g.F, g.sub) * 8 + 2 * gran_count(g.F, g.back) * 8 + 2 * (size_t)rows * 8 + 256;
}

static inline GranBuffers gran_carve(void* workspace, const GranGeom& g, int rows) {
  const size_t ns = gran_count(g.F, g.sub), nb = gran_count(g.F, g.back);
  unsigned char* w = (unsigned char*)workspace;
  GranBuffers b;
  b.bufA = (double*)w;   w += ns * 8;
  b.bufB = (double*)w;   w += ns * 8;
  b.bufC = (double*)w;   w += ns * 8;
  b.bufD = (double*)w;   w += ns * 8;
  b.backA = (double*)w;  w += nb * 8;
  b.backB = (double*)w;  w += nb * 8;
  b.prev = (double*)w;   w += (size_t)rows * 8;
  b.start = (double*)w;  w += (size_t)rows * 8;
  b.flag = (int*)w;      w += 256;
  b.tail = w;
  return b;
}

static inline unsigned gran_grid(size_t n) { return (unsigned)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384); }

#ifdef __HIPCC__

// element i of a [F, d, h, w] array
struct GranIndex { int f, z, y, x; };
template <int DIM>
__device__ __forceinline__ GranIndex gran_index(size_t i, GranExtent e) {
  GranIndex v;
  v.x = (int)(i % e.w);
  size_t r = i / e.w;
  v.y = (int)(r % e.h);
  if constexpr (DIM == 3) {
    r /= e.h;
    v.z = (int)(r % e.d);
    v.f = (int)(r / e.d);
  } else {
    v.z = 0;
    v.f = (int)(i / ((size_t)e.w * e.h));
  }
  return v;
}
__device__ __forceinline__ size_t gran_offset(GranIndex v, GranExtent e) { return ((size_t)v.z * e.h + v.y) * e.w + v.x; }  // inside its own image

// scipy.ndimage.map_coordinates(order=1, mode="constant", cval=0): linear interpolation inside [0, n-1] on every axis, 0 outside.
// load(z, y, x) reads the source.  z is the outermost blend, and DIM = 2 is one plane of it: no z test, four loads at z = 0, no blend.
template <int DIM, typename LoadF>
__device__ __forceinline__ double lerp(LoadF load, GranExtent n, double z, double y, double x) {
  if (!((DIM < 3 || (z >= 0.0 && z <= (double)(n.d - 1))) && y >= 0.0 && y <= (double)(n.h - 1) && x >= 0.0 && x <= (double)(n.w - 1))) return 0.0;
  const int y0 = (int)floor(y), x0 = (int)floor(x);
  const int y1 = min(y0 + 1, n.h - 1), x1 = min(x0 + 1, n.w - 1);
  const double fy = y - (double)y0, fx = x - (double)x0;
  auto plane = [&](int zz) {
    const double a = load(zz, y0, x0), b = load(zz, y0, x1), c = load(zz, y1, x0), d = load(zz, y1, x1);
    return (a * (1.0 - fx) + b * fx) * (1.0 - fy) + (c * (1.0 - fx) + d * fx) * fy;
  };
  if constexpr (DIM < 3) {
    return plane(0);
  } else {
    const int z0 = (int)floor(z), z1 = min(z0 + 1, n.d - 1);
    const double fz = z - (double)z0;
    const double p = plane(z0), q = plane(z1);
    return p * (1.0 - fz) + q * fz;
  }
}

// The sampling kernels take their positions as i / size, as the reference divides: i * (1 / size) can differ in the last place, which
// at the far edge decides between the pixel and 0 (size 0.7 at 61, 121, 241 pixels, ...).
template <int DIM, typename T>
__global__ void k_gran_sample(const T* __restrict__ pixels, int C, int channel, GranGeom g, double size, double* __restrict__ dst) {
  const size_t total = gran_count<DIM>(g.F, g.sub), vol = gran_count<DIM>(1, g.src);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const GranIndex v = gran_index<DIM>(i, g.sub);
    const T* p = pixels + ((size_t)v.f * C + channel) * vol;
    dst[i] = lerp<DIM>([&](int zz, int yy, int xx) { return (double)px_load<T>(p, ((size_t)zz * g.src.h + yy) * g.src.w + xx); }, g.src,
                       (double)v.z / size, (double)v.y / size, (double)v.x / size);
  }
}

// generic [F, from] double -> [F, to] double resample at (i, j, k) / size (order 1)
template <int DIM>
__global__ void k_gran_resample(const double* __restrict__ src, int F, GranExtent from, GranExtent to, double size, double* __restrict__ dst) {
  const size_t total = gran_count<DIM>(F, to);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const GranIndex v = gran_index<DIM>(i, to);
    const double* p = src + (size_t)v.f * gran_count<DIM>(1, from);
    dst[i] = lerp<DIM>([&](int zz, int yy, int xx) { return p[((size_t)zz * from.h + yy) * from.w + xx]; }, from, (double)v.z / size,
                       (double)v.y / size, (double)v.x / size);
  }
}

// ndimage mode="reflect": d c b a | a b c d | d c b a.  The footprint may be many times longer than the axis: fold until inside.
__device__ __forceinline__ int gran_reflect(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - 1 - i;
  return i;
}

// the largest w >= 0 with w * w <= r.  Exact for 0 <= r < 2^24, where (float)r is r and the rounded float sqrt is within one of the
// answer, which the two corrections settle: far beyond the 64^2 that the 2-D entry allows (the 3-D entry allows 16^2).
__device__ __forceinline__ int gran_isqrt(int r) {
  int w = (int)sqrtf((float)r);
  if (w * w > r) --w;
  if ((w + 1) * (w + 1) <= r) ++w;
  return w;
}

// grey erosion (DILATE = false) / dilation restricted to the mask (pixels outside it count as 0, as in `tmp = zeros; tmp[mask] =
// src[mask]`), disk / ball(radius) footprint ((dz^2 +) dy^2 + dx^2 <= radius^2, scanned as spans), reflect border.  min and max are
// exact, so the order of the scan does not matter.
template <int DIM, bool DILATE>
__global__ void k_gran_morph(const double* __restrict__ src, const unsigned char* __restrict__ msk, int F, GranExtent e, int radius,
                             double* __restrict__ dst) {
  const size_t total = gran_count<DIM>(F, e);
  const int r2 = radius * radius, rz_max = DIM == 3 ? radius : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const GranIndex v = gran_index<DIM>(i, e);
    const size_t base = i - gran_offset(v, e);
    double best = DILATE ? -INFINITY : INFINITY;
    for (int dz = -rz_max; dz <= rz_max; ++dz) {
      const size_t zoff = DIM == 3 ? (size_t)gran_reflect(v.z + dz, e.d) * e.h : 0;
      const int rz = r2 - dz * dz;
      const int wy = gran_isqrt(rz);
      for (int dy = -wy; dy <= wy; ++dy) {
        const size_t line = base + (zoff + gran_reflect(v.y + dy, e.h)) * e.w;
        const int wx = gran_isqrt(rz - dy * dy);
        for (int dx = -wx; dx <= wx; ++dx) {
          const size_t j = line + gran_reflect(v.x + dx, e.w);
          const double q = (!msk || msk[j]) ? src[j] : 0.0;
          best = DILATE ? fmax(best, q) : fmin(best, q);
        }
      }
    }
    dst[i] = best;
  }
}

// pix = max(sub - linear(back), 0); ero = pix inside the mask, 0 outside
template <int DIM>
__global__ void k_gran_subtract(const double* __restrict__ sub, const double* __restrict__ back, const unsigned char* __restrict__ msk,
                                GranGeom g, int resized, double cz, double cy, double cx, double* __restrict__ pix, double* __restrict__ ero) {
  const size_t total = gran_count<DIM>(g.F, g.sub);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    double b;
    if (resized) {
      const GranIndex v = gran_index<DIM>(i, g.sub);
      const double* p = back + (size_t)v.f * gran_count<DIM>(1, g.back);
      b = lerp<DIM>([&](int zz, int yy, int xx) { return p[((size_t)zz * g.back.h + yy) * g.back.w + xx]; }, g.back, (double)v.z * cz,
                    (double)v.y * cy, (double)v.x * cx);
    } else {
      b = back[i];
    }
    const double q = fmax(sub[i] - b, 0.0);
    pix[i] = q;
    ero[i] = (!msk || msk[i]) ? q : 0.0;
  }
}

// one Jacobi sweep of the reconstruction by dilation with disk / ball(1) (the centre and its four or six face neighbours), bounded by
// pix; pixels outside the image never contribute
template <int DIM>
__global__ void k_gran_recon_sweep(const double* __restrict__ in, const double* __restrict__ pix, int F, GranExtent e, double* __restrict__ out,
                                   int* __restrict__ changed) {
  const size_t total = gran_count<DIM>(F, e), row = (size_t)e.w, plane = (size_t)e.h * e.w;
  int any = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const GranIndex v = gran_index<DIM>(i, e);
    double m = in[i];
    if constexpr (DIM == 3) {
      if (v.z > 0) m = fmax(m, in[i - plane]);
      if (v.z + 1 < e.d) m = fmax(m, in[i + plane]);
    }
    if (v.y > 0) m = fmax(m, in[i - row]);
    if (v.y + 1 < e.h) m = fmax(m, in[i + row]);
    if (v.x > 0) m = fmax(m, in[i - 1]);
    if (v.x + 1 < e.w) m = fmax(m, in[i + 1]);
    m = fmin(m, pix[i]);
    any |= m != in[i];
    out[i] = m;
  }
  if (__any(any) && (threadIdx.x & 63) == 0) atomicOr(changed, 1);
}

// The end of a means kernel, on lane 0 after wave_sum: s over the n pixels of row (NaN for a row without pixels).  Step 0 writes prev
// and start = max(mean_0, eps); a later step writes its percentage to *out and updates prev.
template <bool STEP0, typename N>
__device__ __forceinline__ void gran_means_write(double s, N n, double* prev, double* start, double* out) {
  const double mean = n > 0 ? s / (double)n : NAN;
  if (STEP0) {
    *prev = mean;
    *start = fmax(mean, 2.220446049250313e-16);
  } else {
    *out = (*prev - mean) * 100.0 / *start;
    *prev = mean;
  }
}

// Stages 1, 2 and 4 of a call, and the means between them: means(0, nullptr) takes the objects' starting means on the original pixels,
// means(step, rec) those of rec [F, sub] into column step - 1.  msk / bmsk: the image mask on the subsampled and the background grid,
// or null.  sweeps_host, where given, receives the sweeps of every step.
template <int DIM, typename Means>
static int gran_run(const GranGeom& g, const void* pixels, int dtype, int C, int channel, double subsample_size, double image_sample_size,
                    int element_size, int spectrum_length, const GranBuffers& b, const unsigned char* msk, const unsigned char* bmsk,
                    int32_t* sweeps_host, const char* who, Means means, hipStream_t s) {
  const size_t ns = gran_count(g.F, g.sub), nb = gran_count(g.F, g.back);
  const dim3 gs(gran_grid(ns)), gb(gran_grid(nb)), block(256);
  // 1. subsample (bufA = sub)
  if (dtype == ALIBY_U16) hipLaunchKernelGGL((k_gran_sample<DIM, uint16_t>), gs, block, 0, s, (const uint16_t*)pixels, C, channel, g, subsample_size, b.bufA);
  else hipLaunchKernelGGL((k_gran_sample<DIM, float>), gs, block, 0, s, (const float*)pixels, C, channel, g, subsample_size, b.bufA);
  // 2. background: subsample again, erode, dilate, resize back, subtract, clamp (bufB = pix, bufC = ero)
  const bool resized = image_sample_size < 1;
  if (resized) hipLaunchKernelGGL((k_gran_resample<DIM>), gb, block, 0, s, b.bufA, g.F, g.sub, g.back, image_sample_size, b.backA);
  const double* back_src = resized ? b.backA : b.bufA;
  double* eroded = resized ? b.backB : b.bufC;
  double* dilated = resized ? b.backA : b.bufD;
  hipLaunchKernelGGL((k_gran_morph<DIM, false>), gb, block, 0, s, back_src, bmsk, g.F, g.back, element_size, eroded);
  hipLaunchKernelGGL((k_gran_morph<DIM, true>), gb, block, 0, s, eroded, bmsk, g.F, g.back, element_size, dilated);
  hipLaunchKernelGGL((k_gran_subtract<DIM>), gs, block, 0, s, b.bufA, dilated, msk, g, resized ? 1 : 0, gran_scale(g.back.d, g.sub.d),
                     gran_scale(g.back.h, g.sub.h), gran_scale(g.back.w, g.sub.w), b.bufB, b.bufC);
  KERNEL_CHECK();
  const double* pix = b.bufB;
  double* ero = b.bufC;
  double* spare[2] = {b.bufA, b.bufD};  // (sub is no longer needed; with image_sample_size == 1 bufD held the dilated image, consumed above)
  // 3. the objects' starting means, on the original pixels
  means(0, nullptr);
  // 4. the spectrum
  // Jacobi sweeps move a value one pixel per sweep along a geodesic path, which in a serpentine mask or corridor can be as long as half
  // the image has pixels: that is the hard cap (reaching it without convergence is reported, never returned as a result).
  const long long max_total = (long long)g.sub.d * g.sub.h * g.sub.w / 2 + 64;
  for (int step = 1; step <= spectrum_length; ++step) {
    double* next = spare[0];
    hipLaunchKernelGGL((k_gran_morph<DIM, false>), gs, block, 0, s, ero, msk, g.F, g.sub, 1, next);
    spare[0] = ero;
    ero = next;
    // reconstruction: rec0 = ero (<= pix), Jacobi sweeps in chunks until a whole chunk changes nothing
    const double* cur = ero;
    double* pp[2] = {spare[0], spare[1]};
    int which = 0, sweeps = 0;
    for (;;) {
      HIP_TRY(hipMemsetAsync(b.flag, 0, sizeof(int), s));
      for (int k = 0; k < GRANULARITY_CHUNK; ++k) {
        hipLaunchKernelGGL((k_gran_recon_sweep<DIM>), gs, block, 0, s, cur, pix, g.F, g.sub, pp[which], b.flag);
        cur = pp[which];
        which ^= 1;
      }
      sweeps += GRANULARITY_CHUNK;
      int changed = 0;
      HIP_TRY(hipMemcpyAsync(&changed, b.flag, sizeof(int), hipMemcpyDeviceToHost, s));
      const int rc = aliby_wait_stream(s);
      if (rc != ALIBY_OK) return rc;
      if (!changed) break;
      if (sweeps >= max_total) {
        if (DIM == 3) aliby_set_error("%s: the reconstruction of spectrum step %d did not converge within %d sweeps on a %d x %d x %d stack", who, step,
                                      sweeps, g.sub.d, g.sub.h, g.sub.w);
        else aliby_set_error("%s: the reconstruction of spectrum step %d did not converge within %d sweeps on a %d x %d image", who, step, sweeps,
                             g.sub.h, g.sub.w);
        return ALIBY_ERR_TOO_LARGE;
      }
    }
    KERNEL_CHECK();
    if (sweeps_host) sweeps_host[step - 1] = sweeps;
    means(step, cur);
  }
  KERNEL_CHECK();
  return ALIBY_OK;  // (the last means kernel is still in flight on `s`: the workspace is released in stream order)
}

#endif  // __HIPCC__

}  // namespace
