// tile_crop.hip — the crop tiler: whole-frame normalisation per channel, then a grid of non-overlapping square tiles.
//
//   CropTiler.get_fczyx (src/aliby/tile/tiler.py:138-189) = clip_outliers (75-88) -> convert_8bit (91-92) -> standard_scale
//   (95-102) -> tile (105-135), each stage optional, every statistic taken per channel over the whole [Z,Y,X] frame.
//
// Three kernels, all stream-ordered, nothing read back in between:
//
//   k_crop_hist   [C,65536] u32 histogram of a uint16 [C, n] stack.  Privatised in LDS as HALF-range u32 tables (32 768 bins =
//                 128 KiB of the CU's 160 KiB) with two workgroup roles: a workgroup of role 0 counts grey levels below 32 768,
//                 one of role 1 those from 32 768 up, and both stream the whole of their slice.  Reading the frame twice costs
//                 ~20 us of HBM time on a 5 x 2160^2 frame; what it buys is plain 32-bit LDS counters that cannot overflow
//                 (n < 2^32 is checked), so there is no flush-before-overflow bookkeeping as packed 16-bit counters would need,
//                 and the only global atomics are one add per non-empty bin and workgroup at the end.  Integer atomics only:
//                 the result does not depend on the launch geometry or on the order of arrival.
//   k_crop_stats  one workgroup per channel -> stats[c] = (pmin, pmax, mean, std) in float64.  Percentiles are NumPy's
//                 method="linear" on the order statistics read off the histogram's prefix sum; mean and population std are
//                 sums over the 65 536 grey levels of h[v] g(v), g = the value a voxel of grey level v has after the clip /
//                 8-bit stages that are on.  Thread t folds levels 64 t .. 64 t + 63 in order, the 1024 partials go through
//                 block_sum_f64 (fixed tree): deterministic.  A statistic whose stage is off is NaN.
//   k_crop_tiles  out[t,c,z,r,q] = g'(stack[c,z, i ts + r, j ts + q]), t = i n_tw + j; g' = g followed by the standard scale
//                 when that is on.  float64 arithmetic in the reference's order (-ffp-contract=off), written as uint16,
//                 float64 or float32 (the float64 value rounded once).  16-byte loads where ts and X are multiples of 8
//                 pixels and both bases are 16-byte aligned, pixel by pixel otherwise; HBM-bound either way.
#include "common.h"

typedef unsigned short u16;

#define CROP_BINS 65536
#define CROP_HALF 32768
#define CROP_HIST_THREADS 1024
#define CROP_HIST_SLICES_MAX 64  // workgroups per (channel, role)
#define CROP_TILE_BLOCKS_MAX 64  // workgroups per (tile, plane), as k_crop_copy

// The value of grey level v after the clip / 8-bit stages that are on (range = pmax - pmin, subtracted once per channel as the
// reference does).  NaN (0 / 0 on a constant channel) passes the clip as np.clip passes it and becomes 0 in the 8-bit cast,
// which is what the reference's astype(np.uint8) gives on x86.  8-bit without clip: NumPy multiplies in the source's integer
// type (wraps), then narrows: (v * 255) mod 256.
__device__ __forceinline__ double crop_pre(unsigned v, int flags, double pmin, double range) {
  if (flags & ALIBY_CROP_CLIP) {
    double x = ((double)v - pmin) / range;
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    if (flags & ALIBY_CROP_8BIT) {
      const double y = x * 255.0;
      return (y == y) ? (double)(int)y : 0.0;  // (y in [0, 255]: the cast truncates)
    }
    return x;
  }
  if (flags & ALIBY_CROP_8BIT) return (double)((v * 255u) & 255u);
  return (double)v;
}

__device__ __forceinline__ double crop_value(unsigned v, int flags, double pmin, double range, double mean, double sd) {
  const double x = crop_pre(v, flags, pmin, range);
  return (flags & ALIBY_CROP_STD) ? (x - mean) / sd : x;
}

// ---------------------------------------------------------------------------------------------
// histogram
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CROP_HIST_THREADS) k_crop_hist(const u16* __restrict__ stack, size_t n, unsigned* __restrict__ hist) {
  extern __shared__ unsigned bins[];  // [CROP_HALF]
  const unsigned role = blockIdx.x & 1u;
  const size_t slice = blockIdx.x >> 1, n_slices = gridDim.x >> 1;
  const int c = blockIdx.y;
  for (int b = threadIdx.x; b < CROP_HALF; b += CROP_HIST_THREADS) bins[b] = 0u;
  __syncthreads();
  const u16* src = stack + (size_t)c * n;
  const size_t first = slice * CROP_HIST_THREADS + threadIdx.x, step = n_slices * CROP_HIST_THREADS;
  if (((size_t)(const void*)src) % 16 == 0) {
    const size_t ng = n / 8;
    for (size_t g = first; g < ng; g += step) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + g * 8);
      const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned a = w[k] & 0xFFFFu, b = w[k] >> 16;
        if ((a >> 15) == role) atomicAdd(&bins[a & (CROP_HALF - 1)], 1u);
        if ((b >> 15) == role) atomicAdd(&bins[b & (CROP_HALF - 1)], 1u);
      }
    }
    const size_t i = ng * 8 + threadIdx.x;  // the last n mod 8 pixels: slice 0's
    if (slice == 0 && threadIdx.x < 8 && i < n) {
      const unsigned a = src[i];
      if ((a >> 15) == role) atomicAdd(&bins[a & (CROP_HALF - 1)], 1u);
    }
  } else {
    for (size_t i = first; i < n; i += step) {
      const unsigned a = src[i];
      if ((a >> 15) == role) atomicAdd(&bins[a & (CROP_HALF - 1)], 1u);
    }
  }
  __syncthreads();
  unsigned* dst = hist + (size_t)c * CROP_BINS + (size_t)role * CROP_HALF;
  for (int b = threadIdx.x; b < CROP_HALF; b += CROP_HIST_THREADS) {
    const unsigned cnt = bins[b];
    if (cnt) atomicAdd(&dst[b], cnt);
  }
}

// ---------------------------------------------------------------------------------------------
// statistics
// ---------------------------------------------------------------------------------------------
#define CROP_STATS_THREADS 1024
#define CROP_PER_THREAD (CROP_BINS / CROP_STATS_THREADS)  // 64 consecutive grey levels per thread

__global__ void __launch_bounds__(CROP_STATS_THREADS) k_crop_stats(const unsigned* __restrict__ hist, unsigned long long n, int flags,
                                                                    double clip, double* __restrict__ stats) {
  __shared__ unsigned long long wave_total[CROP_STATS_THREADS / WAVE];
  __shared__ int ord[4];
  __shared__ double red[CROP_STATS_THREADS / WAVE];
  const int c = blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), wid = t / WAVE;
  const unsigned* h = hist + (size_t)c * CROP_BINS + (size_t)t * CROP_PER_THREAD;
  const uint4* h4 = reinterpret_cast<const uint4*>(h);  // (the thread's 64 counts as 16 groups of four: 256-byte aligned)
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double pmin = nan, pmax = nan, mean = nan, sd = nan;

  if (flags & ALIBY_CROP_CLIP) {
    // exclusive prefix of the per-thread counts: shuffle scan inside the wave, wave totals through LDS
    unsigned long long s = 0;
#pragma unroll 4
    for (int k = 0; k < CROP_PER_THREAD / 4; ++k) {
      const uint4 q = h4[k];
      s += (unsigned long long)q.x + q.y + q.z + q.w;
    }
    unsigned long long incl = s;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const unsigned long long up = __shfl_up(incl, o, WAVE);
      if (lane >= o) incl += up;
    }
    if (lane == WAVE - 1) wave_total[wid] = incl;
    __syncthreads();
    unsigned long long excl = incl - s;
    for (int i = 0; i < wid; ++i) excl += wave_total[i];
    // ranks (0-based) of the four order statistics: pmin's pair, pmax's pair
    unsigned long long rank[4];
    double frac[2];
    if (clip > 0.0) {
      const double q[2] = {clip / 100.0, (100.0 - clip) / 100.0};
      for (int k = 0; k < 2; ++k) {
        const double index = (double)(n - 1) * q[k];
        const double lo = floor(index);
        frac[k] = index - lo;
        unsigned long long r = (unsigned long long)lo;
        if (r > n - 1) r = n - 1;
        rank[2 * k] = r;
        rank[2 * k + 1] = (r + 1 > n - 1) ? n - 1 : r + 1;
      }
    } else {
      rank[0] = rank[1] = 0;
      rank[2] = rank[3] = n - 1;
      frac[0] = frac[1] = 0.0;
    }
    // order statistic of rank r = the grey level v with cum[v - 1] <= r < cum[v]: exactly one thread owns it
    for (int k = 0; k < 4; ++k) {
      if (rank[k] >= excl && rank[k] < excl + s) {
        unsigned long long cum = excl;
        for (int b = 0; b < CROP_PER_THREAD; ++b) {
          cum += h[b];
          if (rank[k] < cum) { ord[k] = t * CROP_PER_THREAD + b; break; }
        }
      }
    }
    __syncthreads();
    double p[2];
    for (int k = 0; k < 2; ++k) {  // numpy's _lerp
      const double a = (double)ord[2 * k], b = (double)ord[2 * k + 1], d = b - a, tt = frac[k];
      p[k] = (tt >= 0.5) ? b - d * (1.0 - tt) : a + d * tt;
    }
    pmin = p[0];
    pmax = p[1];
  }

  if (flags & ALIBY_CROP_STD) {
    const double range = pmax - pmin, dn = (double)n;
    double s1 = 0.0;
    for (int k = 0; k < CROP_PER_THREAD / 4; ++k) {
      const uint4 q = h4[k];
      const unsigned cnt[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (cnt[j]) s1 += (double)cnt[j] * crop_pre((unsigned)(t * CROP_PER_THREAD + 4 * k + j), flags, pmin, range);
    }
    mean = block_sum_f64(s1, red) / dn;
    double s2 = 0.0;
    for (int k = 0; k < CROP_PER_THREAD / 4; ++k) {
      const uint4 q = h4[k];
      const unsigned cnt[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (cnt[j]) {
          const double d = crop_pre((unsigned)(t * CROP_PER_THREAD + 4 * k + j), flags, pmin, range) - mean;
          s2 += (double)cnt[j] * (d * d);
        }
    }
    sd = sqrt(block_sum_f64(s2, red) / dn);
  }
  if (t == 0) {
    double* o = stats + (size_t)c * 4;
    o[0] = pmin; o[1] = pmax; o[2] = mean; o[3] = sd;
  }
}

// ---------------------------------------------------------------------------------------------
// normalise + crop
// ---------------------------------------------------------------------------------------------
struct CropTileArgs {
  const u16* stack;     // [C,Z,Y,X]
  const double* stats;  // [C,4] (device) or nullptr when no statistic is needed
  void* out;            // [T,C,Z,ts,ts]
  int C, Z, Y, X, ts, n_tw, flags;
};

template <typename TO>
__device__ __forceinline__ void crop_store8(TO* dst, const TO (&v)[8]);
template <>
__device__ __forceinline__ void crop_store8<u16>(u16* dst, const u16 (&v)[8]) {
  uint4 q;
  q.x = v[0] | ((unsigned)v[1] << 16); q.y = v[2] | ((unsigned)v[3] << 16);
  q.z = v[4] | ((unsigned)v[5] << 16); q.w = v[6] | ((unsigned)v[7] << 16);
  *reinterpret_cast<uint4*>(dst) = q;
}
template <>
__device__ __forceinline__ void crop_store8<float>(float* dst, const float (&v)[8]) {
  reinterpret_cast<float4*>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
template <>
__device__ __forceinline__ void crop_store8<double>(double* dst, const double (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) reinterpret_cast<double2*>(dst)[k] = make_double2(v[2 * k], v[2 * k + 1]);
}

template <typename TO>
__global__ void k_crop_tiles(CropTileArgs a) {
  const int t = blockIdx.z, cz = blockIdx.y, c = cz / a.Z;
  const int y0 = (t / a.n_tw) * a.ts, x0 = (t % a.n_tw) * a.ts;
  double pmin = 0.0, range = 1.0, mean = 0.0, sd = 1.0;
  if (a.stats) {
    const double* st = a.stats + (size_t)c * 4;
    pmin = st[0]; range = st[1] - st[0]; mean = st[2]; sd = st[3];
  }
  const u16* src = a.stack + (size_t)cz * a.Y * a.X + (size_t)y0 * a.X + x0;  // (every tile lies inside the frame)
  TO* dst = reinterpret_cast<TO*>(a.out) + ((size_t)t * a.C * a.Z + cz) * (size_t)a.ts * a.ts;
  const int n = a.ts * a.ts;
  const bool vec = (a.ts % 8 == 0) && (a.X % 8 == 0) && ((((size_t)(const void*)a.stack) | ((size_t)a.out)) % 16 == 0);
  if (vec) {
    const int ng = n / 8, wg = a.ts / 8;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += gridDim.x * blockDim.x) {
      const int r = g / wg, q = (g - r * wg) * 8;
      const uint4 in = *reinterpret_cast<const uint4*>(src + (size_t)r * a.X + q);
      const unsigned w[4] = {in.x, in.y, in.z, in.w};
      TO v[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = (TO)crop_value(w[k] & 0xFFFFu, a.flags, pmin, range, mean, sd);
        v[2 * k + 1] = (TO)crop_value(w[k] >> 16, a.flags, pmin, range, mean, sd);
      }
      crop_store8<TO>(dst + (size_t)g * 8, v);
    }
    return;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int r = i / a.ts, q = i - r * a.ts;
    dst[i] = (TO)crop_value(src[(size_t)r * a.X + q], a.flags, pmin, range, mean, sd);
  }
}

// uint16 while no float stage is on (raw crop, 8-bit results); anything else is float
static inline bool crop_float_out(int flags) {
  return (flags & ALIBY_CROP_STD) || ((flags & ALIBY_CROP_CLIP) && !(flags & ALIBY_CROP_8BIT));
}

extern "C" {

int aliby_crop_hist_u16(aliby_ctx* ctx, const uint16_t* stack, int C, size_t n, uint32_t* hist, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(C > 0 && C <= 65535 && n > 0, "bad shape");
  ARG_CHECK(n < ((size_t)1 << 32), "Z*Y*X must stay below 2^32 (32-bit bins)");
  ARG_CHECK(stack && hist, "NULL argument");
  hipStream_t s = as_stream(stream);
  HIP_TRY(hipMemsetAsync(hist, 0, sizeof(uint32_t) * (size_t)C * CROP_BINS, s));
  // one 128 KiB workgroup per CU: as many slices as give every CU one workgroup, no more than the frame has work for
  const int lds = CROP_HALF * (int)sizeof(unsigned);
  int slices = ctx->cu_count / (2 * C);
  if (slices > CROP_HIST_SLICES_MAX) slices = CROP_HIST_SLICES_MAX;
  const size_t want = (n + (size_t)CROP_HIST_THREADS * 8 - 1) / ((size_t)CROP_HIST_THREADS * 8);
  if ((size_t)slices > want) slices = (int)want;
  if (slices < 1) slices = 1;
  HIP_TRY(hipFuncSetAttribute((const void*)k_crop_hist, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(k_crop_hist, dim3(2 * slices, C), dim3(CROP_HIST_THREADS), lds, s, stack, n, hist);
  KERNEL_CHECK();
  return ALIBY_OK;
}

int aliby_crop_stats(aliby_ctx* ctx, const uint32_t* hist, int C, size_t n, int flags, double clip, double* stats, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(C > 0 && n > 0 && n < ((size_t)1 << 32), "bad shape");
  ARG_CHECK((flags & ~(ALIBY_CROP_CLIP | ALIBY_CROP_8BIT | ALIBY_CROP_STD)) == 0, "unknown flag");
  ARG_CHECK(clip == clip && clip < 50.0, "clip must be a percentage below 50");
  ARG_CHECK(hist && stats, "NULL argument");
  hipLaunchKernelGGL(k_crop_stats, dim3(C), dim3(CROP_STATS_THREADS), 0, as_stream(stream), hist, (unsigned long long)n, flags, clip,
                     stats);
  KERNEL_CHECK();
  return ALIBY_OK;
}

int aliby_crop_cut_u16(aliby_ctx* ctx, const uint16_t* stack, int C, int Z, int Y, int X, int tile_size, int flags,
                       const double* stats, void* out, int out_dtype, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(C > 0 && Z > 0 && Y > 0 && X > 0 && tile_size > 0, "bad shape");
  ARG_CHECK((flags & ~(ALIBY_CROP_CLIP | ALIBY_CROP_8BIT | ALIBY_CROP_STD)) == 0, "unknown flag");
  ARG_CHECK(crop_float_out(flags) ? (out_dtype == ALIBY_F64 || out_dtype == ALIBY_F32) : out_dtype == ALIBY_U16,
            "out_dtype: uint16 while no float stage is on, float64 or float32 otherwise");
  if (tile_size > Y || tile_size > X) return ALIBY_OK;  // no tile fits: nothing to write
  const int n_th = (Y - tile_size) / tile_size + 1, n_tw = (X - tile_size) / tile_size + 1;
  ARG_CHECK((size_t)C * Z <= 65535 && (size_t)n_th * n_tw <= 65535, "grid dimension overflow");
  ARG_CHECK(tile_size <= 32768, "tile too large");
  ARG_CHECK(stack && out, "NULL argument");
  ARG_CHECK(stats || !(flags & (ALIBY_CROP_CLIP | ALIBY_CROP_STD)), "clip / standard scale need the channel statistics");
  CropTileArgs a;
  a.stack = stack; a.stats = (flags & (ALIBY_CROP_CLIP | ALIBY_CROP_STD)) ? stats : nullptr; a.out = out;
  a.C = C; a.Z = Z; a.Y = Y; a.X = X; a.ts = tile_size; a.n_tw = n_tw; a.flags = flags;
  const long long work = (long long)tile_size * tile_size;
  long long bx = (work + 255) / 256;
  if (bx > CROP_TILE_BLOCKS_MAX) bx = CROP_TILE_BLOCKS_MAX;
  const dim3 g((unsigned)bx, C * Z, n_th * n_tw), b(256);
  hipStream_t s = as_stream(stream);
  if (out_dtype == ALIBY_U16) hipLaunchKernelGGL(k_crop_tiles<u16>, g, b, 0, s, a);
  else if (out_dtype == ALIBY_F32) hipLaunchKernelGGL(k_crop_tiles<float>, g, b, 0, s, a);
  else hipLaunchKernelGGL(k_crop_tiles<double>, g, b, 0, s, a);
  KERNEL_CHECK();
  return ALIBY_OK;
}

int aliby_crop_tiles_u16(aliby_ctx* ctx, const uint16_t* stack, int C, int Z, int Y, int X, int tile_size, int flags, double clip,
                         void* out, int out_dtype, double* stats_out, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(C > 0 && Z > 0 && Y > 0 && X > 0 && tile_size > 0, "bad shape");
  if (tile_size > Y || tile_size > X) return ALIBY_OK;
  const bool need_stats = (flags & (ALIBY_CROP_CLIP | ALIBY_CROP_STD)) != 0;
  double* stats = stats_out;
  if (need_stats) {
    const size_t n = (size_t)Z * Y * X;
    const size_t hist_bytes = sizeof(uint32_t) * (size_t)C * CROP_BINS;
    int rc = aliby_ensure_scratch(ctx, hist_bytes + sizeof(double) * 4 * (size_t)C);
    if (rc) return rc;
    uint32_t* hist = (uint32_t*)ctx->scratch;
    if (!stats) stats = (double*)((char*)ctx->scratch + hist_bytes);
    rc = aliby_crop_hist_u16(ctx, stack, C, n, hist, stream);
    if (rc) return rc;
    rc = aliby_crop_stats(ctx, hist, C, n, flags, clip, stats, stream);
    if (rc) return rc;
  }
  const int rc = aliby_crop_cut_u16(ctx, stack, C, Z, Y, X, tile_size, flags, stats, out, out_dtype, stream);
  if (rc) return rc;
  // histogram and statistics live in ctx scratch: they are consumed before another call of this context may reuse it
  if (need_stats) return aliby_wait_stream(as_stream(stream));
  return ALIBY_OK;
}

}  // extern "C"
