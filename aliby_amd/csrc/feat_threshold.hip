// feat_threshold.hip — the automatic threshold of a `propagate` call: Otsu's threshold of every tile of a uint16 [F,Y,X] block, with
// two or three classes, CellProfiler's correction factor and bounds, left on the device for k_propagate_weights to read (definition
// and worked examples: include/aliby_hip.h; tests/threshold_ref.py restates it as a Python loop and in NumPy).
//
// Launches (the workspace is the caller's: the [F,65536] u32 histogram):
// aliby_crop_hist_u16   the tiler's LDS-privatised integer histogram (csrc/tile_crop.hip) with C = F, n = Y X.
// k_threshold_search    one workgroup of 1024 threads per tile, laid out as k_crop_stats: thread t owns the grey levels 64 t .. 64 t + 63.
//                       The exclusive prefixes of the counts and of v h[v] (u64, exact) come from a shuffle scan inside the wave and
//                       the wave totals through LDS; lo and hi from two block reductions.
//                       Two classes: a thread walks its occupied levels v in order; t = v + 1 is a candidate while v < hi, with
//                       J(t) = s0 s0 / n0 + s1 s1 / n1 in float64, one rounding per operation (the library is built with
//                       -ffp-contract=off).  A t behind an empty level has the J of t - 1, bit for bit, and loses the tie to it: only
//                       occupied levels are evaluated.  A thread keeps its first maximum; the workgroup reduces by "larger J, then
//                       smaller t", which is associative and commutative: any tree gives the same bits.
//                       Three classes: the thread folds its levels into 256 bins over lo..hi in LDS (u64 counts and sums, integer
//                       atomics, one per run of levels of one bin), 256 threads take the inclusive prefix of a bin each, and the
//                       254 x 255 (k1, k2) cells, of which the 32 385 with k1 < k2 are pairs, are strided over the threads; the key
//                       k1 * 255 + k2 orders ties as the definition does.  No valid pair: the two-class threshold.
//                       Thread 0 applies the correction and the bounds and writes thresholds[f] and, if asked, details[f][4].
// Integers and correctly rounded float64 only: the same bits whatever the batch and the stream.  Nothing is read back.
#include "common.h"

typedef unsigned long long u64;

#define THRESHOLD_LEVELS 65536
#define THRESHOLD_THREADS 1024
#define THRESHOLD_PER (THRESHOLD_LEVELS / THRESHOLD_THREADS)  // 64 consecutive grey levels per thread
#define THRESHOLD_WAVES (THRESHOLD_THREADS / WAVE)
#define THRESHOLD_BINS 256
#define THRESHOLD_NONE INT_MAX

__device__ __forceinline__ bool threshold_better(double j, int key, double best_j, int best_key) {
  return j > best_j || (j == best_j && key < best_key);
}

// The workgroup's best (J, key) by "larger J, then smaller key", in every thread.  `red_j`, `red_key`: LDS, one slot per wave.
__device__ __forceinline__ void threshold_reduce(double& j, int& key, double* red_j, int* red_key) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const double oj = __shfl_xor(j, o, WAVE);
    const int ok = __shfl_xor(key, o, WAVE);
    if (threshold_better(oj, ok, j, key)) { j = oj; key = ok; }
  }
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  __syncthreads();  // (the slots may still be read from a reduction before this one)
  if (lane == 0) { red_j[wid] = j; red_key[wid] = key; }
  __syncthreads();
  j = red_j[0]; key = red_key[0];
  for (int i = 1; i < THRESHOLD_WAVES; ++i) {
    const double oj = red_j[i];
    const int ok = red_key[i];
    if (threshold_better(oj, ok, j, key)) { j = oj; key = ok; }
  }
}

__device__ __forceinline__ double threshold_term(u64 s, u64 n) {
  const double ds = (double)s;  // (exact: s < 2^48)
  return ds * ds / (double)n;
}

// grid = F
__global__ void __launch_bounds__(THRESHOLD_THREADS) k_threshold_search(const unsigned* __restrict__ hist, int classes, int middle,
                                                                         double correction, int bound_lo, int bound_hi,
                                                                         int* __restrict__ thresholds, int* __restrict__ details) {
  __shared__ u64 wave_n[THRESHOLD_WAVES], wave_s[THRESHOLD_WAVES];
  __shared__ int red_i[THRESHOLD_WAVES];
  __shared__ double red_j[THRESHOLD_WAVES];
  __shared__ int red_key[THRESHOLD_WAVES];
  __shared__ u64 bin_n[THRESHOLD_BINS], bin_s[THRESHOLD_BINS], cum_n[THRESHOLD_BINS], cum_s[THRESHOLD_BINS];
  const int f = blockIdx.x, t = threadIdx.x, lane = t & (WAVE - 1), wid = t / WAVE;
  const int v0 = t * THRESHOLD_PER;
  const uint4* h4 = reinterpret_cast<const uint4*>(hist + (size_t)f * THRESHOLD_LEVELS + v0);  // (16 groups of four: 256-byte aligned)

  // the thread's count, its sum of v h[v], its lowest and highest occupied level
  u64 n_own = 0, s_own = 0;
  int lo = THRESHOLD_LEVELS, hi = -1;
#pragma unroll 4
  for (int k = 0; k < THRESHOLD_PER / 4; ++k) {
    const uint4 q = h4[k];
    const unsigned c[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int v = v0 + 4 * k + i;
      n_own += c[i];
      s_own += (u64)c[i] * (u64)v;
      if (c[i]) { lo = min(lo, v); hi = v; }
    }
  }
  lo = block_min_i32(lo, red_i);
  hi = block_max_i32(hi, red_i);  // (its first barrier comes after every read of the minimum)

  // exclusive prefixes over the threads: shuffle scan inside the wave, wave totals through LDS
  u64 incl_n = n_own, incl_s = s_own;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const u64 up_n = __shfl_up(incl_n, o, WAVE), up_s = __shfl_up(incl_s, o, WAVE);
    if (lane >= o) { incl_n += up_n; incl_s += up_s; }
  }
  if (lane == WAVE - 1) { wave_n[wid] = incl_n; wave_s[wid] = incl_s; }
  __syncthreads();
  u64 before_n = incl_n - n_own, before_s = incl_s - s_own, total_n = 0, total_s = 0;
  for (int i = 0; i < THRESHOLD_WAVES; ++i) {
    if (i < wid) { before_n += wave_n[i]; before_s += wave_s[i]; }
    total_n += wave_n[i];
    total_s += wave_s[i];
  }

  // two classes.  lo == hi (a constant tile) has no candidate: the threshold is lo.
  double best_j = -1.0;  // (J >= 0)
  int best_t = THRESHOLD_NONE;
  if (n_own != 0) {
    u64 n0 = before_n, s0 = before_s;
    for (int k = 0; k < THRESHOLD_PER / 4; ++k) {
      const uint4 q = h4[k];
      const unsigned c[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = v0 + 4 * k + i;
        if (c[i] == 0) continue;
        n0 += c[i];
        s0 += (u64)c[i] * (u64)v;
        if (v >= hi) continue;  // (class 1 would be empty)
        const double j = threshold_term(s0, n0) + threshold_term(total_s - s0, total_n - n0);
        if (j > best_j) { best_j = j; best_t = v + 1; }  // (levels ascend: the first maximum)
      }
    }
  }
  threshold_reduce(best_j, best_t, red_j, red_key);
  const int two = best_t == THRESHOLD_NONE ? lo : best_t;
  int t1 = two, t2 = two;

  if (classes == 3) {
    const int width = hi - lo + 1;
    if (t < THRESHOLD_BINS) { bin_n[t] = 0; bin_s[t] = 0; }
    __syncthreads();
    if (n_own != 0) {
      int run = -1;
      u64 rn = 0, rs = 0;
      for (int k = 0; k < THRESHOLD_PER / 4; ++k) {
        const uint4 q = h4[k];
        const unsigned c[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int v = v0 + 4 * k + i;
          if (c[i] == 0) continue;
          const int b = ((v - lo) * THRESHOLD_BINS) / width;  // (lo <= v <= hi: 0 <= b <= 255; the product is below 2^24)
          if (b != run) {
            if (run >= 0) { atomicAdd(&bin_n[run], rn); atomicAdd(&bin_s[run], rs); }
            run = b; rn = 0; rs = 0;
          }
          rn += c[i];
          rs += (u64)c[i] * (u64)v;
        }
      }
      if (run >= 0) { atomicAdd(&bin_n[run], rn); atomicAdd(&bin_s[run], rs); }
    }
    __syncthreads();
    if (t < THRESHOLD_BINS) {  // inclusive prefix of bin t
      u64 n = 0, s = 0;
      for (int k = 0; k <= t; ++k) { n += bin_n[k]; s += bin_s[k]; }
      cum_n[t] = n;
      cum_s[t] = s;
    }
    __syncthreads();
    double pair_j = -1.0;
    int pair_key = THRESHOLD_NONE;
    for (int cell = t; cell < (THRESHOLD_BINS - 2) * (THRESHOLD_BINS - 1); cell += THRESHOLD_THREADS) {
      const int k1 = cell / (THRESHOLD_BINS - 1), k2 = cell % (THRESHOLD_BINS - 1);  // 0 <= k1 <= 253, 0 <= k2 <= 254
      if (k2 <= k1) continue;
      const u64 n0 = cum_n[k1], s0 = cum_s[k1], n01 = cum_n[k2], s01 = cum_s[k2];
      const u64 n1 = n01 - n0, n2 = total_n - n01;
      if (n0 == 0 || n1 == 0 || n2 == 0) continue;
      const double j = threshold_term(s0, n0) + threshold_term(s01 - s0, n1) + threshold_term(total_s - s01, n2);
      if (j > pair_j) { pair_j = j; pair_key = cell; }  // (cells ascend in a thread: the first maximum)
    }
    threshold_reduce(pair_j, pair_key, red_j, red_key);
    if (pair_key != THRESHOLD_NONE) {
      const int k1 = pair_key / (THRESHOLD_BINS - 1), k2 = pair_key % (THRESHOLD_BINS - 1);
      t1 = lo + ((k1 + 1) * width + THRESHOLD_BINS - 1) / THRESHOLD_BINS;  // the first grey level of the next bin
      t2 = lo + ((k2 + 1) * width + THRESHOLD_BINS - 1) / THRESHOLD_BINS;
    }
  }

  if (t == 0) {
    const int raw = (classes == 3 && middle == ALIBY_THRESHOLD_MIDDLE_BACKGROUND) ? t2 : t1;
    double scaled = (double)raw * correction;
    scaled = scaled < 65535.0 ? scaled : 65535.0;
    long long r = __double2ll_rn(scaled);  // half to even
    r = r > bound_lo ? r : bound_lo;
    r = r < bound_hi ? r : bound_hi;
    thresholds[f] = (int)r;
    if (details) {
      details[4 * f + 0] = lo;
      details[4 * f + 1] = hi;
      details[4 * f + 2] = t1;
      details[4 * f + 3] = t2;
    }
  }
}

extern "C" size_t aliby_auto_threshold_workspace_bytes(int F) {
  return F > 0 ? (size_t)F * THRESHOLD_LEVELS * sizeof(uint32_t) : 0;
}

extern "C" int aliby_auto_threshold(aliby_ctx* ctx, const uint16_t* image, int F, int Y, int X, int classes, int middle, double correction,
                                    int bound_lo, int bound_hi, void* workspace, size_t workspace_bytes, int32_t* thresholds,
                                    int32_t* details, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(F >= 0 && Y >= 0 && X >= 0, "bad shape");
  ARG_CHECK(classes == 2 || classes == 3, "classes must be 2 or 3");
  ARG_CHECK(middle == ALIBY_THRESHOLD_MIDDLE_FOREGROUND || middle == ALIBY_THRESHOLD_MIDDLE_BACKGROUND,
            "middle must be ALIBY_THRESHOLD_MIDDLE_FOREGROUND or ALIBY_THRESHOLD_MIDDLE_BACKGROUND");
  ARG_CHECK(correction > 0.0 && correction <= 16.0, "correction must be in (0, 16]");
  ARG_CHECK(bound_lo >= 0 && bound_lo <= bound_hi && bound_hi <= 65535, "bounds must be 0 <= lo <= hi <= 65535");
  if (F == 0 || Y == 0 || X == 0) return ALIBY_OK;
  ARG_CHECK(F <= 65535, "more than 65535 tiles in one call (the histogram launch's limit)");
  ARG_CHECK((unsigned long long)Y * (unsigned long long)X < (1ull << 32), "a tile has 2^32 pixels or more (32-bit histogram bins)");
  ARG_CHECK(image && thresholds, "NULL argument");
  ARG_CHECK(workspace != nullptr && ((uintptr_t)workspace & 15) == 0, "workspace is NULL or not 16-byte aligned");
  ARG_CHECK(workspace_bytes >= aliby_auto_threshold_workspace_bytes(F), "workspace is smaller than aliby_auto_threshold_workspace_bytes");
  uint32_t* hist = static_cast<uint32_t*>(workspace);
  const int rc = aliby_crop_hist_u16(ctx, image, F, (size_t)Y * X, hist, stream);
  if (rc != ALIBY_OK) return rc;
  hipLaunchKernelGGL(k_threshold_search, dim3(F), dim3(THRESHOLD_THREADS), 0, as_stream(stream), hist, classes, middle, correction,
                     bound_lo, bound_hi, thresholds, details);
  KERNEL_CHECK();
  return ALIBY_OK;
}
