// haralick_stats.h — what the 2-D texture kernel (feat_texture.hip, k_texture) and the volume kernel (feat_texture3d.hip,
// k_texture3d) share: the grey level of a pixel, the log2 table, and the stage from the integer cell counts of one symmetric
// co-occurrence matrix to mahotas' 13 Haralick statistics.  The caller counts the matrix (its own business: sorted keys,
// 16-bit or 32-bit counters) and hands every non-zero cell of the upper triangle to haralick_cell, which fills the integer
// marginals p_x, p_{x+y}, p_{x-y} (LDS histograms) and three per-thread sums; haralick_marginal_sums reduces those over the
// workgroup and haralick_finish, after the caller's second walk over the cells (HXY1), writes the 13 numbers.  Every probability is an integer count over the total T = 2 x pairs, divided once: nothing here
// depends on the order in which the matrix was counted, and for a given workgroup size the result depends on the counts only.
// Conventions (oracle/texture_restated.py): SumVariance without the "haralick bug", DifferenceVariance = variance of the
// p_{x-y} VECTOR of length maxv (largest grey level of the crop + 1), entropies in bits.
#pragma once
#include "common.h"
#include <atomic>

#ifdef __HIPCC__

#define TX_NSTAT 13

__device__ __forceinline__ int grey_of(unsigned short v, int gl, int shift) {
  int q = v >> shift;
  if (gl != 256) q = (int)((double)q / 255.0 * (double)(gl - 1));
  return q;
}
__device__ __forceinline__ int grey_of(float v, int gl, int) {
  double x = rint((double)v * 255.0);
  x = fmin(fmax(x, 0.0), 255.0);
  int q = (int)x;
  if (gl != 256) q = (int)((double)q / 255.0 * (double)(gl - 1));
  return q;
}

// Every probability of the co-occurrence statistics is an integer count over the total T, so p log2(p) is
// (c / T) (log2 c - log2 T): log2 of the integers below 2^16 comes from a table in device memory (512 KB, L2-resident,
// filled once per device with the same log2() it replaces); the fp64 log2 sequence was most of the kernel's instructions.
// The table belongs to the translation unit that includes this header (device variables are not shared between code objects).
#define TX_LOGTAB 65536
namespace {
__device__ double g_log2_int[TX_LOGTAB];
__global__ void k_init_log2_table() {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < TX_LOGTAB) g_log2_int[i] = i > 0 ? log2((double)i) : 0.0;
}
// fills this translation unit's table on the context's device, once
inline int haralick_log2_table_ready(aliby_ctx* ctx, hipStream_t s) {
  static std::atomic<unsigned long long> ready{0};  // one bit per device
  const unsigned long long bit = 1ull << (ctx->device & 63);
  if (!(ready.load(std::memory_order_acquire) & bit)) {
    hipLaunchKernelGGL(k_init_log2_table, dim3(TX_LOGTAB / 256), dim3(256), 0, s);
    KERNEL_CHECK();
    HIP_TRY(hipStreamSynchronize(s));  // other streams may run this kernel next
    ready.fetch_or(bit, std::memory_order_release);
  }
  return ALIBY_OK;
}
}  // namespace
__device__ __forceinline__ double log2_int(int n) { return n < TX_LOGTAB ? g_log2_int[n] : log2((double)n); }
// (c / T) log2(c / T), logT = log2(T)
__device__ __forceinline__ double plog2p_count(int c, double Tt, double logT) {
  return c > 0 ? ((double)c / Tt) * (log2_int(c) - logT) : 0.0;
}

// index of a cell in the row-major lower triangle (hi (hi + 1) / 2 + lo, lo <= hi) -> its row hi; lo = idx - hi (hi + 1) / 2
__device__ __forceinline__ int haralick_tri_row(int idx) {
  int rh = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
  while (rh * (rh + 1) / 2 > idx) --rh;
  while ((rh + 1) * (rh + 2) / 2 <= idx) ++rh;
  return rh;
}

// c pixel pairs with the unordered grey-level pair (lo, hi): into the integer marginals (LDS atomics) and this thread's
// acc = {sum p^2 (as counts^2), sum i j count, sum p log2(p)}
__device__ __forceinline__ void haralick_cell(int c, int lo, int hi, double Tt, double logT, int* hx, int* hplus, int* hminus, double (&acc)[3]) {
  if (lo == hi) {
    atomicAdd(&hx[lo], 2 * c);
    acc[0] += 4.0 * (double)c * (double)c;
    acc[2] += plog2p_count(2 * c, Tt, logT);
  } else {
    atomicAdd(&hx[lo], c);
    atomicAdd(&hx[hi], c);
    acc[0] += 2.0 * (double)c * (double)c;
    acc[2] += 2.0 * plog2p_count(c, Tt, logT);
  }
  atomicAdd(&hplus[lo + hi], 2 * c);
  atomicAdd(&hminus[hi - lo], 2 * c);
  acc[1] += 2.0 * (double)c * (double)lo * (double)hi;
}

// a cell's term of HXY1 = -sum_ij p_ij log2(px_i py_j), once p_x is complete
__device__ __forceinline__ double haralick_hxy1_term(int c, int lo, int hi, const int* hx, double Tt, double logT) {
  return (2.0 * (double)c / Tt) * (log2_int(hx[lo]) + log2_int(hx[hi]) - 2.0 * logT);
}

// The stage after the cells, in two halves with the caller's second walk over the cells (haralick_hxy1_term) between them.  All
// threads of the workgroup call both (they contain barriers) after every cell went through haralick_cell.
struct HaralickSums {
  double f_asm, sum_ij, f_entropy;
  double m[8];  // ux, sum k^2 px, HX (sum p log p), contrast, IDM, sum p_minus, sum p_minus^2, difference entropy (sum p log p)
  double s[3];  // sum average, sum k^2 p_plus, sum entropy (sum p log p)
};
// acc: this thread's sums of haralick_cell; hx / hplus / hminus: the marginals, non-zero only in [minlev, maxlev],
// [2 minlev, 2 maxlev], [0, maxlev - minlev]; vec: LDS double[32].  On return p_x is complete for every thread.
__device__ __forceinline__ void haralick_marginal_sums(HaralickSums& r, double (&acc)[3], const int* hx, const int* hplus, const int* hminus,
                                                       const int minlev, const int maxlev, const int maxv, const double Tt, const double logT,
                                                       double* vec) {
  const int tid = threadIdx.x;
  block_sum_vec_all<3>(acc, vec);
  __syncthreads();
  r.f_asm = acc[0] / (Tt * Tt);
  r.sum_ij = acc[1] / Tt;
  r.f_entropy = -acc[2];

  // ---- marginal statistics --------------------------------------------------------------------
  double m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = minlev + tid; k <= maxlev; k += blockDim.x) {  // p_x is zero outside the present levels
    const double pxk = (double)hx[k] / Tt;
    m[0] += (double)k * pxk;
    m[1] += (double)k * (double)k * pxk;
    m[2] += plog2p_count(hx[k], Tt, logT);
  }
  for (int k = tid; k <= maxlev - minlev; k += blockDim.x) {  // |i - j| never exceeds the level range
    const double pm = (double)hminus[k] / Tt;
    m[3] += (double)k * (double)k * pm;
    m[4] += pm / (1.0 + (double)k * (double)k);
    if (k < maxv) { m[5] += pm; m[6] += pm * pm; }
    m[7] += plog2p_count(hminus[k], Tt, logT);
  }
  block_sum_vec_all<8>(m, vec);
  double s[3] = {0, 0, 0};  // sum average, sum k^2 p_plus, sum entropy (sum p log p)
  for (int k = 2 * minlev + tid; k <= 2 * maxlev; k += blockDim.x) {
    const double pp = (double)hplus[k] / Tt;
    s[0] += (double)k * pp;
    s[1] += (double)k * (double)k * pp;
    s[2] += plog2p_count(hplus[k], Tt, logT);
  }
  block_sum_vec_all<3>(s, vec);
#pragma unroll
  for (int k = 0; k < 8; ++k) r.m[k] = m[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) r.s[k] = s[k];
}

// hxy: this thread's sum of haralick_hxy1_term over the cells.  Thread 0 writes fo[0 .. 13); the caller puts a barrier before it
// touches the marginals again.
__device__ __forceinline__ void haralick_finish(double* fo, const HaralickSums& r, const double hxy, const int maxv, double* vec) {
  const double* m = r.m;
  const double* s = r.s;
  const double f_asm = r.f_asm, sum_ij = r.sum_ij, f_entropy = r.f_entropy;
  double hv[1] = {hxy};
  block_sum_vec_all<1>(hv, vec);

  if (threadIdx.x == 0) {
    const double ux = m[0], vx = m[1] - ux * ux, sx = sqrt(vx);
    const double HX = -m[2];
    const double HXY1 = -hv[0];
    const double HXY2 = 2.0 * HX;  // -sum (px_i py_j) log2(px_i py_j) with p symmetric
    fo[0] = f_asm;
    fo[1] = m[3];
    fo[2] = (sx == 0.0) ? 1.0 : (1.0 / sx / sx) * (sum_ij - ux * ux);
    fo[3] = vx;
    fo[4] = m[4];
    fo[5] = s[0];
    fo[6] = s[1] - s[0] * s[0];
    fo[7] = -s[2];
    fo[8] = f_entropy;
    {
      // numpy var of the length-maxv vector p_{x-y}: mean(|x - mean|^2)
      const double mean = m[5] / (double)maxv;
      fo[9] = m[6] / (double)maxv - mean * mean;
    }
    fo[10] = -m[7];
    fo[11] = (HX == 0.0) ? (f_entropy - HXY1) : (f_entropy - HXY1) / HX;
    fo[12] = sqrt(fmax(0.0, 1.0 - exp(-2.0 * (HXY2 - f_entropy))));
  }
}

#endif  // __HIPCC__
