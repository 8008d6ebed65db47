// feat_localisation.hip — nuc_est_conv, the reference's nuclear localisation metric, one workgroup per object.
//
// Reference: src/extraction/core/functions/custom/localisation.py:75-120 (nuc_est_conv; the filter is matlab_style_gauss2D,
// 16-28).  Per object, with v = the object's pixels, N = the number of NON-ZERO values among them, med = np.median(v):
//   r = sqrt(object_radius_estimation N / pi), hw = ceil(2 r), sigma = gaussian_sigma or r / sqrt(chi), chi = -2 ln(1 - alpha)
//   h = the (2 hw + 1)^2 Gaussian of that sigma, normalised to sum 1
//   J = pixels - med inside the object, 0 elsewhere (uint16 pixels: exact; float32 pixels: subtracted in float32, as NumPy does)
//   result = max over the WHOLE tile of convolve(J, h, "same"), divided by sum(h^2) alpha pi chi sigma^2
// N == 0 with a derived sigma, or an empty object, is NaN (0 / 0 in the filter, the median of nothing); a uniform object is 0.0.
//
// The filter is taken in its separable form, h = g g^T with g[k] = exp(-k^2 / (2 sigma^2)) / sum: the reference zeroes entries of
// the 2-D filter below eps max(h) before normalising, which moves the result by parts in 1e16.  sum(h^2) = (sum g^2)^2.
// Two 1-D passes over the object's box dilated by hw and clipped to the tile ("same": positions off the tile are no candidates):
// rows first (box rows x dilated columns, float64), then columns.  Where the tile extends past the dilated box the response is 0
// there, and that 0 takes part in the maximum.
//
// Arithmetic: float64 sums; every output position is summed by ONE thread over its taps in increasing source order, so its bits do
// not depend on the workgroup size, and the maximum of such values is exact in any order: a row carries the same bits whatever
// the batch, the neighbours and the launch form.
//
// The median is not selected here: it comes in as one float64 per object (column `median` of aliby_features_cell, whose selection is
// exact).
//
// Working set of a workgroup, from the table's capacities (hw_max = ceil(2 sqrt(object_radius_estimation max_area / pi)),
// wd_max = min(X, max_w + 2 hw_max)):
//   need = r16(8 (max_h wd_max + 2 hw_max + 1) + 4 max_h max_w)     row-pass sums (f64), filter (f64), J (f32: exact, see k_nuc)
// LDS budget 64 KiB: the kernel has 104 bytes of static LDS, so two workgroups fit a CU's 160 KiB at the budget, and a table whose
// largest object has a few thousand pixels (45 x 45 box, hw_max = 13: 33 KiB) runs four to a CU.  Above it the global form
// (object_launch.h).
// LDS access: both passes walk a row with consecutive lanes (consecutive f32 / f64 addresses, the filter tap a broadcast), so no
// padding of the row pitch is needed.
#include "common.h"
#include "object_launch.h"

typedef unsigned short u16;

#define NUC_LDS_BUDGET (64 * 1024)

struct NucArgs {
  const u16* labels;
  const void* planes;
  int F, C, Y, X, channel;
  const aliby_object* tab;
  int n_obj;
  int max_h, max_w, hw_max;
  size_t cap_rows;  // max_h * wd_max doubles
  size_t slab;      // bytes of one working set
  const double* median;
  double alpha, ore, sigma, chi;  // sigma <= 0: derived per object
  unsigned char* gscratch;
  double* out;
  int ld, col0;
};

template <typename T, bool GLOBAL>
__global__ __launch_bounds__(256) void k_nuc(NucArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_d[8];
  __shared__ int red_i[8];
  __shared__ double s_sum;
  unsigned char* ws = GLOBAL ? (a.gscratch + (size_t)blockIdx.x * a.slab) : lds_raw;
  double* rowp = reinterpret_cast<double*>(ws);               // row pass: [h][wd]
  double* g = rowp + a.cap_rows;                              // filter taps [2 hw + 1]
  float* J = reinterpret_cast<float*>(g + 2 * a.hw_max + 1);  // [h][w]
  const int tid = threadIdx.x;
  const size_t plane = (size_t)a.Y * a.X;

  for (int oi = blockIdx.x; oi < a.n_obj; oi += gridDim.x) {
    const aliby_object o = a.tab[oi];
    double* out = a.out + (size_t)oi * a.ld + a.col0;
    const int h = o.y1 - o.y0, w = o.x1 - o.x0;
    // (a box beyond the capacities the working set was sized from cannot come from the table the capacities were taken from)
    if (o.area <= 0 || h > a.max_h || w > a.max_w) {
      if (tid == 0) *out = NAN;
      continue;
    }
    const u16* lab = a.labels + (size_t)o.tile * plane;
    const T* px = reinterpret_cast<const T*>(a.planes) + ((size_t)o.tile * a.C + a.channel) * plane;
    const u16 L = (u16)o.label;
    const double med = a.median[oi];
    __syncthreads();
    // ---- J = pixel - median inside the object.  uint16: |J| <= 65535.5 in steps of 0.5, exact in float32 ----------------------
    int n = 0;
    for (int i = tid; i < h * w; i += blockDim.x) {
      const size_t idx = (size_t)(o.y0 + i / w) * a.X + o.x0 + i % w;
      float j = 0.0f;
      if (lab[idx] == L) {
        const float v = px_load<T>(px, idx);
        n += (v != 0.0f);
        j = (sizeof(T) == 2) ? (float)((double)v - med) : v - (float)med;
      }
      J[i] = j;
    }
    const int N = block_sum_i32(n, red_i);
    const double r = sqrt(a.ore * (double)N / M_PI);
    const int hw = (int)ceil(2.0 * r);
    if (N == 0 || hw > a.hw_max) {
      // no non-zero pixel: with a derived sigma the filter is exp(-0 / 0); with a given one it is the 1 x 1 filter over J == 0
      if (tid == 0) *out = (N == 0 && a.sigma > 0.0) ? 0.0 : NAN;
      __syncthreads();
      continue;
    }
    const double sigma = a.sigma > 0.0 ? a.sigma : r / sqrt(a.chi);
    const int nt = 2 * hw + 1;
    for (int k = tid; k < nt; k += blockDim.x) {
      const double d = (double)(k - hw);
      g[k] = exp(-(d * d) / (2.0 * sigma * sigma));
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int k = 0; k < nt; ++k) s += g[k];
      s_sum = s;
    }
    __syncthreads();
    const double gsum = s_sum;
    for (int k = tid; k < nt; k += blockDim.x) g[k] /= gsum;
    __syncthreads();
    if (tid == 0) {
      double s = 0.0;
      for (int k = 0; k < nt; ++k) s += g[k] * g[k];
      s_sum = s;
    }
    // ---- row pass: the box's rows over the dilated, clipped columns ---------------------------------------------------------------
    const int ya = max(0, o.y0 - hw), yb = min(a.Y, o.y1 + hw), xa = max(0, o.x0 - hw), xb = min(a.X, o.x1 + hw);
    const int hd = yb - ya, wd = xb - xa;
    for (int i = tid; i < h * wd; i += blockDim.x) {
      const int rr = i / wd, dx = xa + i % wd - o.x0;  // column relative to the box
      const int s_lo = max(0, dx - hw), s_hi = min(w - 1, dx + hw);
      double acc = 0.0;
      for (int s = s_lo; s <= s_hi; ++s) acc += g[dx - s + hw] * (double)J[rr * w + s];
      rowp[i] = acc;
    }
    __syncthreads();
    // ---- column pass and the maximum; the 0 of the tile beyond the dilated box takes part ----------------------------------------
    double m = ((long long)hd * wd < (long long)a.Y * a.X) ? 0.0 : (double)-INFINITY;
    for (int i = tid; i < hd * wd; i += blockDim.x) {
      const int c = i % wd, dy = ya + i / wd - o.y0;
      const int t_lo = max(0, dy - hw), t_hi = min(h - 1, dy + hw);
      double acc = 0.0;
      for (int t = t_lo; t <= t_hi; ++t) acc += g[dy - t + hw] * rowp[t * wd + c];
      m = fmax(m, acc);
    }
    const double M = block_max_f64(m, red_d);
    if (tid == 0) {
      const double s2 = s_sum * s_sum;  // sum(h^2)
      *out = M / (s2 * a.alpha * M_PI * a.chi * (sigma * sigma)) + 0.0;
    }
    __syncthreads();
  }
}

extern "C" int aliby_features_nuc_est_conv(aliby_ctx* ctx, const uint16_t* labels, const void* planes, int dtype, int F, int C,
                                           int Y, int X, int channel, const aliby_object* table_dev, int n_obj, int max_h,
                                           int max_w, int max_area, const double* median_dev, double alpha,
                                           double object_radius_estimation, double gaussian_sigma, double* out, int ld, int col0,
                                           void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(alpha > 0.0 && alpha < 1.0, "alpha must lie in (0, 1)");
  ARG_CHECK(object_radius_estimation > 0.0 && isfinite(object_radius_estimation), "object_radius_estimation must be positive");
  ARG_CHECK(isfinite(gaussian_sigma), "gaussian_sigma must be finite (<= 0: derived from the object)");
  if (n_obj == 0) return ALIBY_OK;
  ARG_CHECK(labels && planes && table_dev && median_dev && out, "NULL argument");
  ARG_CHECK(F > 0 && Y > 0 && X > 0 && max_h >= 0 && max_w >= 0 && max_area >= 0, "bad shape");
  ARG_CHECK(col0 >= 0 && col0 + 1 <= ld, "columns exceed row stride");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "dtype must be ALIBY_U16 or ALIBY_F32");
  ARG_CHECK(channel >= 0 && channel < C, "channel out of range");
  const double hw_d = ceil(2.0 * sqrt(object_radius_estimation * (double)max_area / M_PI));
  ARG_CHECK(hw_d <= 32768.0, "object_radius_estimation too large");
  NucArgs a;
  a.labels = labels; a.planes = planes; a.F = F; a.C = C; a.Y = Y; a.X = X; a.channel = channel;
  a.tab = table_dev; a.n_obj = n_obj; a.max_h = max_h; a.max_w = max_w; a.median = median_dev;
  a.alpha = alpha; a.ore = object_radius_estimation; a.sigma = gaussian_sigma; a.chi = -2.0 * log1p(-alpha);
  a.out = out; a.ld = ld; a.col0 = col0;
  a.hw_max = (int)hw_d;
  const long long wd_max = (long long)max_w + 2 * a.hw_max < X ? (long long)max_w + 2 * a.hw_max : X;
  a.cap_rows = (size_t)max_h * (size_t)wd_max;
  const size_t need = (8 * (a.cap_rows + 2 * (size_t)a.hw_max + 1) + 4 * (size_t)max_h * max_w + 15) & ~(size_t)15;
  a.slab = need;
  const long long hd_max = (long long)max_h + 2 * a.hw_max < Y ? (long long)max_h + 2 * a.hw_max : Y;
  return object_launch(ctx, object_kernel(dtype, k_nuc<u16, false>, k_nuc<float, false>), object_kernel(dtype, k_nuc<u16, true>, k_nuc<float, true>),
                       a, n_obj, need, NUC_LDS_BUDGET, hd_max * wd_max, as_stream(stream));
}
