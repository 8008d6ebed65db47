// feat_localisation.hip — nuc_est_conv and nuc_conv_3d, the reference's nuclear localisation metrics, one workgroup per object.
// nuc_est_conv (k_nuc) comes first; nuc_conv_3d (k_nuc3d), its Z-stack sibling, has a header of its own further down.
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

// ======================================================================================================================= nuc_conv_3d
// Reference: src/extraction/core/functions/custom/localisation.py:123-140 (nuc_conv_3d; the filter is gauss3D, 31-44).  Per
// object, with the 2-D mask repeated on every plane of the [Z,Y,X] stack, v = the Z area voxels under it, N = the number of
// NON-ZERO values among them, med = np.median(v):
//   chi = -2 ln(0.05), r = sqrt(0.085 N / pi), sd = r / sqrt(chi), hw = ceil(2 r), ratio = z_spacing / pixel_size
//   h = the (2 hw + 1)^3 filter exp(-(x^2 / (2 sd) + y^2 / (2 sd) + z^2 / (2 sd ratio))), normalised to sum 1.  The exponents
//       divide by sd, NOT sd^2, and the extent is the same on all three axes even where 2 hw + 1 > Z: both are the reference's.
//   J = stack - med under the mask, 0 elsewhere (uint16: exact; float32: med = the float32 mean of the two middle values,
//       subtracted in float32, as NumPy does)
//   result = max over the WHOLE stack of convolve(J, h, "same"), divided by sum(h^2) 0.95 pi chi sd^2 (here it IS sd squared)
// NaN for an empty object and for N == 0 (the filter is exp(-0 / 0)); an object whose voxels are all equal gives 0.0.
//
// The filter is taken in its separable form gx (x) gx (x) gz, each normalised to sum 1, sum(h^2) = (sum gx^2)^2 sum gz^2: the
// reference zeroes entries below eps max(h) before normalising, which moves the result by parts in 1e15.
//
// N and the median are found here (aliby_features_cell knows one plane).  The object's box of every plane is loaded raw into
// J [Z][h][w] (float32: exact for uint16 pixels), and the middle order statistic(s) of the masked values are selected exactly by a
// bytewise radix selection over order-preserving keys (2 passes for uint16, 4 for float32; both middle values when the count is
// even): integer histograms in LDS, so the result does not depend on the order in which threads deposit or count values.  Then
// J -= med in place, 0 off the mask.
//
// Order of the axes: z, then x, then y.  Per output plane zo = 0 .. Z-1:
//   mix     P[h][w]    = sum over zi, |zo - zi| <= hw, of gz[zo - zi + hw] J[zi]        (float64; increasing zi)
//   rows    R[h][wd]   = P correlated with gx along x over the dilated, clipped columns  (increasing source column)
//   columns the response at [hd][wd], fused with the running maximum                     (increasing source row)
// so the float64 part of the working set does not grow with Z.  Along z every plane of the stack is an output position and only
// the taps that meet data are summed; the normalising sums run over all 2 hw + 1 taps.  Where a plane extends past the box dilated
// by hw and clipped, the response is 0 there and that 0 takes part in the maximum, as in k_nuc.
//
// Arithmetic: as k_nuc.  Every intermediate and every output position is summed by ONE thread over its taps in a fixed order, in
// float64; the normalisers are summed by one thread in index order; a maximum is exact in any order.  A row carries the same bits
// whatever the workgroup size, the launch form, the batch and the neighbours.
//
// Working set of a workgroup, from the table's capacities (hw_max = ceil(2 sqrt(0.085 max_area Z / pi)),
// wd_max = min(X, max_w + 2 hw_max)):
//   need = r16(8 (max_h wd_max + max_h max_w + 2 (2 hw_max + 1)) + 4 Z max_h max_w)      R, P, gx and gz (f64); J (f32)
// LDS budget 64 KiB, k_nuc's: this kernel has 1.2 KiB of static LDS (the 256-bin histogram on top of k_nuc's), so two workgroups
// still fit a CU's 160 KiB at the budget; the benchmark's nuclei at Z = 5 (32 x 32 boxes, hw_max = 16) need 45 584 bytes (44.5 KiB) and run three to
// a CU.  Above the budget the global form (object_launch.h).
// LDS access: every pass walks a row with consecutive lanes: consecutive f32 (mix) or f64 addresses (ds_read_b64: 32 lanes fill
// one 256-byte bank row), the filter tap a broadcast, so no row pitch needs padding.
struct Nuc3dArgs {
  const u16* labels;
  const void* stack;
  int F, C, Z, Y, X, channel;
  const aliby_object* tab;
  int n_obj;
  int max_h, max_w, hw_max;
  size_t cap_rows;  // max_h * wd_max doubles
  size_t cap_box;   // max_h * max_w
  size_t slab;      // bytes of one working set
  double ratio, chi;
  unsigned char* gscratch;
  double* out;
  int ld, col0;
};

// order-preserving integer keys of the raw values held in J: uint16 pixels are whole numbers below 65536
template <typename T> struct Nuc3dKey;
template <> struct Nuc3dKey<u16> {
  static constexpr int BITS = 16;
  static __device__ __forceinline__ unsigned key(float v) { return (unsigned)v; }
  static __device__ __forceinline__ float value(unsigned k) { return (float)k; }
};
template <> struct Nuc3dKey<float> {
  static constexpr int BITS = 32;
  static __device__ __forceinline__ unsigned key(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  static __device__ __forceinline__ float value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
};

// The k-th smallest (0-based) of the masked raw values in J [Z][hw_box]: one 256-bin histogram per key byte, from the top.
template <typename T>
__device__ float nuc3d_select(const float* J, const u16* lab, u16 L, const aliby_object& o, int X, int Z, int k, unsigned* hist,
                              unsigned* s_pick) {
  const int tid = threadIdx.x, h = o.y1 - o.y0, w = o.x1 - o.x0, box = h * w;
  unsigned prefix = 0, himask = 0;
  for (int shift = Nuc3dKey<T>::BITS - 8; shift >= 0; shift -= 8) {
    for (int b = tid; b < 256; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    for (int i = tid; i < box; i += blockDim.x) {
      if (lab[(size_t)(o.y0 + i / w) * X + o.x0 + i % w] != L) continue;
      for (int z = 0; z < Z; ++z) {
        const unsigned key = Nuc3dKey<T>::key(J[(size_t)z * box + i]);
        if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid < 64) {  // the first wave: four bins a lane, an inclusive scan over the lanes, and the one lane whose bins hold k
      const unsigned c0 = hist[4 * tid], c1 = hist[4 * tid + 1], c2 = hist[4 * tid + 2], c3 = hist[4 * tid + 3];
      unsigned incl = c0 + c1 + c2 + c3;
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        if (tid >= d) incl += up;
      }
      unsigned below = incl - (c0 + c1 + c2 + c3);
      if ((unsigned)k >= below && (unsigned)k < incl) {
        int b = 4 * tid;
        if ((unsigned)k >= below + c0) { below += c0; ++b;
          if ((unsigned)k >= below + c1) { below += c1; ++b;
            if ((unsigned)k >= below + c2) { below += c2; ++b; } } }
        s_pick[0] = (unsigned)b;
        s_pick[1] = (unsigned)k - below;
      }
    }
    __syncthreads();
    prefix |= s_pick[0] << shift;
    k = (int)s_pick[1];
    himask |= 255u << shift;
    __syncthreads();
  }
  return Nuc3dKey<T>::value(prefix);
}

template <typename T, bool GLOBAL>
__global__ __launch_bounds__(256) void k_nuc3d(Nuc3dArgs a) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ double red_d[8];
  __shared__ int red_i[8];
  __shared__ double s_sum[2];
  __shared__ unsigned hist[256];
  __shared__ unsigned s_pick[2];
  unsigned char* ws = GLOBAL ? (a.gscratch + (size_t)blockIdx.x * a.slab) : lds_raw;
  double* rowp = reinterpret_cast<double*>(ws);  // row pass: [h][wd]
  double* P = rowp + a.cap_rows;                 // z mix: [h][w]
  double* gx = P + a.cap_box;                    // filter taps [2 hw + 1], in plane
  double* gz = gx + 2 * a.hw_max + 1;            // and along z
  float* J = reinterpret_cast<float*>(gz + 2 * a.hw_max + 1);  // [Z][h][w]
  const int tid = threadIdx.x, Z = a.Z;
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
    const int box = h * w;
    const u16* lab = a.labels + (size_t)o.tile * plane;
    const T* px = reinterpret_cast<const T*>(a.stack) + ((size_t)o.tile * a.C + a.channel) * Z * plane;
    const u16 L = (u16)o.label;
    __syncthreads();
    // ---- the raw values of the box on every plane; N and the number of masked values -------------------------------------------
    int n = 0, cnt = 0;
    for (int i = tid; i < box; i += blockDim.x) {
      const size_t idx = (size_t)(o.y0 + i / w) * a.X + o.x0 + i % w;
      const bool in = lab[idx] == L;
      for (int z = 0; z < Z; ++z) {
        const float v = in ? px_load<T>(px, (size_t)z * plane + idx) : 0.0f;
        n += (in && v != 0.0f);
        J[(size_t)z * box + i] = v;
      }
      cnt += in ? Z : 0;
    }
    const int N = block_sum_i32(n, red_i);
    const int count = block_sum_i32(cnt, red_i);
    const double r = sqrt(0.085 * (double)N / M_PI);
    const int hw = (int)ceil(2.0 * r);
    if (N == 0 || count == 0 || hw > a.hw_max) {
      if (tid == 0) *out = NAN;  // no non-zero voxel: the filter is exp(-0 / 0)
      __syncthreads();
      continue;
    }
    // ---- np.median of the masked values: the middle one, or the mean of the two middle ones ----------------------------------------
    __syncthreads();
    const float lo = nuc3d_select<T>(J, lab, L, o, a.X, Z, (count - 1) / 2, hist, s_pick);
    const float hi = (count & 1) ? lo : nuc3d_select<T>(J, lab, L, o, a.X, Z, count / 2, hist, s_pick);
    const double med = (count & 1) ? (double)lo : ((double)lo + (double)hi) * 0.5;  // uint16 -> float64, exact
    const float medf = (count & 1) ? lo : (lo + hi) * 0.5f;                         // float32: NumPy's float32 mean of two
    // ---- J = value - median under the mask.  uint16: |J| <= 65535.5 in steps of 0.5, exact in float32 --------------------------
    for (int i = tid; i < box; i += blockDim.x) {
      const bool in = lab[(size_t)(o.y0 + i / w) * a.X + o.x0 + i % w] == L;
      for (int z = 0; z < Z; ++z) {
        const float v = J[(size_t)z * box + i];
        J[(size_t)z * box + i] = !in ? 0.0f : (sizeof(T) == 2) ? (float)((double)v - med) : v - medf;
      }
    }
    // ---- the taps.  sd divides the exponents as a variance would: the reference's gauss3D --------------------------------------------
    const double sd = r / sqrt(a.chi);
    const int nt = 2 * hw + 1;
    for (int k = tid; k < nt; k += blockDim.x) {
      const double d = (double)(k - hw);
      gx[k] = exp(-((d * d) / (2.0 * sd)));
      gz[k] = exp(-((d * d) / (2.0 * (sd * a.ratio))));
    }
    __syncthreads();
    if (tid == 0) {
      double sx = 0.0, sz = 0.0;
      for (int k = 0; k < nt; ++k) sx += gx[k];
      for (int k = 0; k < nt; ++k) sz += gz[k];
      s_sum[0] = sx;
      s_sum[1] = sz;
    }
    __syncthreads();
    const double gxs = s_sum[0], gzs = s_sum[1];
    for (int k = tid; k < nt; k += blockDim.x) {
      gx[k] /= gxs;
      gz[k] /= gzs;
    }
    __syncthreads();
    if (tid == 0) {
      double sx = 0.0, sz = 0.0;
      for (int k = 0; k < nt; ++k) sx += gx[k] * gx[k];
      for (int k = 0; k < nt; ++k) sz += gz[k] * gz[k];
      s_sum[0] = sx;
      s_sum[1] = sz;
    }
    const int ya = max(0, o.y0 - hw), yb = min(a.Y, o.y1 + hw), xa = max(0, o.x0 - hw), xb = min(a.X, o.x1 + hw);
    const int hd = yb - ya, wd = xb - xa;
    // every plane is an output position, so the dilated box covers the stack exactly when it covers a plane
    double m = ((long long)hd * wd < (long long)a.Y * a.X) ? 0.0 : (double)-INFINITY;
    for (int zo = 0; zo < Z; ++zo) {
      // ---- mix along z ----------------------------------------------------------------------------------------------------------
      const int z_lo = max(0, zo - hw), z_hi = min(Z - 1, zo + hw);
      for (int i = tid; i < box; i += blockDim.x) {
        double acc = 0.0;
        for (int zi = z_lo; zi <= z_hi; ++zi) acc += gz[zo - zi + hw] * (double)J[(size_t)zi * box + i];
        P[i] = acc;
      }
      __syncthreads();
      // ---- row pass: the box's rows over the dilated, clipped columns -------------------------------------------------------------
      for (int i = tid; i < h * wd; i += blockDim.x) {
        const int rr = i / wd, dx = xa + i % wd - o.x0;  // column relative to the box
        const int s_lo = max(0, dx - hw), s_hi = min(w - 1, dx + hw);
        double acc = 0.0;
        for (int s = s_lo; s <= s_hi; ++s) acc += gx[dx - s + hw] * P[rr * w + s];
        rowp[i] = acc;
      }
      __syncthreads();
      // ---- column pass and the running maximum ------------------------------------------------------------------------------------
      for (int i = tid; i < hd * wd; i += blockDim.x) {
        const int c = i % wd, dy = ya + i / wd - o.y0;
        const int t_lo = max(0, dy - hw), t_hi = min(h - 1, dy + hw);
        double acc = 0.0;
        for (int t = t_lo; t <= t_hi; ++t) acc += gx[dy - t + hw] * rowp[t * wd + c];
        m = fmax(m, acc);
      }
      // (the next plane's mix writes P, last read before the barrier above; its row pass comes after the mix's barrier)
    }
    const double M = block_max_f64(m, red_d);
    if (tid == 0) {
      const double s2 = s_sum[0] * s_sum[0] * s_sum[1];  // sum(h^2)
      *out = M / (s2 * 0.95 * M_PI * a.chi * (sd * sd)) + 0.0;
    }
    __syncthreads();
  }
}

extern "C" int aliby_features_nuc_conv_3d(aliby_ctx* ctx, const uint16_t* labels, const void* stack, int dtype, int F, int C, int Z,
                                          int Y, int X, int channel, const aliby_object* table_dev, int n_obj, int max_h, int max_w,
                                          int max_area, double pixel_size, double z_spacing, double* out, int ld, int col0,
                                          void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(pixel_size > 0.0 && isfinite(pixel_size), "pixel_size must be positive and finite");
  ARG_CHECK(z_spacing > 0.0 && isfinite(z_spacing), "z_spacing must be positive and finite");
  ARG_CHECK(Z >= 1, "the stack needs at least one plane");
  if (n_obj == 0) return ALIBY_OK;
  ARG_CHECK(labels && stack && table_dev && out, "NULL argument");
  ARG_CHECK(F > 0 && Y > 0 && X > 0 && max_h >= 0 && max_w >= 0 && max_area >= 0, "bad shape");
  ARG_CHECK(col0 >= 0 && col0 + 1 <= ld, "columns exceed row stride");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "dtype must be ALIBY_U16 or ALIBY_F32");
  ARG_CHECK(channel >= 0 && channel < C, "channel out of range");
  ARG_CHECK((long long)max_area * Z <= INT_MAX && (long long)max_h * max_w * Z <= INT_MAX, "objects times planes exceed the int range");
  const double ratio = z_spacing / pixel_size;
  ARG_CHECK(ratio > 0.0 && isfinite(ratio), "z_spacing / pixel_size must be positive and finite");
  const double hw_d = ceil(2.0 * sqrt(0.085 * (double)max_area * (double)Z / M_PI));
  ARG_CHECK(hw_d <= 32768.0, "objects too large: filter half-width above 32768");
  Nuc3dArgs a;
  a.labels = labels; a.stack = stack; a.F = F; a.C = C; a.Z = Z; a.Y = Y; a.X = X; a.channel = channel;
  a.tab = table_dev; a.n_obj = n_obj; a.max_h = max_h; a.max_w = max_w;
  a.ratio = ratio; a.chi = -2.0 * log1p(-0.95);
  a.out = out; a.ld = ld; a.col0 = col0;
  a.hw_max = (int)hw_d;
  const long long wd_max = (long long)max_w + 2 * a.hw_max < X ? (long long)max_w + 2 * a.hw_max : X;
  a.cap_rows = (size_t)max_h * (size_t)wd_max;
  a.cap_box = (size_t)max_h * (size_t)max_w;
  const size_t need = (8 * (a.cap_rows + a.cap_box + 2 * (2 * (size_t)a.hw_max + 1)) + 4 * (size_t)Z * a.cap_box + 15) & ~(size_t)15;
  a.slab = need;
  const long long hd_max = (long long)max_h + 2 * a.hw_max < Y ? (long long)max_h + 2 * a.hw_max : Y;
  return object_launch(ctx, object_kernel(dtype, k_nuc3d<u16, false>, k_nuc3d<float, false>),
                       object_kernel(dtype, k_nuc3d<u16, true>, k_nuc3d<float, true>), a, n_obj, need, NUC_LDS_BUDGET, hd_max * wd_max,
                       as_stream(stream));
}
