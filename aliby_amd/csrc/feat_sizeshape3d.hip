// feat_sizeshape3d.hip — per-object size and shape over volume labels [F, Z, Y, X]: the morphology half of BASELINE config 5
// ("3-D Cellpose + 3-D features"; feat_intensity3d.hip is the intensity half).  Like that file an EXTENSION beyond what the
// reference wires (it collapses 3-D labels to 2-D before every feature call), named after CellProfiler's 3-D
// MeasureObjectSizeShape; parity with cp_measure is unpinned.
//
// 19 columns per object: Volume, BoundingBoxMinimum_X/Y/Z, BoundingBoxMaximum_X/Y/Z (exclusive), BoundingBoxVolume,
// Center_X/Y/Z, Extent, EquivalentDiameter, EulerNumber, MajorAxisLength, MinorAxisLength, InertiaTensorEigenvalues_0/1/2.
// SurfaceArea is the opt-in 20th column, written by feat_surface3d.hip (scikit-image 0.18.3's Lewiner mesh at level 0 through a table of
// cell areas; vertices on the outside voxels' centres: one voxel measures 4 sqrt(3), not 6).  Solidity is left out on purpose: a
// 3-D convex hull has nothing to be exact with here.
//
// One pass over the labels.  A workgroup stages an 8 x 8 x 64 tile of the (Z+1) x (Y+1) x (X+1) corner grid, i.e. the voxels
// of the tile plus a one-voxel halo on the low side of every axis (9 x 9 x 65 uint16 = 10.3 KB of LDS; 1.29 x the tile's own
// voxels, the halo re-reads are neighbours' lines in L2), so that the eight voxel reads of every 2 x 2 x 2 window come from
// LDS.  A lane then walks 16 consecutive corners of a row with the previous column of the window in registers:
//   * moments: voxel p itself (the window's high corner) extends a run of equal labels; a run is flushed once, with its sums
//     over x in closed form: n, sum z / y / x, sum zz / yy / xx / zy / zx / yx and the bounding box;
//   * Euler number: for every distinct label L of the window, which of the eight low-side elements at p (the vertex, three
//     edges, three faces, the cube) belong to L's cubical complex; +1 - edges + faces - cubes goes to L's signed counter.
//     A window that is all one label contributes 1 - 3 + 3 - 1 = 0 and all background nothing, so only surfaces cost anything.
// Every accumulator is an exact 64-bit integer: the result does not depend on the order of the atomics, on the tile or grid
// geometry, or on what else is in the batch.  Bounds (X, Y, Z <= 65536, Z*Y*X <= 2^32): sum x^2 over any object is below
// Z*Y * X^3/3 = (Z*Y*X) * X^2/3 <= 2^64/3 < 2^63, a mixed sum below (Z*Y*X) * (X*Y)/4 <= 2^62, a first moment below 2^48;
// the Euler counter is bounded by 8 elements per corner, |chi| < 2^36.
#include "volume_pass.h"

typedef unsigned short u16;
typedef unsigned long long u64;

#define S3_ACC 10  // n, sum z, sum y, sum x, sum zz, sum yy, sum xx, sum zy, sum zx, sum yx
#define S3_COLS 19

namespace {

// sum of i^2 for 0 <= i < k
__device__ __forceinline__ u64 squares_below(u64 k) { return k ? (k - 1) * k * (2 * k - 1) / 6 : 0; }

// voxels (z, y, xs .. xe - 1) of one label
__device__ __forceinline__ void flush_run(unsigned xs, unsigned xe, unsigned y, unsigned z, u64* acc, unsigned* bmin, unsigned* bmax) {
  const u64 n = xe - xs, sx = n * ((u64)xs + xe - 1) / 2, sxx = squares_below(xe) - squares_below(xs);
  atomicAdd(&acc[0], n); atomicAdd(&acc[1], n * z); atomicAdd(&acc[2], n * y); atomicAdd(&acc[3], sx);
  atomicAdd(&acc[4], n * z * z); atomicAdd(&acc[5], n * y * y); atomicAdd(&acc[6], sxx);
  atomicAdd(&acc[7], n * z * y); atomicAdd(&acc[8], (u64)z * sx); atomicAdd(&acc[9], (u64)y * sx);
  atomicMin(&bmin[0], z); atomicMin(&bmin[1], y); atomicMin(&bmin[2], xs);
  atomicMax(&bmax[0], z); atomicMax(&bmax[1], y); atomicMax(&bmax[2], xe - 1);
}

// m: which voxels of the window p - {0,1}^3 carry the label, bit 4a + 2b + c = voxel (pz - a, py - b, px - c).
// The vertex at p touches all eight; the edge leaving p along x the four with c = 0 (0x55), along y b = 0 (0x33), along z
// a = 0 (0x0f); the face at p normal to z the two with b = c = 0 (0x11), normal to y a = c = 0 (0x05), normal to x
// a = b = 0 (0x03); the cube is voxel p (0x01).
__device__ __forceinline__ int chi_low_side(unsigned m) {
  return 1 - ((m & 0x55u) != 0) - ((m & 0x33u) != 0) - ((m & 0x0fu) != 0) + ((m & 0x11u) != 0) + ((m & 0x05u) != 0) + ((m & 0x03u) != 0) -
         (int)(m & 1u);
}

// labels [F, Z, Y, X]; offsets[f] = first row of stack f; row = offsets[f] + label - 1; bmin / bmax [row][z, y, x]
__global__ __launch_bounds__(256) void k_sizeshape3d(const u16* __restrict__ labels, int F, int Z, int Y, int X, const int* __restrict__ offsets,
                                                     u64* __restrict__ acc, long long* __restrict__ euler, unsigned* __restrict__ bmin,
                                                     unsigned* __restrict__ bmax) {
  __shared__ u16 tile[VP_HZ * VP_HY * VP_HX];
  const size_t vol = (size_t)Z * Y * X;
  const int ntx = X / VP_TX + 1, nty = Y / VP_TY + 1, ntz = Z / VP_TZ + 1;  // tiles of the corner grid, (X + 1) corners per row
  const size_t tiles = (size_t)F * ntz * nty * ntx;
  const int tid = threadIdx.x;
  const int seg = tid & 3, ly = (tid >> 2) & 7, lz = tid >> 5;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const StackIndex tl = stack_index(t, ntz, nty, ntx);
    const int z0 = tl.z * VP_TZ, y0 = tl.y * VP_TY, x0 = tl.x * VP_TX;
    window_stage<true>(tile, labels + (size_t)tl.f * vol, Z, Y, X, z0 - 1, y0 - 1, x0 - 1);
    const int base = offsets[tl.f], nrows = offsets[tl.f + 1] - base;
    const unsigned cz = (unsigned)(z0 + lz), cy = (unsigned)(y0 + ly);
    // rows of the window: r00 = (z, y), r01 = (z, y - 1), r10 = (z - 1, y), r11 = (z - 1, y - 1); voxel x sits at [x - x0 + 1]
    const u16* r00 = tile + ((lz + 1) * VP_HY + (ly + 1)) * VP_HX + seg * VP_RUN;
    const u16* r01 = tile + ((lz + 1) * VP_HY + ly) * VP_HX + seg * VP_RUN;
    const u16* r10 = tile + (lz * VP_HY + (ly + 1)) * VP_HX + seg * VP_RUN;
    const u16* r11 = tile + (lz * VP_HY + ly) * VP_HX + seg * VP_RUN;
    unsigned p00 = r00[0], p01 = r01[0], p10 = r10[0], p11 = r11[0];
    unsigned run = 0, run_x = 0;  // the open run of voxels: label, first x
    unsigned e_lab = 0;           // the open Euler contribution: label, sum
    long long e_sum = 0;
    const unsigned xb = (unsigned)(x0 + seg * VP_RUN);
    for (int c = 0; c < VP_RUN; ++c) {
      const unsigned x = xb + c;
      const unsigned c00 = r00[c + 1], c01 = r01[c + 1], c10 = r10[c + 1], c11 = r11[c + 1];
      if (c00 != run) {
        if (run && (int)run <= nrows) flush_run(run_x, x, cy, cz, acc + (size_t)(base + run - 1) * S3_ACC, bmin + (size_t)(base + run - 1) * 3,
                                                bmax + (size_t)(base + run - 1) * 3);
        run = c00;
        run_x = x;
      }
      const unsigned w[8] = {c00, p00, c01, p01, c10, p10, c11, p11};
      window_labels(w, nrows, [&](unsigned L, unsigned m) {
        const int chi = chi_low_side(m);
        if (!chi) return;
        if (L != e_lab) {
          if (e_lab && e_sum) atomicAdd((u64*)&euler[base + e_lab - 1], (u64)e_sum);
          e_lab = L;
          e_sum = 0;
        }
        e_sum += chi;
      });
      p00 = c00; p01 = c01; p10 = c10; p11 = c11;
    }
    if (run && (int)run <= nrows) flush_run(run_x, xb + VP_RUN, cy, cz, acc + (size_t)(base + run - 1) * S3_ACC, bmin + (size_t)(base + run - 1) * 3,
                                            bmax + (size_t)(base + run - 1) * 3);
    if (e_lab && e_sum) atomicAdd((u64*)&euler[base + e_lab - 1], (u64)e_sum);
  }
}

// n * sum ab - sum a * sum b, exact (|.| < 2^32 * 2^63), as a double
__device__ __forceinline__ double central(u64 n, u64 sab, u64 sa, u64 sb) {
  const unsigned __int128 l = (unsigned __int128)n * sab, r = (unsigned __int128)sa * sb;
  return l >= r ? (double)(l - r) : -(double)(r - l);
}

// one cyclic-Jacobi rotation of the symmetric 3 x 3 matrix a in the (P, Q) plane; R is the third index
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = a[Q][P] = 0.0;
  const double arp = a[R][P], arq = a[R][Q];
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
}

// spacing (dz, dy, dx) enters here and only here
__global__ void k_sizeshape3d_finish(const u64* __restrict__ acc, const long long* __restrict__ euler, const unsigned* __restrict__ bmin,
                                     const unsigned* __restrict__ bmax, int n, double dz, double dy, double dx, double* __restrict__ out, int ld,
                                     int col0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64* a = acc + (size_t)i * S3_ACC;
  double* o = out + (size_t)i * ld + col0;
  if (a[0] == 0) {  // a label without voxels: Volume 0, everything else NaN (as intensity3d)
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int k = 0; k < S3_COLS; ++k) o[k] = nan;
    o[0] = 0.0;
    return;
  }
  const double cnt = (double)a[0], voxel = dz * dy * dx;
  const unsigned* lo = bmin + (size_t)i * 3;
  const unsigned* hi = bmax + (size_t)i * 3;
  const double ez = (double)(hi[0] - lo[0] + 1), ey = (double)(hi[1] - lo[1] + 1), ex = (double)(hi[2] - lo[2] + 1);
  const double volume = cnt * voxel;
  o[0] = volume;
  o[1] = (double)lo[2]; o[2] = (double)lo[1]; o[3] = (double)lo[0];
  o[4] = (double)hi[2] + 1.0; o[5] = (double)hi[1] + 1.0; o[6] = (double)hi[0] + 1.0;
  o[7] = (ez * ey * ex) * voxel;
  o[8] = (double)a[3] / cnt; o[9] = (double)a[2] / cnt; o[10] = (double)a[1] / cnt;  // Center_X / _Y / _Z, voxel indices
  o[11] = cnt / (ez * ey * ex);
  o[12] = cbrt(6.0 * volume / 3.14159265358979323846);
  o[13] = (double)euler[i];
  // population covariance of the scaled coordinates, axes (z, y, x)
  const double n2 = cnt * cnt;
  double c[3][3];
  c[0][0] = central(a[0], a[4], a[1], a[1]) / n2 * (dz * dz);
  c[1][1] = central(a[0], a[5], a[2], a[2]) / n2 * (dy * dy);
  c[2][2] = central(a[0], a[6], a[3], a[3]) / n2 * (dx * dx);
  c[0][1] = c[1][0] = central(a[0], a[7], a[1], a[2]) / n2 * (dz * dy);
  c[0][2] = c[2][0] = central(a[0], a[8], a[1], a[3]) / n2 * (dz * dx);
  c[1][2] = c[2][1] = central(a[0], a[9], a[2], a[3]) / n2 * (dy * dx);
  const double tr = c[0][0] + c[1][1] + c[2][2];
  for (int sweep = 0; sweep < 8; ++sweep) {  // quadratic convergence: a 3 x 3 is at rounding level after 4 - 5 sweeps
    jacobi_rotate<0, 1, 2>(c);
    jacobi_rotate<0, 2, 1>(c);
    jacobi_rotate<1, 2, 0>(c);
  }
  double e0 = c[0][0], e1 = c[1][1], e2 = c[2][2], tmp;  // ascending
  if (e0 > e1) { tmp = e0; e0 = e1; e1 = tmp; }
  if (e1 > e2) { tmp = e1; e1 = e2; e2 = tmp; }
  if (e0 > e1) { tmp = e0; e0 = e1; e1 = tmp; }
  o[14] = sqrt(20.0 * fmax(e2, 0.0));
  o[15] = sqrt(20.0 * fmax(e0, 0.0));
  o[16] = tr - e0; o[17] = tr - e1; o[18] = tr - e2;  // eigenvalues of tr(C) Id - C, descending
}

}  // namespace

extern "C" int aliby_features_sizeshape3d(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host,
                                          const double* spacing, double* out, int ld, int col0, void* stream) {
  ARG_CHECK(ctx && labels && offsets_host && spacing && out, "sizeshape3d: null argument");
  // (see the bounds at the top of the file)
  if (!volume_shape_ok("sizeshape3d", F, Z, Y, X, offsets_host, 1ull << 32)) return ALIBY_ERR_INVALID;
  ARG_CHECK(col0 >= 0 && ld >= col0 + S3_COLS, "sizeshape3d: bad output stride");
  ARG_CHECK(spacing_ok(spacing), "sizeshape3d: spacing must be positive and finite");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);
  const size_t acc_bytes = sizeof(u64) * (size_t)n * (S3_ACC + 1), box_bytes = sizeof(unsigned) * (size_t)n * 3;
  int rc = aliby_ensure_scratch(ctx, acc_bytes + 2 * box_bytes + sizeof(int) * (size_t)(F + 1) + 64);
  if (rc) return rc;
  u64* acc = (u64*)ctx->scratch;
  long long* euler = (long long*)(acc + (size_t)n * S3_ACC);
  unsigned* bmin = (unsigned*)((char*)ctx->scratch + acc_bytes);
  unsigned* bmax = bmin + (size_t)n * 3;
  int* d_off = (int*)(bmax + (size_t)n * 3);
  HIP_TRY(hipMemsetAsync(acc, 0, acc_bytes, s));
  HIP_TRY(hipMemsetAsync(bmin, 0xFF, box_bytes, s));
  HIP_TRY(hipMemsetAsync(bmax, 0, box_bytes, s));
  HIP_TRY(hipMemcpyAsync(d_off, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
  const size_t tiles = (size_t)F * (Z / VP_TZ + 1) * (Y / VP_TY + 1) * (X / VP_TX + 1);
  const unsigned grid = (unsigned)(tiles < 65536 ? tiles : 65536);
  hipLaunchKernelGGL(k_sizeshape3d, dim3(grid), dim3(256), 0, s, labels, F, Z, Y, X, d_off, acc, euler, bmin, bmax);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_sizeshape3d_finish, dim3((n + 255) / 256), dim3(256), 0, s, acc, euler, bmin, bmax, n, spacing[0], spacing[1], spacing[2],
                     out, ld, col0);
  KERNEL_CHECK();
  // the offsets live in ctx scratch: they must be consumed before the host reuses it
  return aliby_wait_stream(s);
}
