// feat_intensity3d_detail.hip — the columns of CellProfiler's MeasureObjectIntensity that feat_intensity3d.hip's single pass of
// atomics cannot give, on the same volume labels [F, Z, Y, X], one channel per call: the five edge statistics, MassDisplacement,
// the quartiles, the median, the MAD and the position of the maximum.  torch.cat([intensity3d, intensity3d_detail], 1) is the 2-D
// `intensity` family's 21 columns plus Volume and Location_Center_*.  An EXTENSION like the other volume families: the 2-D
// definitions (the header of feat_intensity.hip; oracle get_intensity / find_boundaries_inner) applied to an object's voxels in
// raster order (z, y, x); parity with cp_measure is unpinned.  Restated:
//   order statistic at fraction p of the n values v sorted ascending: q = n p, i = floor(q), f = q - i; v[i] (1 - f) + v[i + 1] f
//     if i < n - 1, else v[i]; float64.  LowerQuartile, Median, UpperQuartile: p = 1/4, 1/2, 3/4.
//   MAD: the same rule at p = 1/2 on the sorted |v - median|, the difference taken in float64.
//   edge voxel: a voxel of the object with at least one of its six face neighbours INSIDE the volume carrying another value
//     (0, another label, a label above the stack's count); neighbours outside the volume do not count (replicated border).
//     Integrated, Mean, Std (population), Min, Max over the edge voxels; 0.0 in all five for an object with voxels but no edge
//     voxel (it fills its stack), as in 2-D.
//   MassDisplacement: sqrt((dx dx + dy dy) + dz dz), d = Location_Center - Location_CenterMassIntensity, both as feat_intensity3d
//     computes them (sums, one rounded division each); NaN when the integrated intensity is 0.
//   Location_MaxIntensity_X/Y/Z: the voxel of the maximum, ties to the LAST in raster order.
//   A label of 1..n_f without voxels: NaN in every column (the volume families' convention; the 2-D family writes 0 in the edge
//   columns).  Labels above n_f are not measured.  NaN pixels: unspecified.
//
// Two passes; the first, the split of the rows between the two forms of the second and the kernel's prologue are volume_table.h.
//   1. k_volume_table: voxel count and bounding box per (stack, label), one read of the labels.
//   2. k_intensity3d_detail: one workgroup of 256 lanes per object.  The object's voxels are gathered from its bounding box in
//      raster order by order-preserving compaction (volume_gather of volume_table.h, shared with feat_coloc3d.hip) into ONE
//      list; on the way every voxel's six neighbours are tested and the edge statistics, the centre sums and the last-raster
//      maximum are accumulated per lane.  The list is sorted (bitonic, padded to a power of two with +inf) for the three order
//      statistics, overwritten with |v - median|, and sorted again for the MAD.
//      List element: float for uint16 pixels (the values, and |v - median|, a multiple of 1/2 below 2^16, are exact), double for
//      float32 pixels (|v - median| does not fit a float).  uint16: every sum is an exact 64-bit integer, the edge variance
//      (n sum v^2 - (sum v)^2) / n^2 with a 128-bit numerator, as in feat_intensity3d.hip.  float32: float64 sums, and the edge
//      deviation in a second pass over the list, which a bit per voxel marks the edge voxels of.
//      Lists up to D3_LDS_VOXELS live in LDS (8 bytes x 16384 + the bits = 130 KiB of the CU's 160 at most; the launch asks for
//      what its largest such object needs, so small objects share a CU), longer ones in global scratch (GLOBAL, same code).
// Reproducibility: the workgroup size is fixed, the lane of a voxel is its rank in the object's own bounding box, and the sorts
// and every reduction tree depend on the object's own voxel list only, never on the other objects of the launch, the batch,
// the LDS the launch asked for or which of the two forms ran: rows are bitwise independent of all of them.
#include <type_traits>
#include "common.h"
#include "volume_table.h"

typedef unsigned short u16;
typedef unsigned long long u64;

#define D3_BLOCK 256
#define D3_LDS_VOXELS 16384  // power of two (the sort pads to one)
#define D3_PER_LANE 4        // voxels of the bounding box per lane and compaction round
#define D3_MAX_GRID 4096     // workgroups of the LDS form, at most: the rows beyond take the grid-stride loop
#define D3_NI 10             // integer sums: sum x, y, z; edge count; and for uint16 pixels sum v, x v, y v, z v; edge sum v, v^2
#define D3_NF 5              // float32 only: sum v, x v, y v, z v; edge sum v

namespace {

struct D3Args {
  VolumeArgs v;
  const void* pixels;  // [F,C,Z,Y,X]
  int C, channel, edge;
  int cap;                  // list elements of a workgroup: a power of two >= the largest voxel count of the form
  unsigned char* gscratch;  // GLOBAL: gridDim.x working sets of d3_bytes(cap) bytes
  double* out;
  int ld, col0;
};

// one workgroup's working set: the list, then (float32 pixels) a bit per list element
template <typename T>
__host__ __device__ constexpr size_t d3_bytes(size_t cap) {
  return sizeof(T) == 2 ? cap * 4 : cap * 8 + cap / 8;  // (cap >= 64)
}

// sums of a K-vector of 64-bit integers over the block; every thread gets them.  `lds` holds 4 K entries.
template <int K>
__device__ __forceinline__ void block_sum_vec_i64(long long (&v)[K], long long* lds) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long long s = wave_sum(v[k]);
    if (lane == 0) lds[wid * K + k] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    long long r = 0;
    for (int i = 0; i < D3_BLOCK / 64; ++i) r += lds[i * K + k];
    v[k] = r;
  }
}

// the order statistic at fraction p of sorted[0 .. n), n > 0 (the header's rule); p a multiple of 1/4, so q and f are exact
template <typename E>
__device__ __forceinline__ double order_statistic(const E* sorted, int n, double p) {
  const double q = (double)n * p;
  const int i = (int)q;
  const double f = q - (double)i;
  if (i < n - 1) return (double)sorted[i] * (1.0 - f) + (double)sorted[i + 1] * f;
  return (double)sorted[i];
}

template <typename T, bool GLOBAL>
__global__ __launch_bounds__(D3_BLOCK) void k_intensity3d_detail(D3Args a) {
  constexpr bool U16 = sizeof(T) == 2;
  constexpr int NI = U16 ? D3_NI : 4;
  typedef typename std::conditional<U16, float, double>::type E;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  __shared__ long long veci[4 * D3_NI];
  __shared__ double vecf[4 * D3_NF];
  __shared__ float red_f[8];
  __shared__ int red_i[8];
  __shared__ int wsum[4];
  const int cap = a.cap;
  unsigned char* ws = GLOBAL ? (a.gscratch + (size_t)blockIdx.x * d3_bytes<T>((size_t)cap)) : lds_raw;
  E* list = reinterpret_cast<E*>(ws);
  unsigned* ebits = reinterpret_cast<unsigned*>(ws + (size_t)cap * sizeof(E));  // (float32 pixels only)
  const int tid = threadIdx.x;
  const int Y = a.v.Y, X = a.v.X, Z = a.v.Z;
  const size_t plane = (size_t)Y * X, vol = (size_t)Z * plane;
  const int ncols = a.edge ? 13 : 8;

  for (int it = blockIdx.x; it < a.v.n_items; it += gridDim.x) {
    const int row = volume_row<GLOBAL>(a.v.items, it);
    const unsigned cnt = a.v.count[row];
    if (GLOBAL ? cnt > (unsigned)cap : cnt > (unsigned)D3_LDS_VOXELS) continue;  // (the other form's object; uniform)
    double* out = a.out + (size_t)row * a.ld + a.col0;
    if (cnt == 0) {  // a label without voxels
      if (tid < ncols) out[tid] = NAN;
      continue;
    }
    const int f = volume_stack_of(a.v.offsets, a.v.F, row);
    const u16 L = (u16)(row - a.v.offsets[f] + 1);
    const u16* lab = a.v.labels + (size_t)f * vol;
    const T* px = reinterpret_cast<const T*>(a.pixels) + ((size_t)f * a.C + a.channel) * vol;
    const VolumeBox box = volume_box(a.v.bmin, a.v.bmax, row);

    __syncthreads();  // the previous object's list is done with
    if (!U16 && a.edge)
      for (unsigned i = tid; i < (cnt + 31) / 32; i += D3_BLOCK) ebits[i] = 0;  // (the first barrier of the gather lies before any bit is set)

    // ---- gather (raster order), and per voxel the neighbour test and the lane's accumulators ------------------------------------
    long long si[NI];
    double sf[D3_NF];
#pragma unroll
    for (int k = 0; k < NI; ++k) si[k] = 0;
#pragma unroll
    for (int k = 0; k < D3_NF; ++k) sf[k] = 0.0;
    float emin = INFINITY, emax = -INFINITY, vmax = -INFINITY;
    int imax = -1;  // box index of the lane's last maximum
    const int base = volume_gather<D3_BLOCK, D3_PER_LANE>(lab, L, box, Y, X, wsum, [&](int pos, unsigned i, size_t idx) {
      const unsigned bx = i % box.w, br = i / box.w;
      const unsigned x = box.x0 + bx, y = box.y0 + br % box.h, z = box.z0 + br / box.h;
      const T raw = px[idx];
      const float v = (float)raw;
      if (pos < cap) list[pos] = (E)v;  // (pos < count <= cap: a guard, not a path)
      si[0] += x; si[1] += y; si[2] += z;
      if constexpr (U16) {
        const u64 u = (u64)raw;
        si[4] += u; si[5] += x * u; si[6] += y * u; si[7] += z * u;
      } else {
        const double d = (double)v;
        sf[0] += d; sf[1] += (double)x * d; sf[2] += (double)y * d; sf[3] += (double)z * d;
      }
      if (v >= vmax) { vmax = v; imax = (int)i; }  // (i grows along a lane's walk: the last of equal values stays)
      if (a.edge) {
        const u16* p = lab + idx;
        const bool e = (x > 0 && p[-1] != L) || (x + 1 < (unsigned)X && p[1] != L) || (y > 0 && p[-(ptrdiff_t)X] != L) ||
                       (y + 1 < (unsigned)Y && p[X] != L) || (z > 0 && p[-(ptrdiff_t)plane] != L) || (z + 1 < (unsigned)Z && p[plane] != L);
        if (e) {
          si[3] += 1;
          emin = fminf(emin, v); emax = fmaxf(emax, v);
          if constexpr (U16) {
            const u64 u = (u64)raw;
            si[8] += u; si[9] += u * u;
          } else {
            sf[4] += (double)v;
            if (pos < cap) atomicOr(&ebits[pos >> 5], 1u << (pos & 31));
          }
        }
      }
    });
    __syncthreads();
    const int N = min(base, cap);

    // ---- the lanes' partial results, in a fixed tree ------------------------------------------------------------------------
    block_sum_vec_i64<NI>(si, veci);
    if constexpr (!U16) block_sum_vec_all<D3_NF>(sf, vecf);
    const float gmax = block_max_f32(vmax, red_f);
    const int at = block_max_i32(vmax == gmax ? imax : -1, red_i);  // the largest box index among the maxima: the last in raster order
    if (a.edge) {
      emin = block_min_f32(emin, red_f);
      emax = block_max_f32(emax, red_f);
    }
    const long long ne = si[3];
    double estd = 0.0;
    if (a.edge && ne > 0) {
      if constexpr (U16) {
        const unsigned __int128 num = (unsigned __int128)(u64)ne * (u64)si[9] - (unsigned __int128)(u64)si[8] * (u64)si[8];
        estd = sqrt((double)num / ((double)ne * (double)ne));
      } else {
        const double mean = sf[4] / (double)ne;
        double ss = 0.0;
        for (int j = tid; j < N; j += D3_BLOCK)
          if ((ebits[j >> 5] >> (j & 31)) & 1u) { const double d = (double)list[j] - mean; ss += d * d; }
        estd = sqrt(block_sum_f64(ss, vecf) / (double)ne);
      }
    }
    if (tid == 0) {
      double* o = out;
      if (a.edge) {
        double es;
        if constexpr (U16) es = (double)si[8]; else es = sf[4];
        o[0] = ne ? es : 0.0;
        o[1] = ne ? es / (double)ne : 0.0;
        o[2] = estd;
        o[3] = ne ? (double)emin : 0.0;
        o[4] = ne ? (double)emax : 0.0;
        o += 5;
      }
      double m[4];  // sum v, x v, y v, z v
      bool dark;
      if constexpr (U16) { for (int k = 0; k < 4; ++k) m[k] = (double)si[4 + k]; dark = si[4] == 0; }
      else { for (int k = 0; k < 4; ++k) m[k] = sf[k]; dark = sf[0] == 0.0; }
      const double n = (double)cnt;
      const double dx = (double)si[0] / n - m[1] / m[0], dy = (double)si[1] / n - m[2] / m[0], dz = (double)si[2] / n - m[3] / m[0];
      o[0] = dark ? (double)NAN : sqrt((dx * dx + dy * dy) + dz * dz);
      const unsigned br = (unsigned)at / box.w;
      o[5] = (double)(box.x0 + (unsigned)at % box.w);
      o[6] = (double)(box.y0 + br % box.h);
      o[7] = (double)(box.z0 + br / box.h);
    }

    // ---- the order statistics: sort, read, overwrite with |v - median|, sort again -------------------------------------------
    const int n2 = next_pow2(N);
    for (int i = N + tid; i < n2; i += D3_BLOCK) list[i] = (E)INFINITY;
    block_bitonic_sort(list, n2);
    const double med = order_statistic(list, N, 0.5);
    if (tid == 0) {
      double* o = out + (a.edge ? 5 : 0);
      o[1] = order_statistic(list, N, 0.25);
      o[2] = med;
      o[4] = order_statistic(list, N, 0.75);
    }
    __syncthreads();  // the sorted list has been read
    for (int i = tid; i < N; i += D3_BLOCK) list[i] = (E)fabs((double)list[i] - med);
    block_bitonic_sort(list, n2);
    if (tid == 0) out[(a.edge ? 5 : 0) + 3] = order_statistic(list, N, 0.5);
  }
}

}  // namespace

extern "C" int aliby_intensity3d_detail_lds_voxels(void) { return D3_LDS_VOXELS; }

extern "C" int aliby_features_intensity3d_detail(aliby_ctx* ctx, const uint16_t* labels, const void* pixels, int dtype, int F, int C, int Z, int Y,
                                                 int X, int channel, const int32_t* offsets_host, int edge, double* out, int ld, int col0,
                                                 void* stream) {
  ARG_CHECK(ctx && labels && pixels && offsets_host && out, "intensity3d_detail: null argument");
  ARG_CHECK(dtype == ALIBY_U16 || dtype == ALIBY_F32, "intensity3d_detail: dtype must be ALIBY_U16 or ALIBY_F32");
  // (x, y, z < 65536 and at most 2^30 voxels per object keep every integer sum below 2^63, and a box index in an int)
  if (!volume_shape_ok("intensity3d_detail", F, Z, Y, X, offsets_host, 1ull << 30)) return ALIBY_ERR_INVALID;
  ARG_CHECK(C > 0 && channel >= 0 && channel < C, "intensity3d_detail: channel out of range");
  ARG_CHECK(edge == 0 || edge == 1, "intensity3d_detail: edge must be 0 or 1");
  ARG_CHECK(col0 >= 0 && (long long)col0 + (edge ? 13 : 8) <= ld, "intensity3d_detail: bad output stride");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);
  const bool u16px = dtype == ALIBY_U16;

  // a row is measured by its voxel count; a workgroup of the global-scratch form holds one list of the next power of two (the sort
  // pads to one) of the largest count, and for float32 pixels its bits
  VolumePlan plan;
  const int rc = volume_plan(
      ctx, labels, F, Z, Y, X, offsets_host, nullptr, 0, D3_LDS_VOXELS, [](unsigned count, const unsigned*, const unsigned*) { return (size_t)count; },
      [u16px](size_t max_count) {
        const size_t cap = (size_t)aliby_pow2_at_least((int)max_count, D3_LDS_VOXELS);
        return u16px ? d3_bytes<u16>(cap) : d3_bytes<float>(cap);  // (a multiple of 256)
      },
      1, s, &plan, "intensity3d_detail");
  if (rc) return rc;

  D3Args a;
  a.v = plan.args; a.pixels = pixels; a.C = C; a.channel = channel; a.edge = edge; a.out = out; a.ld = ld; a.col0 = col0;
  hipError_t e = hipSuccess;
  unsigned largest_lds = 1, largest = 1;  // voxel counts: of the rows within the LDS budget, of all rows
  for (int i = 0; i < n; ++i) {
    const unsigned c = plan.host[i];
    if (c <= D3_LDS_VOXELS && c > largest_lds) largest_lds = c;
    if (c > largest) largest = c;
  }
  if (plan.n_big < n) {  // rows within the LDS budget, absent labels included; not launched when every row is of the other form
    a.cap = aliby_pow2_at_least((int)largest_lds, 64); a.gscratch = nullptr;
    const size_t lds = u16px ? d3_bytes<u16>((size_t)a.cap) : d3_bytes<float>((size_t)a.cap);
    e = volume_launch(dtype, k_intensity3d_detail<u16, false>, k_intensity3d_detail<float, false>, a, dim3(std::min(n, D3_MAX_GRID)), D3_BLOCK, lds, s);
  }
  if (e == hipSuccess && plan.n_big) {
    a.v.n_items = plan.n_big; a.gscratch = plan.gscratch;
    a.cap = aliby_pow2_at_least((int)largest, D3_LDS_VOXELS);  // (plan.need = d3_bytes of it)
    e = volume_launch(dtype, k_intensity3d_detail<u16, true>, k_intensity3d_detail<float, true>, a, dim3(plan.grid_big), D3_BLOCK, 0, s);
  }
  if (e != hipSuccess) { aliby_set_error("intensity3d_detail: kernel launch failed: %s", hipGetErrorString(e)); return ALIBY_ERR_HIP; }
  // the table and the offsets live in ctx scratch: they must be consumed before the host reuses it
  return aliby_wait_stream(s);
}
