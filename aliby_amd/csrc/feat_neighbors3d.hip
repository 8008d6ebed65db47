// feat_neighbors3d.hip — "neighbors3d": the `neighbors` family (feat_neighbors.hip: CellProfiler's MeasureObjectNeighbors with the
// objects as their own neighbours) on volume labels [F, Z, Y, X], the fifth volume family beside feat_intensity3d.hip,
// feat_sizeshape3d.hip, feat_coloc3d.hip and feat_texture3d.hip.  PARITY UNPINNED: the definition below is recalled from
// CellProfiler 4's measureobjectneighbors.py and centrosome's outline / strel_disk, and neither library can be run beside this
// one; tests/neighbors3d_ref.py restates it.
//
// One stack [Z,Y,X] (labels 1..n, 0 = background), an object L, an integer distance d in 1..16:
//   S = the offsets with dz^2 + dy^2 + dx^2 <= d^2      (skimage.morphology.ball(d); the 6-neighbour cross for d = 1)
//   T = the offsets with dz^2 + dy^2 + dx^2 <= d^2 + d  (the integer-offset form of radius d + 0.5; the 18-neighbourhood for d = 1)
//   offsets that leave the volume are dropped (no wrap, no padding value)
//   outline of L, plane by plane as CellProfiler outlines a volume: its voxels on the first or last row or column of their plane, or
//   with one of the 8 in-plane neighbours of another value (0 included).  The first and last planes are no borders, and the voxels
//   above and below do not make an outline voxel.
// Seven columns, the 2-D family's:
//   0 NumberOfNeighbors         distinct labels v not in {0, L}, v <= n, at q + o for a voxel q of L and an o in S
//   1 PercentTouching           double(t) / double(p) * 100, p = outline voxels of L, t = those with a non-zero value other than L
//                               at q + o for an o in T (a value above n counts here, as in 2-D)
//   2 FirstClosestObjectNumber  3 FirstClosestDistance  4 SecondClosestObjectNumber  5 SecondClosestDistance
//                               centres (sum z, sum y, sum x) / count: exact 64-bit sums, one float64 division each.  Candidates
//                               are the other present labels of the stack, ranked by (dz dz + dy dy) + dx dx in float64 (every
//                               operation rounded on its own: -ffp-contract=off), ties to the lower label; the distance is sqrt of
//                               the key.  Without a first candidate columns 2-3 are 0, without a second columns 4-6 are 0.
//   6 AngleBetweenNeighbors     atan2(|v1 x v2|, v1 . v2) 180 / pi with the 3-D cross product, for the vectors from L's centre to
//                               the two centres; NaN when one of them is zero (the 2-D family's deliberate departure from
//                               CellProfiler's arccos).
// A label of 1..n without voxels gets NaN in all seven columns and is neither a neighbour nor a candidate; labels above n are not
// measured.  Voxel spacing is not used.  On a stack of one plane every column is the 2-D family's.
// Not built: "Expand until adjacent" (its nearest-label fill rests on EDT index ties), neighbours from a second object set,
// physical-unit (anisotropic) balls.
//
// Three launches; the first and the plan around it are volume_table.h, shared with feat_coloc3d.hip and feat_texture3d.hip.
//   1. k_volume_table: voxel count and bounding box per (stack, label), one read of the labels.  The plan is asked with an LDS limit
//      that no row exceeds: the family has no global-scratch form.
//   2. k_neighbors3d_scan: one workgroup of 256 threads per table row, striding over the row's bounding box in raster order.  A
//      voxel of L walks the offsets of T, generated plane by plane from the integer inequalities and clamped to the volume, and
//      reads the labels from global memory (the windows of neighbouring lanes overlap almost entirely: cache hits).  A foreign
//      non-zero value sets the lane's touching flag, and, where the offset is in S too and v <= n, its bit in an LDS bitmap of one
//      bit per label of the stack (atomicOr on 32-bit words; at most 8 KiB, sized by the largest stack of the call), behind the 2-D
//      kernel's two filters: the last label set, and a test of the bit before the atomic.  Then: popcount of the bitmap, integer
//      block reductions of p, t, the count and the three coordinate sums, columns 0-1 and the centre into centres_dev [rows, 3].
//   3. k_neighbors_closest<3> (neighbors_stats.h, the 2-D family's kernel): one wave per row.  The lanes stride over the centres of
//      the row's own stack (a NaN centre = absent), each keeps its two best (key, label) pairs, and a butterfly merges them under the
//      order "lower key, then lower label": a total order on distinct labels, so the result is the same whichever lane saw a row.  Columns 2-6.
// The object table lives in the context's scratch, so this is a main-stream family: one such call in flight per context (the
// scratch rule, object_launch.h); the entry waits for its stream before it returns.
// Everything but sqrt and atan2 is integer or a single rounded float64 operation, and the workgroup size is fixed: a row carries
// the same bits whatever the batch, the other stacks of the call, the grid and the stream.
#include "common.h"
#include "neighbors_stats.h"
#include "volume_table.h"

typedef unsigned short u16;

#define N3_BLOCK 256
#define NEIGHBORS3D_MAX_DISTANCE 16  // bounds the per-voxel scan (a ball of radius 16.5: about 19 k offsets); not a structural limit

namespace {

struct N3Args {
  VolumeArgs v;
  int max_count;    // the largest stack's rows: what the bitmap was sized from
  int d;
  double* centres;  // [rows, 3] (z, y, x)
  double* out;
  int ld, col0;
  __device__ __forceinline__ int rows() const { return v.n_items; }
  __device__ __forceinline__ bool stack_rows(int row, int& lo, int& hi) const {  // k_neighbors_closest: found in the offsets
    const int f = volume_stack_of(v.offsets, v.F, row);
    lo = max(v.offsets[f], 0); hi = min(v.offsets[f + 1], v.n_items);
    return true;
  }
};

// the largest w >= 0 with w * w <= r, for 0 <= r <= 16^2 + 16 (exact: float sqrt is within one of it)
__device__ __forceinline__ int n3_isqrt(int r) {
  int w = (int)sqrtf((float)r);
  if (w * w > r) --w;
  if ((w + 1) * (w + 1) <= r) ++w;
  return w;
}

__global__ __launch_bounds__(N3_BLOCK) void k_neighbors3d_scan(N3Args a) {
  __shared__ int red_i[8];
  __shared__ long long red_l[8];
  const int row = blockIdx.x, tid = threadIdx.x;
  double* out = a.out + (size_t)row * a.ld + a.col0;
  double* ctr = a.centres + 3 * (size_t)row;
  if (a.v.count[row] == 0) {  // a label without voxels
    if (tid == 0) neighbors_absent<3>(out, ctr);
    return;
  }
  const int Z = a.v.Z, Y = a.v.Y, X = a.v.X;
  const int f = volume_stack_of(a.v.offsets, a.v.F, row);
  const int L = row - a.v.offsets[f] + 1;
  const u16* lab = a.v.labels + (size_t)f * Z * Y * X;
  const VolumeBox box = volume_box(a.v.bmin, a.v.bmax, row);
  const NeighborsBitmap<N3_BLOCK> bm{max(0, min(a.v.offsets[f + 1] - a.v.offsets[f], a.max_count))};
  bm.clear();

  const int d = a.d, s2 = d * d, t2 = s2 + d;
  int n = 0, outline = 0, touching = 0, last_set = 0;
  long long sz = 0, sy = 0, sx = 0;
  for (unsigned i = tid; i < box.nbox; i += N3_BLOCK) {
    const unsigned r = i / box.w;
    const int x = (int)(box.x0 + i % box.w), y = (int)(box.y0 + r % box.h), z = (int)(box.z0 + r / box.h);
    if (lab[((size_t)z * Y + y) * X + x] != L) continue;
    ++n;
    sz += z;
    sy += y;
    sx += x;
    bool edge = y == 0 || y == Y - 1 || x == 0 || x == X - 1, touch = false;
    const int za = max(z - d, 0), zb = min(z + d, Z - 1), ya = max(y - d, 0), yb = min(y + d, Y - 1);
    for (int zz = za; zz <= zb; ++zz) {
      const int dz = zz - z, rtz = t2 - dz * dz, rsz = s2 - dz * dz;  // dy^2 + dx^2 <= rtz: in T (rtz >= d > 0); <= rsz: in S
      const bool plane = dz == 0;
      for (int yy = ya; yy <= yb; ++yy) {
        const int dy = yy - y, rt = rtz - dy * dy, rs = rsz - dy * dy;  // dx^2 <= rt: in T; <= rs: in S
        if (rt < 0) continue;
        const int wx = n3_isqrt(rt);
        const int xa = max(x - wx, 0), xb = min(x + wx, X - 1);
        const u16* line = lab + ((size_t)zz * Y + yy) * X;
        const bool near_y = plane && dy >= -1 && dy <= 1;
        for (int xx = xa; xx <= xb; ++xx) {
          const int v = line[xx];
          if (v == L) continue;
          const int dx = xx - x;
          if (near_y && dx >= -1 && dx <= 1) edge = true;  // (the in-plane 3 x 3 square lies inside T for every d >= 1)
          if (v == 0) continue;
          touch = true;
          bm.mark(dx * dx <= rs, v, last_set);
        }
      }
    }
    outline += edge;
    touching += edge && touch;
  }
  __syncthreads();
  const int cnt = block_sum_i32(bm.popcount(), red_i);
  n = block_sum_i32(n, red_i); outline = block_sum_i32(outline, red_i); touching = block_sum_i32(touching, red_i);
  sz = block_sum_i64(sz, red_l); sy = block_sum_i64(sy, red_l); sx = block_sum_i64(sx, red_l);
  if (tid == 0) neighbors_scan_write(out, ctr, cnt, n, outline, touching, sz, sy, sx);
}

}  // namespace

extern "C" int aliby_features_neighbors3d(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host,
                                          int distance, double* centres_dev, double* out, int ld, int col0, void* stream) {
  ARG_CHECK(ctx && labels && offsets_host && centres_dev && out, "neighbors3d: null argument");
  if (!volume_shape_ok("neighbors3d", F, Z, Y, X, offsets_host, 1ull << 30)) return ALIBY_ERR_INVALID;
  ARG_CHECK(distance >= 1 && distance <= NEIGHBORS3D_MAX_DISTANCE, "neighbors3d: distance must lie in 1..16");
  ARG_CHECK(col0 >= 0 && (long long)col0 + 7 <= ld, "neighbors3d: bad output stride");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);

  // every row is of the LDS form (the limit is one no row exceeds): the plan is the table, the offsets and nothing else
  VolumePlan plan;
  const int rc = volume_plan(
      ctx, labels, F, Z, Y, X, offsets_host, nullptr, 0, ~(size_t)0, [](unsigned count, const unsigned*, const unsigned*) { return (size_t)count; },
      [](size_t) { return (size_t)0; }, 1, s, &plan, "neighbors3d");
  if (rc) return rc;

  N3Args a;
  a.v = plan.args; a.d = distance; a.centres = centres_dev; a.out = out; a.ld = ld; a.col0 = col0;
  a.max_count = 0;
  for (int f = 0; f < F; ++f) a.max_count = std::max(a.max_count, offsets_host[f + 1] - offsets_host[f]);  // <= 65535 (volume_offsets_ok)
  hipLaunchKernelGGL(k_neighbors3d_scan, dim3(n), dim3(N3_BLOCK), neighbors_bitmap_bytes(a.max_count), s, a);
  KERNEL_CHECK();
  neighbors_closest_launch<3>(a, n, s);
  KERNEL_CHECK();
  // the table and the offsets live in ctx scratch: they must be consumed before the host reuses it
  return aliby_wait_stream(s);
}
