// feat_relate3d.hip — "relate3d": the `relate` family (feat_relate.hip: CellProfiler's RelateObjects) on volume labels [F, Z, Y, X],
// the 2-D family one dimension up, beside feat_neighbors3d.hip.  PARITY UNPINNED: the definition below is recalled from CellProfiler
// 4's relateobjects.py and identifytertiaryobjects.py and centrosome's outline, and neither library can be run beside this one;
// tests/relate3d_ref.py restates it.
//
// Per stack, A and B are two label volumes of one shape [Z,Y,X] (uint16, 0 = background, labels 1..n_A and 1..n_B from the counts; a
// label may be absent; values above the count are not measured and have no counter).  Row L of A relative to B, the 2-D family's
// five columns:
//   0 Parent              the label p >= 1 of B under the most voxels of L, ties to the smallest p; 0 when no voxel of L lies under a B
//                         label in 1..n_B, or when L is absent
//   1 ParentOverlap       that voxel count, exact; 0 without a parent
//   2 Children count      the B objects whose parent in A, by the same rule with the roles swapped, is L
//   3 Distance_Centroid   centres (sum z, sum y, sum x) / count from exact 64-bit sums and one float64 division each
//                         (neighbors_centre).  With spacing (sz, sy, sx): ez = (pz - cz) sz, ey = (py - cy) sy, ex = (px - cx) sx,
//                         sqrt((ez ez + ey ey) + ex ex), every operation rounded on its own (-ffp-contract=off); NaN without a parent
//   4 Distance_Minimum    the same expression with a voxel (z, y, x) in place of the parent's centre, over the outline voxels of the
//                         parent: reduced with fmin (order-free, exact), then one sqrt; NaN without a parent.  The outline is taken
//                         plane by plane, exactly as neighbors3d defines it: a voxel of p on the first or last row or column of its
//                         plane, or with one of its 8 in-plane neighbours of another value (neighbors_outline on the voxel's plane).
//                         The first and last planes are no borders, and the voxels above and below do not make an outline voxel.
// Consequences:
//   With Z = 1 and spacing (1, 1, 1): cz = pz = 0.0, so ez = 0, 0 + ey ey is exact and a product with 1.0 is exact: every column
//   carries the bits of the 2-D `relate`.
//   Distances are in the units of `spacing` (default 1, 1, 1; positive and finite).  Anisotropic Z is the normal case for stacks.
// The tertiary volume T(outer, inner, shrink_inner): T[q] = outer[q] where inner[q] == 0, or where shrink_inner is set and q is a
// plane-by-plane outline voxel of its inner object; 0 elsewhere.  It keeps outer's labels and counts; a label that loses every voxel
// is absent.  With the plane-wise outline this is aliby_tertiary_labels over the F Z planes of the [F Z, Y, X] view: it has no kernel
// here.  At a nucleus's top and bottom caps the plane-wise rule removes the interior of the cap although cytoplasm lies above (below)
// it: only the cap's in-plane rim is kept.  That is CellProfiler's way of outlining a volume.
// Worked example, a stack [3, 6, 8] (z, y, x), spacing (1, 1, 1).  B = cells: 1 on x 0..3, 2 on x 4..7, every plane and row.
// A = nuclei: 1 on z 0..1, y 1..2, x 1..2; 2 on z 1..2, y 3..4, x 3..4; 3 on z 2, y 0, x 6..7.
//   nucleus  Parent  ParentOverlap  Children  Distance_Centroid  Distance_Minimum
//   1        1       8              1         sqrt(1.25)         sqrt(2.75)
//   2        1       4              1         sqrt(5.25)         sqrt(0.75)    (a tie, 4 voxels in either cell: the smaller label)
//   3        2       2              0         sqrt(8.25)         0.5
//   cell     Parent  ParentOverlap  Children  Distance_Centroid  Distance_Minimum
//   1        1       8              2         sqrt(1.25)         sqrt(0.5)
//   2        2       4              1         sqrt(5.25)         sqrt(2.5)
// Tertiary volumes of cells 1 and 2: 60 and 66 voxels with shrink_inner = 0; 72 and 72 with shrink_inner = 1 (every voxel of these
// 2 x 2 cross-sections is an outline voxel).
// Not built: per-parent means of child measurements, a batched run_positions form.
//
// Launches, all on the caller's stream; the object tables and the plans around them are volume_table.h's (k_volume_table, one read of
// each label volume), the second plan placed behind the first in the context's scratch.
// k_relate3d_overlap<GLOBAL>  once per direction: one workgroup of 256 threads per table row of one set ("self"), striding over the
//                      row's bounding box (VolumeBox) in raster order; the grid is capped at RELATE3D_MAX_GRID workgroups, which
//                      stride over the rows.  The counters are one int per label of the OTHER set's stack, sized from the largest
//                      count of the call: dynamic LDS up to 32 KiB (8191 labels, the 2-D family's rule), else the workgroup's slab of
//                      the context's scratch (at most OBJECT_GLOBAL_BLOCKS workgroups), read back at agent scope: the same bits.  A
//                      thread folds runs of equal labels in its own voxel sequence before the integer atomicAdd (a nucleus inside
//                      one cell: one atomic per thread, not one per voxel).  Then the block argmax, ties to the smallest label, the
//                      three exact coordinate sums and the centre, and one integer atomicAdd on the parent's children counter.
//                      Integers only, apart from the three divisions.
// k_relate3d_finish    after the overlap launches of BOTH directions: one WORKGROUP of 256 threads per row (the 2-D kernel gives a
//                      row a wave; a volume parent's box is 10^4..10^5 voxels), the grid capped likewise.  The threads stride over
//                      the parent's box in the other volume, apply the plane outline predicate and fmin, a wave reduction and a fold
//                      of the four waves' minima follow, and thread 0 writes the five columns.  fmin is exact and order-free: the
//                      choice is invisible in the bits.
// The family uses the context's scratch (tables, per-row workspace, counter slabs): a main-stream call, one in flight per context
// (the scratch rule, object_launch.h); the entry waits for its stream before it returns.  The workgroup sizes are fixed: a row
// carries the same bits whatever the batch, the other stacks of the call, the launch form, the grid and the stream.
#include "common.h"
#include "object_launch.h"
#include "relate_stats.h"
#include "volume_table.h"

typedef unsigned short u16;

#define RELATE3D_BLOCK 256
#define RELATE3D_MAX_GRID 4096                     // workgroups of the LDS-form overlap launch and of the finish launch, at most
#define RELATE3D_LDS_BUDGET OBJECT_LDS_ATTR_ABOVE  // 32 KiB of counters: stacks of up to 8191 labels stay in LDS

namespace {

struct Relate3dArgs {
  VolumeArgs v;              // self: the label volume whose rows the workgroups walk, with its table (v.n_items = its rows)
  const u16* other;          // the volume they are related to
  const int* off_other;      // [F + 1], device: the other table's row offsets
  int n_other, max_count;    // the other table's rows, and its largest stack's: what the counters were sized from
  double* centres;           // [rows, 3] (z, y, x); NaN = absent
  int* parent;               // [rows]
  int* overlap;              // [rows]
  int* children_other;       // [n_other], zeroed before the launch
  size_t need;               // bytes of one workgroup's counters
  unsigned char* gscratch;
};

template <bool GLOBAL>
__global__ __launch_bounds__(RELATE3D_BLOCK) void k_relate3d_overlap(Relate3dArgs a) {
  __shared__ int red_i[8];
  __shared__ long long red_l[8];
  const int tid = threadIdx.x;
  const RelateCounts<GLOBAL> cnt{GLOBAL ? reinterpret_cast<int*>(a.gscratch + (size_t)blockIdx.x * a.need) : nullptr};
  const int Z = a.v.Z, Y = a.v.Y, X = a.v.X;
  for (int row = blockIdx.x; row < a.v.n_items; row += gridDim.x) {
    if (a.v.count[row] == 0) {  // a label without voxels (block-uniform)
      if (tid == 0) relate_absent<3>(a.centres, a.parent, a.overlap, row);
      continue;
    }
    const int f = volume_stack_of(a.v.offsets, a.v.F, row);
    const int L = row - a.v.offsets[f] + 1;
    const size_t stack = (size_t)f * Z * Y * X;
    const u16 *ls = a.v.labels + stack, *lo = a.other + stack;
    const VolumeBox box = volume_box(a.v.bmin, a.v.bmax, row);  // (from the labels themselves: inside the stack)
    const int row0 = max(a.off_other[f], 0), row1 = min(a.off_other[f + 1], a.n_other);
    const int nt = max(0, min(row1 - row0, a.max_count));  // labels of the other set with a counter
    for (int k = tid; k <= nt; k += RELATE3D_BLOCK) cnt.zero(k);
    __syncthreads();

    int n = 0, run_v = 0, run = 0;
    long long sz = 0, sy = 0, sx = 0;
    for (unsigned i = tid; i < box.nbox; i += RELATE3D_BLOCK) {
      const unsigned r = i / box.w;
      const int x = (int)(box.x0 + i % box.w), y = (int)(box.y0 + r % box.h), z = (int)(box.z0 + r / box.h);
      const size_t q = ((size_t)z * Y + y) * X + x;
      if (ls[q] != L) continue;
      ++n;
      sz += z;
      sy += y;
      sx += x;
      int v = lo[q];
      if (v > nt) v = 0;
      if (v != run_v) {  // (the 2-D kernel's run folding: relate_stats.h says why it is written out here)
        if (run_v) cnt.add(run_v, run);
        run_v = v;
        run = 0;
      }
      ++run;
    }
    if (run_v) cnt.add(run_v, run);
    __syncthreads();

    int best = 0, best_l = INT_MAX;
    for (int v = 1 + tid; v <= nt; v += RELATE3D_BLOCK) {  // ascending per thread: a later label wins only with a larger count
      const int c = cnt.get(v);
      if (c > best) { best = c; best_l = v; }
    }
    const int top = block_max_i32(best, red_i);
    const int p = block_min_i32(best == top && top > 0 ? best_l : INT_MAX, red_i);
    n = block_sum_i32(n, red_i);
    sz = block_sum_i64(sz, red_l);
    sy = block_sum_i64(sy, red_l);
    sx = block_sum_i64(sx, red_l);
    if (tid == 0) {
      if (n == 0) {  // (cannot happen with a table counted from these labels; kept as the 2-D kernel keeps it)
        relate_absent<3>(a.centres, a.parent, a.overlap, row);
      } else {
        double* ctr = a.centres + 3 * (size_t)row;
        ctr[0] = neighbors_centre(sz, n);
        ctr[1] = neighbors_centre(sy, n);
        ctr[2] = neighbors_centre(sx, n);
        relate_parent_write(a.parent, a.overlap, a.children_other, row, row0, top, p);
      }
    }
    __syncthreads();  // the counters are read before the next row clears them
  }
}

struct Relate3dFinishArgs {
  VolumeArgs v;      // self's offsets and rows (its labels are not read)
  VolumeArgs other;  // the other volume with its table: the parents' boxes
  const double *centres, *centres_other;
  const int *parent, *overlap, *children;
  double sz, sy, sx;
  double* out;
  int ld, col0;
};

__global__ __launch_bounds__(RELATE3D_BLOCK) void k_relate3d_finish(Relate3dFinishArgs a) {
  __shared__ double red_d[RELATE3D_BLOCK / WAVE];
  const int tid = threadIdx.x;
  const int Y = a.other.Y, X = a.other.X;
  for (int row = blockIdx.x; row < a.v.n_items; row += gridDim.x) {
    const int p = a.parent[row];  // (block-uniform)
    double d_centre = NAN, d_min = NAN;
    const int f = volume_stack_of(a.v.offsets, a.v.F, row);
    const int j = max(a.other.offsets[f], 0) + p - 1;
    if (p > 0 && j < a.other.n_items && a.other.count[j] > 0) {
      const double cz = a.centres[3 * (size_t)row], cy = a.centres[3 * (size_t)row + 1], cx = a.centres[3 * (size_t)row + 2];
      const double pz = a.centres_other[3 * (size_t)j], py = a.centres_other[3 * (size_t)j + 1], px = a.centres_other[3 * (size_t)j + 2];
      const double dz = (pz - cz) * a.sz, dy = (py - cy) * a.sy, dx = (px - cx) * a.sx;
      d_centre = sqrt((dz * dz + dy * dy) + dx * dx);
      const u16* lab = a.other.labels + (size_t)f * a.other.Z * Y * X;
      const VolumeBox box = volume_box(a.other.bmin, a.other.bmax, j);
      double best = INFINITY;
      for (unsigned i = tid; i < box.nbox; i += RELATE3D_BLOCK) {
        const unsigned r = i / box.w;
        const int x = (int)(box.x0 + i % box.w), y = (int)(box.y0 + r % box.h), z = (int)(box.z0 + r / box.h);
        const u16* plane = lab + (size_t)z * Y * X;
        if (plane[(size_t)y * X + x] != p || !neighbors_outline(plane, Y, X, y, x, p)) continue;
        const double ez = ((double)z - cz) * a.sz, ey = ((double)y - cy) * a.sy, ex = ((double)x - cx) * a.sx;
        best = fmin(best, (ez * ez + ey * ey) + ex * ex);
      }
      best = wave_reduce_dpp(best, (double)INFINITY, [](double u, double v) { return fmin(u, v); });
      __syncthreads();  // the previous row's minima have been read
      if ((tid & (WAVE - 1)) == WAVE - 1) red_d[tid / WAVE] = best;
      __syncthreads();
      for (int w = 0; w < RELATE3D_BLOCK / WAVE; ++w) best = w == 0 ? red_d[0] : fmin(best, red_d[w]);
      d_min = sqrt(best);
    }
    if (tid == 0) relate_row_write(a.out + (size_t)row * a.ld + a.col0, p, a.overlap[row], a.children[row], d_centre, d_min);
  }
}

int relate3d_overlap_launch(aliby_ctx* ctx, const VolumePlan& self, const VolumePlan& other, int max_count_other, const RelateSide& mine,
                            const RelateSide& theirs, unsigned char* slabs, hipStream_t s) {
  if (self.n == 0) return ALIBY_OK;
  Relate3dArgs a;
  a.v = self.args; a.other = other.args.labels; a.off_other = other.args.offsets; a.n_other = other.n; a.max_count = max_count_other;
  a.centres = mine.centres; a.parent = mine.parent; a.overlap = mine.overlap; a.children_other = theirs.children;
  a.need = relate_counter_bytes(max_count_other);
  if (a.need <= RELATE3D_LDS_BUDGET) {
    a.gscratch = nullptr;
    hipLaunchKernelGGL(k_relate3d_overlap<false>, dim3(std::min(self.n, RELATE3D_MAX_GRID)), dim3(RELATE3D_BLOCK), a.need, s, a);
  } else {
    a.gscratch = slabs;
    hipLaunchKernelGGL(k_relate3d_overlap<true>, dim3(std::min(self.n, OBJECT_GLOBAL_BLOCKS)), dim3(RELATE3D_BLOCK), 0, s, a);
  }
  KERNEL_CHECK();
  return ALIBY_OK;
}

void relate3d_finish_launch(const VolumePlan& self, const VolumePlan& other, const RelateSide& mine, const RelateSide& theirs,
                            const double* spacing, double* out, int ld, int col0, hipStream_t s) {
  if (self.n == 0 || out == nullptr) return;
  Relate3dFinishArgs a;
  a.v = self.args; a.other = other.args; a.centres = mine.centres; a.centres_other = theirs.centres; a.parent = mine.parent;
  a.overlap = mine.overlap; a.children = mine.children; a.sz = spacing[0]; a.sy = spacing[1]; a.sx = spacing[2];
  a.out = out; a.ld = ld; a.col0 = col0;
  hipLaunchKernelGGL(k_relate3d_finish, dim3(std::min(self.n, RELATE3D_MAX_GRID)), dim3(RELATE3D_BLOCK), 0, s, a);
}

// a plan without rows: the shape, the labels and a device offsets array are all the other side's kernels read of it
int relate3d_plan(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host, size_t base, hipStream_t s,
                  VolumePlan* p) {
  if (offsets_host[F] > 0)
    return volume_plan(
        ctx, labels, F, Z, Y, X, offsets_host, nullptr, 0, ~(size_t)0, [](unsigned count, const unsigned*, const unsigned*) { return (size_t)count; },
        [](size_t) { return (size_t)0; }, 1, s, p, "relate3d", base);
  int* d_off = (int*)((unsigned char*)ctx->scratch + base);
  HIP_TRY(hipMemsetAsync(d_off, 0, sizeof(int) * (size_t)(F + 1), s));
  p->n = 0;
  p->args = VolumeArgs{labels, F, Z, Y, X, d_off, nullptr, nullptr, nullptr, nullptr, 0};
  return ALIBY_OK;
}

}  // namespace

extern "C" int aliby_features_relate3d(aliby_ctx* ctx, const uint16_t* vol_a, const uint16_t* vol_b, int F, int Z, int Y, int X,
                                       const int32_t* offsets_a, const int32_t* offsets_b, const double* spacing, double* out_a, int ld_a,
                                       int col0_a, double* out_b, int ld_b, int col0_b, void* stream) {
  ARG_CHECK(ctx && vol_a && vol_b && offsets_a && offsets_b && spacing, "relate3d: null argument");
  if (!volume_shape_ok("relate3d (a)", F, Z, Y, X, offsets_a, 1ull << 30) || !volume_shape_ok("relate3d (b)", F, Z, Y, X, offsets_b, 1ull << 30))
    return ALIBY_ERR_INVALID;
  ARG_CHECK(spacing_ok(spacing), "relate3d: spacing must be positive and finite");
  ARG_CHECK(out_a == nullptr || (col0_a >= 0 && (long long)col0_a + 5 <= ld_a), "relate3d: columns exceed row stride (a)");
  ARG_CHECK(out_b == nullptr || (col0_b >= 0 && (long long)col0_b + 5 <= ld_b), "relate3d: columns exceed row stride (b)");
  const int n_a = offsets_a[F], n_b = offsets_b[F];
  if (n_a == 0 && n_b == 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);

  int max_a = 0, max_b = 0;  // (<= 65535: volume_offsets_ok)
  for (int f = 0; f < F; ++f) {
    max_a = std::max(max_a, offsets_a[f + 1] - offsets_a[f]);
    max_b = std::max(max_b, offsets_b[f + 1] - offsets_b[f]);
  }
  // The scratch of the call, sized before the first plan so that no later request moves the block: [plan a][plan b][side a][side b]
  // [counter slabs of the scratch form], each 256-byte aligned.  The two overlap launches run one after the other on the stream and
  // share the slabs.
  const auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t head_a = n_a ? volume_plan_head_bytes(n_a, F, 0) : align(sizeof(int) * (size_t)(F + 1));
  const size_t head_b = n_b ? volume_plan_head_bytes(n_b, F, 0) : align(sizeof(int) * (size_t)(F + 1));
  const size_t side_a = align(relate_side_bytes<3>(n_a)), side_b = align(relate_side_bytes<3>(n_b));
  size_t slab_bytes = 0;  // workgroups x counters, the larger of the two directions
  if (n_a && relate_counter_bytes(max_b) > RELATE3D_LDS_BUDGET) slab_bytes = (size_t)std::min(n_a, OBJECT_GLOBAL_BLOCKS) * relate_counter_bytes(max_b);
  if (n_b && relate_counter_bytes(max_a) > RELATE3D_LDS_BUDGET)
    slab_bytes = std::max(slab_bytes, (size_t)std::min(n_b, OBJECT_GLOBAL_BLOCKS) * relate_counter_bytes(max_a));
  int rc = aliby_ensure_scratch(ctx, head_a + head_b + side_a + side_b + slab_bytes);
  if (rc) return rc;

  VolumePlan pa, pb;
  rc = relate3d_plan(ctx, vol_a, F, Z, Y, X, offsets_a, 0, s, &pa);
  if (rc) return rc;
  rc = relate3d_plan(ctx, vol_b, F, Z, Y, X, offsets_b, head_a, s, &pb);
  if (rc) return rc;
  unsigned char* base = (unsigned char*)ctx->scratch + head_a + head_b;
  const RelateSide sa = relate_side<3>(base, n_a), sb = relate_side<3>(base + side_a, n_b);
  unsigned char* slabs = base + side_a + side_b;
  if (n_a) HIP_TRY(hipMemsetAsync(sa.children, 0, (size_t)n_a * sizeof(int), s));
  if (n_b) HIP_TRY(hipMemsetAsync(sb.children, 0, (size_t)n_b * sizeof(int), s));
  rc = relate3d_overlap_launch(ctx, pa, pb, max_b, sa, sb, slabs, s);
  if (rc) return rc;
  rc = relate3d_overlap_launch(ctx, pb, pa, max_a, sb, sa, slabs, s);
  if (rc) return rc;
  relate3d_finish_launch(pa, pb, sa, sb, spacing, out_a, ld_a, col0_a, s);
  KERNEL_CHECK();
  relate3d_finish_launch(pb, pa, sb, sa, spacing, out_b, ld_b, col0_b, s);
  KERNEL_CHECK();
  // the tables, the workspace and the slabs live in ctx scratch: they must be consumed before the host reuses it
  return aliby_wait_stream(s);
}
