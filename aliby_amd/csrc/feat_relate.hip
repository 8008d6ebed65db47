// feat_relate.hip — "relate": two object sets of one tile read together.  CellProfiler's RelateObjects (parent, children count,
// centroid and minimum distances) and IdentifyTertiaryObjects (the cytoplasm: cell minus nucleus).  PARITY UNPINNED: the definition
// below is recalled from CellProfiler 4's relateobjects.py and identifytertiaryobjects.py and centrosome's outline, and neither
// library can be run beside this one; tests/relate_ref.py restates it.
//
// Per tile, A and B are two label images of one shape [Y,X] (uint16, 0 = background, labels 1..n_A and 1..n_B; a label may be
// absent: area 0).  Row L of A relative to B, five columns:
//   0 Parent              the label p >= 1 of B that covers the most pixels of L, ties to the smallest p; 0 when no pixel of L has a
//                         non-zero B label, or when L is absent
//   1 ParentOverlap       that pixel count, exact; 0 without a parent (an extension: the number column 0 is the argmax of)
//   2 Children count      the B objects whose parent in A, by the same rule with the roles swapped, is L
//   3 Distance_Centroid   between the centre of L and the centre of its parent: centres (sum y / area, sum x / area) from exact 64-bit
//                         sums and one float64 division each (neighbors_centre), dy = py - cy, dx = px - cx, sqrt(dy dy + dx dx);
//                         NaN without a parent
//   4 Distance_Minimum    from the centre of L to the centre of the nearest outline pixel (y, x) of its parent: dy = y - cy,
//                         dx = x - cx, the minimum of dy dy + dx dx over the outline pixels (order-free), then one sqrt; NaN without a
//                         parent.  Outline = the `neighbors` family's (neighbors_outline): on the first or last row or column of
//                         the tile, or with an 8-neighbour of another value.
// The tertiary image T(outer, inner, shrink_inner): T[q] = outer[q] where inner[q] == 0, or where shrink_inner is set and q is an
// outline pixel of its inner object; 0 elsewhere.  It keeps outer's labels, removes the interior of ANY inner object, and a label
// that loses all its pixels is simply absent.
// Not built: per-parent means of child measurements, a batched run_positions form.  (Volume labels: feat_relate3d.hip, which shares
// the counters, the absent row, the children atomic, the row write and the workspace layout with this file: relate_stats.h.  The run
// folding and the argmax loop are written out in either overlap kernel: as shared functions they changed this kernel's code.)
//
// k_relate_overlap<GLOBAL>  one workgroup per object of one set ("self"), threads striding over its box (object_launch.h's two forms).
//                      The working set is one int per label of the OTHER set's tile (sized from the largest tile's count: no cap on
//                      how many objects one object may meet): dynamic LDS up to 32 KiB (8191 labels), else the workgroup's slab of
//                      ctx->scratch.  A thread folds runs of equal labels in its own pixel sequence before the integer atomicAdd
//                      (a nucleus inside one cell: one atomic per thread, not one per pixel).  Then the argmax, ties to the smallest
//                      label (block max of the count, block min of the labels that reach it), the centre, and one integer atomicAdd
//                      on the parent's children counter.  Integers only; the centre is two single divisions.
// k_relate_finish      after the overlap launches of BOTH directions on the same stream: one wave per row.  The lanes stride over the
//                      parent's box in the other label image, take the minimum squared distance over its outline pixels (fmin: exact
//                      and order-free) and lane 0 writes the five columns.
// k_tertiary_vec       one pass over [F,Y,X]: 2 reads + 1 write x 2 B per pixel = 6 B per pixel of algorithmic traffic, a pure
//                      bandwidth kernel.  Eight pixels (16 B) per thread where X is a multiple of 8 and the three images are 16-byte
//                      aligned; a workgroup covers 8 rows x 256 pixels.  A group without an inner pixel (most of a tile) is copied
//                      without looking at rows y +- 1; the others load those rows as two more 16-byte reads and six single pixels
//                      (L1 / L2 hits for six rows of eight: no LDS halo) and evaluate the stencil in registers.
// k_tertiary_scalar    the same image one pixel per thread, for any width and alignment.
// A row carries the same bits whatever the batch, the launch form, the workgroup size and the stream.
#include "common.h"
#include "object_launch.h"
#include "relate_stats.h"

typedef unsigned short u16;

#define RELATE_LDS_BUDGET OBJECT_LDS_ATTR_ABOVE  // 32 KiB of counters: tiles of up to 8191 labels stay in LDS, no attribute call
#define RELATE_FINISH_BLOCK 256                  // k_relate_finish: one wave per row

struct RelateArgs {
  const u16* self;   // the label image whose objects the workgroups walk
  const u16* other;  // the one they are related to
  int F, Y, X;
  const aliby_object* tab;  // self's table
  int n_obj;
  const int32_t* off_other;  // [F + 1], device: the other table's row offsets
  int n_other, max_count;    // the other table's rows, and its largest tile's: what the counters were sized from
  double* centres;           // [n_obj, 2] (y, x); NaN = absent
  int* parent;               // [n_obj]
  int* overlap;              // [n_obj]
  int* children_other;       // [n_other], zeroed before the launch
  size_t need;               // bytes of one workgroup's counters
  unsigned char* gscratch;
};

template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_relate_overlap(RelateArgs a) {
  __shared__ int red_i[8];
  __shared__ long long red_l[8];
  const int tid = threadIdx.x;
  const RelateCounts<GLOBAL> cnt{GLOBAL ? reinterpret_cast<int*>(a.gscratch + (size_t)blockIdx.x * a.need) : nullptr};
  for (int oi = blockIdx.x; oi < a.n_obj; oi += gridDim.x) {  // (LDS form: one object per workgroup)
    const aliby_object o = a.tab[oi];
    double* ctr = a.centres + 2 * (size_t)oi;
    const int y0 = max(o.y0, 0), y1 = min(o.y1, a.Y), x0 = max(o.x0, 0), x1 = min(o.x1, a.X);
    if (o.area <= 0 || o.tile < 0 || o.tile >= a.F || y0 >= y1 || x0 >= x1) {  // (block-uniform)
      if (tid == 0) relate_absent<2>(a.centres, a.parent, a.overlap, oi);
      continue;
    }
    const int X = a.X, h = y1 - y0, w = x1 - x0, L = o.label;
    const size_t plane = (size_t)o.tile * a.Y * X;
    const u16 *ls = a.self + plane, *lo = a.other + plane;
    const int row0 = max(a.off_other[o.tile], 0), row1 = min(a.off_other[o.tile + 1], a.n_other);
    const int nt = max(0, min(row1 - row0, a.max_count));  // labels of the other set with a counter; above it: a wrong table, not counted
    for (int k = tid; k <= nt; k += blockDim.x) cnt.zero(k);
    __syncthreads();

    int n = 0, run_v = 0, run = 0;
    long long sy = 0, sx = 0;
    for (int i = tid; i < h * w; i += blockDim.x) {
      const int y = y0 + i / w, x = x0 + i % w;
      const size_t q = (size_t)y * X + x;
      if (ls[q] != L) continue;
      ++n;
      sy += y;
      sx += x;
      int v = lo[q];
      if (v > nt) v = 0;
      if (v != run_v) {
        if (run_v) cnt.add(run_v, run);
        run_v = v;
        run = 0;
      }
      ++run;
    }
    if (run_v) cnt.add(run_v, run);
    __syncthreads();

    int best = 0, best_l = INT_MAX;
    for (int v = 1 + tid; v <= nt; v += blockDim.x) {  // ascending per thread: a later label wins only with a larger count
      const int c = cnt.get(v);
      if (c > best) { best = c; best_l = v; }
    }
    const int top = block_max_i32(best, red_i);
    const int p = block_min_i32(best == top && top > 0 ? best_l : INT_MAX, red_i);
    n = block_sum_i32(n, red_i);
    sy = block_sum_i64(sy, red_l);
    sx = block_sum_i64(sx, red_l);
    if (tid == 0) {
      if (n == 0) {  // (a row whose area the labels do not bear out: absent)
        relate_absent<2>(a.centres, a.parent, a.overlap, oi);
      } else {
        ctr[0] = neighbors_centre(sy, n);
        ctr[1] = neighbors_centre(sx, n);
        relate_parent_write(a.parent, a.overlap, a.children_other, oi, row0, top, p);  // (p <= nt <= row1 - row0: inside the other table)
      }
    }
    __syncthreads();  // the counters are read before the next object clears them
  }
}

struct RelateFinishArgs {
  const u16* other;
  int F, Y, X;
  const aliby_object* tab;  // self's table
  int n_obj;
  const aliby_object* tab_other;
  const int32_t* off_other;
  int n_other;
  const double *centres, *centres_other;
  const int *parent, *overlap, *children;
  double* out;
  int ld, col0;
};

__global__ __launch_bounds__(RELATE_FINISH_BLOCK) void k_relate_finish(RelateFinishArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int row = blockIdx.x * (RELATE_FINISH_BLOCK / WAVE) + threadIdx.x / WAVE;  // wave-uniform
  if (row >= a.n_obj) return;
  const int p = a.parent[row], tile = a.tab[row].tile;
  double d_centre = NAN, d_min = NAN;
  if (p > 0 && tile >= 0 && tile < a.F) {
    const int j = max(a.off_other[tile], 0) + p - 1;
    if (j < a.n_other) {
      const aliby_object ob = a.tab_other[j];
      const double cy = a.centres[2 * (size_t)row], cx = a.centres[2 * (size_t)row + 1];
      const double py = a.centres_other[2 * (size_t)j], px = a.centres_other[2 * (size_t)j + 1];
      const double dy = py - cy, dx = px - cx;
      d_centre = sqrt(dy * dy + dx * dx);
      const int Y = a.Y, X = a.X;
      const int y0 = max(ob.y0, 0), y1 = min(ob.y1, Y), x0 = max(ob.x0, 0), x1 = min(ob.x1, X);
      const int h = max(y1 - y0, 0), w = max(x1 - x0, 0);
      const u16* lab = a.other + (size_t)tile * Y * X;
      double best = INFINITY;
      for (int i = lane; i < h * w; i += WAVE) {
        const int y = y0 + i / w, x = x0 + i % w;
        if (lab[(size_t)y * X + x] != p || !neighbors_outline(lab, Y, X, y, x, p)) continue;
        const double ey = (double)y - cy, ex = (double)x - cx;
        best = fmin(best, ey * ey + ex * ex);
      }
      best = wave_reduce_dpp(best, (double)INFINITY, [](double u, double v) { return fmin(u, v); });
      d_min = sqrt(best);
    }
  }
  if (lane == 0) relate_row_write(a.out + (size_t)row * a.ld + a.col0, p, a.overlap[row], a.children[row], d_centre, d_min);
}

static int relate_overlap_launch(aliby_ctx* ctx, const u16* self, const u16* other, int F, int Y, int X, const aliby_object* tab, int n_obj,
                                 int max_h, int max_w, const int32_t* off_other, int n_other, int max_count_other, const RelateSide& mine,
                                 const RelateSide& theirs, hipStream_t s) {
  if (n_obj == 0) return ALIBY_OK;
  RelateArgs a;
  a.self = self; a.other = other; a.F = F; a.Y = Y; a.X = X; a.tab = tab; a.n_obj = n_obj; a.off_other = off_other;
  a.n_other = n_other; a.max_count = max_count_other; a.centres = mine.centres; a.parent = mine.parent; a.overlap = mine.overlap;
  a.children_other = theirs.children;
  a.need = relate_counter_bytes(max_count_other);
  return object_launch(ctx, k_relate_overlap<false>, k_relate_overlap<true>, a, n_obj, a.need, (size_t)RELATE_LDS_BUDGET,
                       (long long)max_h * max_w, s);
}

static void relate_finish_launch(const u16* other, int F, int Y, int X, const aliby_object* tab, int n_obj, const aliby_object* tab_other,
                                 const int32_t* off_other, int n_other, const RelateSide& mine, const RelateSide& theirs, double* out, int ld,
                                 int col0, hipStream_t s) {
  if (n_obj == 0 || out == nullptr) return;
  RelateFinishArgs a;
  a.other = other; a.F = F; a.Y = Y; a.X = X; a.tab = tab; a.n_obj = n_obj; a.tab_other = tab_other; a.off_other = off_other;
  a.n_other = n_other; a.centres = mine.centres; a.centres_other = theirs.centres; a.parent = mine.parent; a.overlap = mine.overlap;
  a.children = mine.children; a.out = out; a.ld = ld; a.col0 = col0;
  const int per_block = RELATE_FINISH_BLOCK / WAVE;
  hipLaunchKernelGGL(k_relate_finish, dim3((n_obj + per_block - 1) / per_block), dim3(RELATE_FINISH_BLOCK), 0, s, a);
}

extern "C" size_t aliby_relate_workspace_bytes(int n_a, int n_b) {
  if (n_a < 0 || n_b < 0) return 0;
  return relate_side_bytes<2>(n_a) + relate_side_bytes<2>(n_b);
}

extern "C" int aliby_features_relate(aliby_ctx* ctx, const uint16_t* labels_a, const uint16_t* labels_b, int F, int Y, int X,
                                     const aliby_object* table_a, int n_a, int max_h_a, int max_w_a, const aliby_object* table_b, int n_b,
                                     int max_h_b, int max_w_b, const int32_t* offsets_a_dev, int max_count_a,
                                     const int32_t* offsets_b_dev, int max_count_b, void* work_dev, double* out_a, int ld_a, int col0_a,
                                     double* out_b, int ld_b, int col0_b, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(n_a >= 0 && n_b >= 0, "negative object count");
  if (n_a == 0 && n_b == 0) return ALIBY_OK;
  ARG_CHECK(labels_a && labels_b && offsets_a_dev && offsets_b_dev && work_dev, "NULL argument");
  ARG_CHECK((table_a || n_a == 0) && (table_b || n_b == 0), "NULL table");
  ARG_CHECK(F > 0 && Y > 0 && X > 0 && (long long)Y * X <= INT_MAX, "bad shape");
  ARG_CHECK(max_h_a >= 0 && max_w_a >= 0 && max_h_b >= 0 && max_w_b >= 0, "bad box");
  ARG_CHECK(max_count_a >= 0 && max_count_a <= 65535 && max_count_b >= 0 && max_count_b <= 65535,
            "max_count must lie in 0..65535 (labels are uint16)");
  ARG_CHECK(out_a == nullptr || (col0_a >= 0 && col0_a + 5 <= ld_a), "columns exceed row stride (a)");
  ARG_CHECK(out_b == nullptr || (col0_b >= 0 && col0_b + 5 <= ld_b), "columns exceed row stride (b)");
  ARG_CHECK(((uintptr_t)work_dev & 7) == 0, "work_dev must be 8-byte aligned");
  hipStream_t s = as_stream(stream);
  unsigned char* base = static_cast<unsigned char*>(work_dev);
  const RelateSide sa = relate_side<2>(base, n_a), sb = relate_side<2>(base + relate_side_bytes<2>(n_a), n_b);
  if (n_a) HIP_TRY(hipMemsetAsync(sa.children, 0, (size_t)n_a * sizeof(int), s));
  if (n_b) HIP_TRY(hipMemsetAsync(sb.children, 0, (size_t)n_b * sizeof(int), s));
  int rc = relate_overlap_launch(ctx, labels_a, labels_b, F, Y, X, table_a, n_a, max_h_a, max_w_a, offsets_b_dev, n_b, max_count_b, sa, sb, s);
  if (rc) return rc;
  rc = relate_overlap_launch(ctx, labels_b, labels_a, F, Y, X, table_b, n_b, max_h_b, max_w_b, offsets_a_dev, n_a, max_count_a, sb, sa, s);
  if (rc) return rc;
  relate_finish_launch(labels_b, F, Y, X, table_a, n_a, table_b, offsets_b_dev, n_b, sa, sb, out_a, ld_a, col0_a, s);
  KERNEL_CHECK();
  relate_finish_launch(labels_a, F, Y, X, table_b, n_b, table_a, offsets_a_dev, n_a, sb, sa, out_b, ld_b, col0_b, s);
  KERNEL_CHECK();
  return ALIBY_OK;
}

// ---- the tertiary image ---------------------------------------------------------------------------------------------------------
struct TertiaryArgs {
  const u16 *outer, *inner;
  u16* out;
  int F, Y, X, shrink;
  size_t total;  // pixels (k_tertiary_scalar) or tiles (k_tertiary_vec)
};

__device__ __forceinline__ u16 tertiary_pixel(const TertiaryArgs& a, const u16* tile, int y, int x, u16 in, u16 ou) {
  const bool keep = in == 0 || (a.shrink && neighbors_outline(tile, a.Y, a.X, y, x, (int)in));
  return keep ? ou : (u16)0;
}

// one pixel per thread: any X, any alignment
__global__ __launch_bounds__(256) void k_tertiary_scalar(TertiaryArgs a) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.total; g += stride) {
    const size_t r = g / a.X;  // f * Y + y
    const int x = (int)(g - r * a.X), y = (int)(r % a.Y);
    a.out[g] = tertiary_pixel(a, a.inner + (r - y) * a.X, y, x, a.inner[g], a.outer[g]);
  }
}

#define TERTIARY_ROWS 8     // a workgroup of k_tertiary_vec: 8 rows x 32 groups of eight pixels, so that rows y +- 1 of six of its
#define TERTIARY_GROUPS 32  // eight rows were loaded by the workgroup itself (consecutive workgroups run on different XCDs)

// eight pixels of a row with the pixel before and after them: r[0] = left, r[1..8], r[9] = right
__device__ __forceinline__ void tertiary_unpack(const uint4& v, int left, int right, int (&r)[10]) {
  r[0] = left;
  r[1] = (int)(v.x & 0xffffu); r[2] = (int)(v.x >> 16);
  r[3] = (int)(v.y & 0xffffu); r[4] = (int)(v.y >> 16);
  r[5] = (int)(v.z & 0xffffu); r[6] = (int)(v.z >> 16);
  r[7] = (int)(v.w & 0xffffu); r[8] = (int)(v.w >> 16);
  r[9] = right;
}

// Eight pixels (16 B) per thread; X is a multiple of 8 and the images are 16-byte aligned.  a.total = tiles of 8 rows x 256 pixels.
__global__ __launch_bounds__(TERTIARY_ROWS* TERTIARY_GROUPS) void k_tertiary_vec(TertiaryArgs a) {
  const int Y = a.Y, X = a.X, xg = X >> 3;
  const int tiles_x = (xg + TERTIARY_GROUPS - 1) / TERTIARY_GROUPS, tiles_y = (Y + TERTIARY_ROWS - 1) / TERTIARY_ROWS;
  const int gx_in = threadIdx.x % TERTIARY_GROUPS, ry = threadIdx.x / TERTIARY_GROUPS;
  for (size_t t = blockIdx.x; t < a.total; t += gridDim.x) {
    const int tx = (int)(t % tiles_x);
    const size_t rest = t / tiles_x;
    const int ty = (int)(rest % tiles_y);
    const size_t f = rest / tiles_y;
    const int y = ty * TERTIARY_ROWS + ry, gx = tx * TERTIARY_GROUPS + gx_in;
    if (y >= Y || gx >= xg) continue;
    const int x0 = gx << 3;
    const size_t q = (f * Y + y) * X + x0;
    const uint4 in = *reinterpret_cast<const uint4*>(a.inner + q);
    uint4 ou = *reinterpret_cast<const uint4*>(a.outer + q);
    if ((in.x | in.y | in.z | in.w) != 0u) {  // (else: a copy, rows y +- 1 untouched)
      unsigned int keep = 0u;  // bit k: pixel k keeps the outer label
      int mid[10];
      const u16* rm = a.inner + q;
      // neighbours that leave the frame are read from the nearest pixel inside it: a pixel on the frame's border is an outline pixel
      // whatever they hold
      const int xl = x0 > 0 ? -1 : 0, xr = x0 + 8 < X ? 8 : 7;
      tertiary_unpack(in, rm[xl], rm[xr], mid);
      if (a.shrink) {
        const u16 *ru = y > 0 ? rm - X : rm, *rd = y < Y - 1 ? rm + X : rm;
        int up[10], dn[10];
        tertiary_unpack(*reinterpret_cast<const uint4*>(ru), ru[xl], ru[xr], up);
        tertiary_unpack(*reinterpret_cast<const uint4*>(rd), rd[xl], rd[xr], dn);
        const bool border_row = y == 0 || y == Y - 1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int v = mid[k + 1];
          const bool edge = border_row || x0 + k == 0 || x0 + k == X - 1 || up[k] != v || up[k + 1] != v || up[k + 2] != v || mid[k] != v ||
                            mid[k + 2] != v || dn[k] != v || dn[k + 1] != v || dn[k + 2] != v;
          keep |= (unsigned int)(v == 0 || edge) << k;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) keep |= (unsigned int)(mid[k + 1] == 0) << k;
      }
      const unsigned int lo = 0x0000ffffu, hi = 0xffff0000u;
      ou.x &= (keep & 1u ? lo : 0u) | (keep & 2u ? hi : 0u);
      ou.y &= (keep & 4u ? lo : 0u) | (keep & 8u ? hi : 0u);
      ou.z &= (keep & 16u ? lo : 0u) | (keep & 32u ? hi : 0u);
      ou.w &= (keep & 64u ? lo : 0u) | (keep & 128u ? hi : 0u);
    }
    *reinterpret_cast<uint4*>(a.out + q) = ou;
  }
}

extern "C" int aliby_tertiary_labels(aliby_ctx* ctx, const uint16_t* outer, const uint16_t* inner, int F, int Y, int X, int shrink_inner,
                                     uint16_t* out, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(F >= 0 && Y > 0 && X > 0 && (long long)Y * X <= INT_MAX, "bad shape");
  if (F == 0) return ALIBY_OK;
  ARG_CHECK(outer && inner && out, "NULL argument");
  ARG_CHECK(out != outer && out != inner, "out must not alias an input (the stencil reads rows a neighbour writes)");
  TertiaryArgs a;
  a.outer = outer; a.inner = inner; a.out = out; a.F = F; a.Y = Y; a.X = X; a.shrink = shrink_inner ? 1 : 0;
  const bool vec = (X & 7) == 0 && (((uintptr_t)outer | (uintptr_t)inner | (uintptr_t)out) & 15) == 0;
  const size_t tiles_x = ((size_t)(X >> 3) + TERTIARY_GROUPS - 1) / TERTIARY_GROUPS, tiles_y = ((size_t)Y + TERTIARY_ROWS - 1) / TERTIARY_ROWS;
  a.total = vec ? (size_t)F * tiles_y * tiles_x : (size_t)F * Y * X;
  const size_t blocks = vec ? a.total : (a.total + 255) / 256;
  const dim3 grid((unsigned int)(blocks < (1u << 20) ? blocks : (1u << 20)));
  hipStream_t s = as_stream(stream);
  if (vec) hipLaunchKernelGGL(k_tertiary_vec, grid, dim3(TERTIARY_ROWS * TERTIARY_GROUPS), 0, s, a);
  else hipLaunchKernelGGL(k_tertiary_scalar, grid, dim3(256), 0, s, a);
  KERNEL_CHECK();
  return ALIBY_OK;
}
