// feat_neighbors.hip — "neighbors": CellProfiler's MeasureObjectNeighbors with the objects as their own neighbours (cp_measure
// carries it among its multi-mask measurements; the reference's loader does not bind it).  PARITY UNPINNED: the definition below
// is recalled from CellProfiler 4's measureobjectneighbors.py and centrosome's outline / strel_disk, and neither library can be
// run beside this one; tests/neighbors_ref.py restates it.
//
// One label image (a tile [Y,X], labels 1..n, 0 = background), an object L, an integer distance d in 1..64:
//   S = the offsets with dy^2 + dx^2 <= d^2      (strel_disk(d); the 4-neighbour cross for d = 1)
//   T = the offsets with dy^2 + dx^2 <= d^2 + d  (strel_disk(d + 0.5); the 3 x 3 square for d = 1)
//   offsets that leave the frame are dropped (no wrap, no padding value)
//   outline of L = its pixels on the first or last row or column of the frame, or with an 8-neighbour of another value (0 included)
// Seven columns:
//   0 NumberOfNeighbors         distinct labels v not in {0, L} at q + o for a pixel q of L and an o in S
//   1 PercentTouching           double(t) / double(p) * 100, p = outline pixels of L, t = those with a label not in {0, L} at q + o
//                               for an o in T
//   2 FirstClosestObjectNumber  3 FirstClosestDistance  4 SecondClosestObjectNumber  5 SecondClosestDistance
//                               centres (sum y / area, sum x / area): exact 64-bit sums, one float64 division each.  Candidates are
//                               the other present labels of the tile, ranked by dy dy + dx dx in float64 (every operation rounded
//                               on its own: -ffp-contract=off), ties to the lower label; the distance is sqrt of the key.  Without
//                               a first candidate columns 2-3 are 0, without a second columns 4-6 are 0 (CellProfiler leaves its
//                               zero-initialised arrays).
//   6 AngleBetweenNeighbors     atan2(|v1 x v2|, v1 . v2) 180 / pi for the vectors from L's centre to the two centres; NaN when one
//                               of them is zero.  CellProfiler takes arccos of the normalised dot product: the same angle, but
//                               ill-conditioned near 0 and 180 degrees and NaN when rounding pushes the quotient past 1.  The
//                               departure is deliberate.
// A label of 1..n without pixels gets NaN in all seven columns and is neither a neighbour nor a candidate.
// Not built: "Expand until adjacent" (its nearest-label fill rests on EDT index ties), neighbours from a second object set.
//
// k_neighbors_scan     one workgroup per table row, threads striding over the object's box.  A pixel of L walks the offsets of T,
//                      generated from the two integer inequalities, and reads labels[q + o] from global memory (the windows of
//                      neighbouring threads overlap almost entirely: cache hits).  A foreign label sets the thread's touching flag,
//                      and, where the offset is in S too, its bit in an LDS bitmap of one bit per label of the tile (atomicOr on
//                      32-bit words; at most 8 KiB, sized by the largest tile of the launch).  A label above the tile's table count
//                      can only come from a wrong max_labels hint: it has no bit and is not counted.  Then: popcount of the
//                      bitmap, integer block reductions of the two outline counts and the two coordinate sums, columns 0-1 and the
//                      centre into centres_dev [n_obj, 2].  LDS form only: the kernel never touches ctx->scratch, so it may run on
//                      a side stream beside any other launch of the context (the scratch rule, object_launch.h).
// k_neighbors_closest  after it on the same stream: one wave per row.  The lanes stride over the centres of the tile's rows
//                      [offsets[tile], offsets[tile + 1]) (a NaN centre = absent), each keeps its two best (key, label) pairs, and a
//                      butterfly merges them under the order "lower key, then lower label": a total order on distinct labels, so
//                      the result does not depend on which lane saw which row.  Columns 2-6.
// Everything but sqrt and atan2 is integer or a single rounded float64 operation: a row carries the same bits whatever the batch,
// the workgroup size and the stream.
#include "common.h"
#include "neighbors_stats.h"

typedef unsigned short u16;

#define NEIGHBORS_MAX_DISTANCE 64

struct NeighborsArgs {
  const u16* labels;
  int F, Y, X;
  const aliby_object* tab;
  int n_obj;
  const int32_t* offsets;  // [F + 1], device
  int max_count;           // the largest tile's rows: what the bitmap was sized from
  int d;
  double* centres;  // [n_obj, 2] (y, x)
  double* out;
  int ld, col0;
  __device__ __forceinline__ int rows() const { return n_obj; }
  __device__ __forceinline__ bool stack_rows(int row, int& lo, int& hi) const {  // k_neighbors_closest: a row's stack is its tile
    const int tile = tab[row].tile;
    if (tile < 0 || tile >= F) return false;
    lo = max(offsets[tile], 0); hi = min(offsets[tile + 1], n_obj);
    return true;
  }
};

__global__ __launch_bounds__(256) void k_neighbors_scan(NeighborsArgs a) {
  __shared__ int red_i[8];
  __shared__ long long red_l[8];
  const int oi = blockIdx.x, tid = threadIdx.x;
  const aliby_object o = a.tab[oi];
  double* out = a.out + (size_t)oi * a.ld + a.col0;
  double* ctr = a.centres + 2 * (size_t)oi;
  // the box, clipped to the frame (a table made from these labels never needs it)
  const int y0 = max(o.y0, 0), y1 = min(o.y1, a.Y), x0 = max(o.x0, 0), x1 = min(o.x1, a.X);
  if (o.area <= 0 || o.tile < 0 || o.tile >= a.F || y0 >= y1 || x0 >= x1) {
    if (tid == 0) neighbors_absent<2>(out, ctr);
    return;
  }
  const int Y = a.Y, X = a.X, h = y1 - y0, w = x1 - x0;
  const u16* lab = a.labels + (size_t)o.tile * Y * X;
  const int L = o.label;
  const NeighborsBitmap<0> bm{max(0, min(a.offsets[o.tile + 1] - a.offsets[o.tile], a.max_count))};
  bm.clear();

  const int d = a.d, s2 = d * d, t2 = s2 + d;
  int n = 0, outline = 0, touching = 0, last_set = 0;
  long long sy = 0, sx = 0;
  for (int i = tid; i < h * w; i += blockDim.x) {
    const int y = y0 + i / w, x = x0 + i % w;
    if (lab[(size_t)y * X + x] != L) continue;
    ++n;
    sy += y;
    sx += x;
    bool edge = y == 0 || y == Y - 1 || x == 0 || x == X - 1, touch = false;
    const int ya = max(y - d, 0), yb = min(y + d, Y - 1), xa = max(x - d, 0), xb = min(x + d, X - 1);
    for (int yy = ya; yy <= yb; ++yy) {
      const int dy = yy - y, rt = t2 - dy * dy, rs = s2 - dy * dy;  // dx^2 <= rt: in T; <= rs: in S
      const u16* row = lab + (size_t)yy * X;
      for (int xx = xa; xx <= xb; ++xx) {
        const int dx = xx - x, dd = dx * dx;
        if (dd > rt) continue;
        const int v = row[xx];
        if (v == L) continue;
        if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) edge = true;  // (the 3 x 3 square lies inside T for every d >= 1)
        if (v == 0) continue;
        touch = true;
        bm.mark(dd <= rs, v, last_set);
      }
    }
    outline += edge;
    touching += edge && touch;
  }
  __syncthreads();
  const int cnt = block_sum_i32(bm.popcount(), red_i);
  n = block_sum_i32(n, red_i); outline = block_sum_i32(outline, red_i); touching = block_sum_i32(touching, red_i);
  sy = block_sum_i64(sy, red_l); sx = block_sum_i64(sx, red_l);
  if (tid == 0) neighbors_scan_write(out, ctr, cnt, n, outline, touching, sy, sx);
}

extern "C" int aliby_features_neighbors(aliby_ctx* ctx, const uint16_t* labels, int F, int Y, int X, const aliby_object* table_dev,
                                        int n_obj, int max_h, int max_w, const int32_t* offsets_dev, int max_count, int distance,
                                        double* centres_dev, double* out, int ld, int col0, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(distance >= 1 && distance <= NEIGHBORS_MAX_DISTANCE, "distance must lie in 1..64");
  ARG_CHECK(n_obj >= 0, "negative object count");
  if (n_obj == 0) return ALIBY_OK;
  ARG_CHECK(labels && table_dev && offsets_dev && centres_dev && out, "NULL argument");
  ARG_CHECK(F > 0 && Y > 0 && X > 0 && (long long)Y * X <= INT_MAX && max_h >= 0 && max_w >= 0, "bad shape");
  ARG_CHECK(max_count >= 0 && max_count <= 65535, "max_count must lie in 0..65535 (labels are uint16)");
  ARG_CHECK(col0 >= 0 && col0 + 7 <= ld, "columns exceed row stride");
  NeighborsArgs a;
  a.labels = labels; a.F = F; a.Y = Y; a.X = X; a.tab = table_dev; a.n_obj = n_obj; a.offsets = offsets_dev;
  a.max_count = max_count; a.d = distance; a.centres = centres_dev; a.out = out; a.ld = ld; a.col0 = col0;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_neighbors_scan, dim3(n_obj), dim3(aliby_pick_block((long long)max_h * max_w)), neighbors_bitmap_bytes(max_count), s, a);
  KERNEL_CHECK();
  neighbors_closest_launch<2>(a, n_obj, s);
  KERNEL_CHECK();
  return ALIBY_OK;
}
