// feat_propagate.hip — "propagate": CellProfiler's IdentifySecondaryObjects, method "Propagation" (its default): the primary labels
// grow along a stain.  A pixel takes the label of the seed it reaches most cheaply over a metric that charges for crossing grey-level
// differences (a membrane is expensive), and a threshold on the stain says where the cells end.  centrosome's `propagate` does it in
// float64 with a priority queue; here the metric is an exact integer, so that every relaxation order reaches the same unique fixed
// point and a tile carries the same bits whatever the batch, the launch form and the stream (definition and worked examples:
// include/aliby_hip.h; tests/propagate_ref.py restates it as a heap Dijkstra and as a Jacobi iteration).
//
// Per tile of primary uint16 [F,Y,X] (0 = background) and image uint16 [F,Y,X]:
//   passable(p)  primary[p] != 0, or image[p] >= threshold and (no distance, or secondary_labels(primary, distance)[p] != 0)
//   P(p,q)       sum over o in {-1,0,1}^2 of |image[clamp(p+o)] - image[clamp(q+o)]| for passable 8-neighbours p, q of one tile
//   W(p,q)       isqrt(256 (P^2 + m L)), m = |dy| + |dx|, L = the caller's lambda2: sixteenths of a grey level
//   key[p]       (D[p] << 16) | label, the lexicographic minimum over paths from labelled pixels; D < 2^48 as Y X <= 2^23
// out = the key's label, 0 where no path arrives; a labelled pixel keeps its label.  "Distance - B" is threshold 0 with a distance.
//
// Launches (the workspace is the caller's: two key buffers of 8 B per pixel, four weight planes of 4 B per pixel, eight flags):
// aliby_secondary_labels   only with a distance: the reach mask, into out_labels (its own 4 B per pixel lie over the weight planes,
//                          which are written after it).
// k_propagate_weights      once per call.  A workgroup stages the image of its 32 x 32 region plus a halo of 2, clamped coordinate
//                          by coordinate, and the passable bits plus a halo of 1 in LDS; a thread writes for each of its four pixels
//                          the weights to the E, SW, S and SE neighbour (PROPAGATE_NOEDGE where either end is impassable or outside
//                          the tile) and the starting key.  isqrt: float64 sqrt, then one integer step down and one up.  Its argument
//                          is below 2^50 (P <= 9 * 65535 and lambda2 <= 2^40 give 256 (P^2 + 2 lambda2) < 2^49.3): a double holds it
//                          exactly and the rounded root is within one of the floor.
// k_propagate_round        a workgroup owns a 32 x 32 region of one tile.  It loads the region's keys plus a halo of 1 from the source
//                          buffer into LDS (9.2 KiB; a row of 34 keys is 272 B, and the 32 lanes of a ds_read_b64 group read 32
//                          consecutive keys: no bank conflict), keeps the 8 weights of each of its 4 pixels in registers (they do not
//                          change; none for a labelled pixel, which is a source only), and runs Jacobi sweeps inside LDS (all reads,
//                          a barrier that also votes "any change", the writes, a barrier) until the region is at its fixed point
//                          for this halo.  Then it writes the region to the OTHER buffer and raises the round's flag if any key
//                          changed.  The halo comes from the buffer no workgroup of the launch writes: a round is deterministic.
//                          Round k > 0 of a chunk returns at once when round k - 1 raised no flag: then both buffers already hold
//                          the fixed point.
// k_propagate_finish       unpacks labels and, if asked, D.
// The host launches PROPAGATE_CHUNK rounds, each with a flag of its own, between reads of the flags; a round without a flag ends the
// call.  Every round that changes a key settles at least one more pixel (the unsettled pixel of smallest D has a settled neighbour
// on its path, in its region or its halo), so Y X + 1 changing rounds always suffice: more than that is an error, never a result.
// The host counts when it reads the flags, so the error comes at the end of the chunk of eight in which the bound is passed;
// stats_host then holds the rounds and reads so far.
#include "common.h"

typedef unsigned short u16;
typedef unsigned long long u64;

#define PROPAGATE_R 32         // a region is PROPAGATE_R x PROPAGATE_R pixels
#define PROPAGATE_BLOCK 256    // 32 lanes along x, 8 rows; a thread owns rows ty, ty + 8, ty + 16, ty + 24 of its column
#define PROPAGATE_PER 4
#define PROPAGATE_CHUNK 8      // rounds between two reads of the flags
#define PROPAGATE_NOEDGE 0xffffffffu
#define PROPAGATE_NONE 0xffffffffffffffffull
#define PROPAGATE_MAX_PIXELS (1 << 23)
#define PROPAGATE_MAX_SWEEPS 2048  // per round and region; a region that needs more goes on in the next round
#define PROPAGATE_FLAG_BYTES 256

struct PropagateArgs {
  const u16* primary;
  const u16* image;
  const u16* reach;  // secondary_labels(primary, distance), or null
  u64* keys[2];      // [F,Y,X] each
  uint32_t* weights; // 4 planes [F,Y,X]: E, SW, S, SE
  int* flags;        // [PROPAGATE_CHUNK]
  u16* out_labels;
  u64* out_dist;
  u64 lambda2;
  const int* thresholds;  // [F], one per tile, or null: `threshold` for every tile
  int F, Y, X, threshold;
  int regions_x, regions_y;
};

// floor(sqrt(v)) for v < 2^50 (the bound of this file's arguments): (double)v is v, the rounded root is within one of the answer
__device__ __forceinline__ u64 propagate_isqrt(u64 v) {
  u64 r = (u64)sqrt((double)v);
  if (r * r > v) --r;
  if ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

struct PropagateRegion { size_t tile; int y0, x0; };  // the tile's first pixel in a [F,Y,X] block; the region's corner

__device__ __forceinline__ PropagateRegion propagate_region(const PropagateArgs& a) {
  PropagateRegion r;
  r.x0 = (int)(blockIdx.x % (unsigned int)a.regions_x) * PROPAGATE_R;
  const unsigned int rest = blockIdx.x / (unsigned int)a.regions_x;
  r.y0 = (int)(rest % (unsigned int)a.regions_y) * PROPAGATE_R;
  r.tile = (size_t)(rest / (unsigned int)a.regions_y) * (size_t)a.Y * a.X;
  return r;
}

// grid = F * regions_y * regions_x, x fastest
__global__ __launch_bounds__(PROPAGATE_BLOCK) void k_propagate_weights(PropagateArgs a) {
  __shared__ u16 img[PROPAGATE_R + 4][PROPAGATE_R + 4];             // pixel (y0 - 2 + i, x0 - 2 + j), each coordinate clamped
  __shared__ unsigned char pass[PROPAGATE_R + 2][PROPAGATE_R + 2];  // pixel (y0 - 1 + i, x0 - 1 + j); 0 outside the tile
  const int Y = a.Y, X = a.X, tid = (int)threadIdx.x;
  const PropagateRegion g = propagate_region(a);
  const u16* image = a.image + g.tile;
  const u16* primary = a.primary + g.tile;
  const int threshold = a.thresholds ? a.thresholds[blockIdx.x / (unsigned int)(a.regions_x * a.regions_y)] : a.threshold;
  for (int i = tid; i < (PROPAGATE_R + 4) * (PROPAGATE_R + 4); i += PROPAGATE_BLOCK) {
    const int r = i / (PROPAGATE_R + 4), c = i % (PROPAGATE_R + 4);
    const int y = min(max(g.y0 - 2 + r, 0), Y - 1), x = min(max(g.x0 - 2 + c, 0), X - 1);
    img[r][c] = image[(size_t)y * X + x];
  }
  for (int i = tid; i < (PROPAGATE_R + 2) * (PROPAGATE_R + 2); i += PROPAGATE_BLOCK) {
    const int r = i / (PROPAGATE_R + 2), c = i % (PROPAGATE_R + 2);
    const int y = g.y0 - 1 + r, x = g.x0 - 1 + c;
    bool ok = false;
    if (y >= 0 && y < Y && x >= 0 && x < X) {
      const size_t p = (size_t)y * X + x;
      ok = primary[p] != 0 || ((int)image[p] >= threshold && (a.reach == nullptr || a.reach[g.tile + p] != 0));
    }
    pass[r][c] = ok ? 1 : 0;
  }
  __syncthreads();
  const int tx = tid & (PROPAGATE_R - 1), ty = tid / PROPAGATE_R;
  const size_t plane = (size_t)a.F * Y * X;
  const int ddy[4] = {0, 1, 1, 1}, ddx[4] = {1, -1, 0, 1};
#pragma unroll
  for (int j = 0; j < PROPAGATE_PER; ++j) {
    const int ly = ty + j * (PROPAGATE_BLOCK / PROPAGATE_R), y = g.y0 + ly, x = g.x0 + tx;
    if (y >= Y || x >= X) continue;
    const size_t p = g.tile + (size_t)y * X + x;
    const u16 lab = a.primary[p];
    a.keys[0][p] = lab != 0 ? (u64)lab : PROPAGATE_NONE;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      uint32_t w = PROPAGATE_NOEDGE;
      if (pass[ly + 1][tx + 1] && pass[ly + 1 + ddy[d]][tx + 1 + ddx[d]]) {
        uint32_t P = 0;
#pragma unroll
        for (int oy = -1; oy <= 1; ++oy) {
#pragma unroll
          for (int ox = -1; ox <= 1; ++ox) {
            const int u = (int)img[ly + 2 + oy][tx + 2 + ox], v = (int)img[ly + 2 + oy + ddy[d]][tx + 2 + ox + ddx[d]];
            P += (uint32_t)abs(u - v);
          }
        }
        const u64 m = d == 2 || d == 0 ? 1 : 2;
        w = (uint32_t)propagate_isqrt(256ull * ((u64)P * P + m * a.lambda2));
      }
      a.weights[(size_t)d * plane + p] = w;
    }
  }
}

// the weight plane `d` of the edge that starts at pixel (y, x) of the tile; no edge from outside the tile
__device__ __forceinline__ uint32_t propagate_weight(const uint32_t* tile_weights, size_t plane, int d, int y, int x, int Y, int X) {
  return y >= 0 && y < Y && x >= 0 && x < X ? tile_weights[(size_t)d * plane + (size_t)y * X + x] : PROPAGATE_NOEDGE;
}

__device__ __forceinline__ u64 propagate_via(u64 best, u64 neighbour, uint32_t w) {
  const u64 cand = neighbour + ((u64)w << 16);  // (D + W) << 16 | label: no carry into a label, D + W < 2^48
  return w != PROPAGATE_NOEDGE && neighbour != PROPAGATE_NONE && cand < best ? cand : best;
}

// grid = F * regions_y * regions_x, x fastest.  Reads keys[from], writes keys[from ^ 1]; raises flags[k].
__global__ __launch_bounds__(PROPAGATE_BLOCK) void k_propagate_round(PropagateArgs a, int from, int k) {
  __shared__ u64 keys[PROPAGATE_R + 2][PROPAGATE_R + 2];  // pixel (y0 - 1 + i, x0 - 1 + j)
  if (k > 0 && a.flags[k - 1] == 0) return;  // the round before changed nothing: both buffers hold the fixed point
  const int Y = a.Y, X = a.X, tid = (int)threadIdx.x;
  const PropagateRegion g = propagate_region(a);
  const u64* src = a.keys[from] + g.tile;
  u64* dst = a.keys[from ^ 1] + g.tile;
  for (int i = tid; i < (PROPAGATE_R + 2) * (PROPAGATE_R + 2); i += PROPAGATE_BLOCK) {
    const int r = i / (PROPAGATE_R + 2), c = i % (PROPAGATE_R + 2);
    const int y = g.y0 - 1 + r, x = g.x0 - 1 + c;
    keys[r][c] = y >= 0 && y < Y && x >= 0 && x < X ? src[(size_t)y * X + x] : PROPAGATE_NONE;
  }
  const int tx = tid & (PROPAGATE_R - 1), ty = tid / PROPAGATE_R;
  const size_t plane = (size_t)a.F * Y * X;
  const uint32_t* tw = a.weights + g.tile;
  // a pixel's eight edges: its own four (E, SW, S, SE) and the four that end at it (from W, NE, N, NW)
  uint32_t w[PROPAGATE_PER][8];
  const int x = g.x0 + tx;
#pragma unroll
  for (int j = 0; j < PROPAGATE_PER; ++j) {
    const int y = g.y0 + ty + j * (PROPAGATE_BLOCK / PROPAGATE_R);
    // (a labelled pixel keeps its key: with lambda2 = 0 on a flat stain another seed would arrive at distance 0 with a smaller label)
    const bool inside = y < Y && x < X && a.primary[g.tile + (size_t)y * X + x] == 0;
    w[j][0] = inside ? propagate_weight(tw, plane, 0, y, x, Y, X) : PROPAGATE_NOEDGE;          // to E
    w[j][1] = inside ? propagate_weight(tw, plane, 1, y, x, Y, X) : PROPAGATE_NOEDGE;          // to SW
    w[j][2] = inside ? propagate_weight(tw, plane, 2, y, x, Y, X) : PROPAGATE_NOEDGE;          // to S
    w[j][3] = inside ? propagate_weight(tw, plane, 3, y, x, Y, X) : PROPAGATE_NOEDGE;          // to SE
    w[j][4] = inside ? propagate_weight(tw, plane, 0, y, x - 1, Y, X) : PROPAGATE_NOEDGE;      // from W: its E edge
    w[j][5] = inside ? propagate_weight(tw, plane, 1, y - 1, x + 1, Y, X) : PROPAGATE_NOEDGE;  // from NE: its SW edge
    w[j][6] = inside ? propagate_weight(tw, plane, 2, y - 1, x, Y, X) : PROPAGATE_NOEDGE;      // from N: its S edge
    w[j][7] = inside ? propagate_weight(tw, plane, 3, y - 1, x - 1, Y, X) : PROPAGATE_NOEDGE;  // from NW: its SE edge
  }
  __syncthreads();
  u64 cur[PROPAGATE_PER];
#pragma unroll
  for (int j = 0; j < PROPAGATE_PER; ++j) cur[j] = keys[ty + j * (PROPAGATE_BLOCK / PROPAGATE_R) + 1][tx + 1];
  bool any = false;  // (the same in every thread: the barrier's vote)
  for (int sweep = 0; sweep < PROPAGATE_MAX_SWEEPS; ++sweep) {
    u64 next[PROPAGATE_PER];
    int changed = 0;
#pragma unroll
    for (int j = 0; j < PROPAGATE_PER; ++j) {
      const int r = ty + j * (PROPAGATE_BLOCK / PROPAGATE_R) + 1, c = tx + 1;
      u64 best = cur[j];
      best = propagate_via(best, keys[r][c + 1], w[j][0]);
      best = propagate_via(best, keys[r + 1][c - 1], w[j][1]);
      best = propagate_via(best, keys[r + 1][c], w[j][2]);
      best = propagate_via(best, keys[r + 1][c + 1], w[j][3]);
      best = propagate_via(best, keys[r][c - 1], w[j][4]);
      best = propagate_via(best, keys[r - 1][c + 1], w[j][5]);
      best = propagate_via(best, keys[r - 1][c], w[j][6]);
      best = propagate_via(best, keys[r - 1][c - 1], w[j][7]);
      next[j] = best;
      changed |= best != cur[j];
    }
    if (!__syncthreads_or(changed)) break;  // (every read of the sweep is done)
    any = true;
#pragma unroll
    for (int j = 0; j < PROPAGATE_PER; ++j) {
      if (next[j] != cur[j]) {
        cur[j] = next[j];
        keys[ty + j * (PROPAGATE_BLOCK / PROPAGATE_R) + 1][tx + 1] = next[j];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < PROPAGATE_PER; ++j) {
    const int y = g.y0 + ty + j * (PROPAGATE_BLOCK / PROPAGATE_R);
    if (y < Y && x < X) dst[(size_t)y * X + x] = cur[j];
  }
  if (any && tid == 0) atomicOr(a.flags + k, 1);
}

__global__ __launch_bounds__(PROPAGATE_BLOCK) void k_propagate_finish(const u64* __restrict__ keys, size_t n, u16* __restrict__ out_labels,
                                                                      u64* __restrict__ out_dist) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const u64 key = keys[i];
    out_labels[i] = key == PROPAGATE_NONE ? (u16)0 : (u16)(key & 0xffffu);
    if (out_dist) out_dist[i] = key == PROPAGATE_NONE ? PROPAGATE_NONE : key >> 16;
  }
}

// keys 2 x 8 B, weights 4 x 4 B per pixel, the flags
extern "C" size_t aliby_propagate_workspace_bytes(int F, int Y, int X) {
  if (F <= 0 || Y <= 0 || X <= 0) return 0;
  return (size_t)F * (size_t)Y * (size_t)X * 32 + PROPAGATE_FLAG_BYTES;
}

// the body of both entries: `thresholds` [dev, F] or null for the scalar
static int propagate_labels(aliby_ctx* ctx, const uint16_t* primary, const uint16_t* image, int F, int Y, int X, int threshold,
                            const int32_t* thresholds, uint64_t lambda2, int distance, void* workspace, size_t workspace_bytes,
                            uint16_t* out_labels, uint64_t* out_dist, int32_t* stats_host, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(F >= 0 && Y >= 0 && X >= 0, "bad shape");
  ARG_CHECK((long long)Y * X <= PROPAGATE_MAX_PIXELS, "a tile has more than 2^23 pixels (the packed key holds distances below 2^48)");
  ARG_CHECK(threshold >= 0 && threshold <= 65535, "threshold must be in 0..65535");
  ARG_CHECK(lambda2 <= (1ull << 40), "lambda2 must be at most 2^40 (regularization * image_max at most 2^20)");
  ARG_CHECK(distance >= 0 && distance <= 64, "distance must be 0 (none) or in 1..64");
  if (stats_host) stats_host[0] = stats_host[1] = 0;
  if (F == 0 || Y == 0 || X == 0) return ALIBY_OK;
  ARG_CHECK(primary && image && out_labels, "NULL argument");
  ARG_CHECK(out_labels != primary, "out_labels must not alias primary (the primary labels are an input of the steps after this one)");
  ARG_CHECK(workspace != nullptr && ((uintptr_t)workspace & 7) == 0, "workspace is NULL or not 8-byte aligned");
  ARG_CHECK(workspace_bytes >= aliby_propagate_workspace_bytes(F, Y, X), "workspace is smaller than aliby_propagate_workspace_bytes");
  ARG_CHECK(out_dist == nullptr || ((uintptr_t)out_dist & 7) == 0, "out_dist is not 8-byte aligned");
  const size_t n = (size_t)F * Y * X;
  PropagateArgs a;
  a.primary = primary; a.image = image; a.reach = distance > 0 ? out_labels : nullptr;
  a.keys[0] = static_cast<u64*>(workspace); a.keys[1] = a.keys[0] + n;
  a.weights = reinterpret_cast<uint32_t*>(a.keys[1] + n);
  a.flags = reinterpret_cast<int*>(a.weights + 4 * n);
  a.out_labels = out_labels; a.out_dist = reinterpret_cast<u64*>(out_dist);
  a.lambda2 = lambda2; a.thresholds = thresholds; a.F = F; a.Y = Y; a.X = X; a.threshold = threshold;
  a.regions_x = (X + PROPAGATE_R - 1) / PROPAGATE_R;
  a.regions_y = (Y + PROPAGATE_R - 1) / PROPAGATE_R;
  const long long blocks = (long long)F * a.regions_y * a.regions_x;
  ARG_CHECK(blocks <= INT_MAX, "too many regions for one launch (F * ceil(Y / 32) * ceil(X / 32) > INT_MAX)");
  hipStream_t s = as_stream(stream);
  if (distance > 0) {  // the reach mask; its workspace lies over the weight planes, which are written after it
    const int rc = aliby_secondary_labels(ctx, primary, F, Y, X, distance, a.weights, 4 * n, out_labels, stream);
    if (rc != ALIBY_OK) return rc;
  }
  const dim3 grid((unsigned int)blocks), block(PROPAGATE_BLOCK);
  hipLaunchKernelGGL(k_propagate_weights, grid, block, 0, s, a);
  KERNEL_CHECK();
  const long long max_rounds = (long long)Y * X + 1;
  long long rounds = 0;
  int from = 0, reads = 0;
  for (;;) {
    HIP_TRY(hipMemsetAsync(a.flags, 0, PROPAGATE_CHUNK * sizeof(int), s));
    for (int k = 0; k < PROPAGATE_CHUNK; ++k) {
      hipLaunchKernelGGL(k_propagate_round, grid, block, 0, s, a, from, k);
      from ^= 1;
    }
    KERNEL_CHECK();
    int raised[PROPAGATE_CHUNK];
    HIP_TRY(hipMemcpyAsync(raised, a.flags, sizeof(raised), hipMemcpyDeviceToHost, s));
    const int rc = aliby_wait_stream(s);
    if (rc != ALIBY_OK) return rc;
    ++reads;
    int changing = 0;
    while (changing < PROPAGATE_CHUNK && raised[changing]) ++changing;
    rounds += changing;
    if (changing < PROPAGATE_CHUNK) break;  // a round changed nothing: keys[from] and keys[from ^ 1] are equal, the fixed point
    if (rounds > max_rounds) {
      if (stats_host) {
        stats_host[0] = (int32_t)rounds;
        stats_host[1] = reads;
      }
      aliby_set_error("aliby_propagate_labels: no fixed point within %lld rounds on %d x %d tiles", rounds, Y, X);
      return ALIBY_ERR_TOO_LARGE;
    }
  }
  if (stats_host) {
    stats_host[0] = (int32_t)rounds;
    stats_host[1] = reads;
  }
  const unsigned int fgrid = (unsigned int)((n + PROPAGATE_BLOCK - 1) / PROPAGATE_BLOCK < 16384 ? (n + PROPAGATE_BLOCK - 1) / PROPAGATE_BLOCK : 16384);
  hipLaunchKernelGGL(k_propagate_finish, dim3(fgrid), block, 0, s, a.keys[from], n, out_labels, a.out_dist);
  KERNEL_CHECK();
  return ALIBY_OK;
}

extern "C" int aliby_propagate_labels(aliby_ctx* ctx, const uint16_t* primary, const uint16_t* image, int F, int Y, int X, int threshold,
                                      uint64_t lambda2, int distance, void* workspace, size_t workspace_bytes, uint16_t* out_labels,
                                      uint64_t* out_dist, int32_t* stats_host, void* stream) {
  return propagate_labels(ctx, primary, image, F, Y, X, threshold, nullptr, lambda2, distance, workspace, workspace_bytes, out_labels,
                          out_dist, stats_host, stream);
}

// one threshold per tile, read on the device by k_propagate_weights (aliby_auto_threshold's output); a value above 65535 passes nothing
extern "C" int aliby_propagate_labels_per_tile(aliby_ctx* ctx, const uint16_t* primary, const uint16_t* image, int F, int Y, int X,
                                               const int32_t* thresholds, uint64_t lambda2, int distance, void* workspace,
                                               size_t workspace_bytes, uint16_t* out_labels, uint64_t* out_dist, int32_t* stats_host,
                                               void* stream) {
  ARG_CHECK(thresholds != nullptr || F <= 0 || Y <= 0 || X <= 0, "thresholds is NULL");
  return propagate_labels(ctx, primary, image, F, Y, X, 0, thresholds, lambda2, distance, workspace, workspace_bytes, out_labels, out_dist,
                          stats_host, stream);
}
