// feat_secondary3d.hip — "secondary" on volume labels: CellProfiler's IdentifySecondaryObjects, method "Distance - N", one dimension
// up.  Every primary object of a stack grows by up to N into the background, distances measured on the integer lattice
// spacing = (sz, sy, sx), and a grown voxel carries the label of its nearest labelled voxel, ties to the smaller label.  It is
// scipy.ndimage.distance_transform_edt(vol == 0, sampling=spacing, return_indices=True) and out[dist <= N] = vol[idx]
// (skimage.segmentation.expand_labels(..., spacing=)) with the one freedom SciPy leaves to its sweep order fixed by that tie rule.
// tests/secondary3d_ref.py restates it by brute force and tests/test_cpu_secondary3d_ref.py holds the restatement against SciPy on
// every voxel that is not a tie.
//
// Per stack of primary uint16 [F,Z,Y,X] (0 = background), for a voxel p:
//   primary[p] != 0                      out[p] = primary[p]
//   else, m = min over the labelled q of the stack of (sz dz)^2 + (sy dy)^2 + (sx dx)^2 (an integer):
//     no such q, or m > N^2              out[p] = 0
//     else                               out[p] = min{ primary[q] : d2(p, q) = m }
// N and every spacing component in 1..255 (N^2 <= 65025 stays below the 16-bit sentinel field), the reach N / s_a at most 64 voxels
// on every axis (it bounds the scans; not a structural limit).  65535 is a label like any other, nothing crosses a stack edge, and
// every step is integer arithmetic: a stack carries the same bits whatever the batch, the launch form and the stream.  With Z == 1
// and unit spacing it is feat_secondary.hip's function on the one plane, bit for bit.
// Not built: "Propagation" and "Distance - B" on volumes (2-D: feat_propagate.hip), "Watershed", a float spacing, discarding objects that touch the border.
//
// The exact separable form: the lexicographic minimum of (distance, label) decomposes over the axes, so three passes equal the brute
// force.  Three launches and two 4-byte-per-voxel intermediates (the caller's workspace):
// k_secondary3d_z  a lane owns one column (y, x) of a segment of SECONDARY3D_SEG planes of one stack; the (y, x) of a plane are one
//                  flat index, so accesses are coalesced whatever X is.  It walks down from N / sz planes above the segment carrying
//                  the last label seen and its plane distance, keeps the segment's results in registers, walks up from N / sz planes
//                  below it, and writes per voxel the smaller of the two words (g << 16) | label: g = sz dz to the column's nearest
//                  labelled voxel (at most N <= 255), that voxel's label, above and below equally near -> the smaller label.  Nothing
//                  within reach: SECONDARY3D_NONE (g field 0xffff).  A farther voxel of the same column can never win at any
//                  (dy, dx), so the nearest one is all a column contributes.  The walks start inside the stack.  2 B read + 4 B
//                  written per voxel.
// k_secondary3d_y  a thread owns one voxel and takes the minimum over |dy| <= N / sy of ((g^2 + (sy dy)^2) << 16) | label over the z
//                  words of its plane, read through the cache (a wave reads 256 contiguous bytes per dy, and the rows a workgroup
//                  reads are those its neighbours read).  A true windowed minimum: the words carry distances, so nearest-first does
//                  not suffice.  A candidate above N^2 is dropped before it is packed, so the 16-bit field never overflows.  Outwards
//                  from dy = 0, and only while (sy dy)^2 <= min(best distance, N^2): a voxel of an object stops at once; the
//                  comparison is strict, so an equally distant voxel farther out is still seen.  4 B read + 4 B written per voxel.
// k_secondary3d_x  the same along x over the y words, staged in LDS as k_secondary_rows does: 256 words of each of 8 rows plus the
//                  reach on either side (outside the row: NONE).  The rows of all planes and stacks are one list, so a group of 8
//                  may span a plane or a stack edge: rows do not see one another in this pass.  It writes the label, or 0 where
//                  nothing is within N: 4 B read + 2 B written per voxel.
// No kernel caps its grid: the entry refuses a block count above INT_MAX.
#include "common.h"

typedef unsigned short u16;

#define SECONDARY3D_MAX_DISTANCE 255
#define SECONDARY3D_MAX_REACH 64  // voxels along one axis: bounds the scans and the LDS halo
#define SECONDARY3D_NONE 0xffffffffu
#define SECONDARY3D_SEG 32     // planes of a column segment: their down-walk words stay in registers
#define SECONDARY3D_BLOCK 256  // every kernel: one voxel of a row (one column of a segment) per thread
#define SECONDARY3D_ROWS 8     // rows of a workgroup of the x pass
#define SECONDARY3D_FAR (1 << 20)  // a plane distance no walk reaches: "no labelled voxel seen"

struct Secondary3dArgs {
  const u16* labels;
  uint32_t* zwords;  // [F,Z,Y,X]
  uint32_t* ywords;  // [F,Z,Y,X]
  u16* out;
  int Z, Y, X, P;  // P = Y * X
  int N, sz, sy, sx;
  int rz, ry, rx;  // the reach in voxels, N / s_a
  int blocks_p;    // ceil(P / SECONDARY3D_BLOCK)
  int blocks_x;    // ceil(X / SECONDARY3D_BLOCK)
  int segs;        // ceil(Z / SECONDARY3D_SEG)
  long long rows;  // F * Z * Y
};

// one step of a column walk over a voxel of value v
__device__ __forceinline__ void secondary3d_step(int v, int& lab, int& dist) {
  if (v != 0) {
    lab = v;
    dist = 0;
  } else if (dist < SECONDARY3D_FAR) {
    ++dist;
  }
}

__device__ __forceinline__ uint32_t secondary3d_word(int lab, int dist, int reach, int step) {
  return dist <= reach ? ((uint32_t)(dist * step) << 16) | (uint32_t)lab : SECONDARY3D_NONE;
}

// grid = F * segs * blocks_p, p fastest
__global__ __launch_bounds__(SECONDARY3D_BLOCK) void k_secondary3d_z(Secondary3dArgs a) {
  const int Z = a.Z, rz = a.rz, sz = a.sz;
  const size_t P = (size_t)a.P;
  const int bp = (int)(blockIdx.x % (unsigned int)a.blocks_p);
  const unsigned int rest = blockIdx.x / (unsigned int)a.blocks_p;
  const int seg = (int)(rest % (unsigned int)a.segs);
  const size_t f = rest / (unsigned int)a.segs;
  const int p = bp * SECONDARY3D_BLOCK + (int)threadIdx.x;
  if (p >= a.P) return;
  const int z0 = seg * SECONDARY3D_SEG;
  const u16* col = a.labels + f * (size_t)Z * P + (size_t)p;  // col[z * P]: this stack's column
  uint32_t* wcol = a.zwords + f * (size_t)Z * P + (size_t)p;

  uint32_t down[SECONDARY3D_SEG];
  int lab = 0, dist = SECONDARY3D_FAR;
#pragma unroll 4
  for (int z = max(z0 - rz, 0); z < z0; ++z) secondary3d_step((int)col[(size_t)z * P], lab, dist);
#pragma unroll
  for (int i = 0; i < SECONDARY3D_SEG; ++i) {
    const int z = z0 + i;
    down[i] = SECONDARY3D_NONE;
    if (z < Z) {
      secondary3d_step((int)col[(size_t)z * P], lab, dist);
      down[i] = secondary3d_word(lab, dist, rz, sz);
    }
  }
  lab = 0;
  dist = SECONDARY3D_FAR;
#pragma unroll 4
  for (int z = min(z0 + SECONDARY3D_SEG + rz, Z) - 1; z >= z0 + SECONDARY3D_SEG; --z) secondary3d_step((int)col[(size_t)z * P], lab, dist);
#pragma unroll
  for (int i = SECONDARY3D_SEG - 1; i >= 0; --i) {
    const int z = z0 + i;
    if (z < Z) {
      // (a labelled voxel is the down word with g = 0: the label volume is not read again inside the segment)
      secondary3d_step((down[i] >> 16) == 0u ? (int)(down[i] & 0xffffu) : 0, lab, dist);
      wcol[(size_t)z * P] = min(down[i], secondary3d_word(lab, dist, rz, sz));
    }
  }
}

// one candidate of a scan: the word w (distance field `field`, squared already or not) seen at the squared offset s2
__device__ __forceinline__ uint32_t secondary3d_take(uint32_t best, uint32_t w, uint32_t field2, uint32_t s2, uint32_t limit) {
  const uint32_t d2 = field2 + s2;  // at most 2 * 255^2
  return (w >> 16) != 0xffffu && d2 <= limit ? min(best, (d2 << 16) | (w & 0xffffu)) : best;
}

// grid = F * Z * blocks_p, p fastest: one plane per group of blocks_p workgroups
__global__ __launch_bounds__(SECONDARY3D_BLOCK) void k_secondary3d_y(Secondary3dArgs a) {
  const int Y = a.Y, X = a.X, ry = a.ry, sy = a.sy;
  const int bp = (int)(blockIdx.x % (unsigned int)a.blocks_p);
  const size_t plane = blockIdx.x / (unsigned int)a.blocks_p;  // f * Z + z
  const int p = bp * SECONDARY3D_BLOCK + (int)threadIdx.x;
  if (p >= a.P) return;
  const int y = p / X;
  const size_t at = plane * (size_t)a.P + (size_t)p;
  const uint32_t* w = a.zwords + at;
  const uint32_t limit = (uint32_t)(a.N * a.N);
  const int up = min(ry, y), down = min(ry, Y - 1 - y);  // the rows of this plane on either side
  uint32_t best = SECONDARY3D_NONE;
  {
    const uint32_t w0 = w[0], g = w0 >> 16;
    best = secondary3d_take(best, w0, g * g, 0u, limit);
  }
  for (int dy = 1; dy <= max(up, down); ++dy) {
    const uint32_t s = (uint32_t)(sy * dy), s2 = s * s;
    if (s2 > min(best >> 16, limit)) break;  // no row farther out can reach, or tie with, the best distance
    if (dy <= up) {
      const uint32_t wu = w[-(ptrdiff_t)dy * X], g = wu >> 16;
      best = secondary3d_take(best, wu, g * g, s2, limit);
    }
    if (dy <= down) {
      const uint32_t wd = w[(ptrdiff_t)dy * X], g = wd >> 16;
      best = secondary3d_take(best, wd, g * g, s2, limit);
    }
  }
  a.ywords[at] = best;
}

// grid = ceil(rows / SECONDARY3D_ROWS) * blocks_x, x fastest: SECONDARY3D_ROWS rows x SECONDARY3D_BLOCK voxels per workgroup
__global__ __launch_bounds__(SECONDARY3D_BLOCK) void k_secondary3d_x(Secondary3dArgs a) {
  __shared__ uint32_t seg[SECONDARY3D_ROWS][SECONDARY3D_BLOCK + 2 * SECONDARY3D_MAX_REACH];
  const int X = a.X, rx = a.rx, sx = a.sx;
  const int bx = (int)(blockIdx.x % (unsigned int)a.blocks_x);
  const long long row0 = (long long)(blockIdx.x / (unsigned int)a.blocks_x) * SECONDARY3D_ROWS;
  const int x0 = bx * SECONDARY3D_BLOCK, tid = (int)threadIdx.x;
  // every thread stages its own word of each row, and the first 2 rx threads one halo word of each row (rx to the left of the
  // segment, rx to its right): all loads of the workgroup are issued before the one barrier
  const int x = x0 + tid;
  const bool halo = tid < 2 * rx;
  const int hi = tid < rx ? tid : SECONDARY3D_BLOCK + tid;  // the halo word's place in a staged row; its voxel is x0 - rx + hi
  const int xh = x0 - rx + hi;
  uint32_t m[SECONDARY3D_ROWS], h[SECONDARY3D_ROWS];
#pragma unroll
  for (int r = 0; r < SECONDARY3D_ROWS; ++r) {
    const bool live = row0 + r < a.rows;
    const uint32_t* wrow = a.ywords + (size_t)(row0 + r) * (size_t)X;
    m[r] = live && x < X ? wrow[x] : SECONDARY3D_NONE;
    h[r] = live && halo && xh >= 0 && xh < X ? wrow[xh] : SECONDARY3D_NONE;
  }
#pragma unroll
  for (int r = 0; r < SECONDARY3D_ROWS; ++r) {
    seg[r][rx + tid] = m[r];
    if (halo) seg[r][hi] = h[r];
  }
  __syncthreads();
  if (x >= X) return;
  const uint32_t limit = (uint32_t)(a.N * a.N);
  for (int r = 0; r < SECONDARY3D_ROWS && row0 + r < a.rows; ++r) {
    const uint32_t* mid = seg[r] + rx + tid;
    uint32_t best = mid[0];  // a y word: its distance is squared and within N^2 already, or it is NONE
    for (int dx = 1; dx <= rx; ++dx) {
      const uint32_t s = (uint32_t)(sx * dx), s2 = s * s;
      if (s2 > min(best >> 16, limit)) break;  // no column farther out can reach, or tie with, the best distance
      const uint32_t wl = mid[-dx], wr = mid[dx];
      best = secondary3d_take(best, wl, wl >> 16, s2, limit);
      best = secondary3d_take(best, wr, wr >> 16, s2, limit);
    }
    a.out[(size_t)(row0 + r) * (size_t)X + (size_t)x] = (best >> 16) <= limit ? (u16)(best & 0xffffu) : (u16)0;
  }
}

// F * Z * Y * X * bytes, or SIZE_MAX where that does not fit
static size_t secondary3d_bytes(int F, int Z, int Y, int X, size_t bytes) {
  size_t n = bytes;
  const int dims[4] = {F, Z, Y, X};
  for (int d : dims)
    if (__builtin_mul_overflow(n, (size_t)d, &n)) return SIZE_MAX;
  return n;
}

extern "C" size_t aliby_secondary_volume_workspace_bytes(int F, int Z, int Y, int X) {
  if (F <= 0 || Z <= 0 || Y <= 0 || X <= 0) return 0;
  return secondary3d_bytes(F, Z, Y, X, 2 * sizeof(uint32_t));
}

extern "C" int aliby_secondary_volume(aliby_ctx* ctx, const uint16_t* primary, int F, int Z, int Y, int X, int distance, int sz,
                                      int sy, int sx, void* workspace, size_t workspace_bytes, uint16_t* out, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  // (a plane's flat index plus a workgroup's width stays an int)
  ARG_CHECK(F >= 0 && Z >= 0 && Y >= 0 && X >= 0 && (long long)Y * X <= INT_MAX - SECONDARY3D_BLOCK && (long long)F * Z <= INT_MAX,
            "bad shape");
  ARG_CHECK(distance >= 1 && distance <= SECONDARY3D_MAX_DISTANCE, "distance must be in 1..255");
  ARG_CHECK(sz >= 1 && sz <= 255 && sy >= 1 && sy <= 255 && sx >= 1 && sx <= 255, "every spacing component must be in 1..255");
  ARG_CHECK(distance / sz <= SECONDARY3D_MAX_REACH && distance / sy <= SECONDARY3D_MAX_REACH && distance / sx <= SECONDARY3D_MAX_REACH,
            "the reach distance / spacing must be at most 64 voxels on every axis");
  if (F == 0 || Z == 0 || Y == 0 || X == 0) return ALIBY_OK;
  ARG_CHECK(primary && out, "NULL argument");
  ARG_CHECK(out != primary, "out must not alias primary (the primary labels are an input of the steps after this one)");
  ARG_CHECK(workspace != nullptr && ((uintptr_t)workspace & 3) == 0, "workspace is NULL or not 4-byte aligned");
  Secondary3dArgs a;
  a.labels = primary; a.out = out; a.Z = Z; a.Y = Y; a.X = X; a.P = Y * X;
  a.N = distance; a.sz = sz; a.sy = sy; a.sx = sx; a.rz = distance / sz; a.ry = distance / sy; a.rx = distance / sx;
  a.blocks_p = (a.P + SECONDARY3D_BLOCK - 1) / SECONDARY3D_BLOCK;
  a.blocks_x = (X + SECONDARY3D_BLOCK - 1) / SECONDARY3D_BLOCK;
  a.segs = (Z + SECONDARY3D_SEG - 1) / SECONDARY3D_SEG;
  a.rows = (long long)F * Z * Y;  // (F * Z and Y are ints: no overflow)
  const long long blocks_z = (long long)F * a.segs * a.blocks_p, blocks_y = (long long)F * Z * a.blocks_p;
  const long long blocks_x = (a.rows + SECONDARY3D_ROWS - 1) / SECONDARY3D_ROWS * a.blocks_x;
  ARG_CHECK(blocks_y <= INT_MAX, "too many voxels for one launch (F * Z * ceil(Y * X / 256) > INT_MAX)");
  ARG_CHECK(blocks_x <= INT_MAX, "too many rows for one launch (ceil(F * Z * Y / 8) * ceil(X / 256) > INT_MAX)");
  ARG_CHECK(workspace_bytes >= aliby_secondary_volume_workspace_bytes(F, Z, Y, X),
            "workspace is smaller than aliby_secondary_volume_workspace_bytes");
  a.zwords = static_cast<uint32_t*>(workspace);
  a.ywords = a.zwords + (size_t)a.rows * (size_t)X;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_secondary3d_z, dim3((unsigned int)blocks_z), dim3(SECONDARY3D_BLOCK), 0, s, a);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_secondary3d_y, dim3((unsigned int)blocks_y), dim3(SECONDARY3D_BLOCK), 0, s, a);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_secondary3d_x, dim3((unsigned int)blocks_x), dim3(SECONDARY3D_BLOCK), 0, s, a);
  KERNEL_CHECK();
  return ALIBY_OK;
}
