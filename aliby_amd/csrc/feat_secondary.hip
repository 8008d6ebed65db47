// feat_secondary.hip — "secondary": CellProfiler's IdentifySecondaryObjects, method "Distance - N": every primary object grows by up
// to N pixels into the background and the grown pixels carry its label.  CellProfiler computes it as
// scipy.ndimage.distance_transform_edt(labels == 0, return_indices=True) and labels_out[dist <= N] = labels_in[i, j]
// (skimage.segmentation.expand_labels); this file is that, with the one freedom SciPy leaves (which of several equally near pixels
// the index points to, a matter of its sweep order) fixed by a rule: ties go to the smaller label.  tests/secondary_ref.py restates it
// by brute force and tests/test_cpu_secondary_ref.py holds the restatement against SciPy on every pixel that is not a tie.
//
// Per tile of labels uint16 [F,Y,X] (0 = background), for a pixel p:
//   labels[p] != 0                       out[p] = labels[p]
//   else, m = min |p - q|^2 over the pixels q of the tile with labels[q] != 0 (an integer):
//     no such q, or m > N^2              out[p] = 0
//     else                               out[p] = min{ labels[q] : |p - q|^2 = m }
// N in 1..64.  Labels keep the primary numbering (65535 is a label like any other), nothing crosses a tile edge, and every step is
// integer arithmetic: a tile carries the same bits whatever the batch, the launch form and the stream.
// Not built: "Watershed", discarding objects that touch the border.  ("Propagation", "Distance - B": feat_propagate.hip; volume labels:
// feat_secondary3d.hip.)
//
// The exact separable form, two launches and one 4-byte-per-pixel intermediate (the caller's workspace):
// k_secondary_columns  a lane owns one column x of a segment of SECONDARY_SEG rows of one tile.  It walks down from N rows above the
//                      segment carrying the last label seen and its vertical distance, keeps the segment's SECONDARY_SEG results in
//                      registers, walks up from N rows below it the same way, and writes for every pixel of the segment the smaller
//                      of the two words (g << 16) | label: g = the vertical distance to the nearest labelled pixel of the column,
//                      that pixel's label, above and below equally near -> the smaller label (the word order is that rule).  A
//                      column without a labelled pixel within N rows gets SECONDARY_NONE (g field 0xffff; label 65535 with g = 0 is
//                      0x0000ffff: no collision).  A farther pixel of the same column can never win at any dx, so the nearest one is
//                      all a column contributes.  The walks start inside the tile: rows of another tile are never read.  Accesses
//                      are coalesced along x; the halo rows re-read what a neighbouring segment reads (cache hits), so the
//                      algorithmic traffic is 2 B read + 4 B written per pixel.  (Two adjacent columns per lane, with 4-byte reads
//                      and 8-byte writes, took 142 registers for the kept words and was slower at every N: 0.31 against 0.27 ms at
//                      N = 1 on 64 tiles of 1024 x 1024.)
// k_secondary_rows     a workgroup stages 256 words of each of 8 rows of one tile plus N on either side in LDS (outside the tile:
//                      SECONDARY_NONE; one row per workgroup left each thread a single load ahead of its barrier, and the launch
//                      bound by that latency), and every pixel takes the minimum over |dx| <= N of the key
//                      ((dx^2 + g^2) << 16) | label, a uint32 (at most 2 * 64^2 = 8192 in the upper half), outwards from dx = 0 and
//                      only while dx^2 <= the best distance so far:
//                      a pixel of an object stops at once, a pixel next to one after a step or two.  It writes the key's label, or
//                      0 where the distance exceeds N^2: 4 B read + 2 B written per pixel.
// Neither kernel caps its grid: the entry refuses a block count above INT_MAX.
#include "common.h"

typedef unsigned short u16;

#define SECONDARY_MAX_DISTANCE 64
#define SECONDARY_NONE 0xffffffffu
#define SECONDARY_SEG 32    // rows of a column segment: their down-walk words stay in registers
#define SECONDARY_BLOCK 256  // either kernel: one pixel of a row (one column of a segment) per thread
#define SECONDARY_ROWS 8     // rows of a workgroup of the row pass: eight independent loads per thread ahead of its barrier
#define SECONDARY_FAR (1 << 20)  // a vertical distance no walk reaches: "no labelled pixel seen"

struct SecondaryArgs {
  const u16* labels;
  uint32_t* words;  // [F,Y,X]
  u16* out;
  int F, Y, X, N;
  int blocks_x;  // ceil(X / SECONDARY_BLOCK)
  int segs;      // ceil(Y / SECONDARY_SEG)
  int row_groups;  // ceil(Y / SECONDARY_ROWS)
};

// one step of a column walk over a pixel of value v
__device__ __forceinline__ void secondary_step(int v, int& lab, int& dist) {
  if (v != 0) {
    lab = v;
    dist = 0;
  } else if (dist < SECONDARY_FAR) {
    ++dist;
  }
}

__device__ __forceinline__ uint32_t secondary_word(int lab, int dist, int N) {
  return dist <= N ? ((uint32_t)dist << 16) | (uint32_t)lab : SECONDARY_NONE;
}

// grid = F * segs * blocks_x, x fastest
__global__ __launch_bounds__(SECONDARY_BLOCK) void k_secondary_columns(SecondaryArgs a) {
  const int Y = a.Y, X = a.X, N = a.N;
  const int bx = (int)(blockIdx.x % (unsigned int)a.blocks_x);
  const unsigned int rest = blockIdx.x / (unsigned int)a.blocks_x;
  const int seg = (int)(rest % (unsigned int)a.segs);
  const size_t f = rest / (unsigned int)a.segs;
  const int x = bx * SECONDARY_BLOCK + (int)threadIdx.x;
  if (x >= X) return;
  const int y0 = seg * SECONDARY_SEG;
  const u16* col = a.labels + f * (size_t)Y * X + x;  // col[y * X]: this tile's column
  uint32_t* wcol = a.words + f * (size_t)Y * X + x;

  uint32_t down[SECONDARY_SEG];
  int lab = 0, dist = SECONDARY_FAR;
#pragma unroll 4
  for (int y = max(y0 - N, 0); y < y0; ++y) secondary_step((int)col[(size_t)y * X], lab, dist);
#pragma unroll
  for (int i = 0; i < SECONDARY_SEG; ++i) {
    const int y = y0 + i;
    down[i] = SECONDARY_NONE;
    if (y < Y) {
      secondary_step((int)col[(size_t)y * X], lab, dist);
      down[i] = secondary_word(lab, dist, N);
    }
  }
  lab = 0;
  dist = SECONDARY_FAR;
#pragma unroll 4
  for (int y = min(y0 + SECONDARY_SEG + N, Y) - 1; y >= y0 + SECONDARY_SEG; --y) secondary_step((int)col[(size_t)y * X], lab, dist);
#pragma unroll
  for (int i = SECONDARY_SEG - 1; i >= 0; --i) {
    const int y = y0 + i;
    if (y < Y) {
      // (a labelled pixel is the down word with g = 0: the label image is not read again inside the segment)
      secondary_step((down[i] >> 16) == 0u ? (int)(down[i] & 0xffffu) : 0, lab, dist);
      wcol[(size_t)y * X] = min(down[i], secondary_word(lab, dist, N));
    }
  }
}

// grid = F * row_groups * blocks_x, x fastest: SECONDARY_ROWS rows of one tile x SECONDARY_BLOCK pixels per workgroup
__global__ __launch_bounds__(SECONDARY_BLOCK) void k_secondary_rows(SecondaryArgs a) {
  __shared__ uint32_t seg[SECONDARY_ROWS][SECONDARY_BLOCK + 2 * SECONDARY_MAX_DISTANCE];
  const int Y = a.Y, X = a.X, N = a.N;
  const int bx = (int)(blockIdx.x % (unsigned int)a.blocks_x);
  const unsigned int rest = blockIdx.x / (unsigned int)a.blocks_x;
  const int y0 = (int)(rest % (unsigned int)a.row_groups) * SECONDARY_ROWS;
  const size_t f = rest / (unsigned int)a.row_groups;
  const int x0 = bx * SECONDARY_BLOCK, tid = (int)threadIdx.x;
  const uint32_t* wtile = a.words + f * (size_t)Y * X;
  // every thread stages its own word of each row, and the first 2 N threads one halo word of each row (N to the left of the
  // segment, N to its right): all loads of the workgroup are issued before the one barrier
  const int x = x0 + tid;
  const bool halo = tid < 2 * N;
  const int hi = tid < N ? tid : SECONDARY_BLOCK + tid;  // the halo word's place in a staged row; its pixel is x0 - N + hi
  const int xh = x0 - N + hi;
  uint32_t m[SECONDARY_ROWS], h[SECONDARY_ROWS];
#pragma unroll
  for (int r = 0; r < SECONDARY_ROWS; ++r) {
    const int y = y0 + r;
    const uint32_t* wrow = wtile + (size_t)y * X;
    m[r] = y < Y && x < X ? wrow[x] : SECONDARY_NONE;
    h[r] = y < Y && halo && xh >= 0 && xh < X ? wrow[xh] : SECONDARY_NONE;
  }
#pragma unroll
  for (int r = 0; r < SECONDARY_ROWS; ++r) {
    seg[r][N + tid] = m[r];
    if (halo) seg[r][hi] = h[r];
  }
  __syncthreads();
  if (x >= X) return;
  const uint32_t limit = (uint32_t)(N * N);
  for (int r = 0; r < SECONDARY_ROWS && y0 + r < Y; ++r) {
    const uint32_t* mid = seg[r] + N + tid;
    uint32_t best = SECONDARY_NONE;
    {
      const uint32_t w = mid[0];
      if ((w >> 16) != 0xffffu) best = (((w >> 16) * (w >> 16)) << 16) | (w & 0xffffu);
    }
    for (int dx = 1; dx <= N; ++dx) {
      const uint32_t dx2 = (uint32_t)(dx * dx);
      if (dx2 > min(best >> 16, limit)) break;  // no column farther out can reach, or tie with, the best distance
      const uint32_t wl = mid[-dx], wr = mid[dx];
      const uint32_t gl = wl >> 16, gr = wr >> 16;
      if (gl != 0xffffu) best = min(best, ((dx2 + gl * gl) << 16) | (wl & 0xffffu));
      if (gr != 0xffffu) best = min(best, ((dx2 + gr * gr) << 16) | (wr & 0xffffu));
    }
    a.out[f * (size_t)Y * X + (size_t)(y0 + r) * X + x] = (best >> 16) <= limit ? (u16)(best & 0xffffu) : (u16)0;
  }
}

extern "C" size_t aliby_secondary_workspace_bytes(int F, int Y, int X) {
  if (F <= 0 || Y <= 0 || X <= 0) return 0;
  return (size_t)F * (size_t)Y * (size_t)X * sizeof(uint32_t);
}

extern "C" int aliby_secondary_labels(aliby_ctx* ctx, const uint16_t* primary, int F, int Y, int X, int distance, void* workspace,
                                      size_t workspace_bytes, uint16_t* out, void* stream) {
  ARG_CHECK(ctx != nullptr, "ctx is NULL");
  ARG_CHECK(F >= 0 && Y >= 0 && X >= 0 && (long long)Y * X <= INT_MAX, "bad shape");
  ARG_CHECK(distance >= 1 && distance <= SECONDARY_MAX_DISTANCE, "distance must be in 1..64");
  if (F == 0 || Y == 0 || X == 0) return ALIBY_OK;
  ARG_CHECK(primary && out, "NULL argument");
  ARG_CHECK(out != primary, "out must not alias primary (the primary labels are an input of the steps after this one)");
  ARG_CHECK(workspace != nullptr && ((uintptr_t)workspace & 3) == 0, "workspace is NULL or not 4-byte aligned");
  ARG_CHECK(workspace_bytes >= aliby_secondary_workspace_bytes(F, Y, X), "workspace is smaller than aliby_secondary_workspace_bytes");
  SecondaryArgs a;
  a.labels = primary; a.words = static_cast<uint32_t*>(workspace); a.out = out; a.F = F; a.Y = Y; a.X = X; a.N = distance;
  a.blocks_x = (X + SECONDARY_BLOCK - 1) / SECONDARY_BLOCK;
  a.segs = (Y + SECONDARY_SEG - 1) / SECONDARY_SEG;
  a.row_groups = (Y + SECONDARY_ROWS - 1) / SECONDARY_ROWS;
  const long long blocks_rows = (long long)F * a.row_groups * a.blocks_x, blocks_cols = (long long)F * a.segs * a.blocks_x;
  ARG_CHECK(blocks_rows <= INT_MAX, "too many rows for one launch (F * ceil(Y / 8) * ceil(X / 256) > INT_MAX)");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_secondary_columns, dim3((unsigned int)blocks_cols), dim3(SECONDARY_BLOCK), 0, s, a);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_secondary_rows, dim3((unsigned int)blocks_rows), dim3(SECONDARY_BLOCK), 0, s, a);
  KERNEL_CHECK();
  return ALIBY_OK;
}
