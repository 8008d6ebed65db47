// volume_pass.h — what the kernels that walk a whole label stack [F, Z, Y, X] share (feat_intensity3d.hip, feat_sizeshape3d.hip,
// feat_surface3d.hip, and k_volume_table of volume_table.h): the decode of a work item, the 2 x 2 x 2 window walk over an 8 x 8 x 64
// tile in LDS, and the host's checks of the shape, the offsets and the spacing.
#pragma once
#include "common.h"

// A workgroup's tile of window positions and the lanes' share of it: 8 * 8 * (64 / 16) = 256 lanes of 16 positions along x.  The
// staged voxels are the tile's own plus a one-voxel halo on one side of every axis: 9 x 9 x 65 uint16 = 10.3 KB of LDS.
#define VP_TZ 8
#define VP_TY 8
#define VP_TX 64
#define VP_RUN 16
#define VP_HZ (VP_TZ + 1)
#define VP_HY (VP_TY + 1)
#define VP_HX (VP_TX + 1)

// Work item i = ((f * nz + z) * ny + y) * nx + x of a grid-stride loop: the tile of a window kernel, the 16-voxel segment x of row
// (z, y) in a row-run kernel
struct StackIndex { int f, z, y, x; };
__device__ __forceinline__ StackIndex stack_index(size_t i, int nz, int ny, int nx) {
  StackIndex p;
  p.x = (int)(i % nx);
  size_t rest = i / nx;
  p.y = (int)(rest % ny);
  rest /= ny;
  p.z = (int)(rest % nz);
  p.f = (int)(rest / nz);
  return p;
}

// tile[hz][hy][hx] = voxel (oz + hz, oy + hy, ox + hx) of the stack lab [Z, Y, X], background outside it; all 256 lanes, between two
// barriers.  LOW: the origin is a low-side halo and may be -1 (without it those tests are not compiled).
template <bool LOW>
__device__ __forceinline__ void window_stage(uint16_t* tile, const uint16_t* lab, int Z, int Y, int X, int oz, int oy, int ox) {
  __syncthreads();  // the previous tile has been read
  for (int i = threadIdx.x; i < VP_HZ * VP_HY * VP_HX; i += 256) {
    const int hx = i % VP_HX, r = i / VP_HX, hy = r % VP_HY, hz = r / VP_HY;
    const int gz = oz + hz, gy = oy + hy, gx = ox + hx;
    uint16_t v = 0;
    if ((!LOW || (gz >= 0 && gy >= 0 && gx >= 0)) && gz < Z && gy < Y && gx < X) v = lab[((size_t)gz * Y + gy) * X + gx];
    tile[i] = v;
  }
  __syncthreads();
}

// visit(L, m) once for every distinct label L of the window w with 0 < L <= nrows, bit j of m set where w[j] == L.  A window that is
// all one value is skipped: all background holds no label, and all one label is the interior of an object.
template <class Visit>
__device__ __forceinline__ void window_labels(const unsigned (&w)[8], int nrows, Visit visit) {
  const unsigned any = w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7];
  const bool same = w[0] == w[1] && w[0] == w[2] && w[0] == w[3] && w[0] == w[4] && w[0] == w[5] && w[0] == w[6] && w[0] == w[7];
  if (!any || same) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned L = w[k];
    unsigned m = 0;
    bool first = L != 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (w[j] == L) {
        m |= 1u << j;
        if (j < k) first = false;
      }
    }
    if (first && (int)L <= nrows) visit(L, m);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// Shape and row offsets of a volume family `who`; max_voxels = what its sums or lists hold per stack.  (With other offsets labelled
// voxels would write past the accumulators.)
static inline bool volume_shape_ok(const char* who, int F, int Z, int Y, int X, const int32_t* offsets_host, size_t max_voxels) {
  const char* bad = nullptr;
  if (!(F > 0 && Z > 0 && Y > 0 && X > 0)) bad = "bad shape";
  else if (!(X <= 65536 && Y <= 65536 && Z <= 65536 && (size_t)Z * Y * X <= max_voxels)) bad = "stack too large";
  else if (!volume_offsets_ok(offsets_host, F)) bad = "bad offsets";
  if (bad) aliby_set_error("invalid argument: %s: %s", who, bad);
  return !bad;
}

static inline bool spacing_ok(const double* sp) {
  return sp[0] > 0.0 && sp[1] > 0.0 && sp[2] > 0.0 && sp[0] < 1e300 && sp[1] < 1e300 && sp[2] < 1e300;
}
