// feat_projection3d.hip — how the reference's collapse of a 3-D label result (the maximum over z, then a sequential relabel:
// segment/dispatch.py:218-223, aliby_amd.segment.model.max_project_and_relabel) sees each object of a labelled Z-stack [F, Z, Y, X]:
// in how many columns (y, x) it has a voxel, in how many of them it is the value the maximum keeps, and which label it carries in the
// collapsed image.  The last is the join key between the rows of the volume families and the rows measured on the collapse.
// The definition is in include/aliby_hip.h (aliby_features_projection3d); tests/projection3d_ref.py restates it.
//
// One pass over the labels, F * Z * Y * X * 2 bytes: a lane walks one column down z, the lanes of a wave are adjacent in x, so a
// wave reads 128 consecutive bytes per plane.  Integer atomics only (two counts per object and one presence bit per value that is
// the top of some column), so the result is exact whatever the order; a second kernel, one workgroup per stack, ranks the bits.
#include "volume_pass.h"

#define P3_GRID_CAP 4096               // workgroups of the column walk, at most: more columns go round the grid-stride loop
#define P3_WORDS 2048                  // presence bits of one stack: 65536 values / 32
#define P3_NONE 0xffffffffffffffffull  // key of a lane that has nothing to add

namespace {

// visit(key, how many lanes hold it), by the first lane of every group of lanes with the same key; P3_NONE takes no part.  All 64
// lanes of the wave call it.  Lanes of a wave mostly lie in the same object: one atomic per object and wave instead of one per lane.
template <class Visit>
__device__ __forceinline__ void wave_groups(unsigned long long key, Visit visit) {
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(key != P3_NONE);
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const unsigned long long k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k);
    if (lane == leader) visit(k, (unsigned)__popcll(same));
    pending &= ~same;
  }
}

// labels [F, Z, Y, X]; offsets[f] = first row of stack f; row = offsets[f] + label - 1; area / vis [rows]; present [F][P3_WORDS]
__global__ __launch_bounds__(256) void k_projection3d(const uint16_t* __restrict__ labels, int F, int Z, int Y, int X, const int* __restrict__ offsets,
                                                      unsigned* __restrict__ area, unsigned* __restrict__ vis, unsigned* __restrict__ present) {
  const size_t plane = (size_t)Y * X, vol = plane * Z, total = plane * F;
  // (the bound is the workgroup's: every lane of a wave goes round together, for the ballots of wave_groups)
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x; i0 < total; i0 += (size_t)gridDim.x * blockDim.x) {
    const size_t i = i0 + threadIdx.x;
    unsigned long long k0 = P3_NONE, k1 = P3_NONE, ktop = P3_NONE;
    if (i < total) {
      const size_t f = i / plane;
      const uint16_t* col = labels + f * vol + (i - f * plane);
      const int base = offsets[f], nrows = offsets[f + 1] - base;
      // l0, l1: the first two labels of the column that have a row; a third and later ones are counted on the spot, after a look
      // back up the column once the two no longer tell whether a label is new
      unsigned prev = 0, top = 0, l0 = 0, l1 = 0;
      bool more = false;
      for (int z0 = 0; z0 < Z; z0 += 8) {
        unsigned v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = z0 + k < Z ? col[(size_t)(z0 + k) * plane] : 0u;  // (background below the stack changes nothing)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const unsigned L = v[k];
          if (L == prev) continue;
          prev = L;
          top = L > top ? L : top;
          if (!L || (int)L > nrows || L == l0 || L == l1) continue;
          if (!l0) l0 = L;
          else if (!l1) l1 = L;
          else {
            bool seen = false;
            if (more)
              for (int zb = 0; zb < z0 + k && !seen; ++zb) seen = col[(size_t)zb * plane] == L;
            if (!seen) atomicAdd(&area[base + (int)L - 1], 1u);
            more = true;
          }
        }
      }
      if (l0) k0 = (unsigned long long)(base + (int)l0 - 1);
      if (l1) k1 = (unsigned long long)(base + (int)l1 - 1);
      if (top) ktop = ((unsigned long long)f << 16) | top;
    }
    wave_groups(k0, [&](unsigned long long row, unsigned n) { atomicAdd(&area[row], n); });
    wave_groups(k1, [&](unsigned long long row, unsigned n) { atomicAdd(&area[row], n); });
    wave_groups(ktop, [&](unsigned long long key, unsigned n) {
      const size_t f = (size_t)(key >> 16);
      const unsigned top = (unsigned)(key & 0xffffu);
      const int base = offsets[f], nrows = offsets[f + 1] - base;
      unsigned* word = present + f * P3_WORDS + (top >> 5);
      const unsigned bit = 1u << (top & 31u);
      if (!(*word & bit)) atomicOr(word, bit);  // (a stale read costs one more atomic, nothing else: bits are only ever set)
      if ((int)top <= nrows) atomicAdd(&vis[base + (int)top - 1], n);
    });
  }
}

// One workgroup per stack: the rank of every value among the present ones, then the four columns of the stack's rows.
__global__ __launch_bounds__(256) void k_projection3d_finish(const int* __restrict__ offsets, const unsigned* __restrict__ area,
                                                             const unsigned* __restrict__ vis, const unsigned* __restrict__ present,
                                                             double* __restrict__ out, int ld, int col0) {
  __shared__ int before[P3_WORDS];  // present values in the words up to and including this one
  __shared__ int part[256];
  const int f = blockIdx.x;
  const int base = offsets[f], nrows = offsets[f + 1] - base;
  if (nrows <= 0) return;
  const unsigned* bits = present + (size_t)f * P3_WORDS;
  for (int w = threadIdx.x; w < P3_WORDS; w += blockDim.x) before[w] = __popc(bits[w]);
  __syncthreads();
  block_inclusive_scan(before, P3_WORDS, part);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int L = 1 + (int)threadIdx.x; L <= nrows; L += blockDim.x) {
    const unsigned word = bits[L >> 5], bit = 1u << (L & 31);
    // the 1-based rank of L among the present values: those in lower words, those below it in its own word, and itself
    const int rank = before[L >> 5] - __popc(word) + __popc(word & (bit - 1u)) + 1;
    const unsigned a = area[base + L - 1], v = vis[base + L - 1];
    double* o = out + (size_t)(base + L - 1) * ld + col0;
    o[0] = (double)a;
    o[1] = (double)v;
    o[2] = a ? (double)v / (double)a : nan;
    o[3] = (word & bit) ? (double)rank : 0.0;
  }
}

}  // namespace

extern "C" int aliby_features_projection3d(aliby_ctx* ctx, const uint16_t* labels, int F, int Z, int Y, int X, const int32_t* offsets_host,
                                           double* out, int ld, int col0, void* stream) {
  ARG_CHECK(ctx && labels && offsets_host && out, "projection3d: null argument");
  // (a count is at most Y * X <= 2^32 - 1 only below that many columns: a stack of 2^32 columns of one label is refused)
  if (!volume_shape_ok("projection3d", F, Z, Y, X, offsets_host, 1ull << 40)) return ALIBY_ERR_INVALID;
  ARG_CHECK((size_t)Y * X < (1ull << 32), "projection3d: too many columns per stack");
  ARG_CHECK(col0 >= 0 && ld >= col0 + 4, "projection3d: bad output stride");
  const int n = offsets_host[F];
  if (n <= 0) return ALIBY_OK;
  hipStream_t s = as_stream(stream);
  // scratch: [area n][vis n][present F * P3_WORDS][offsets F + 1]
  const size_t count_words = (size_t)n * 2, bit_words = (size_t)F * P3_WORDS;
  int rc = aliby_ensure_scratch(ctx, sizeof(unsigned) * (count_words + bit_words + (size_t)(F + 1)) + 64);
  if (rc) return rc;
  unsigned* area = (unsigned*)ctx->scratch;
  unsigned* vis = area + n;
  unsigned* present = vis + n;
  int* d_off = (int*)(present + bit_words);
  HIP_TRY(hipMemsetAsync(area, 0, sizeof(unsigned) * (count_words + bit_words), s));
  HIP_TRY(hipMemcpyAsync(d_off, offsets_host, sizeof(int) * (size_t)(F + 1), hipMemcpyHostToDevice, s));
  const size_t blocks = ((size_t)F * Y * X + 255) / 256;
  hipLaunchKernelGGL(k_projection3d, dim3((unsigned)(blocks < P3_GRID_CAP ? blocks : P3_GRID_CAP)), dim3(256), 0, s, labels, F, Z, Y, X, d_off, area,
                     vis, present);
  KERNEL_CHECK();
  hipLaunchKernelGGL(k_projection3d_finish, dim3((unsigned)F), dim3(256), 0, s, d_off, area, vis, present, out, ld, col0);
  KERNEL_CHECK();
  // the counts, the bits and the offsets live in ctx scratch: they must be consumed before the host reuses it
  return aliby_wait_stream(s);
}
