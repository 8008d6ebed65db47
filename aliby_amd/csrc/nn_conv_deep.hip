// nn_conv_deep.hip — the U-Net's 3x3 convolution unit at the deep levels (128 / 256 channels, 56 x 56 and 28 x 28 maps)
// as ONE launch with the whole K = 9 * CIN reduction accumulated in fp32 registers.
//
// Same unit as nn_conv.hip (cellpose's batchconv / batchconvstyle as driven by segment/dispatch.py:208-215):
//     OUT = conv3x3( relu(scale[c] * IN[n, y>>up, x>>up, c] + shift[n, c]) ) + bias + RES[n, y>>ru, x>>ru, :]
// Round 1 ran these layers as K-slices (64 input channels per launch) x N-slices (128 output channels) of the 64 -> 128
// kernel, each launch adding to the previous one through a bf16 tensor in HBM: a 256 -> 256 convolution was 8 launches that
// moved ~5x its algorithmic bytes and rounded its partial sums to 8 bits of mantissa three times.  Here:
//
//   * positions, not rows: the N images of a launch are stacked into one tall zero-separated image of width LW = W + 2 and
//     period HP = H + 1 rows (one shared zero row between images, one zero column left and right), flattened row-major.
//     A 3x3 tap is then a CONSTANT offset (dy-1)*LW + (dx-1) in that flat index, so a workgroup tile is simply RUN = 224
//     consecutive output positions (7 MFMA blocks of 32) and its input window RUN + 2*LW + 2 consecutive positions — no
//     per-row bookkeeping, no seam handling for 28- and 56-pixel images (cost: the zero row / columns are computed and
//     dropped, 1 - W/(W+2) * H/(H+1) = 10 % at 28, 5 % at 56);
//   * a wave owns 32 output channels x 7 position blocks = 7 accumulators (112 VGPRs) for the WHOLE reduction; a workgroup
//     is 4 waves = 128 output channels (layers with 256 are two tiles per run, adjacent in the schedule so that the second
//     finds the window in L2);
//   * K loop over 64-channel slices: the slice's window is staged once into LDS as channel-octet planes with the prologue
//     (BatchNorm affine + style shift + ReLU, zero padding after the activation — conv_act8 of conv_mfma.h) applied on the
//     way, then 4 k-steps x 9 taps x 7 blocks of v_mfma_f32_32x32x16_bf16 run from it;
//   * weights are NOT resident (9 * CIN/16 fragments per wave do not fit beside the accumulators): each (tap, k-step)
//     fragment — 1 KiB per wave, already in fragment order in the packed array, L2-resident — is loaded straight into VGPRs
//     through a 3-deep ring, seven MFMAs of cover each;
//   * two workgroups per CU (<= 256 VGPRs, 44 KiB of LDS each) overlap each other's staging and MFMA phases;
//   * input read through the 2x upsample (UP): the window is kept at INPUT resolution, the same tall image built over the
//     H/2 x W/2 inputs (conv_upmap.h).  A tile's window is then the <= DCU_WIN_MAX low positions that cover it: every raw pixel
//     is fetched, activated and written to LDS once per slice (5 staging rounds per thread instead of 11, 20 window registers
//     instead of 44, 25 KiB of LDS instead of 71), and the MFMA loop's fragment address is the lane's low base plus 0 / row parity / 1 low rows
//     and 0 / column parity / 1 columns: one v_add per read.  The same values enter the same MFMAs in the same order as with the
//     window at output resolution: same bits (tests/test_gpu_conv_upstage.py, against in_up = 0 on the materialised upsample).
#include "common.h"
#include "conv_launch.h"
#include "conv_mfma.h"
#include "conv_upmap.h"

namespace {

struct DeepArgs {
  const uint4* in;     // [N, H>>up, W>>up, CIN] bf16
  const uint4* wpk;    // aliby_nn_pack_conv3x3_bf16 over the full CIN: [cout block][tap][k-step][lane][8]
  uint4* out;          // [N, H, W, COUT] bf16
  const float* scale;  // [CIN]
  const float* shift;  // [N, CIN] (shift_stride = row stride) or [CIN] (0)
  const float* bias;   // [COUT] or NULL
  const uint4* res;    // [N, H>>res_up, W>>res_up, COUT] bf16 or NULL
  int shift_stride, res_up;
  int N, H, W, COUT;
  int LW, HP;          // W + 2, H + 1
  int q_begin, q_end;  // flat output positions [q_begin, q_end) of the tall image
  int nruns, nhalf, ntiles;
  int order;           // direction of the tile walk (tile_walk), set by launch<>
  int stagger;         // the second workgroup of every CU starts this many x 64 x 64 cycles late (see the kernel)
  unsigned long long* trace;  // diagnostics: shader-clock stamps of workgroup 0's first tiles (NULL in production)
};

#define DC_STAMP(slot_)                                                                                  \
  do {                                                                                                   \
    if (a.trace && blockIdx.x == 0 && tid == 0 && stamp_tile < 8 && (slot_) < 32)                        \
      a.trace[stamp_tile * 32 + (slot_)] = __builtin_amdgcn_s_memtime();                                 \
  } while (0)

constexpr int DC_NB = 7;              // position blocks of 32 per wave
constexpr int DC_RUN = DC_NB * 32;    // output positions per tile
constexpr int DC_WMAX = 56;           // widest image the LDS window is sized for
constexpr int DC_WIN_MAX = DC_RUN + 2 * (DC_WMAX + 2) + 2;
constexpr int DC_PLANE = DC_WIN_MAX | 1;       // odd slot pitch: the 8 octets of a position land in 8 distinct 16-byte slots
constexpr int DC_ITERS = (DC_WIN_MAX + 31) / 32;  // staging rounds: 32 positions x 8 octets per round of 256 threads
// planes + per-thread input offsets + prologue constants + per-thread output / residual offsets
constexpr int DC_LDS_BYTES = 8 * DC_PLANE * 16 + DC_ITERS * 256 * 4 + 3 * 256 * 4 + 2 * DC_NB * 256 * 4;
constexpr int DC_WDEPTH = 3;  // weight fragments in flight
constexpr int DC_PDEPTH = 4;  // pixel fragments in flight
constexpr int DC_REQ_AT = 27;  // weight fragment (of 36 per slice) before which the next slice's window is requested
// The UP instantiations keep the window at INPUT resolution (conv_upmap.h): a quarter of the pixels, each fetched, activated and
// written to LDS once; the MFMA loop's fragment reads go through the upsample.  DCU_WIN_MAX low positions cover every tile of every
// shape the entry point admits (up_win_fits checks the launch's own tiles; 145 is the most any even H, W <= DC_WMAX needs).
constexpr int DCU_WIN_MAX = 160;
constexpr int DCU_PLANE = DCU_WIN_MAX | 1;  // odd slot pitch: a ds_write_b128 lane group is the 8 octets of one position
constexpr int DCU_ITERS = DCU_WIN_MAX / 32;
constexpr int DCU_LDS_BYTES = 8 * DCU_PLANE * 16 + DCU_ITERS * 256 * 4;  // planes + per-thread input offsets
static_assert(DCU_WIN_MAX % 32 == 0 && DCU_WIN_MAX >= 2 * (DC_WMAX / 2 + 2) + 2, "window image of the UP form");

// ---- the stages that the three kernels of this file share (they differ in their K loops)
// 32 positions further in the tall image: column c, row y of image n
__device__ __forceinline__ void dc_step32(int& c, int& y, int& n, int LW, int HP) {
  c += 32;
  while (c >= LW) {  // (at most two wraps: LW >= 30 at the levels these kernels serve)
    c -= LW;
    if (++y == HP) { y = 0; ++n; }
  }
}
// pos positions further, any pos >= 0
__device__ __forceinline__ void dc_step(int& c, int& y, int& n, int LW, int HP, int pos) {
  c += pos;
  while (c >= LW) {
    c -= LW;
    if (++y == HP) { y = 0; ++n; }
  }
}
// window position P (flat index, >= -1) -> column, row, image (y < 0: rows above the first image)
__device__ __forceinline__ void dc_win_pos(int P, int LW, int HP, int& c, int& y, int& n) {
  const int r = P >= 0 ? P / LW : -1;
  c = P - r * LW;
  n = r >= 1 ? (r - 1) / HP : 0;
  y = r >= 1 ? (r - 1) - n * HP : r - 1;
}
// output position q -> column, row, image (its row is >= 1 always: q >= q_begin = LW)
__device__ __forceinline__ void dc_out_pos(int q, int LW, int HP, int& c, int& y, int& n) {
  const int r = q / LW;
  c = q - r * LW;
  n = (r - 1) / HP;
  y = (r - 1) - n * HP;
}
// input offset (16-byte units) of channel octet `oct` at window position (c, y, n), clamped to a valid address.  Bit `bit` of
// `inside`: the position is a pixel (and `valid`); of `later`: it belongs to an image after the window's first one, n0
template <bool UP>
__device__ __forceinline__ int dc_win_off(const DeepArgs& a, int c, int y, int n, int n0, int cs, int oct, bool valid, int bit,
                                          unsigned& inside, unsigned& later) {
  const int IH = UP ? a.H >> 1 : a.H, IW = UP ? a.W >> 1 : a.W;
  const bool ok = valid && y >= 0 && y < a.H && c >= 1 && c <= a.W && n < a.N;
  inside |= (unsigned)ok << bit;
  later |= (unsigned)(n > n0) << bit;
  const int nn = min(n, a.N - 1), yy = min(max(y, 0), a.H - 1), xx = min(max(c - 1, 0), a.W - 1);
  return ((nn * IH + (UP ? yy >> 1 : yy)) * IW + (UP ? xx >> 1 : xx)) * cs + oct;
}
// the same for a position (c, y, n) of the tall image at INPUT resolution (the UP forms: conv_upmap.h)
__device__ __forceinline__ int dc_low_off(const DeepArgs& a, int c, int y, int n, int n0, int cs, int oct, bool valid, int bit,
                                          unsigned& inside, unsigned& later) {
  const int IH = a.H >> 1, IW = a.W >> 1;
  const bool ok = valid && y >= 0 && y < IH && c >= 1 && c <= IW && n < a.N;
  inside |= (unsigned)ok << bit;
  later |= (unsigned)(n > n0) << bit;
  const int nn = min(n, a.N - 1), yy = min(max(y, 0), IH - 1), xx = min(max(c - 1, 0), IW - 1);
  return ((nn * IH + yy) * IW + xx) * cs + oct;
}
// UP forms: this lane's window addresses.  lb[b]: slot of the first window position of output position q0 + px + 32 b in the
// low window image that starts at low position lstart, bit b of rbits: its row parity bit (up_row_bit).  Clamped so that every
// tap of every lane reads inside a plane of `plane` slots (the positions that are not stored may read anything there)
__device__ __forceinline__ void dc_low_bases(int q0, int px, int LW, int HP, int lstart, int plane, int (&lb)[DC_NB], unsigned& rbits) {
  const int LWl = up_low_width(LW);
  int c, y, n;
  dc_out_pos(q0 + px, LW, HP, c, y, n);
  rbits = 0;
#pragma unroll
  for (int b = 0; b < DC_NB; ++b) {
    lb[b] = min(max(up_base(c, y, n, LW, HP) - lstart, 0), plane - LWl - 2);
    rbits |= (unsigned)up_row_bit(y) << b;
    dc_step32(c, y, n, LW, HP);
  }
}
// (The fragment addresses of a k-step are sums of lb[b], the row term and the column bit.  Re-read through an empty asm at the head of
// every k-step, the sums are formed again where they are used, one v_add per read, instead of being kept for the slice's other
// k-steps in registers that the accumulators do not leave: that spills.)
__device__ __forceinline__ void dc_fresh(int (&lb)[DC_NB]) {
  asm volatile("" : "+v"(lb[0]), "+v"(lb[1]), "+v"(lb[2]), "+v"(lb[3]), "+v"(lb[4]), "+v"(lb[5]), "+v"(lb[6]));
}
// prologue constants of K slice s for one channel octet: scale, and the style shifts of images n0 and n1
__device__ __forceinline__ void dc_prologue_consts(const DeepArgs& a, int s, int oct, int n0, int n1, f32x2_t (&sc)[4], f32x2_t (&sh)[4],
                                                   f32x2_t (&sh1)[4]) {
  const int ch = s * 64 + oct * 8;
  const float* sp0 = a.shift + (size_t)n0 * a.shift_stride + ch;
  const float* sp1 = a.shift + (size_t)n1 * a.shift_stride + ch;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sc[k] = f32x2_t{a.scale[ch + 2 * k], a.scale[ch + 2 * k + 1]};
    sh[k] = f32x2_t{sp0[2 * k], sp0[2 * k + 1]};
    sh1[k] = f32x2_t{sp1[2 * k], sp1[2 * k + 1]};
  }
}
// residual offset (16-byte units) of output channel c0 at (n, y, x); clamped: positions that are not stored (zero row / columns,
// past the last image) read some valid address
__device__ __forceinline__ unsigned dc_res_off(const DeepArgs& a, int n, int y, int x, int ocs, int c0) {
  const int RH = a.H >> a.res_up, RW = a.W >> a.res_up;
  const int nn = min(n, a.N - 1), yy = min(y, a.H - 1), xx = min(max(x, 0), a.W - 1);
  return (unsigned)(((nn * RH + (yy >> a.res_up)) * RW + (xx >> a.res_up)) * ocs + (c0 >> 3));
}
// 32x32x16 layout (a lane holds channels c0 .. c0 + 15 of positions q0 + px + 32 b).  The accumulators start at bias + residual
// (as in nn_conv.hip): the residual's loads are in flight together with the first window's, behind the first staging phase,
// instead of twice exposed in the epilogue, which is then convert + store
__device__ __forceinline__ void dc_seed32(const DeepArgs& a, int q0, int px, int c0, int ocs, int LW, int HP, f32x16_t (&acc)[DC_NB]) {
  float b16[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) b16[k] = a.bias ? a.bias[c0 + k] : 0.f;
  if (a.res) {
    uint4 rr[DC_NB][2];
    int c, y, n;
    dc_out_pos(q0 + px, LW, HP, c, y, n);
#pragma unroll
    for (int b = 0; b < DC_NB; ++b) {
      const unsigned roff = dc_res_off(a, n, y, c - 1, ocs, c0);
      rr[b][0] = a.res[roff];
      rr[b][1] = a.res[roff + 1];
      dc_step32(c, y, n, LW, HP);
    }
#pragma unroll
    for (int b = 0; b < DC_NB; ++b) {
      const unsigned rw[8] = {rr[b][0].x, rr[b][0].y, rr[b][0].z, rr[b][0].w, rr[b][1].x, rr[b][1].y, rr[b][1].z, rr[b][1].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        acc[b][2 * j] = b16[2 * j] + cv_bf2f(rw[j] & 0xffffu);
        acc[b][2 * j + 1] = b16[2 * j + 1] + cv_bf2f(rw[j] >> 16);
      }
    }
  } else {
#pragma unroll
    for (int b = 0; b < DC_NB; ++b)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[b][k] = b16[k];
  }
}
// ... and the epilogue: fp32 -> bf16, 32 contiguous bytes per lane and position.  Positions by stepping (no divisions)
__device__ __forceinline__ void dc_store32(const DeepArgs& a, int q0, int px, int c0, int ocs, int LW, int HP,
                                           const f32x16_t (&acc)[DC_NB]) {
  int c, y, n;
  dc_out_pos(q0 + px, LW, HP, c, y, n);
#pragma unroll
  for (int b = 0; b < DC_NB; ++b) {
    const int x = c - 1;
    const bool ok = q0 + b * 32 + px < a.q_end && y < a.H && x >= 0 && x < a.W && n < a.N;
    if (ok) {
      uint4* op = a.out + (unsigned)(((n * a.H + y) * a.W + x) * ocs + (c0 >> 3));
      acc_pack16(acc[b], op[0], op[1]);
    }
    dc_step32(c, y, n, LW, HP);
  }
}

template <int CIN, bool UP>
__global__ __launch_bounds__(256, 2) void k_conv3x3_deep(DeepArgs a) {
  constexpr int S = CIN / 64, KCT = CIN / 16;  // K slices, k-steps in the packed array
  extern __shared__ uint4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, cb = tid >> 6;
  const int px = lane & 31, hh = lane >> 5;
  const int pl = tid & 7, pos0 = tid >> 3;  // staging role: a fixed channel octet of position pos0 + 32 * round
  const int LW = a.LW, HP = a.HP;
  // the window image in LDS: at output resolution, or (UP) at input resolution, DCU_* and conv_upmap.h
  constexpr int PLANE = UP ? DCU_PLANE : DC_PLANE, ITERS = UP ? DCU_ITERS : DC_ITERS;
  const int LWI = UP ? up_low_width(LW) : LW, HPI = UP ? up_low_period(HP) : HP;  // its row width and period
  int WIN = DC_RUN + 2 * LW + 2;  // its positions (UP: per tile)
  const int cs = CIN / 8;
  int* const goff = reinterpret_cast<int*>(lds + 8 * PLANE) + tid;  // goff[it * 256]: this thread's input offsets of the tile

  const TileWalk walk = tile_walk(a.ntiles, a.order);
  if ((blockIdx.x >> 3) >= (gridDim.x >> 4))  // the upper half of every XCD's slots
    for (int i = 0; i < a.stagger; ++i) __builtin_amdgcn_s_sleep(64);

  for (int stamp_tile = 0; stamp_tile < walk.count; ++stamp_tile) {
    const int tile = walk.first + stamp_tile * walk.step;
    DC_STAMP(0);
    const int half = tile % a.nhalf, run = tile / a.nhalf;
    const int q0 = a.q_begin + run * DC_RUN;
    int p_first = q0 - LW - 1;  // flat index of window position 0 (UP: in the low tall image)
    // ---- this thread's window positions -> input pixel offsets, once per tile (they do not depend on the K slice):
    // (r, c) of the first position by division, the following ones by stepping 32 positions at a time
    unsigned inside = 0, later = 0;
    const int n0 = max(0, ((p_first / LW) - 1) / HP);  // image of the window's first row (clamped)
    int c, y, n;
    if constexpr (UP) {  // (the first low position as column, row, image, and this thread's by stepping: no division by LWI, HPI)
      up_win_span(q0, DC_RUN, LW, HP, p_first, WIN, n, y, c);
      WIN = min(WIN, DCU_WIN_MAX);  // (the launch has checked that no tile needs more)
      if (--y < 0 && n > 0) { y = HPI - 1; --n; }
      dc_step(c, y, n, LWI, HPI, pos0);
    } else {
      dc_win_pos(p_first + pos0, LWI, HPI, c, y, n);
    }
    {
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        if constexpr (UP) goff[it * 256] = dc_low_off(a, c, y, n, n0, cs, pl, pos0 + 32 * it < WIN, it, inside, later);
        else goff[it * 256] = dc_win_off<UP>(a, c, y, n, n0, cs, pl, true, it, inside, later);
        dc_step32(c, y, n, LWI, HPI);
      }
    }
    const int n1 = min(n0 + 1, a.N - 1);
    // The raw window of a slice travels global -> registers while the matrix cores still work on the previous slice (the
    // loads are issued before the last k-step's 63 MFMAs): a slice's staging phase is then prologue + LDS writes only.
    uint4 v[ITERS];
    auto request = [&](int s) {
      const uint4* inS = a.in + s * 8;
#pragma unroll
      for (int it = 0; it < ITERS; ++it) v[it] = inS[(unsigned)goff[it * 256]];
    };
    request(0);

    const int c0 = half * 128 + cb * 32 + hh * 16;
    const int ocs = a.COUT / 8;
    f32x16_t acc[DC_NB];
    dc_seed32(a, q0, px, c0, ocs, LW, HP, acc);
    int lb[DC_NB];  // UP: this lane's window slots and row parities (dc_low_bases)
    unsigned rbits;
    if constexpr (UP) dc_low_bases(q0, px, LW, HP, p_first, PLANE, lb, rbits);
    const bf16x8_t* wbase = reinterpret_cast<const bf16x8_t*>(a.wpk) + (size_t)(half * 4 + cb) * 9 * KCT * 64 + lane;
    DC_STAMP(1);

    for (int s = 0; s < S; ++s) {
      // the slice's first weight fragments are requested before the staging phase: they do not depend on it, and their
      // L2 latency would otherwise sit between the second barrier and the first MFMA of every slice
      const bf16x8_t* wp = wbase + (size_t)(4 * s) * 64;  // fragment (tap, kc) of this slice at wp[(tap * KCT + kc) * 64]
      constexpr int NW = 36;  // weight fragments per slice, in (kc, tap) order
      bf16x8_t wring[DC_WDEPTH];
      auto wfrag = [&](int i) { return wp[((i % 9) * KCT + (i / 9)) * 64]; };
#pragma unroll
      for (int i = 0; i < DC_WDEPTH - 1; ++i) wring[i] = wfrag(i);
      f32x2_t sc[4], sh[4], sh1[4];  // the slice's prologue constants for this thread's octet
      dc_prologue_consts(a, s, pl, n0, n1, sc, sh, sh1);
      __syncthreads();  // every wave is done reading the previous slice's planes
      DC_STAMP(2 + 4 * s);
      // ---- stage: prologue (BatchNorm affine + style shift + ReLU, zero outside the image) into the octet planes
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        f32x2_t shs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) shs[k] = ((later >> it) & 1u) ? sh1[k] : sh[k];
        const uint4 o = conv_act8(v[it], sc, shs, 0u - ((inside >> it) & 1u));
        const int wp_ = pos0 + 32 * it;
        if (wp_ < WIN) lds[pl * PLANE + wp_] = o;
      }
      DC_STAMP(3 + 4 * s);
      __syncthreads();
      DC_STAMP(4 + 4 * s);

      // ---- 4 k-steps x 9 taps x 7 blocks; weight fragment (tap, k-step) comes from global through the ring
      const bf16x8_t* L = reinterpret_cast<const bf16x8_t*>(lds) + hh * PLANE + (UP ? 0 : px);
      const int row_off[3] = {0, LW, 2 * LW};
      const int cbit = up_col_bit(px);  // (LW and the tile's first position are even: the column's parity is the lane's)
      constexpr int NF = NW * DC_NB;  // pixel fragments (= MFMAs) per slice
      bf16x8_t pring[DC_PDEPTH];
      auto pfrag = [&](int f) {
        const int i = f / DC_NB, b = f % DC_NB, kc = i / 9, tap = i % 9;
        if constexpr (UP) return L[2 * kc * PLANE + up_tap(lb[b], (rbits >> b) & 1u, cbit, LWI, tap / 3, tap % 3)];
        else return L[2 * kc * PLANE + b * 32 + row_off[tap / 3] + tap % 3];
      };
#pragma unroll
      for (int f = 0; f < DC_PDEPTH - 1; ++f) pring[f] = pfrag(f);
      static_for<NW>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (UP && i % 9 == 0) dc_fresh(lb);
        if constexpr (i == DC_REQ_AT) {  // request the next slice's window (see DC_REQ_AT)
          if (s + 1 < S) request(s + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (i + DC_WDEPTH - 1 < NW) wring[(i + DC_WDEPTH - 1) % DC_WDEPTH] = wfrag(i + DC_WDEPTH - 1);
        static_for<DC_NB>([&](auto bc) {
          constexpr int b = decltype(bc)::value, f = i * DC_NB + b;
          if constexpr (f + DC_PDEPTH - 1 < NF) pring[(f + DC_PDEPTH - 1) % DC_PDEPTH] = pfrag(f + DC_PDEPTH - 1);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wring[i % DC_WDEPTH], pring[f % DC_PDEPTH], acc[b], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
      });
      DC_STAMP(5 + 4 * s);
    }

    // ---- epilogue: fp32 -> bf16, 32 contiguous bytes per lane and position.  Positions by stepping (no divisions)
    __builtin_amdgcn_sched_barrier(0);  // nothing of the epilogue is hoisted into the MFMA loop (it would spill there)
    dc_store32(a, q0, px, c0, ocs, LW, HP, acc);
    DC_STAMP(2 + 4 * S);
  }
}

// ------------------------------------------------------------------------------------------------
// The same unit for 64 output channels: the up path's 128 -> 64 convolution at the 112 x 112 level (input read through the 2x
// upsample, skip tensor as the residual), which the two K-slice launches of k_conv3x3 ran through a bf16 partial sum in HBM.
// With 64 output channels a wave still owns 32 channels x 7 position blocks, and the four waves of a workgroup are
// 2 channel groups x 2 POSITION groups: a tile is U_RUN = 448 consecutive positions, so that the window a workgroup stages
// (run + 2 LW + 2) is 1.5 runs at LW = 114 where one position group would stage 2.0.  What changes against k_conv3x3_deep:
//   * K slices of 32 channels (4 octet planes, two k-steps): the window of 448 + 2 LW + 2 positions x 64 channels is 85 KiB and
//     would leave one workgroup per CU (3.2: 691 against 888 TFLOP/s), and its raw copy 88 registers per thread; with 32
//     channels the planes were 44 KiB and the raw window 48 registers, as in k_conv3x3_deep (before the window moved to input
//     resolution: now 20 KiB and 20 registers, the slice width stays);
//   * the slice's weight ring is 6 fragments deep and the next slice's window is requested right after the slice's LAST
//     fragment load has been issued: the vmcnt counter retires in order, so a fragment requested behind the window loads would
//     make its MFMAs wait for HBM (the k_conv3x3_deep_ls note below); here nothing that the running slice needs is behind them;
//   * the window image is kept at INPUT resolution, as in the UP forms of k_conv3x3_deep (DCU_*, conv_upmap.h): every raw pixel
//     of the window is fetched, activated and written to LDS once per slice (5 staging rounds per thread, 11 at output
//     resolution), and the fragment reads go through the upsample.  This kernel has no other form: its one user reads through
//     the upsample.
// Any H, W with W <= U_WMAX; summation order: channels 0-15, 16-31, ... of every tap in turn, fp32 throughout.
constexpr int U_RUN = 2 * DC_RUN;     // output positions per tile: two position groups of DC_NB blocks
constexpr int U_WMAX = 128;           // widest image the LDS window is sized for
constexpr int U_NW = 18;              // weight fragments per slice, in (k-step, tap) order
constexpr int U_WDEPTH = 6;           // weight fragments in flight
constexpr int U_REQ_AT = U_NW - U_WDEPTH;  // the step that issues the slice's last fragment load, then the next window's request
// the window image: 294 low positions is the most any even H, W <= U_WMAX needs (up_win_fits checks the launch's own tiles)
constexpr int UU_WIN_MAX = 320;
constexpr int UU_PLANE = UU_WIN_MAX + 2;  // pitch = 2 mod 4: a ds_write_b128 lane group is 4 octets x 2 positions, 8 distinct slots of 8
constexpr int UU_ITERS = UU_WIN_MAX / 64;  // staging rounds: 64 positions x 4 octets per round of 256 threads
constexpr int UU_LDS_BYTES = 4 * UU_PLANE * 16 + UU_ITERS * 256 * 4;  // planes + per-thread input offsets
static_assert(UU_WIN_MAX % 64 == 0 && UU_PLANE % 4 == 2 && UU_WIN_MAX >= 2 * (U_WMAX / 2 + 2) + 2, "window image of the UP form");

template <int CIN, bool UP>
__global__ __launch_bounds__(256, 2) void k_conv3x3_kloop64(DeepArgs a) {
  static_assert(UP, "k_conv3x3_kloop64 reads its input through the 2x upsample");
  constexpr int S = CIN / 32, KCT = CIN / 16;  // K slices, k-steps in the packed array
  extern __shared__ uint4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cb = wave & 1, pg = wave >> 1;  // channel group, position group
  const int px = lane & 31, hh = lane >> 5;
  const int pl = tid & 3, pos0 = tid >> 2;  // staging role: a fixed channel octet of position pos0 + 64 * round
  const int LW = a.LW, HP = a.HP;
  // the window image in LDS, at input resolution (UU_*, conv_upmap.h)
  constexpr int PLANE = UU_PLANE, ITERS = UU_ITERS;
  const int LWI = up_low_width(LW), HPI = up_low_period(HP);  // its row width and period
  const int cs = CIN / 8;
  int* const goff = reinterpret_cast<int*>(lds + 4 * PLANE) + tid;  // goff[it * 256]: this thread's input offsets of the tile

  const TileWalk walk = tile_walk(a.ntiles, a.order);

  for (int ti = 0; ti < walk.count; ++ti) {
    const int tile = walk.first + ti * walk.step;
    const int q0 = a.q_begin + tile * U_RUN;
    unsigned inside = 0, later = 0;
    const int n0 = max(0, (((q0 - LW - 1) / LW) - 1) / HP);  // image of the window's first row (clamped)
    // the window in the low tall image: WIN positions from p_first on.  The first one as column, row, image, and this thread's by
    // stepping: no division by LWI, HPI
    int p_first, WIN, c, y, n;
    up_win_span(q0, U_RUN, LW, HP, p_first, WIN, n, y, c);
    WIN = min(WIN, UU_WIN_MAX);  // (the launch has checked that no tile needs more)
    if (--y < 0 && n > 0) { y = HPI - 1; --n; }
    dc_step(c, y, n, LWI, HPI, pos0);
    {
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        goff[it * 256] = dc_low_off(a, c, y, n, n0, cs, pl, pos0 + 64 * it < WIN, it, inside, later);
        dc_step32(c, y, n, LWI, HPI);
        dc_step32(c, y, n, LWI, HPI);
      }
    }
    const int n1 = min(n0 + 1, a.N - 1);
    uint4 v[ITERS];
    auto request = [&](int s) {
      const uint4* inS = a.in + s * 4;
#pragma unroll
      for (int it = 0; it < ITERS; ++it) v[it] = inS[(unsigned)goff[it * 256]];
    };
    request(0);

    const int qw = q0 + pg * DC_RUN;  // this wave's first output position
    const int c0 = cb * 32 + hh * 16;
    const int ocs = a.COUT / 8;
    f32x16_t acc[DC_NB];
    dc_seed32(a, qw, px, c0, ocs, LW, HP, acc);
    int lb[DC_NB];  // this lane's window slots and row parities
    unsigned rbits;
    dc_low_bases(qw, px, LW, HP, p_first, PLANE, lb, rbits);
    const bf16x8_t* wbase = reinterpret_cast<const bf16x8_t*>(a.wpk) + (size_t)cb * 9 * KCT * 64 + lane;

#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      const bf16x8_t* wp = wbase + (size_t)(2 * s) * 64;  // fragment (tap, kc) of this slice at wp[(tap * KCT + kc) * 64]
      bf16x8_t wring[U_WDEPTH];
      auto wfrag = [&](int i) { return wp[((i % 9) * KCT + (i / 9)) * 64]; };
#pragma unroll
      for (int i = 0; i < U_WDEPTH - 1; ++i) wring[i] = wfrag(i);
      f32x2_t sc[4], sh[4], sh1[4];  // the slice's prologue constants for this thread's octet (octet 4 (s & 1) + pl of 64 channels)
      dc_prologue_consts(a, s >> 1, (s & 1) * 4 + pl, n0, n1, sc, sh, sh1);
      // (re-read through an empty asm: the per-round masks and selects derived from them are then computed in the staging phase
      // instead of being kept in ~30 registers across the slices, which spills once the weight ring is 6 deep)
      asm volatile("" : "+v"(inside), "+v"(later));
      __syncthreads();  // every wave is done reading the previous slice's planes
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        f32x2_t shs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) shs[k] = ((later >> it) & 1u) ? sh1[k] : sh[k];
        const uint4 o = conv_act8(v[it], sc, shs, 0u - ((inside >> it) & 1u));
        const int wp_ = pos0 + 64 * it;
        if (wp_ < WIN) lds[pl * PLANE + wp_] = o;
      }
      __syncthreads();

      // ---- 2 k-steps x 9 taps x 7 blocks
      const bf16x8_t* L = reinterpret_cast<const bf16x8_t*>(lds) + hh * PLANE;
      const int cbit = up_col_bit(px);  // (LW and the wave's first position are even: the column's parity is the lane's)
      constexpr int NF = U_NW * DC_NB;  // pixel fragments (= MFMAs) per slice
      bf16x8_t pring[DC_PDEPTH];
      auto pfrag = [&](int f) {
        const int i = f / DC_NB, b = f % DC_NB, kc = i / 9, tap = i % 9;
        return L[2 * kc * PLANE + up_tap(lb[b], (rbits >> b) & 1u, cbit, LWI, tap / 3, tap % 3)];
      };
#pragma unroll
      for (int f = 0; f < DC_PDEPTH - 1; ++f) pring[f] = pfrag(f);
      static_for<U_NW>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (i % 9 == 0) dc_fresh(lb);
        if constexpr (i + U_WDEPTH - 1 < U_NW) wring[(i + U_WDEPTH - 1) % U_WDEPTH] = wfrag(i + U_WDEPTH - 1);
        if constexpr (i == U_REQ_AT) {
          __builtin_amdgcn_sched_barrier(0);
          if (s + 1 < S) request(s + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        static_for<DC_NB>([&](auto bc) {
          constexpr int b = decltype(bc)::value, f = i * DC_NB + b;
          if constexpr (f + DC_PDEPTH - 1 < NF) pring[(f + DC_PDEPTH - 1) % DC_PDEPTH] = pfrag(f + DC_PDEPTH - 1);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wring[i % U_WDEPTH], pring[f % DC_PDEPTH], acc[b], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
      });
    }

    __builtin_amdgcn_sched_barrier(0);  // nothing of the epilogue is hoisted into the MFMA loop
    dc_store32(a, qw, px, c0, ocs, LW, HP, acc);
  }
}

// ------------------------------------------------------------------------------------------------
// The same unit on v_mfma_f32_16x16x32_bf16 (round 3).  Under a dense MFMA stream the chip holds a higher clock on this shape
// than on 32x32x16 (MI355X_MICROARCH.md "Clocks under load" item 7; timing-only check in this kernel: +4.5 %), at the same
// cycles per FLOP and the same operand traffic.  What changes against k_conv3x3_deep:
//   * a wave's 32 output channels x 224 positions are 2 x 14 tiles of 16 x 16; a k-step is 32 channels: per (tap, k-step) two
//     weight fragments (channel halves a = 0, 1) and, per block of 32 positions, two pixel fragments (position halves h): each
//     pixel fragment feeds two MFMAs, each weight fragment fourteen;
//   * fragment layout (A[row l & 15][k = 8 (l >> 4) + j], B[k][col l & 15]): lane l reads the octet plane of ITS k-group, so a
//     ds_read_b128 touches four planes.  Its four 16-lane service groups pair k-groups (0, 1) and (2, 3): the two planes of a
//     pair must sit a multiple of 16 slots apart for the group to cover all 64 banks once.  With a plane pitch = 4 mod 16 that
//     holds for planes p and p + 4, so k-step jj of a 64-channel slice takes the octets (jj*2, jj*2 + 4, jj*2 + 1, jj*2 + 5) as
//     its k-groups 0..3 — the packed weights follow (k_pack_deep16).  The staging writes (8 octets of one position per 8 lanes)
//     are 2-way conflicted with this pitch instead of conflict-free: 11 writes per thread and slice against 252 reads;
//   * output rows: row 4 g + i of channel half a is output channel 8 g + 4 a + i of the wave's 32, so a lane (position c, row
//     group g) holds 8 CONTIGUOUS channels of each of its positions: one 16-byte store / residual load per position.
// Another summation order than the 32x32x16 kernel (32 channels per instruction): the two kernels agree to fp32 rounding, not
// bit for bit; exact on integer data (tests/test_gpu_conv.py).
// MEASURED SLOWER than k_conv3x3_deep (5.71 against 4.75 ms per forward; DESIGN.md 3.2: the 2-way write conflicts this pitch
// costs the staging phase, and 124-156 bytes of scratch per lane at 128 / 256 input channels): kept behind the C ABI
// (aliby_nn_conv3x3_deep16_bf16) with its tests, not used by the network.
constexpr int DC_PLANE16 = ((DC_WIN_MAX + 15 - 4) / 16) * 16 + 4 >= DC_WIN_MAX ? ((DC_WIN_MAX + 15 - 4) / 16) * 16 + 4 : ((DC_WIN_MAX + 15 - 4) / 16) * 16 + 20;
static_assert(DC_PLANE16 % 16 == 4 && DC_PLANE16 >= DC_WIN_MAX, "plane pitch of the 16x16x32 kernel");
constexpr int DC16_LDS_BYTES = 8 * DC_PLANE16 * 16 + DC_ITERS * 256 * 4;
typedef float f32x4_t __attribute__((ext_vector_type(4)));

template <int CIN, bool UP>
__global__ __launch_bounds__(256, 2) void k_conv3x3_deep16(DeepArgs a) {
  constexpr int S = CIN / 64, K32T = CIN / 32;  // K slices, 32-channel k-steps in the packed array
  extern __shared__ uint4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, cb = tid >> 6;
  const int c16 = lane & 15, kg = lane >> 4;  // MFMA role: column (position) / k-group = output row group
  const int pl = tid & 7, pos0 = tid >> 3;    // staging role: a fixed channel octet of position pos0 + 32 * round
  const int LW = a.LW, HP = a.HP;
  const int WIN = DC_RUN + 2 * LW + 2;
  const int cs = CIN / 8;
  int* const goff = reinterpret_cast<int*>(lds + 8 * DC_PLANE16) + tid;

  const TileWalk walk = tile_walk(a.ntiles, a.order);

  for (int ti = 0; ti < walk.count; ++ti) {
    const int tile = walk.first + ti * walk.step;
    const int half = tile % a.nhalf, run = tile / a.nhalf;
    const int q0 = a.q_begin + run * DC_RUN;
    const int p_first = q0 - LW - 1;
    unsigned inside = 0, later = 0;
    const int n0 = max(0, ((p_first / LW) - 1) / HP);
    {
      int c, y, n;
      dc_win_pos(p_first + pos0, LW, HP, c, y, n);
#pragma unroll
      for (int it = 0; it < DC_ITERS; ++it) {
        goff[it * 256] = dc_win_off<UP>(a, c, y, n, n0, cs, pl, true, it, inside, later);
        dc_step32(c, y, n, LW, HP);
      }
    }
    const int n1 = min(n0 + 1, a.N - 1);
    uint4 v[DC_ITERS];
    auto request = [&](int s) {
      const uint4* inS = a.in + s * 8;
#pragma unroll
      for (int it = 0; it < DC_ITERS; ++it) v[it] = inS[(unsigned)goff[it * 256]];
    };
    request(0);

    // ---- accumulators start at bias + residual; lane (c16, kg) holds channels c0 .. c0 + 7 of positions q0 + 32 b + 16 h + c16
    const int c0 = half * 128 + cb * 32 + kg * 8;
    const int ocs = a.COUT / 8;
    f32x4_t acc[DC_NB][2][2];  // [block][channel half a][position half h]
    int qbase = q0 + c16;  // (re-read through an empty asm before the epilogue: its 14 positions are then computed again there
    // instead of being kept in 40 registers across the MFMA loops, which is what common-subexpression elimination does otherwise)
    auto where = [&](int b, int h, int& n, int& y, int& x) {  // image, row, column of this lane's position (b, h)
      int c;
      dc_out_pos(qbase + b * 32 + h * 16, LW, HP, c, y, n);
      x = c - 1;
    };
    {
      float b8[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) b8[k] = a.bias ? a.bias[c0 + k] : 0.f;
      if (a.res) {
        uint4 rr[DC_NB][2];
#pragma unroll
        for (int b = 0; b < DC_NB; ++b)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            int n, y, x;
            where(b, h, n, y, x);
            rr[b][h] = a.res[dc_res_off(a, n, y, x, ocs, c0)];
          }
#pragma unroll
        for (int b = 0; b < DC_NB; ++b)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const unsigned rw[4] = {rr[b][h].x, rr[b][h].y, rr[b][h].z, rr[b][h].w};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              acc[b][0][h][2 * j] = b8[2 * j] + cv_bf2f(rw[j] & 0xffffu);
              acc[b][0][h][2 * j + 1] = b8[2 * j + 1] + cv_bf2f(rw[j] >> 16);
              acc[b][1][h][2 * j] = b8[4 + 2 * j] + cv_bf2f(rw[2 + j] & 0xffffu);
              acc[b][1][h][2 * j + 1] = b8[4 + 2 * j + 1] + cv_bf2f(rw[2 + j] >> 16);
            }
          }
      } else {
#pragma unroll
        for (int b = 0; b < DC_NB; ++b)
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc[b][0][h][k] = b8[k]; acc[b][1][h][k] = b8[4 + k]; }
      }
    }
    // packed weights: [cout block][tap][32-channel k-step][a][lane][8]
    const bf16x8_t* wbase = reinterpret_cast<const bf16x8_t*>(a.wpk) + (size_t)(half * 4 + cb) * 9 * K32T * 2 * 64 + lane;

    for (int s = 0; s < S; ++s) {
      const bf16x8_t* wp = wbase + (size_t)(2 * s) * 2 * 64;  // fragment (tap, jj, a) of this slice at wp[((tap * K32T + jj) * 2 + a) * 64]
      constexpr int NW = 18;  // weight steps per slice, in (jj, tap) order; two fragments each
      constexpr int WD = 2;  // weight steps in flight: a step is 28 MFMAs = 448 cycles, the cover two 7-MFMA steps give the 32x32x16 kernel
      bf16x8_t wring[WD][2];
      auto wfrag = [&](int i, int aa) { return wp[(((i % 9) * K32T + (i / 9)) * 2 + aa) * 64]; };
#pragma unroll
      for (int i = 0; i < WD - 1; ++i) { wring[i][0] = wfrag(i, 0); wring[i][1] = wfrag(i, 1); }
      f32x2_t sc[4], sh[4], sh1[4];  // the slice's prologue constants for this thread's octet
      dc_prologue_consts(a, s, pl, n0, n1, sc, sh, sh1);
      __syncthreads();  // every wave is done reading the previous slice's planes
#pragma unroll
      for (int it = 0; it < DC_ITERS; ++it) {
        f32x2_t shs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) shs[k] = ((later >> it) & 1u) ? sh1[k] : sh[k];
        const uint4 o = conv_act8(v[it], sc, shs, 0u - ((inside >> it) & 1u));
        const int wp_ = pos0 + 32 * it;
        if (wp_ < WIN) lds[pl * DC_PLANE16 + wp_] = o;
      }
      __syncthreads();

      // k-group kg of k-step jj reads octet plane 2 jj + (kg >> 1) + 4 (kg & 1) (see the header comment)
      const bf16x8_t* L = reinterpret_cast<const bf16x8_t*>(lds) + ((kg >> 1) + 4 * (kg & 1)) * DC_PLANE16 + c16;
      const int row_off[3] = {0, LW, 2 * LW};
      constexpr int NPF = 2 * DC_NB;     // pixel fragments per weight step
      constexpr int NF = NW * NPF;       // pixel fragments per slice (two MFMAs each)
      constexpr int PD = 3;  // pixel fragments in flight (two MFMAs each)
      bf16x8_t pring[PD];
      auto pfrag = [&](int f) {
        const int i = f / NPF, bh = f % NPF, jj = i / 9, tap = i % 9;
        return L[2 * jj * DC_PLANE16 + (bh >> 1) * 32 + (bh & 1) * 16 + row_off[tap / 3] + tap % 3];
      };
#pragma unroll
      for (int f = 0; f < PD - 1; ++f) pring[f] = pfrag(f);
      static_for<NW>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (i == NW - 5) {  // request the next slice's window (as DC_REQ_AT = 27 of 36 in the 32x32x16 kernel)
          if (s + 1 < S) request(s + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (i + WD - 1 < NW) {
          wring[(i + WD - 1) % WD][0] = wfrag(i + WD - 1, 0);
          wring[(i + WD - 1) % WD][1] = wfrag(i + WD - 1, 1);
        }
        static_for<NPF>([&](auto bc) {
          constexpr int bh = decltype(bc)::value, f = i * NPF + bh, b = bh >> 1, h = bh & 1;
          if constexpr (f + PD - 1 < NF) pring[(f + PD - 1) % PD] = pfrag(f + PD - 1);
          acc[b][0][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wring[i % WD][0], pring[f % PD], acc[b][0][h], 0, 0, 0);
          acc[b][1][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wring[i % WD][1], pring[f % PD], acc[b][1][h], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
      });
    }

    // ---- epilogue: fp32 -> bf16, 16 contiguous bytes (8 channels) per lane and position
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(qbase));
#pragma unroll
    for (int b = 0; b < DC_NB; ++b)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int n, y, x;
        where(b, h, n, y, x);
        const bool ok = q0 + b * 32 + h * 16 + c16 < a.q_end && y < a.H && x >= 0 && x < a.W && n < a.N;
        if (ok)
          a.out[(unsigned)(((n * a.H + y) * a.W + x) * ocs + (c0 >> 3))] =
              make_uint4(cv_pack2(acc[b][0][h][0], acc[b][0][h][1]), cv_pack2(acc[b][0][h][2], acc[b][0][h][3]),
                         cv_pack2(acc[b][1][h][0], acc[b][1][h][1]), cv_pack2(acc[b][1][h][2], acc[b][1][h][3]));
      }
  }
}

// weights for k_conv3x3_deep16: out[(((cb * 9 + tap) * (CIN / 32) + k32) * 2 + a) * 64 + lane][j] =
// W[32 cb + 8 (r >> 2) + 4 a + (r & 3)][64 (k32 >> 1) + 8 oct + j][tap], r = lane & 15, kg = lane >> 4,
// oct = 2 (k32 & 1) + (kg >> 1) + 4 (kg & 1)
__global__ void k_pack_deep16(const float* __restrict__ w, int cout, int cin, unsigned short* __restrict__ out, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
  size_t rest = i >> 9;
  const int aa = (int)(rest & 1);
  rest >>= 1;
  const int k32n = cin / 32;
  const int k32 = (int)(rest % k32n);
  rest /= k32n;
  const int tap = (int)(rest % 9), cb = (int)(rest / 9);
  const int r = lane & 15, kg = lane >> 4;
  const int co = cb * 32 + 8 * (r >> 2) + 4 * aa + (r & 3);
  const int ci = 64 * (k32 >> 1) + 8 * (2 * (k32 & 1) + (kg >> 1) + 4 * (kg & 1)) + j;
  const float v = w[((size_t)co * cin + ci) * 9 + tap];
  out[i] = (unsigned short)cv_f2bf(v);
}

// ------------------------------------------------------------------------------------------------
// Loader-specialised form of the same unit (round 3).  Phase elimination on k_conv3x3_deep (timing-only builds):
// without the window loads 256 -> 256 runs 24 % faster, without residual loads 9 %, without stores 9 %, without all three
// 31 % (1458 TFLOP/s) — although the loads are issued a k-step ahead, and moving the request anywhere in the slice changes
// nothing.  The reason is the in-order vmcnt counter: a wave's weight-fragment waits (L2 hits, a few hundred cycles) cannot pass
// the HBM window loads the same wave issued before them, so every slice stalls for one loaded HBM latency in the middle of its
// MFMA stream.  Here the two kinds of traffic sit in different waves:
//   waves 0-3 (MFMA): stream weight fragments and issue MFMAs, nothing else inside a slice (residual loads and stores once per tile);
//   waves 4-5 (loaders): bring the next slice's window in by LDS-DMA (each wave owns its units of the raw image: no loader-to-loader
//     hand-off), run it through the prologue into the OTHER of two plane images, request the slice after that, and meet the MFMA
//     waves at ONE workgroup barrier per slice.
// One workgroup (4 MFMA + DL_NLW loader waves, ~132 KB of LDS) per CU.  Same MFMA order as k_conv3x3_deep: same bits.
constexpr int DL_NLW = 4;                                 // loader waves
constexpr int DL_LT = DL_NLW * 64;                        // loader threads
constexpr int DL_UNITS = DC_WIN_MAX * 8;                  // 16-byte units of a slice's window (position-major, 8 octets each)
constexpr int DL_ROUNDS = (DL_UNITS + DL_LT - 1) / DL_LT; // DMA instructions per loader wave and slice
constexpr int DL_LDS_BYTES = 2 * 8 * DC_PLANE * 16 + DL_ROUNDS * DL_LT * 16;

template <int CIN, bool UP>
__global__ __launch_bounds__(256 + DL_LT, 1) void k_conv3x3_deep_ls(DeepArgs a) {
  constexpr int S = CIN / 64, KCT = CIN / 16;
  extern __shared__ uint4 lds[];
  uint4* const planes0 = lds;
  uint4* const rawbuf = lds + 2 * 8 * DC_PLANE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int LW = a.LW, HP = a.HP;
  const int WIN = DC_RUN + 2 * LW + 2;
  const int cs = CIN / 8;
  const TileWalk walk = tile_walk(a.ntiles, a.order);
  const int my_tiles = walk.count;
  const int G = my_tiles * S;  // slices this workgroup goes through: one barrier each, for every wave

  if (wave >= 4) {
    // =========================================================================================== loaders
    const int lt = tid - 256;                 // 0..DL_LT-1
    const int oct = lt & 7;                   // this lane's channel octet of the slice (units lt + DL_LT k: positions (lt >> 3) + DL_LT/8 k)
    const int wave_u = __builtin_amdgcn_readfirstlane(wave - 4);
    int goff[DL_ROUNDS];                      // input offsets (16-byte units) of this lane's units, slice 0
    unsigned inside = 0, later = 0;
    int n0 = 0, n1 = 0;
    auto tile_offsets = [&](int tile) {
      const int run = tile / a.nhalf;
      const int q0 = a.q_begin + run * DC_RUN;
      const int p_first = q0 - LW - 1;
      n0 = max(0, ((p_first / LW) - 1) / HP);
      n1 = min(n0 + 1, a.N - 1);
      inside = 0;
      later = 0;
#pragma unroll
      for (int k = 0; k < DL_ROUNDS; ++k) {
        const int wp_ = (lt >> 3) + (DL_LT / 8) * k;    // window position of unit lt + DL_LT k
        int c, y, n;
        dc_win_pos(p_first + wp_, LW, HP, c, y, n);
        goff[k] = dc_win_off<UP>(a, c, y, n, n0, cs, oct, wp_ < WIN, k, inside, later);
      }
    };
    auto issue_dma = [&](int s) {  // this wave's units of slice s -> rawbuf (lane-linear: unit u lands at rawbuf[u])
      const uint4* inS = a.in + s * 8;
#pragma unroll
      for (int k = 0; k < DL_ROUNDS; ++k)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(inS + (unsigned)goff[k]),
                                         (__attribute__((address_space(3))) void*)(rawbuf + k * DL_LT + wave_u * 64), 16, 0, 0);
    };
    auto activate = [&](int s, uint4* planes) {  // rawbuf -> prologue -> channel-octet planes
      f32x2_t sc[4], sh[4], sh1[4];
      dc_prologue_consts(a, s, oct, n0, n1, sc, sh, sh1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces (and the constants above) have landed
#pragma unroll
      for (int k = 0; k < DL_ROUNDS; ++k) {
        const int wp_ = (lt >> 3) + (DL_LT / 8) * k;
        if (wp_ >= WIN) break;
        f32x2_t shs[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) shs[q] = ((later >> k) & 1u) ? sh1[q] : sh[q];
        planes[oct * DC_PLANE + wp_] = conv_act8(rawbuf[k * DL_LT + lt], sc, shs, 0u - ((inside >> k) & 1u));
      }
    };
    // slice g of the workgroup = (tile g / S, slice g % S); prepared one barrier ahead of its MFMAs
    if (G > 0) {
      tile_offsets(walk.first);
      issue_dma(0);
      activate(0, planes0);
      if (G > 1) {
        if (S == 1) tile_offsets(walk.first + walk.step);
        issue_dma(1 % S);
      }
    }
    for (int g = 0; g < G; ++g) {
      __syncthreads();  // B_g: planes[g & 1] hold slice g; the MFMA waves are done with planes[(g + 1) & 1]
      if (g + 1 < G) {
        const int s1 = (g + 1) % S;
        activate(s1, planes0 + ((g + 1) & 1) * 8 * DC_PLANE);  // (its offsets / masks are the ones its DMA was issued with)
        if (g + 2 < G) {
          const int s2 = (g + 2) % S;
          if (s2 == 0) tile_offsets(walk.first + ((g + 2) / S) * walk.step);
          issue_dma(s2);
        }
      }
    }
    return;
  }

  // ============================================================================================= MFMA waves
  const int cb = wave, px = lane & 31, hh = lane >> 5;
  const int ocs = a.COUT / 8;
  const int row_off[3] = {0, LW, 2 * LW};
  int g = 0;
  for (int ti = 0; ti < my_tiles; ++ti) {
    const int tile = walk.first + ti * walk.step;
    const int half = tile % a.nhalf, run = tile / a.nhalf;
    const int q0 = a.q_begin + run * DC_RUN;
    const int c0 = half * 128 + cb * 32 + hh * 16;
    f32x16_t acc[DC_NB];
    dc_seed32(a, q0, px, c0, ocs, LW, HP, acc);
    const bf16x8_t* wbase = reinterpret_cast<const bf16x8_t*>(a.wpk) + (size_t)(half * 4 + cb) * 9 * KCT * 64 + lane;
    for (int s = 0; s < S; ++s, ++g) {
      const bf16x8_t* wp = wbase + (size_t)(4 * s) * 64;
      constexpr int NW = 36;
      bf16x8_t wring[DC_WDEPTH];
      auto wfrag = [&](int i) { return wp[((i % 9) * KCT + (i / 9)) * 64]; };
#pragma unroll
      for (int i = 0; i < DC_WDEPTH - 1; ++i) wring[i] = wfrag(i);
      __syncthreads();  // B_g
      const bf16x8_t* L = reinterpret_cast<const bf16x8_t*>(planes0 + (g & 1) * 8 * DC_PLANE) + hh * DC_PLANE + px;
      constexpr int NF = NW * DC_NB;
      bf16x8_t pring[DC_PDEPTH];
      auto pfrag = [&](int f) {
        const int i = f / DC_NB, b = f % DC_NB, kc = i / 9, tap = i % 9;
        return L[2 * kc * DC_PLANE + b * 32 + row_off[tap / 3] + tap % 3];
      };
#pragma unroll
      for (int f = 0; f < DC_PDEPTH - 1; ++f) pring[f] = pfrag(f);
      static_for<NW>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (i + DC_WDEPTH - 1 < NW) wring[(i + DC_WDEPTH - 1) % DC_WDEPTH] = wfrag(i + DC_WDEPTH - 1);
        static_for<DC_NB>([&](auto bc) {
          constexpr int b = decltype(bc)::value, f = i * DC_NB + b;
          if constexpr (f + DC_PDEPTH - 1 < NF) pring[(f + DC_PDEPTH - 1) % DC_PDEPTH] = pfrag(f + DC_PDEPTH - 1);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wring[i % DC_WDEPTH], pring[f % DC_PDEPTH], acc[b], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    __builtin_amdgcn_sched_barrier(0);
    dc_store32(a, q0, px, c0, ocs, LW, HP, acc);
  }
}

// max_pool2d(x, 2, 2) on bf16 NHWC: one 16-byte channel octet per thread (the comparison runs on the bf16 values as
// floats; max commutes with the rounding)
__global__ void k_maxpool2(const uint4* __restrict__ in, uint4* __restrict__ out, int N, int H, int W, int cs) {
  const int PH = H >> 1, PW = W >> 1;
  const size_t total = (size_t)N * PH * PW * cs;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int o = (int)(i % cs);
    size_t p = i / cs;
    const int x = (int)(p % PW);
    p /= PW;
    const int y = (int)(p % PH), n = (int)(p / PH);
    const uint4* q = in + ((size_t)(n * H + 2 * y) * W + 2 * x) * cs + o;
    const uint4 v[4] = {q[0], q[cs], q[(size_t)W * cs], q[(size_t)W * cs + cs]};
    unsigned r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned w[4] = {k == 0 ? v[0].x : k == 1 ? v[0].y : k == 2 ? v[0].z : v[0].w, k == 0 ? v[1].x : k == 1 ? v[1].y : k == 2 ? v[1].z : v[1].w,
                             k == 0 ? v[2].x : k == 1 ? v[2].y : k == 2 ? v[2].z : v[2].w, k == 0 ? v[3].x : k == 1 ? v[3].y : k == 2 ? v[3].z : v[3].w};
      float lo = cv_bf2f(w[0] & 0xffffu), hi = cv_bf2f(w[0] >> 16);
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        lo = fmaxf(lo, cv_bf2f(w[j] & 0xffffu));
        hi = fmaxf(hi, cv_bf2f(w[j] >> 16));
      }
      r[k] = (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
    }
    out[i] = make_uint4(r[0], r[1], r[2], r[3]);
  }
}

unsigned long long* g_deep_trace = nullptr;

}  // namespace

extern "C" int aliby_debug_conv_deep_trace(aliby_ctx* ctx, void* stamps_dev) {
  (void)ctx;
  g_deep_trace = static_cast<unsigned long long*>(stamps_dev);
  return ALIBY_OK;
}

// argument checks and the tall-image geometry that the entry points of this file share; `run` = output positions per tile,
// `nhalf` = tiles per run
static int deep_args(DeepArgs& a, aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale, const float* shift,
                     int shift_per_sample, const float* bias, const void* res, int res_up, int N, int H, int W, int CIN, int COUT,
                     int run, int nhalf) {
  a.in = static_cast<const uint4*>(in);
  a.wpk = static_cast<const uint4*>(wpk);
  a.out = static_cast<uint4*>(out);
  a.scale = scale;
  a.shift = shift;
  a.bias = bias;
  a.res = static_cast<const uint4*>(res);
  a.shift_stride = shift_per_sample == 1 ? CIN : shift_per_sample;
  a.res_up = res_up ? 1 : 0;
  a.N = N; a.H = H; a.W = W; a.COUT = COUT;
  a.LW = W + 2;
  a.HP = H + 1;
  const long long rows = (long long)N * a.HP + 1;  // padded tall image: zero row, then N x (H rows + zero row)
  ARG_CHECK(rows * a.LW < (1ll << 30), "conv3x3_deep: batch too large for 32-bit flat positions");
  ARG_CHECK((long long)N * H * W * (CIN > COUT ? CIN : COUT) / 8 < (1ll << 31), "conv3x3_deep: tensor too large for 32-bit offsets");
  a.q_begin = a.LW;                         // row 1, column 0
  a.q_end = (int)((rows - 1) * a.LW);       // the last row is the closing zero row
  a.nruns = (a.q_end - a.q_begin + run - 1) / run;
  a.nhalf = nhalf;
  a.ntiles = a.nruns * a.nhalf;
  a.stagger = 0;
  a.trace = nullptr;
  return ALIBY_OK;
}

// UP forms: does the window image of `cap` low positions hold the window of every tile of this launch?  It does for every
// even H, W within the kernels' width limits that has been tried; the walk over the tiles (remembered for the last shape) is what
// makes that a checked fact for the launch at hand instead of a bound to be proven over all shapes.
static bool up_win_fits(const DeepArgs& a, int run, int cap) {
  thread_local int key[4] = {0, 0, 0, 0}, most = 0;
  if (key[0] != run || key[1] != a.H || key[2] != a.W || key[3] != a.N) {
    most = 0;
    for (int t = 0; t < a.nruns; ++t) {
      int lstart, count;
      up_win_span(a.q_begin + t * run, run, a.LW, a.HP, lstart, count);
      most = count > most ? count : most;
    }
    key[0] = run; key[1] = a.H; key[2] = a.W; key[3] = a.N;
  }
  return most <= cap;
}

static int deep_entry(aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale, const float* shift,
                      int shift_per_sample, const float* bias, const void* res, int res_up, int N, int H, int W, int CIN, int COUT,
                      int in_up, void* stream_, bool m16) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ARG_CHECK(ctx && in && wpk && out && scale && shift, "conv3x3_deep: null argument");
  ARG_CHECK(N > 0 && H > 0 && W > 0, "conv3x3_deep: empty shape");
  ARG_CHECK(!in_up || ((H & 1) == 0 && (W & 1) == 0), "conv3x3_deep: upsampled input needs even H, W");
  ARG_CHECK(!res || !res_up || ((H & 1) == 0 && (W & 1) == 0), "conv3x3_deep: upsampled residual needs even H, W");
  if (!(CIN == 64 || CIN == 128 || CIN == 256) || COUT % 128 != 0 || COUT <= 0 || W > DC_WMAX) {
    aliby_set_error("conv3x3_deep: unsupported (CIN=%d, COUT=%d, W=%d): CIN in {64,128,256}, COUT a multiple of 128, W <= %d", CIN, COUT, W,
                    DC_WMAX);
    return ALIBY_ERR_UNSUPPORTED;
  }
  if (shift_per_sample != 0 && (long long)(H + 1) * (W + 2) < DC_RUN + 2 * (W + 2) + 2) {
    aliby_set_error("conv3x3_deep: images of %dx%d are smaller than one tile window (a window may span two images at most)", H, W);
    return ALIBY_ERR_UNSUPPORTED;
  }
  DeepArgs a;
  if (const int rc = deep_args(a, ctx, in, wpk, out, scale, shift, shift_per_sample, bias, res, res_up, N, H, W, CIN, COUT, DC_RUN, COUT / 128))
    return rc;
  if (in_up && !m16 && !up_win_fits(a, DC_RUN, DCU_WIN_MAX)) {
    aliby_set_error("conv3x3_deep: a tile of the upsampled %dx%d input needs more than %d window positions", H, W, DCU_WIN_MAX);
    return ALIBY_ERR_UNSUPPORTED;
  }
  static const int stagger = env_int("ALIBY_DEEP_STAGGER", 0);
  a.stagger = stagger;
  a.trace = g_deep_trace;
  const bool ls = env_int("ALIBY_DEEP_LS", 0) != 0;  // loader-specialised form: measured slower, kept for A/B; read per call
  // caps: the kernel's workgroups per CU (2; the loader-specialised form 1) x 32 CUs per XCD; ALIBY_DEEP_SLOTS overrides the product form's
  static const int slots = env_int("ALIBY_DEEP_SLOTS", 64);
  auto go = [&](auto cin, auto up) {
    constexpr int C = decltype(cin)::value;
    constexpr bool U = decltype(up)::value;
    if (m16) return launch<k_conv3x3_deep16<C, U>, 256>(ctx, a, DC16_LDS_BYTES, 64, stream);
    if (ls) return launch<k_conv3x3_deep_ls<C, U>, 256 + DL_LT>(ctx, a, DL_LDS_BYTES, 32, stream);
    return launch<k_conv3x3_deep<C, U>, 256>(ctx, a, U ? DCU_LDS_BYTES : DC_LDS_BYTES, slots, stream);
  };
  auto by_up = [&](auto cin) { return in_up ? go(cin, std::true_type{}) : go(cin, std::false_type{}); };
  if (CIN == 64) return by_up(std::integral_constant<int, 64>{});
  if (CIN == 128) return by_up(std::integral_constant<int, 128>{});
  return by_up(std::integral_constant<int, 256>{});
}

extern "C" int aliby_nn_conv3x3_deep_bf16(aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale,
                                          const float* shift, int shift_per_sample, const float* bias, const void* res, int res_up,
                                          int N, int H, int W, int CIN, int COUT, int in_up, void* stream_) {
  return deep_entry(ctx, in, wpk, out, scale, shift, shift_per_sample, bias, res, res_up, N, H, W, CIN, COUT, in_up, stream_, false);
}

extern "C" int aliby_nn_conv3x3_deep16_bf16(aliby_ctx* ctx, const void* in, const void* wpk16, void* out, const float* scale,
                                            const float* shift, int shift_per_sample, const float* bias, const void* res, int res_up,
                                            int N, int H, int W, int CIN, int COUT, int in_up, void* stream_) {
  return deep_entry(ctx, in, wpk16, out, scale, shift, shift_per_sample, bias, res, res_up, N, H, W, CIN, COUT, in_up, stream_, true);
}

extern "C" int aliby_nn_pack_conv3x3_deep16_bf16(aliby_ctx* ctx, const float* w_oihw, int COUT, int CIN, void* wpk16, void* stream_) {
  ARG_CHECK(ctx && w_oihw && wpk16, "pack_conv_deep16: null argument");
  ARG_CHECK(COUT > 0 && COUT % 32 == 0 && CIN > 0 && CIN % 64 == 0, "pack_conv_deep16: COUT must be a multiple of 32 and CIN of 64");
  const size_t total = (size_t)COUT * CIN * 9;
  hipLaunchKernelGGL(k_pack_deep16, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), w_oihw, COUT, CIN,
                     static_cast<unsigned short*>(wpk16), total);
  KERNEL_CHECK();
  return ALIBY_OK;
}

extern "C" int aliby_nn_maxpool2_bf16(aliby_ctx* ctx, const void* in, void* out, int N, int H, int W, int C, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ARG_CHECK(ctx && in && out, "maxpool2: null argument");
  ARG_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0 && (H & 1) == 0 && (W & 1) == 0, "maxpool2: even H, W and C a multiple of 8");
  const size_t total = (size_t)N * (H / 2) * (W / 2) * (C / 8);
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(k_maxpool2, dim3(grid), dim3(256), 0, stream, static_cast<const uint4*>(in), static_cast<uint4*>(out), N, H, W, C / 8);
  KERNEL_CHECK();
  return ALIBY_OK;
}

extern "C" int aliby_nn_conv3x3_kloop64_bf16(aliby_ctx* ctx, const void* in, const void* wpk, void* out, const float* scale,
                                             const float* shift, int shift_per_sample, const float* bias, const void* res, int res_up,
                                             int N, int H, int W, int CIN, int COUT, int in_up, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  ARG_CHECK(ctx && in && wpk && out && scale && shift, "conv3x3_kloop64: null argument");
  ARG_CHECK(N > 0 && H > 0 && W > 0, "conv3x3_kloop64: empty shape");
  if (CIN != 128 || COUT != 64 || !in_up || W > U_WMAX) {
    aliby_set_error("conv3x3_kloop64: unsupported (CIN=%d, COUT=%d, in_up=%d, W=%d): 128 -> 64 through the upsample, W <= %d", CIN, COUT,
                    in_up, W, U_WMAX);
    return ALIBY_ERR_UNSUPPORTED;
  }
  ARG_CHECK((H & 1) == 0 && (W & 1) == 0, "conv3x3_kloop64: upsampled input needs even H, W");
  if (shift_per_sample != 0 && (long long)(H + 1) * (W + 2) < U_RUN + 2 * (W + 2) + 2) {
    aliby_set_error("conv3x3_kloop64: unsupported with a per-sample shift: images of %dx%d are smaller than one tile window (a window may span two images at most)", H, W);
    return ALIBY_ERR_UNSUPPORTED;
  }
  DeepArgs a;
  if (const int rc = deep_args(a, ctx, in, wpk, out, scale, shift, shift_per_sample, bias, res, res_up, N, H, W, CIN, COUT, U_RUN, 1))
    return rc;
  if (!up_win_fits(a, U_RUN, UU_WIN_MAX)) {
    aliby_set_error("conv3x3_kloop64: a tile of the upsampled %dx%d input needs more than %d window positions", H, W, UU_WIN_MAX);
    return ALIBY_ERR_UNSUPPORTED;
  }
  return launch<k_conv3x3_kloop64<128, true>, 256>(ctx, a, UU_LDS_BYTES, 64, stream);  // 2 workgroups per CU, 32 CUs per XCD
}

extern "C" int aliby_nn_conv3x3_kloop_limits(int limits[4]) {
  ARG_CHECK(limits != nullptr, "kloop_limits: null argument");
  limits[0] = DC_RUN; limits[1] = DC_WMAX; limits[2] = U_RUN; limits[3] = U_WMAX;
  return ALIBY_OK;
}
