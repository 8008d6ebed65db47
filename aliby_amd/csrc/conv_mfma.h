// conv_mfma.h — the device-side primitives of the network's MFMA convolution kernels, the counterpart of conv_launch.h (which
// holds their launch front end).  Included by nn_conv.hip, nn_conv_deep.hip and nn_conv1x1.hip; every rule on which the tests'
// "same bits as the two launches" guarantees rest is defined here once: the bf16 conversions, the prologue on a channel octet,
// the MFMA row <-> output channel map that the weight packers and the kernels must agree on, the first layer's activation, and
// the small stages around an accumulator (bias, seed, pack).
// nn_fused.hip is not a user: it rounds float -> bf16 in software with its own NaN rule (NaN stays NaN by a set quiet bit), which
// is not v_cvt_pk_bf16_f32's function, so its two converters stay with it.
#pragma once
#include "common.h"
#include <utility>

#ifdef __HIPCC__
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef short s16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

namespace {

// compile-time loop: every index is a constant expression, so register arrays are never indexed dynamically
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

__device__ __forceinline__ float cv_bf2f(unsigned h) { return __uint_as_float(h << 16); }
// two floats -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned cv_pack2(float lo, float hi) {
  const f32x2_t f = {lo, hi};
  const bf16x2_t b = __builtin_convertvector(f, bf16x2_t);
  return __builtin_bit_cast(unsigned, b);
}
__device__ __forceinline__ unsigned cv_f2bf(float f) { return cv_pack2(f, 0.f) & 0xffffu; }

// The prologue on one channel octet: bf16 -> relu(scale * x + shift) -> bf16, two channels per instruction
// (v_pk_fma_f32, v_cvt_pk_bf16_f32; ReLU as v_pk_max_i16 on the bf16 bit patterns: a set sign bit is a negative
// int16), and zeroed outside the image (`keep` = 0 there: the convolution pads the ACTIVATED tensor).
__device__ __forceinline__ uint4 conv_act8(uint4 v, const f32x2_t (&sc)[4], const f32x2_t (&sh)[4], unsigned keep) {
  const unsigned w4[4] = {v.x, v.y, v.z, v.w};
  unsigned r4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2_t x = {__uint_as_float(w4[q] << 16), __uint_as_float(w4[q] & 0xffff0000u)};
    const f32x2_t y = __builtin_elementwise_fma(sc[q], x, sh[q]);
    s16x2_t b = __builtin_bit_cast(s16x2_t, __builtin_convertvector(y, bf16x2_t));
    const s16x2_t zero = {0, 0};
    b = __builtin_elementwise_max(b, zero);
    r4[q] = __builtin_bit_cast(unsigned, b) & keep;
  }
  return make_uint4(r4[0], r4[1], r4[2], r4[3]);
}

// ---- MFMA row <-> output channel.  The weights are the A operand of v_mfma_f32_32x32x16_bf16 (row m = an output channel of the
// 32-channel block); their rows are permuted at pack time so that the 16 results of a lane are 16 CONTIGUOUS channels:
// MFMA row (reg&3) + 8*(reg>>2) + 4*(lane>>5)  <->  channel 16*(lane>>5) + reg.  conv_row_channel is that map read from the
// row's side, for the code that builds A fragments in a kernel (head_weights, the first layer's weights); k_pack_conv3x3 writes the
// same expression out (through the function its instructions come out in another order).
__host__ __device__ constexpr int conv_row_channel(int m) { return 16 * ((m >> 2) & 1) + (m & 3) + 4 * (m >> 3); }
constexpr bool conv_row_channel_is_permutation() {
  unsigned seen = 0;
  for (int m = 0; m < 32; ++m) seen |= 1u << conv_row_channel(m);
  return seen == 0xffffffffu;
}
constexpr bool conv_row_channel_inverts_lane_layout() {
  for (int hh = 0; hh < 2; ++hh)
    for (int reg = 0; reg < 16; ++reg)
      if (conv_row_channel((reg & 3) + 8 * (reg >> 2) + 4 * hh) != 16 * hh + reg) return false;
  return true;
}
static_assert(conv_row_channel_is_permutation(), "MFMA row -> channel must be a permutation of 0..31");
static_assert(conv_row_channel_inverts_lane_layout(), "MFMA row -> channel must invert the accumulator layout of a lane");

// ---- the stages around one accumulator (a lane's 16 channels c0 .. c0 + 15 of one pixel)
// the lane's 16 bias values; zeros when the unit has no bias
__device__ __forceinline__ void load_bias4(const float* bias, int c0, float4 (&b4)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) b4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) {
    const float4* bp = reinterpret_cast<const float4*>(bias + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) b4[q] = bp[q];
  }
}
// the accumulator starts at the bias
__device__ __forceinline__ void acc_seed(f32x16_t& acc, const float4 (&b4)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) { acc[4 * q] = b4[q].x; acc[4 * q + 1] = b4[q].y; acc[4 * q + 2] = b4[q].z; acc[4 * q + 3] = b4[q].w; }
}
// 16 fp32 accumulators -> two channel octets of bf16
__device__ __forceinline__ uint4 acc_pack8(const f32x16_t& acc, int half) {
  return make_uint4(cv_pack2(acc[8 * half + 0], acc[8 * half + 1]), cv_pack2(acc[8 * half + 2], acc[8 * half + 3]),
                    cv_pack2(acc[8 * half + 4], acc[8 * half + 5]), cv_pack2(acc[8 * half + 6], acc[8 * half + 7]));
}
__device__ __forceinline__ void acc_pack16(const f32x16_t& acc, uint4& lo, uint4& hi) {
  lo = acc_pack8(acc, 0);
  hi = acc_pack8(acc, 1);
}

// ---- the first layer (float32 NCHW, cin <= 2 channels; k_first_conv and the producers of k_conv_first_pair): its activation is
// cv_f2bf(first_relu(x, scale, shift)): separate multiply and add, ReLU in float, and only then the rounding.  Outside the image
// both callers round 0.f instead: the convolution pads the ACTIVATED tensor.
__device__ __forceinline__ float first_relu(float x, float scale, float shift) { return fmaxf(x * scale + shift, 0.f); }

}  // namespace
#endif  // __HIPCC__
