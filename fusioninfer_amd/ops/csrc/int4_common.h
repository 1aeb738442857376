// Device code shared by the int4 (AWQ / GPTQ) GEMM kernels (gfx950):
// int4_gemm.hip (dense W4A16 linear and dequant) and moe_int4_gemm.hip (the
// grouped expert GEMM). Everything here is force-inlined; the bit-exact
// contract between those kernels (a grouped row equals int4_linear on
// dq(W[e]), and both equal int4_dequant) holds because the expansion rule
// below exists once.
//
//   dq(W)[n, k] = bf16_rne( fp32(q - z) * fp32(s) )
//
// W4A16 lane mapping (int4_linear_kernel, moe_int4_gemm_kernel). Lane l
// (column c = l & 15, k-group g = l >> 4) of k-chunk s (128 k) loads the
// 16 B that hold k = 128 s + 32 g ... + 31 of its W row: dword t, byte b
// holds k = 128 s + 32 g + 8 t + 2 b in its low nibble and that k + 1 in its
// high nibble. 32 divides G, so the run lies in one group: one scale and one
// zero, read at index (4 s + g) >> log2(G / 32) of the row. dequant_int4x8
// of dword t is B fragment t of mfma_f32_16x16x32_bf16, and the A operand
// uses the same permuted k: lane (row r, group g) element j of step t is
// x[r][128 s + 32 g + 8 t + j], a contiguous 16 B.
#pragma once

#include "common.h"

namespace fi {

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float floatx4;
typedef __attribute__((ext_vector_type(2))) float floatx2;
typedef __attribute__((ext_vector_type(4))) u32 u32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// Per-run dequant constants from one fp16 scale and one zero byte
struct GroupScale {
  floatx2 s;    // {s, s / 16}: low-nibble and high-nibble multiplier
  floatx2 nzs;  // {-z s, -z s}
};

FI_DEV GroupScale group_scale(u16 scale_bits, u32 zero) {
  union {
    u16 u;
    _Float16 h;
  } c;
  c.u = scale_bits;
  const float s = static_cast<float>(c.h);
  const float nzs = -(static_cast<float>(zero) * s);  // exact
  return GroupScale{floatx2{s, s * 0.0625f}, floatx2{nzs, nzs}};
}

// fp32 of byte B of v: v_cvt_f32_ubyte<B>. Written as the instruction, since
// from `(float)((v >> 8 B) & 0xff)` the compiler splits the two nibble masks
// into one mask per byte and converts with ubyte0 only (about 26 VALU per
// dword instead of 18).
template <int B>
FI_DEV float cvt_f32_ubyte(u32 v) {
  float f = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(v));
  if constexpr (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(v));
  if constexpr (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(v));
  if constexpr (B == 3) asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(v));
#endif
  return f;
}

// Eight codes of one u32 (byte b: k = 2b low nibble, k = 2b + 1 high
// nibble) -> 8 bf16 of dq, k ascending.
FI_DEV short8 dequant_int4x8(u32 w, const GroupScale& gs) {
  const u32 lo = w & 0x0f0f0f0fu;
  const u32 hi = w & 0xf0f0f0f0u;
  const floatx2 qs[4] = {
      {cvt_f32_ubyte<0>(lo), cvt_f32_ubyte<0>(hi)},
      {cvt_f32_ubyte<1>(lo), cvt_f32_ubyte<1>(hi)},
      {cvt_f32_ubyte<2>(lo), cvt_f32_ubyte<2>(hi)},
      {cvt_f32_ubyte<3>(lo), cvt_f32_ubyte<3>(hi)}};
  union {
    bf16x2_t p[4];
    short8 v;
  } u;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const floatx2 q = qs[b];
    const floatx2 f = __builtin_elementwise_fma(q, gs.s, gs.nzs);
    u.p[b] = __builtin_convertvector(f, bf16x2_t);
  }
  return u.v;
}

}  // namespace fi
