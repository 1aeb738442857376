// Device code shared by the MXFP4 GEMM kernels (gfx950): mxfp4_gemm.hip and
// moe_mxfp4_gemm.hip (W4A16: e2m1 expanded to bf16 in registers), and
// mxfp8_gemm.hip and moe_mxfp8_gemm.hip (MXFP4 x MXFP8 scaled MFMA, and the
// MXFP8 row quantiser). Everything here is force-inlined or constexpr; the
// bit-exact contracts between those kernels (a block_m 32 row equals a
// block_m 128 row, a down row equals mxfp4_mxfp8_linear, the fused gate_up
// epilogue equals quant_mxfp8_rows) hold because each rule below exists once.
//
// Fragment layout of one v_mfma_scale_f32_16x16x128_f8f6f4 step, as
// established by the one-hot tests (tests/test_mxfp4_a8_gpu.py). Lane
// l = 16 g + r holds row r of its 16-row tile, for both operands; k below is
// relative to the step's first k, 128 s:
//   * fp4 (W, srcA), 4 operand VGPRs: VGPR v, nibble q is k = 32 g + 8 v + q.
//     A lane holds one whole MX block, ascending: exactly the 16 B per lane
//     mxfp4_linear loads, no unpacking;
//   * fp8 (x, srcB), 8 operand VGPRs: VGPR v, byte b is
//     k = 64 (v / 4) + 16 g + 4 (v % 4) + b. A lane holds two 16 B runs, 64 k
//     apart, i.e. halves of the MX blocks g / 2 and 2 + g / 2: the fp8
//     operand is not laid out like the fp4 one;
//   * scales follow k, not the data lanes: the e8m0 byte of MX block g
//     (k = 32 g ... + 31) of row r is taken from byte 0 (opsel 0) of the
//     scale VGPR of lane 16 g + r, for srcA and srcB alike.
// W is srcA, so D row = n and D column = m: lane l holds m = l & 15 and the
// four consecutive columns n = 4 (l >> 4) ... + 3, one 8 B store.
#pragma once

#include "common.h"

namespace fi {

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float floatx4;
typedef __attribute__((ext_vector_type(4))) u32 u32x4;
typedef __attribute__((ext_vector_type(8))) int intx8;
typedef __attribute__((ext_vector_type(2))) short short2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

constexpr int kRowBytes = 144;   // LDS row: 128 B of e4m3 + 16 B pad
constexpr int kFmtFp8 = 0;       // e4m3
constexpr int kFmtFp4 = 4;       // e2m1

// nothing is scheduled across this point
#if defined(__HIP_DEVICE_COMPILE__)
#define FI_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define FI_SCHED_FENCE()
#endif

// W4A16 lane mapping (mxfp4_linear_kernel, moe_mxfp4_gemm_kernel). Lane l
// (column c = l & 15, group g = l >> 4) of k-chunk s (128 k) loads the 16 B
// that hold k = 128 s + 32 g ... + 31 of its W row: one MX block, one scale
// byte. dequant_fp4x8 of dword t of it is B fragment t of
// mfma_f32_16x16x32_bf16, k = 128 s + 32 g + 8 t + j. The A operand uses the
// same permuted k: lane (row r, group g) element j of step t is
// x[r][128 s + 32 g + 8 t + j], a contiguous 16 B.

// 2^(s - 127) for an e8m0 byte s in [1, 254]
FI_DEV float e8m0_to_f32(u32 s) { return __uint_as_float(s << 23); }

// Eight e2m1 codes of one u32 (k ascending: byte b holds k = 2b in its low
// nibble, k = 2b + 1 in its high nibble) times `scale` -> 8 bf16.
FI_DEV short8 dequant_fp4x8(u32 w, float scale) {
  union {
    bf16x2_t p[4];
    short8 v;
  } u;
#if defined(__HIP_DEVICE_COMPILE__)
  u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
#else
  u.v = short8{0, 0, 0, 0, 0, 0, 0, 0};
#endif
  return u.v;
}

// D = A(fp4, 16 x 128) * B(fp8, 128 x 16) + C with per-lane block scales
FI_DEV floatx4 mfma_w4a8(u32x4 w, u32 wscale, intx8 x, u32 xscale,
                         floatx4 acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  const intx8 a = {static_cast<int>(w[0]), static_cast<int>(w[1]),
                   static_cast<int>(w[2]), static_cast<int>(w[3]), 0, 0, 0, 0};
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      a, x, acc, kFmtFp4, kFmtFp8, 0, static_cast<int>(wscale), 0,
      static_cast<int>(xscale));
#else
  return acc;
#endif
}

// same expression as moe_gemm_kernel's epilogue (moe_gemm.hip)
FI_DEV float swiglu(float g, float u) { return (g / (1.f + __expf(-g))) * u; }

// The MXFP8 block-scale rule: the e8m0 byte s of a block whose largest
// magnitude is `amax`, and *inv = 2^(127 - s), the exact factor that scales
// the block's values before they are converted. floor(log2(amax)) is the
// exponent field; a subnormal amax reads 0 and clamps to 8 as its true
// exponent would.
FI_DEV int mxfp8_block_scale(float amax, float* inv) {
  int s = static_cast<int>((__float_as_uint(amax) >> 23) & 0xff) - 8;
  s = min(max(s, 8), 247);
  if (amax == 0.f) s = 127;
  *inv = __uint_as_float(static_cast<u32>(254 - s) << 23);
  return s;
}

// four scaled values -> four e4m3 bytes (v[0] lowest)
FI_DEV u32 pack_fp8x4(const float* v) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the convert gives NaN past 448 instead of saturating: clamp first
  float c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) c[e] = fminf(fmaxf(v[e], -448.f), 448.f);
  union {
    u32 u;
    short2_t s;
  } p;
  p.u = 0;
  // the block scale is already applied (exactly) because the clamp needs
  // the scaled value; the convert itself runs at scale 1
  p.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(p.s, c[0], c[1], 1.0f, false);
  p.s = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(p.s, c[2], c[3], 1.0f, true);
  // -0 (a negative value that rounds to zero) is stored as +0
  u32 w = p.u;
  if ((w & 0x0000007fu) == 0) w &= 0xffffff00u;
  if ((w & 0x00007f00u) == 0) w &= 0xffff00ffu;
  if ((w & 0x007f0000u) == 0) w &= 0xff00ffffu;
  if ((w & 0x7f000000u) == 0) w &= 0x00ffffffu;
  return w;
#else
  return 0;
#endif
}

// The fp8 (srcB) operand of one step from an LDS panel row: `p` points at
// byte 16 g of the lane's row; bytes 16 g ... + 15 and 64 + 16 g ... + 15.
FI_DEV intx8 lds_read_a8_frag(const unsigned char* p) {
  const u32x4 lo = *reinterpret_cast<const u32x4*>(p);
  const u32x4 hi = *reinterpret_cast<const u32x4*>(p + 64);
  return intx8{static_cast<int>(lo[0]), static_cast<int>(lo[1]),
               static_cast<int>(lo[2]), static_cast<int>(lo[3]),
               static_cast<int>(hi[0]), static_cast<int>(hi[1]),
               static_cast<int>(hi[2]), static_cast<int>(hi[3])};
}

// W fragments and their scale bytes of a wave's four n-fragments in the
// grouped kernels: lane -> row r, MX block g of the step. `wrow0` is the first
// W row of the expert and `wn` the wave's first column. Columns past N are
// clamped in bounds; the epilogues never store them. (The dense kernel sets
// its W pointers up in one loop with its x scale pointers and has no expert
// or gate/up offset; it keeps that loop.)
template <bool GATE_UP>
FI_DEV void w_frag_ptrs(const unsigned char* (&wp)[4],
                        const unsigned char* (&wsp)[4],
                        const unsigned char* wq, const unsigned char* ws,
                        int64_t wrow0, int wn, int r, int g, int N, int K) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // gate_up: fragments 0, 1 are gate rows, 2, 3 the matching up rows
    const int col = GATE_UP ? wn + 16 * (j & 1) + r : wn + 16 * j + r;
    const int64_t n =
        wrow0 + (GATE_UP && j >= 2 ? N : 0) + min(col, N - 1);
    wp[j] = wq + n * (K / 2) + 16 * g;
    wsp[j] = ws + n * (K / 32) + g;
  }
}

// Epilogues of the grouped scaled-MFMA kernels. acc is [n fragment][m
// fragment]; lane -> slot r of each of the MF m fragments, columns 4 g ... + 3
// of each n fragment. `slot` is the wave's first slot and `wn` its first
// column. Every slot of an m-tile exists (tiles are padded), so rows are not
// guarded.

// bf16 tile: 4 n fragments, one 8 B store per fragment
template <int MF>
FI_DEV void store_bf16_tile(u16* out, const floatx4 (&acc)[4][MF], int slot,
                            int wn, int r, int g, int N) {
  // N % 16 == 0, so a fragment is stored whole or not at all
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = wn + 16 * j + 4 * g;
    if (n < N) {
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        const int64_t row = slot + 16 * i + r;
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o.h[e] = f32_to_bf16(acc[j][i][e]);
        *reinterpret_cast<bf16x4*>(out + row * N + n) = o;
      }
    }
  }
}

// SwiGLU + MXFP8 rows: n fragments 0, 1 are gate, 2, 3 the matching up
// columns, so a wave owns one whole 32-column MX block of each act row and
// needs no LDS. Per m fragment: v = bf16(swiglu(g, u)); block amax over the
// lane's 2 x 4 values and across the four lane groups; then the scale, clamp,
// convert and -0 rule of quant_mxfp8_rows. One 4 B store per lane per gate
// fragment, and lane group 0 stores the scale byte.
template <int MF>
FI_DEV void store_swiglu_mxfp8_tile(unsigned char* out,
                                    unsigned char* out_scale,
                                    const floatx4 (&acc)[4][MF], int slot,
                                    int wn, int r, int g, int N) {
  // N % 32 == 0, so a wave's MX block of act columns is whole or absent
  // (wave-uniform; every barrier is behind us)
  if (wn < N) {
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const int64_t row = slot + 16 * i + r;
      float v[2][4];
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[j][e] = bf16_to_f32(
              f32_to_bf16(swiglu(acc[j][i][e], acc[j + 2][i][e])));
          amax = fmaxf(amax, fabsf(v[j][e]));
        }
      amax = fmaxf(amax, __shfl_xor(amax, 16, 64));
      amax = fmaxf(amax, __shfl_xor(amax, 32, 64));
      float inv;
      const int s = mxfp8_block_scale(amax, &inv);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[j][e] *= inv;
        *reinterpret_cast<u32*>(out + row * N + wn + 16 * j + 4 * g) =
            pack_fp8x4(v[j]);
      }
      if (g == 0)
        out_scale[row * (N / 32) + wn / 32] = static_cast<unsigned char>(s);
    }
  }
}

}  // namespace fi
