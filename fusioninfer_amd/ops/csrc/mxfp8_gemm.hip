// MXFP8 activation quantiser and MXFP4 x MXFP8 scaled-MFMA GEMM for gfx950:
// the large-M path of the mxfp4 mode (`--mxfp4-activations mxfp8`).
//
//   out[m, n] = bf16( sum_k dq(x_q, x_scale)[m, k] * dq(W)[n, k] (+ bias[n]) )
//
// with fp32 sums. W is the tensor pair mxfp4_linear reads (e2m1 nibbles, k
// even in the low nibble, one e8m0 byte per 32 k); x_q is e4m3 with one e8m0
// byte per 32 k of a row. Neither operand is ever expanded: both block
// scales are applied by v_mfma_scale_f32_16x16x128_f8f6f4, whose lane layout
// is documented in mx_common.h.
//
// mxfp4_mxfp8_gemm_kernel: 256 threads own a 128 x 128 macro-tile, the four
// waves 2 x 2, each with a 4 x 4 register block of 16x16 accumulators (64
// VGPRs). Per K step a wave reads 4 W fragments (straight from HBM/L2 to
// VGPRs, one step ahead) and 4 x fragments (from LDS) and issues 16 MFMAs:
// every fragment is used four times from registers. The x panel of a step
// (128 rows x 128 B) is staged through registers into LDS once per
// workgroup, double-buffered, one barrier per step; rows are padded to 144 B
// so that the 16 rows a quarter-wave reads in one ds_read_b128 fall on
// distinct 16 B groups modulo 256 B (by construction; no bank-conflict
// counter was collected). The K loop runs two steps per trip over two named
// operand sets with no branch inside the trip (an odd last step is peeled),
// and scheduling fences keep each half in the order "issue the loads (W and
// scales of step s + 1, x panel of step s + 2), MFMAs of step s, store the x
// panel of step s + 1 to LDS, barrier". In the ISA neither half loads a
// register that its own MFMAs or LDS store read: both wait only for loads
// issued in the previous half, one step earlier.
//
// Every accumulator sums the K steps in ascending order and nothing is split
// or combined across waves, so a row's bits depend on its own operands and
// K only: not on M, its position, or its neighbours. Rows past M and
// columns past N are clamped in bounds when loaded and never stored. No
// atomics, no workspace, static grid.
//
// quant_mxfp8_rows_kernel: two lanes own one MX block (16 elements each, two
// 16 B loads, one 16 B store), the block amax takes one cross-lane step, and
// the scale is read off the amax exponent (mxfp8_block_scale of mx_common.h,
// the rule the fused MoE epilogue shares). No LDS. Its clamp, convert and -0
// steps must equal pack_fp8x4 of mx_common.h; they stay written out here
// because going through pack_fp8x4 costs this kernel a VGPR (27 against 26).

#include <hip/hip_runtime.h>

#include <type_traits>

#include "mx_common.h"

namespace fi {

namespace {

constexpr int kTile = 128;       // macro-tile rows and columns

__global__ __launch_bounds__(256, 2) void mxfp4_mxfp8_gemm_kernel(
    u16* __restrict__ out,                  // [M, N] bf16
    const unsigned char* __restrict__ xq,   // [M, K] e4m3
    const unsigned char* __restrict__ xs,   // [M, K/32] e8m0
    const unsigned char* __restrict__ wq,   // [N, K/2]
    const unsigned char* __restrict__ ws,   // [N, K/32]
    const u16* __restrict__ bias,           // [N] bf16 or nullptr
    const int M, const int N, const int K) {
  const int tid = threadIdx.x;
  const int lane = tid % kWaveSize;
  const int wave = tid / kWaveSize;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int m0 = blockIdx.y * kTile;
  const int n0 = blockIdx.x * kTile;
  const int wm = m0 + 64 * (wave >> 1);  // wave's first row
  const int wn = n0 + 64 * (wave & 1);   // wave's first column
  const int nsteps = K / 128;

  __shared__ __attribute__((aligned(16))) unsigned char xl[2][kTile * kRowBytes];

  // x panel staging: thread -> rows tid / 8 + 32 i, 16 B chunk tid % 8
  const unsigned char* xg[4];
  int xo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (tid >> 3) + 32 * i;
    xg[i] = xq + static_cast<int64_t>(min(m0 + row, M - 1)) * K + 16 * (tid & 7);
    xo[i] = row * kRowBytes + 16 * (tid & 7);
  }
  // W fragments and both scale bytes: lane -> row r, MX block g of the step
  const unsigned char* wp[4];
  const unsigned char* wsp[4];
  const unsigned char* xsp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t n = min(wn + 16 * j + r, N - 1);
    wp[j] = wq + n * (K / 2) + 16 * g;
    wsp[j] = ws + n * (K / 32) + g;
    const int64_t m = min(wm + 16 * j + r, M - 1);
    xsp[j] = xs + m * (K / 32) + g;
  }
  // x fragment: bytes 16 g ... + 15 and 64 + 16 g ... + 15 of the row's step
  const int xfrag = (64 * (wave >> 1) + r) * kRowBytes + 16 * g;

  floatx4 acc[4][4];  // [n fragment][m fragment]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = floatx4{0.f, 0.f, 0.f, 0.f};

  // two named operand sets: step s computes from set s & 1 while the loads
  // of step s + 1 land in the other one, so no register is copied and no
  // MFMA waits for a load issued in its own step
  // the x panel is loaded two steps ahead (stage[s & 1] holds step s + 2)
  u32x4 stage[2][4], wv[2][4];
  u32 wsc[2][4], xsc[2][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    stage[0][i] = *reinterpret_cast<const u32x4*>(xg[i]);
    stage[1][i] = *reinterpret_cast<const u32x4*>(
        xg[i] + min(1, nsteps - 1) * 128);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wv[0][j] = *reinterpret_cast<const u32x4*>(wp[j]);
    wsc[0][j] = wsp[j][0];
    xsc[0][j] = xsp[j][0];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<u32x4*>(&xl[0][xo[i]]) = stage[0][i];
  __syncthreads();

  // the 16 MFMAs of one step: operand set and LDS buffer P
  auto mfmas = [&](auto P) {
    constexpr int p = decltype(P)::value;
    const unsigned char* buf = xl[p];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const intx8 xv = lds_read_a8_frag(buf + xfrag + 16 * i * kRowBytes);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j][i] = mfma_w4a8(wv[p][j], wsc[p][j], xv, xsc[p][i], acc[j][i]);
    }
  };
  // one full step s of parity P. Past the end the last step is loaded again
  // and stored into the idle buffer: in bounds, never read.
  auto step = [&](auto P, int s) {
    constexpr int p = decltype(P)::value;
    const int sn = min(s + 1, nsteps - 1);
    const int sx = min(s + 2, nsteps - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      stage[p][i] = *reinterpret_cast<const u32x4*>(xg[i] + sx * 128);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wv[p ^ 1][j] = *reinterpret_cast<const u32x4*>(wp[j] + sn * 64);
      wsc[p ^ 1][j] = wsp[j][sn * 4];
      xsc[p ^ 1][j] = xsp[j][sn * 4];
    }
    FI_SCHED_FENCE();  // the loads are issued before the MFMAs ...
    mfmas(P);
    FI_SCHED_FENCE();  // ... and waited for only after them
    // buffer p ^ 1 was last read in step s - 1, before its barrier
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4*>(&xl[p ^ 1][xo[i]]) = stage[p ^ 1][i];
    __syncthreads();
  };
  // Two steps per trip with no branch between them: the body is one basic
  // block, so the fences hold both halves in place (a conditional second
  // half lets the compiler sink the first half's loads into it). An odd
  // last step is peeled: its operands are already in set 0 and buffer 0.
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  for (int s = 0; s + 1 < nsteps; s += 2) {
    step(P0{}, s);
    step(P1{}, s + 1);
  }
  if (nsteps & 1) mfmas(P0{});

  // lane -> row m = r of each m fragment, columns 4 g ... + 3 of each n
  // fragment; N % 16 == 0, so a fragment is stored whole or not at all
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = wn + 16 * j + 4 * g;
    if (n < N) {
      float b[4] = {0.f, 0.f, 0.f, 0.f};
      if (bias != nullptr) {
        const bf16x4 bv = *reinterpret_cast<const bf16x4*>(bias + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = bf16_to_f32(bv.h[e]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = wm + 16 * i + r;
        if (m < M) {
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o.h[e] = f32_to_bf16(acc[j][i][e] + b[e]);
          *reinterpret_cast<bf16x4*>(out + static_cast<int64_t>(m) * N + n) = o;
        }
      }
    }
  }
}

// two e4m3 bytes into half `hi` of `old` (v[0] in the lower byte)
FI_DEV u32 pack_fp8x2(u32 old, float a, float b, bool hi) {
#if defined(__HIP_DEVICE_COMPILE__)
  union {
    u32 u;
    short2_t v;
  } c;
  c.u = old;
  // the block scale is already applied (exactly) because the clamp needs
  // the scaled value; the convert itself runs at scale 1
  c.v = hi ? __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(c.v, a, b, 1.0f, true)
           : __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(c.v, a, b, 1.0f, false);
  return c.u;
#else
  return old;
#endif
}

__global__ __launch_bounds__(256) void quant_mxfp8_rows_kernel(
    unsigned char* __restrict__ xq,   // [M, K] e4m3
    unsigned char* __restrict__ xs,   // [M, K/32] e8m0
    const u16* __restrict__ x,        // [M, K] bf16
    const int64_t nhalves) {          // M * K / 16 half blocks
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  // a wave is all in or all out (nhalves % 8 == 0 and lanes pair up), but
  // keep every lane alive for the cross-lane step anyway
  const bool ok = t < nhalves;
  const int64_t tc = ok ? t : 0;
  bf16x8 v[2];
  v[0] = *reinterpret_cast<const bf16x8*>(x + tc * 16);
  v[1] = *reinterpret_cast<const bf16x8*>(x + tc * 16 + 8);
  float f[16];
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    f[e] = bf16_to_f32(v[e >> 3].h[e & 7]);
    amax = fmaxf(amax, fabsf(f[e]));
  }
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  float inv;
  const int s = mxfp8_block_scale(amax, &inv);
  u32x4 q = {0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 16; e += 2) {
    // the convert gives NaN past 448 instead of saturating: clamp first
    const float a = fminf(fmaxf(f[e] * inv, -448.f), 448.f);
    const float b = fminf(fmaxf(f[e + 1] * inv, -448.f), 448.f);
    q[e >> 2] = pack_fp8x2(q[e >> 2], a, b, (e & 2) != 0);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    // -0 (a negative value that rounds to zero) is stored as +0
    u32 w = q[e];
    if ((w & 0x0000007fu) == 0) w &= 0xffffff00u;
    if ((w & 0x00007f00u) == 0) w &= 0xffff00ffu;
    if ((w & 0x007f0000u) == 0) w &= 0xff00ffffu;
    if ((w & 0x7f000000u) == 0) w &= 0x00ffffffu;
    q[e] = w;
  }
  if (ok) {
    *reinterpret_cast<u32x4*>(xq + t * 16) = q;
    if ((t & 1) == 0) xs[t >> 1] = static_cast<unsigned char>(s);
  }
}

}  // namespace

// M >= 1, K % 128 == 0, N % 16 == 0, M <= 65535 * 128 (checked by the
// binding)
void launch_mxfp4_mxfp8_linear(u16* out, const unsigned char* xq,
                               const unsigned char* xs,
                               const unsigned char* wq,
                               const unsigned char* ws, const u16* bias, int M,
                               int N, int K, hipStream_t stream) {
  const dim3 grid(ceil_div(N, kTile), ceil_div(M, kTile));
  mxfp4_mxfp8_gemm_kernel<<<grid, 256, 0, stream>>>(out, xq, xs, wq, ws, bias,
                                                    M, N, K);
}

void launch_quant_mxfp8_rows(unsigned char* xq, unsigned char* xs,
                             const u16* x, int64_t nhalves,
                             hipStream_t stream) {
  const int64_t grid = (nhalves + 255) / 256;
  quant_mxfp8_rows_kernel<<<static_cast<unsigned int>(grid), 256, 0, stream>>>(
      xq, xs, x, nhalves);
}

}  // namespace fi
