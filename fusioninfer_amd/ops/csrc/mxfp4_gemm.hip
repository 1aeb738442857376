// MXFP4 weight-only (W4A16) linear and dequant kernels for gfx950.
//
//   out[m, n] = bf16( sum_k x[m, k] * dq(W)[n, k] (+ bias[n]) ),  fp32 sums
//
// W is OCP MXFP4 along K: e2m1 codes, two per byte (k even in the low
// nibble), one e8m0 scale byte per 32 consecutive k of a row. Scale bytes
// are confined to [8, 247] by the host-side validators, so every
// dequantised value is zero or a normal bf16 and dequantisation is exact:
// the kernel is a bf16 GEMM on dq(W). The kernels never scan scale bytes
// and never index from weight or scale data.
//
// mxfp4_linear_kernel<MT, NT> is the small-M, weight-streaming case: one
// workgroup owns NT 16-column tiles and MT 16-row tiles; W goes straight
// from HBM to VGPRs (16 B per lane = one MX block = one scale byte), is
// expanded to four bf16 B fragments and fed to mfma_f32_16x16x32_bf16.
// Lane l (column c = l & 15, group g = l >> 4) of k-chunk s (128 k) holds
// k = 128 s + 32 g ... + 31; fragment t of it is k = 128 s + 32 g + 8 t + j.
// The A operand uses the same permuted k: lane (row r, group g) element j of
// step t is x[r][128 s + 32 g + 8 t + j], a contiguous 16 B.
//
// The four waves split K in interleaved pairs of chunks (a pair is one
// 128 B line of every W row) and combine through LDS in fixed wave order
// ((w0 + w1) + w2) + w3. The split depends on K only, so a row's bits do
// not depend on M, on the row's position or on the <MT, NT> instance that
// served it: deterministic and batch-invariant, no atomics, no workspace.
//
// mxfp4_dequant_kernel expands W to bf16 [N, K]: one MX block per thread,
// 16 B in, 64 B out; it backs the large-M path (dequant + library GEMM).

#include <hip/hip_runtime.h>

#include "common.h"

namespace fi {

namespace {

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float floatx4;
typedef __attribute__((ext_vector_type(4))) u32 u32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

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

// U = chunk pairs a wave keeps in flight per loop trip
template <int MT, int NT, int U>
__global__ __launch_bounds__(256) void mxfp4_linear_kernel(
    u16* __restrict__ out,                  // [M, N] bf16
    const u16* __restrict__ x,              // [M, K] bf16
    const unsigned char* __restrict__ wq,   // [N, K/2]
    const unsigned char* __restrict__ ws,   // [N, K/32]
    const u16* __restrict__ bias,           // [N] bf16 or nullptr
    const int M, const int N, const int K) {
  constexpr int C = 2 * U;  // chunks in flight
  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
  const int col = lane & 15;
  const int g = lane >> 4;
  const int nt0 = blockIdx.x * NT;       // first 16-column tile
  const int ntiles = N / 16;
  const int m0 = blockIdx.y * (16 * MT);  // first row
  const int nchunks = K / 128;

  __shared__ __attribute__((aligned(16))) float red[4][MT * NT][256];

  // per-lane operand bases; rows past M and tiles past N are never read
  const u16* xp[MT];
  bool xok[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int r = m0 + 16 * i + col;
    xok[i] = r < M;
    xp[i] = x + static_cast<int64_t>(min(r, M - 1)) * K + 32 * g;
  }
  const unsigned char* wp[NT];
  const unsigned char* sp[NT];
  bool wok[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    wok[j] = nt0 + j < ntiles;  // wave-uniform
    const int64_t n = static_cast<int64_t>(min(nt0 + j, ntiles - 1)) * 16 + col;
    wp[j] = wq + n * (K / 2) + 16 * g;
    sp[j] = ws + n * (K / 32) + g;
  }

  floatx4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // wave w owns chunk pairs w, w + 4, ...; ascending K within the wave
  for (int p = wave; 2 * p < nchunks; p += 4 * U) {
    short8 xv[C][MT][4];
    u32x4 wv[C][NT];
    u32 sv[C][NT];
    // issue every load of the trip before the first use
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const int c = 2 * (p + 4 * (q >> 1)) + (q & 1);
      const bool cok = c < nchunks;  // wave-uniform
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        wv[q][j] = u32x4{0, 0, 0, 0};
        sv[q][j] = 127;
        if (cok && wok[j]) {
          wv[q][j] = *reinterpret_cast<const u32x4*>(wp[j] + c * 64);
          sv[q][j] = sp[j][c * 4];
        }
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          xv[q][i][t] = short8{0, 0, 0, 0, 0, 0, 0, 0};
          if (cok && xok[i])
            xv[q][i][t] =
                *reinterpret_cast<const short8*>(xp[i] + c * 128 + 8 * t);
        }
    }
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const int c = 2 * (p + 4 * (q >> 1)) + (q & 1);
      if (c < nchunks) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          if (wok[j]) {
            const float sc = e8m0_to_f32(sv[q][j]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const short8 b = dequant_fp4x8(wv[q][j][t], sc);
#pragma unroll
              for (int i = 0; i < MT; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    xv[q][i][t], b, acc[i][j], 0, 0, 0);
            }
          }
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
      *reinterpret_cast<floatx4*>(&red[wave][i * NT + j][lane * 4]) =
          acc[i][j];
  __syncthreads();

  // thread -> one element of each 16x16 tile (C row = 4 (l >> 4) + reg)
  const int orow = threadIdx.x >> 4;
  const int ocol = threadIdx.x & 15;
  const int src = ((orow >> 2) * 16 + ocol) * 4 + (orow & 3);
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + 16 * i + orow;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (m < M && nt0 + j < ntiles) {
        const int n = (nt0 + j) * 16 + ocol;
        const int tl = i * NT + j;
        float v = ((red[0][tl][src] + red[1][tl][src]) + red[2][tl][src]) +
                  red[3][tl][src];
        if (bias != nullptr) v += bf16_to_f32(bias[n]);
        out[static_cast<int64_t>(m) * N + n] = f32_to_bf16(v);
      }
    }
  }
}

// -0.0 (code 8) -> +0.0 in both halves of a packed bf16 pair
FI_DEV u32 canon_zero_x2(u32 v) {
  if ((v & 0x00007fffu) == 0) v &= 0xffff0000u;
  if ((v & 0x7fff0000u) == 0) v &= 0x0000ffffu;
  return v;
}

__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(
    u16* __restrict__ out,                  // [N, K] bf16
    const unsigned char* __restrict__ wq,   // [N, K/2]
    const unsigned char* __restrict__ ws,   // [N, K/32]
    const int64_t nblocks) {                // N * K / 32 MX blocks
  const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (b >= nblocks) return;
  const u32x4 w = *reinterpret_cast<const u32x4*>(wq + b * 16);
  const float sc = e8m0_to_f32(ws[b]);
  u32x4* dst = reinterpret_cast<u32x4*>(out + b * 32);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    union {
      short8 v;
      u32x4 u;
    } f;
    f.v = dequant_fp4x8(w[t], sc);
#pragma unroll
    for (int e = 0; e < 4; ++e) f.u[e] = canon_zero_x2(f.u[e]);
    dst[t] = f.u;
  }
}

template <int MT, int NT, int U>
void launch_linear(u16* out, const u16* x, const unsigned char* wq,
                   const unsigned char* ws, const u16* bias, int M, int N,
                   int K, hipStream_t stream) {
  const dim3 grid(ceil_div(N / 16, NT), ceil_div(M, 16 * MT));
  mxfp4_linear_kernel<MT, NT, U>
      <<<grid, 256, 0, stream>>>(out, x, wq, ws, bias, M, N, K);
}

}  // namespace

// M >= 1, K % 128 == 0, N % 16 == 0 (checked by the binding). The instance
// is chosen from M alone: decode-sized batches keep one column tile per
// workgroup (most workgroups, deepest load queue); larger ones share each x
// fragment among four column tiles. Rows past 64 go to further row blocks.
void launch_mxfp4_linear(u16* out, const u16* x, const unsigned char* wq,
                         const unsigned char* ws, const u16* bias, int M,
                         int N, int K, hipStream_t stream) {
  if (M <= 16)
    launch_linear<1, 1, 2>(out, x, wq, ws, bias, M, N, K, stream);
  else if (M <= 32)
    launch_linear<2, 4, 1>(out, x, wq, ws, bias, M, N, K, stream);
  else
    launch_linear<4, 4, 1>(out, x, wq, ws, bias, M, N, K, stream);
}

void launch_mxfp4_dequant(u16* out, const unsigned char* wq,
                          const unsigned char* ws, int64_t nblocks,
                          hipStream_t stream) {
  const int64_t grid = (nblocks + 255) / 256;
  mxfp4_dequant_kernel<<<static_cast<unsigned int>(grid), 256, 0, stream>>>(
      out, wq, ws, nblocks);
}

}  // namespace fi
