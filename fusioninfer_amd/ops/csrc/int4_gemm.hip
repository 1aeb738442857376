// Int4 group-quantised weight-only (W4A16) linear and dequant kernels for
// gfx950: the AWQ / GPTQ weight format.
//
//   out[m, n] = bf16( sum_k x[m, k] * dq(W)[n, k] (+ bias[n]) ),  fp32 sums
//   dq(W)[n, k] = bf16_rne( fp32(q - z) * fp32(s) )
//
// W is unsigned 4-bit codes q along K, two per byte (k even in the low
// nibble), with one fp16 scale s and one zero point z (a byte, 0..15) per
// group of G = 32, 64 or 128 consecutive k of a row. (q - z) has 5
// significant bits and s has 11, so the fp32 product is exact and dq has
// exactly one rounding. Scales are finite, positive, normal fp16 and zeros
// are at most 15 (host-side validator), so every dq value is zero or a
// normal bf16. The kernels never index from weight, scale or zero data.
//
// Lane -> k map of int4_linear_kernel. Lane l (column c = l & 15, k-group
// g = l >> 4) of k-chunk s (128 k) loads the 16 B that hold
// k = 128 s + 32 g ... + 31 of W row n0 + c: dword t, byte b holds
// k = 128 s + 32 g + 8 t + 2 b in its low nibble and that k + 1 in its high
// nibble. 32 divides G, so the run lies in one group: one scale and one zero,
// read at index (4 s + g) >> log2(G / 32) of the row. dequant_int4x8 of dword
// t is B fragment t of mfma_f32_16x16x32_bf16 with element j = k + 8 t + j:
// the natural order, because an A fragment is 16 contiguous bytes of x and
// each of its dwords is a pair (k even, k + 1) - the two nibbles of one W
// byte. Lane (row r, group g) element j of A step t is
// x[r][128 s + 32 g + 8 t + j].
//
// Expansion of one dword (8 codes), 18 VALU against MXFP4's 4 converts:
//   lo = w & 0x0f0f0f0f          byte b = q[2b]
//   hi = w & 0xf0f0f0f0          byte b = 16 q[2b + 1]
//   v_cvt_f32_ubyte{0..3} of each (cvt_f32_ubyte in int4_common.h), then
//   fma(q, s, -z s) and fma(16 q, s / 16, -z s), paired by the compiler into
//   v_pk_fma_f32, and v_cvt_pk_bf16_f32 per pair: 2 + 8 + 4 + 4 in the ISA.
// z s (4 x 11 bits), s / 16 and 16 q are exact, and q s - z s = (q - z) s is
// representable, so the single rounding of the fma gives exactly
// fp32(q - z) * fp32(s); q == z gives +0. The packed-bf16 route
// (0x4300 | q, subtract 128 + z, multiply) was not built: on paper a pair of
// one byte's nibbles needs a byte permute before the mask and each half a
// widening shift before the fp32 multiply, about 30 VALU per dword. That
// count is an estimate, not a measurement.
//
// The four waves split K in interleaved pairs of chunks (a pair is one
// 128 B line of every W row) and combine through LDS in fixed wave order
// ((w0 + w1) + w2) + w3. The split depends on K only, so a row's bits do not
// depend on M, on the row's position or on the <MT, NT> instance that served
// it: deterministic and batch-invariant, no atomics, no workspace.
//
// int4_dequant_kernel expands W to bf16 [N, K]: 32 k per thread, 16 B in,
// 64 B out, through the same dequant_int4x8; it backs the large-M path
// (dequant + library GEMM).

#include <hip/hip_runtime.h>

#include "int4_common.h"

namespace fi {

namespace {

// U = chunk pairs a wave keeps in flight per loop trip
template <int MT, int NT, int U>
__global__ __launch_bounds__(256) void int4_linear_kernel(
    u16* __restrict__ out,                  // [M, N] bf16
    const u16* __restrict__ x,              // [M, K] bf16
    const unsigned char* __restrict__ wq,   // [N, K/2]
    const u16* __restrict__ ws,             // [N, K/G] fp16 bits
    const unsigned char* __restrict__ wz,   // [N, K/G]
    const u16* __restrict__ bias,           // [N] bf16 or nullptr
    const int M, const int N, const int K,
    const int gshift) {                     // log2(G / 32)
  constexpr int C = 2 * U;  // chunks in flight
  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
  const int col = lane & 15;
  const int g = lane >> 4;
  const int nt0 = blockIdx.x * NT;       // first 16-column tile
  const int ntiles = N / 16;
  const int m0 = blockIdx.y * (16 * MT);  // first row
  const int nchunks = K / 128;
  const int ngroups = (K / 32) >> gshift;  // per row

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
  int64_t gbase[NT];  // first group of the lane's W row
  bool wok[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    wok[j] = nt0 + j < ntiles;  // wave-uniform
    const int64_t n = static_cast<int64_t>(min(nt0 + j, ntiles - 1)) * 16 + col;
    wp[j] = wq + n * (K / 2) + 16 * g;
    gbase[j] = n * ngroups;
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
    u16 sv[C][NT];
    unsigned char zv[C][NT];
    // issue every load of the trip before the first use
#pragma unroll
    for (int q = 0; q < C; ++q) {
      const int c = 2 * (p + 4 * (q >> 1)) + (q & 1);
      const bool cok = c < nchunks;  // wave-uniform
      const int grp = (4 * c + g) >> gshift;  // < ngroups when cok
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        wv[q][j] = u32x4{0, 0, 0, 0};
        sv[q][j] = 0;
        zv[q][j] = 0;
        if (cok && wok[j]) {
          wv[q][j] = *reinterpret_cast<const u32x4*>(wp[j] + c * 64);
          sv[q][j] = ws[gbase[j] + grp];
          zv[q][j] = wz[gbase[j] + grp];
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
            const GroupScale gs = group_scale(sv[q][j], zv[q][j]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const short8 b = dequant_int4x8(wv[q][j][t], gs);
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

__global__ __launch_bounds__(256) void int4_dequant_kernel(
    u16* __restrict__ out,                  // [N, K] bf16
    const unsigned char* __restrict__ wq,   // [N, K/2]
    const u16* __restrict__ ws,             // [N, K/G] fp16 bits
    const unsigned char* __restrict__ wz,   // [N, K/G]
    const int64_t nruns,                    // N * K / 32 runs of 32 k
    const int gshift) {                     // log2(G / 32)
  const int64_t b = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (b >= nruns) return;
  const u32x4 w = *reinterpret_cast<const u32x4*>(wq + b * 16);
  // K / 32 is a multiple of G / 32, so the flat run index shifts to the
  // flat group index
  const int64_t grp = b >> gshift;
  const GroupScale gs = group_scale(ws[grp], wz[grp]);
  u32x4* dst = reinterpret_cast<u32x4*>(out + b * 32);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    union {
      short8 v;
      u32x4 u;
    } f;
    f.v = dequant_int4x8(w[t], gs);
    dst[t] = f.u;
  }
}

template <int MT, int NT, int U>
void launch_linear(u16* out, const u16* x, const unsigned char* wq,
                   const u16* ws, const unsigned char* wz, const u16* bias,
                   int M, int N, int K, int gshift, hipStream_t stream) {
  const dim3 grid(ceil_div(N / 16, NT), ceil_div(M, 16 * MT));
  int4_linear_kernel<MT, NT, U>
      <<<grid, 256, 0, stream>>>(out, x, wq, ws, wz, bias, M, N, K, gshift);
}

}  // namespace

// M >= 1, K % 128 == 0, N % 16 == 0, gshift in {0, 1, 2} (checked by the
// binding). The instance is chosen from M alone: decode-sized batches keep
// one column tile per workgroup (most workgroups, deepest load queue);
// larger ones share each x fragment among four column tiles, which also
// spreads the expansion of a W run over MT row tiles. Rows past 64 go to
// further row blocks.
void launch_int4_linear(u16* out, const u16* x, const unsigned char* wq,
                        const u16* ws, const unsigned char* wz,
                        const u16* bias, int M, int N, int K, int gshift,
                        hipStream_t stream) {
  if (M <= 16)
    launch_linear<1, 1, 2>(out, x, wq, ws, wz, bias, M, N, K, gshift, stream);
  else if (M <= 32)
    launch_linear<2, 4, 1>(out, x, wq, ws, wz, bias, M, N, K, gshift, stream);
  else
    launch_linear<4, 4, 1>(out, x, wq, ws, wz, bias, M, N, K, gshift, stream);
}

void launch_int4_dequant(u16* out, const unsigned char* wq, const u16* ws,
                         const unsigned char* wz, int64_t nruns, int gshift,
                         hipStream_t stream) {
  const int64_t grid = (nruns + 255) / 256;
  int4_dequant_kernel<<<static_cast<unsigned int>(grid), 256, 0, stream>>>(
      out, wq, ws, wz, nruns, gshift);
}

}  // namespace fi
