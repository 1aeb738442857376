// Grouped W4A16 GEMM for MoE experts stored as MXFP4 (gfx950).
//
//   out[slot, n] = bf16( f( sum_k A[row(slot), k] * dq(W[e])[n, k] ) )
//
// joins the two existing halves: the block-aligned grouped-GEMM contract of
// moe_gemm.hip (sorted_ids / expert_ids / the n_valid device scalar, static
// grid, fused SwiGLU epilogue) and the exact e2m1/e8m0 expansion and lane
// mapping of mxfp4_gemm.hip. Expert weights use the row format mxfp4_linear
// reads, per expert: w_packed [E, NB, K/2] (k even in the low nibble) and
// w_scale [E, NB, K/32] e8m0 bytes in [8, 247]; NB = 2N for gate_up (gate
// rows first, then up rows), NB = N for down. Dequantisation is exact, so
// the kernel is a bf16 grouped GEMM on dq(W). It never scans scale bytes
// and never indexes from weight or scale data.
//
// Lane l (column c = l & 15, group g = l >> 4) of k-chunk s (128 k) loads
// the 16 B that hold k = 128 s + 32 g ... + 31 of W row n0 + c: one MX
// block, one scale byte. Fragment t of it is k = 128 s + 32 g + 8 t + j, and
// the A operand uses the same permuted k (a contiguous 16 B of the row), as
// documented at the top of mxfp4_gemm.hip. No bf16 copy of W exists
// anywhere: packed bytes go from HBM to VGPRs and are expanded there.
//
// One template, two instances per epilogue, chosen by block_m:
//  * MITER = 1 (block_m 16, decode): the moe_gemm BM=16 form. A wave owns
//    one 16-column fragment (gate and up rows of it when GATE_UP) over the
//    whole K; no LDS, no barriers. Chunks are issued in pairs (a pair is
//    one 128 B line of every W row) and double-buffered in registers, so
//    two lines per row are in flight while the previous pair is consumed.
//    The waves do not split K: the down GEMM of Qwen3-30B-A3B has K = 768,
//    six chunks, which a four-way split cannot share out evenly, and a
//    split would have to be reproduced by the block_m 128 instance.
//  * MITER = 8 (block_m 128, prefill): a wave owns the same column fragment
//    for all eight row fragments of the m-tile, so every dequantised B
//    fragment is reused from registers eight times; the next chunk's packed
//    W is in flight meanwhile.
//
// Determinism: every accumulator sums its row's K in ascending (chunk,
// fragment) order through the same MFMA in both instances, so the bits of
// a (token, expert) row depend on that row and the weights only — not on
// block_m, the slot or the other tokens. No atomics, no workspace.
//
// C-fragment map (16x16): row = (lane >> 4) * 4 + r, col = lane & 15.

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

// Eight e2m1 codes of one u32 (k ascending) times `scale` -> 8 bf16
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

// same expression as moe_gemm_kernel's epilogue
FI_DEV float swiglu(float g, float u) { return (g / (1.f + __expf(-g))) * u; }

// NF W rows per lane (gate, up) of one k-chunk: packed block + scale byte
template <int NF>
struct WChunk {
  u32x4 w[NF];
  u32 s[NF];
};

template <int MITER, bool GATE_UP>
__global__ __launch_bounds__(256) void moe_mxfp4_gemm_kernel(
    u16* __restrict__ out,                 // [PM, N] bf16
    const u16* __restrict__ a,             // GATE_UP: x [T, K]; else act [PM, K]
    const unsigned char* __restrict__ wq,  // [E, NB, K/2]
    const unsigned char* __restrict__ ws,  // [E, NB, K/32]
    const int* __restrict__ sorted_ids,    // [PM] token row per padded slot
    const int* __restrict__ expert_ids,    // [PM/BM] local expert per m-tile
    const int* __restrict__ n_valid,       // device scalar: real m-tile count
    const int K, const int N) {
  constexpr int BM = 16 * MITER;
  constexpr int NF = GATE_UP ? 2 : 1;
  using WC = WChunk<NF>;
  const int mtile = blockIdx.x;
  if (mtile >= *n_valid) return;

  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
  const int col = lane & 15;
  const int g = lane >> 4;
  // this wave's 16-column fragment; no barrier below, so a wave past N
  // simply leaves
  const int nt = blockIdx.y * 4 + wave;
  if (nt >= N / 16) return;
  const int e = expert_ids[mtile];
  const int nchunks = K / 128;

  const unsigned char* wp[NF];
  const unsigned char* sp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int64_t n = static_cast<int64_t>(e) * (NF * N) + f * N + nt * 16 + col;
    wp[f] = wq + n * (K / 2) + 16 * g;
    sp[f] = ws + n * (K / 32) + g;
  }
  // A rows: gathered through sorted_ids for gate_up (padding slots carry a
  // valid dummy row), read by slot otherwise
  const u16* ap[MITER];
#pragma unroll
  for (int mi = 0; mi < MITER; ++mi) {
    const int slot = mtile * BM + mi * 16 + col;
    const int row = GATE_UP ? sorted_ids[slot] : slot;
    ap[mi] = a + static_cast<int64_t>(row) * K + 32 * g;
  }

  floatx4 acc[MITER][NF];
#pragma unroll
  for (int mi = 0; mi < MITER; ++mi)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[mi][f] = floatx4{0.f, 0.f, 0.f, 0.f};

  auto load_w = [&](WC& d, int c) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      d.w[f] = *reinterpret_cast<const u32x4*>(wp[f] + c * 64);
      d.s[f] = sp[f][c * 4];
    }
  };

  if constexpr (MITER == 1) {
    // pairs of chunks, double-buffered; every buffer index is a compile-time
    // constant (runtime-indexed register arrays go to scratch)
    const int npairs = (nchunks + 1) / 2;
    WC w0[2], w1[2];
    short8 x0[2][4], x1[2][4];
    auto issue = [&](WC (&wd)[2], short8 (&xd)[2][4], int p) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = 2 * p + q;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          wd[q].w[f] = u32x4{0, 0, 0, 0};
          wd[q].s[f] = 127;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) xd[q][t] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        if (c < nchunks) {  // wave-uniform
          load_w(wd[q], c);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            xd[q][t] =
                *reinterpret_cast<const short8*>(ap[0] + c * 128 + 8 * t);
        }
      }
    };
    auto consume = [&](WC (&wv)[2], short8 (&xv)[2][4], int p) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (2 * p + q < nchunks) {  // an absent chunk adds nothing at all
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            const float sc = e8m0_to_f32(wv[q].s[f]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
              acc[0][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  xv[q][t], dequant_fp4x8(wv[q].w[f][t], sc), acc[0][f], 0, 0,
                  0);
          }
        }
      }
    };
    issue(w0, x0, 0);
    for (int p = 0; p < npairs; p += 2) {
      if (p + 1 < npairs) issue(w1, x1, p + 1);
      consume(w0, x0, p);
      if (p + 1 < npairs) {
        if (p + 2 < npairs) issue(w0, x0, p + 2);
        consume(w1, x1, p + 1);
      }
    }
  } else {
    // the next chunk's packed W stays in flight while this chunk's
    // dequantised fragments serve all MITER row fragments
    WC wa, wb;
    auto consume = [&](WC& wv, int c) {
      short8 b[NF][4];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const float sc = e8m0_to_f32(wv.s[f]);
#pragma unroll
        for (int t = 0; t < 4; ++t) b[f][t] = dequant_fp4x8(wv.w[f][t], sc);
      }
#pragma unroll
      for (int mi = 0; mi < MITER; ++mi) {
        short8 xv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
          xv[t] = *reinterpret_cast<const short8*>(ap[mi] + c * 128 + 8 * t);
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[mi][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                xv[t], b[f][t], acc[mi][f], 0, 0, 0);
      }
    };
    load_w(wa, 0);
    for (int c = 0; c < nchunks; c += 2) {
      if (c + 1 < nchunks) load_w(wb, c + 1);
      consume(wa, c);
      if (c + 1 < nchunks) {
        if (c + 2 < nchunks) load_w(wa, c + 2);
        consume(wb, c + 1);
      }
    }
  }

  const int ocol = nt * 16 + col;
#pragma unroll
  for (int mi = 0; mi < MITER; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = mtile * BM + mi * 16 + g * 4 + r;
      float v = acc[mi][0][r];
      if constexpr (GATE_UP) v = swiglu(v, acc[mi][NF - 1][r]);
      out[static_cast<int64_t>(orow) * N + ocol] = f32_to_bf16(v);
    }
  }
}

}  // namespace

// K % 128 == 0, N % 16 == 0, block_m in {16, 128} (checked by the binding).
// Four waves per workgroup, one 16-column fragment each; the grid is static
// (max_mtiles m-tiles) and tiles at or past *n_valid leave at once.
void launch_moe_gemm_mxfp4(u16* out, const u16* a, const unsigned char* wq,
                           const unsigned char* ws, const int* sorted_ids,
                           const int* expert_ids, const int* n_valid,
                           int max_mtiles, int K, int N, int block_m,
                           bool gate_up, hipStream_t stream) {
  decltype(&moe_mxfp4_gemm_kernel<1, true>) kernel;
  if (block_m == 16)
    kernel = gate_up ? moe_mxfp4_gemm_kernel<1, true>
                     : moe_mxfp4_gemm_kernel<1, false>;
  else
    kernel = gate_up ? moe_mxfp4_gemm_kernel<8, true>
                     : moe_mxfp4_gemm_kernel<8, false>;
  hipLaunchKernelGGL(kernel, dim3(max_mtiles, ceil_div(N / 16, 4)), dim3(256),
                     0, stream, out, a, wq, ws, sorted_ids, expert_ids,
                     n_valid, K, N);
}

}  // namespace fi
