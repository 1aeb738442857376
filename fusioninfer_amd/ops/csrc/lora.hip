// Batched multi-LoRA apply (Punica/S-LoRA style) for gfx950.
//
//   out[t] += scales[s] * bf16(x[t] . a_stack[s]^T) . b_stack[s]^T,
//   s = slot_ids[t]; ids outside [0, S) mean "no adapter".
//
// Two static-shape kernels indexed by a per-token slot id, so a decode
// step with adapters is hipGraph-capturable (no host-side grouping, no
// data-dependent launch shapes):
//  * shrink: y[T, R] = x . A_s^T. One workgroup per (16-token tile,
//    16-column r-tile); its four waves split K in interleaved 64-element
//    chunks and reduce through LDS in a fixed order (w0+w1+w2+w3).
//  * expand: out += scale_s * (y . B_s^T). One workgroup per (16-token
//    tile, 256 output columns), each wave owns four 16-column n-tiles;
//    fused fp32 scale + read-add-write of out.
// Both run mfma_f32_16x16x32_bf16 with fp32 accumulation; the shrink
// result is rounded to bf16 once (where the torch path rounds too).
//
// Mixed tiles: each wave reads the tile's 16 slot ids, and the workgroup
// loops over the distinct slots present (ballot over the remaining
// lanes); rows of another slot are fed as zeros and never written. A
// tile without any adapter exits after reading its 16 ints.
//
// Determinism / batch invariance: no atomics; a row's result depends only
// on its own x row and its slot's weights — the K order per wave, the
// cross-wave order and the rank order are fixed and independent of T, of
// the row's position in the tile and of the other rows' slots.
//
// Fragment maps (see moe_gemm.hip): A lane l holds A[l&15][8(l>>4)+e],
// B lane l holds B[8(l>>4)+e][l&15], C row = (l>>4)*4 + r, col = l&15.
// Both operands are K-contiguous in memory here (x / a_stack rows for
// shrink, y / b_stack rows for expand): one 16 B load per fragment.

#include <hip/hip_runtime.h>

#include "common.h"

namespace fi {

namespace {

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float floatx4;

FI_DEV short8 load_b16x8_if(const u16* p, bool ok) {
  short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ok) v = *reinterpret_cast<const short8*>(p);
  return v;
}

// Lane i < 16 returns the validated slot of token t0 + i (-1 = none);
// lanes >= 16 return -1. No read happens past T.
FI_DEV int tile_slot(const int* __restrict__ slot_ids, int t0, int T, int S,
                     int lane) {
  int sid = -1;
  if (lane < 16 && t0 + lane < T) {
    sid = slot_ids[t0 + lane];
    if (sid < 0 || sid >= S) sid = -1;
  }
  return sid;
}

__global__ __launch_bounds__(256) void lora_shrink_kernel(
    u16* __restrict__ y,               // [T, R] bf16 workspace
    const u16* __restrict__ x,         // [T, K] bf16
    const int* __restrict__ slot_ids,  // [T]
    const u16* __restrict__ a_stack,   // [S, R, K] bf16
    const int T, const int K, const int R, const int S) {
  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
  const int t0 = blockIdx.x * 16;
  const int rt = blockIdx.y;  // 16-column tile of R

  const int my = tile_slot(slot_ids, t0, T, S, lane);
  unsigned long long pending = __ballot(my >= 0);
  if (pending == 0) return;  // workgroup-uniform: no adapter in this tile

  __shared__ __attribute__((aligned(16))) float red[4][256];

  const int row = lane & 15;
  const int kq = (lane >> 4) * 8;
  const int in_slot = __shfl(my, row, 64);  // slot of this lane's x row
  const int xrow = min(t0 + row, T - 1);    // never dereferenced past T
  const u16* xp = x + static_cast<int64_t>(xrow) * K + kq;
  // reduce/store role: thread -> one element of the 16x16 result
  const int orow = threadIdx.x >> 4;  // == wave*4 + (lane>>4)
  const int ocol = threadIdx.x & 15;
  const int out_slot = __shfl(my, orow, 64);
  const int src = ((orow >> 2) * 16 + ocol) * 4 + (orow & 3);
  const int nchunks = K / 64;

  while (pending) {
    const int leader = __ffsll(pending) - 1;
    const int s = __shfl(my, leader, 64);
    pending &= ~__ballot(my == s);
    const bool mine = in_slot == s;
    const u16* ap =
        a_stack + (static_cast<int64_t>(s) * R + rt * 16 + row) * K + kq;

    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    // one 64-element chunk = two k-steps; xv/av: [2] fragments
    auto issue = [&](short8 (&xv)[2], short8 (&av)[2], int c) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        xv[h] = load_b16x8_if(xp + c * 64 + h * 32, mine);
        av[h] = *reinterpret_cast<const short8*>(ap + c * 64 + h * 32);
      }
    };
    auto consume = [&](const short8 (&xv)[2], const short8 (&av)[2]) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xv[h], av[h], acc, 0, 0,
                                                      0);
    };
    // manual unroll by two chunks keeps eight loads in flight per wave;
    // the accumulation order stays ascending in K
    int c = wave;
    for (; c + 4 < nchunks; c += 8) {
      short8 xa[2], aa[2], xb[2], ab[2];
      issue(xa, aa, c);
      issue(xb, ab, c + 4);
      consume(xa, aa);
      consume(xb, ab);
    }
    if (c < nchunks) {
      short8 xa[2], aa[2];
      issue(xa, aa, c);
      consume(xa, aa);
    }
    *reinterpret_cast<floatx4*>(&red[wave][lane * 4]) = acc;
    __syncthreads();
    if (out_slot == s) {  // implies t0 + orow < T
      const float v = ((red[0][src] + red[1][src]) + red[2][src]) + red[3][src];
      y[static_cast<int64_t>(t0 + orow) * R + rt * 16 + ocol] = f32_to_bf16(v);
    }
    __syncthreads();  // red is reused by the next slot's pass
  }
}

constexpr int kExpandNIter = 4;  // 16-column n-tiles per wave

__global__ __launch_bounds__(256) void lora_expand_kernel(
    u16* __restrict__ out,             // [T, N] bf16, updated in place
    const u16* __restrict__ y,         // [T, R] bf16
    const int* __restrict__ slot_ids,  // [T]
    const u16* __restrict__ b_stack,   // [S, N, R] bf16
    const float* __restrict__ scales,  // [S]
    const int T, const int N, const int R, const int S) {
  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
  const int t0 = blockIdx.x * 16;
  const int NT = N / 16;
  const int nt0 = (blockIdx.y * 4 + wave) * kExpandNIter;

  const int my = tile_slot(slot_ids, t0, T, S, lane);
  unsigned long long pending = __ballot(my >= 0);
  // wave-uniform exits; the kernel has no barrier
  if (pending == 0 || nt0 >= NT) return;

  const int row = lane & 15;
  const int kq = (lane >> 4) * 8;
  const int in_slot = __shfl(my, row, 64);  // slot of this lane's y row
  int out_slot[4];                          // slots of this lane's C rows
#pragma unroll
  for (int r = 0; r < 4; ++r) out_slot[r] = __shfl(my, (lane >> 4) * 4 + r, 64);
  const int yrow = min(t0 + row, T - 1);
  const u16* yp = y + static_cast<int64_t>(yrow) * R + kq;

  while (pending) {
    const int leader = __ffsll(pending) - 1;
    const int s = __shfl(my, leader, 64);
    pending &= ~__ballot(my == s);
    const bool mine = in_slot == s;
    const float sc = scales[s];

    // R <= 128: at most four 32-wide k-steps; a trailing half step
    // (R % 32 == 16) is zero-filled on both operands
    short8 yv[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      yv[kt] = load_b16x8_if(yp + kt * 32, mine && kt * 32 + kq < R);

    const u16* bs = b_stack + static_cast<int64_t>(s) * N * R + kq;
#pragma unroll
    for (int ni = 0; ni < kExpandNIter; ++ni) {
      const int nt = nt0 + ni;
      if (nt >= NT) break;  // wave-uniform tail
      const u16* bn = bs + static_cast<int64_t>(nt * 16 + row) * R;
      floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        if (kt * 32 < R) {
          const short8 bv = load_b16x8_if(bn + kt * 32, kt * 32 + kq < R);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yv[kt], bv, acc, 0, 0,
                                                        0);
        }
      }
      const int col = nt * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (out_slot[r] == s) {  // implies the row is < T
          const int64_t idx =
              static_cast<int64_t>(t0 + (lane >> 4) * 4 + r) * N + col;
          out[idx] = f32_to_bf16(bf16_to_f32(out[idx]) + sc * acc[r]);
        }
      }
    }
  }
}

}  // namespace

void launch_lora_apply(u16* out, u16* y, const u16* x, const int* slot_ids,
                       const u16* a_stack, const u16* b_stack,
                       const float* scales, int T, int K, int N, int R, int S,
                       hipStream_t stream) {
  const int tiles = ceil_div(T, 16);
  lora_shrink_kernel<<<dim3(tiles, R / 16), 256, 0, stream>>>(
      y, x, slot_ids, a_stack, T, K, R, S);
  lora_expand_kernel<<<dim3(tiles, ceil_div(N / 16, 4 * kExpandNIter)), 256, 0,
                       stream>>>(out, y, slot_ids, b_stack, scales, T, N, R,
                                 S);
}

}  // namespace fi
