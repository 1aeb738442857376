// Grouped MXFP4 x MXFP8 scaled-MFMA GEMM for MoE experts at prefill
// (gfx950): the block_m 128 path of `--mxfp4-moe-activations mxfp8`, and
// below it the block_m 32 instance of `mxfp8-wide` for mid-size batches.
//
//   down:    out[slot, n] = bf16( sum_k dq(a)[slot, k] * dq(W[e])[n, k] )
//   gate_up: (out, out_scale)[slot] = mxfp8_quant_rows( bf16( swiglu(
//                sum_k dq(a)[row(slot), k] * dq(W[e])[n, k],
//                sum_k dq(a)[row(slot), k] * dq(W[e])[N + n, k] ) ) )
//
// joins the block-aligned grouped-GEMM contract of moe_gemm_mxfp4
// (sorted_ids / expert_ids / the n_valid device scalar, static grid; an
// m-tile is 128 padded slots of one expert) and the operand movement of
// mxfp4_mxfp8_gemm_kernel, in the lane layout of
// v_mfma_scale_f32_16x16x128_f8f6f4 documented in mx_common.h, which also
// holds the operand helpers and both epilogues. Expert weights are the
// tensors moe_gemm_mxfp4 reads, unchanged: w_packed [E, NB, K/2] and w_scale
// [E, NB, K/32], NB = 2N (gate rows, then up rows) for gate_up. Neither
// operand is expanded, nothing is repacked, and nothing is indexed from
// weight or scale data.
//
// Operand movement, both instances. W is srcA and the activation is srcB.
// Per 128-k step a wave loads its 4 W fragments (16 B per lane, one MX block
// each) and their scale bytes from HBM/L2 straight to VGPRs, one step ahead.
// The 128-row x 128-byte activation panel of a step is staged through
// registers into LDS once per workgroup (144 B padded rows, double-buffered,
// one barrier per step), and so are the 4 activation scale bytes of every
// row for that step (one dword per row; a lane shifts out the byte of its
// MX block). Panel row i is a_q[row(i)] with row(i) = sorted_ids[slot] for
// gate_up (x is quantised once per token and gathered here; pad slots carry
// row 0) and row(i) = slot for down; the ids are read once per workgroup,
// before the K loop. The loop runs two steps per trip over two named operand
// sets, without a branch in the trip, held in order by scheduling fences; an
// odd last step is peeled.
//
// Down (GATE_UP = false): 128 x 128 tile, the waves 2 x 2 with a 4 x 4 block
// of 16x16 accumulators each; 8 B bf16 stores. Columns past N are clamped in
// bounds when loaded and never stored.
//
// Gate_up (GATE_UP = true): 128 slots x 64 act columns; the workgroup reads
// 64 gate rows and the matching 64 up rows of W. The waves sit 2 x 2, each
// owning 64 slots x 32 act columns: 4 m-fragments x (2 gate + 2 up)
// n-fragments, the register budget of the down instance. With W as srcA a
// lane holds m = l & 15 and n = 4 (l >> 4) ... + 3 of every fragment, so the
// gate and the up value of one act element sit in the same lane and element,
// and a wave owns whole 32-column MX blocks of an act row: the epilogue
// (store_swiglu_mxfp8_tile, mx_common.h) needs no LDS and applies the scale
// byte, scaling, clamp, convert and -0 rule of quant_mxfp8_rows. The output
// equals reference.mxfp8_quant_rows on the bf16 act row, bit for bit; the
// bf16 act tensor never exists.
//
// Determinism: every accumulator sums the K steps in ascending order and
// nothing is split or combined across waves, so a (token, expert) row's bits
// depend on its own operands only, and a down row equals mxfp4_mxfp8_linear
// on that row and its expert's weights bit for bit. No atomics, no
// workspace, no host sync; a workgroup whose m-tile is >= *n_valid returns
// before any barrier.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "mx_common.h"

namespace fi {

namespace {

constexpr int kBlockM = 128;     // slots of an m-tile

template <bool GATE_UP>
__global__ __launch_bounds__(256, 2) void moe_mxfp4_mxfp8_gemm_kernel(
    void* __restrict__ out_v,               // [PM, N] bf16, or e4m3 (GATE_UP)
    unsigned char* __restrict__ out_scale,  // GATE_UP: [PM, N/32] e8m0
    const unsigned char* __restrict__ aq,   // GATE_UP: [T, K]; else [PM, K]
    const unsigned char* __restrict__ asc,  // same rows, [., K/32] e8m0
    const unsigned char* __restrict__ wq,   // [E, NB, K/2]
    const unsigned char* __restrict__ ws,   // [E, NB, K/32]
    const int* __restrict__ sorted_ids,     // [PM] token row per padded slot
    const int* __restrict__ expert_ids,     // [PM/128] local expert per tile
    const int* __restrict__ n_valid,        // device scalar: real tile count
    const int K, const int N) {
  const int mtile = blockIdx.x;
  if (mtile >= *n_valid) return;

  // columns of out per workgroup and per wave
  constexpr int kTileN = GATE_UP ? 64 : 128;
  constexpr int kWaveN = kTileN / 2;
  const int tid = threadIdx.x;
  const int lane = tid % kWaveSize;
  const int wave = tid / kWaveSize;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int slot0 = mtile * kBlockM;
  const int wm = 64 * (wave >> 1);                            // first slot
  const int wn = blockIdx.y * kTileN + kWaveN * (wave & 1);   // first column
  const int nsteps = K / 128;
  const int NB = GATE_UP ? 2 * N : N;
  const int64_t wrow0 = static_cast<int64_t>(expert_ids[mtile]) * NB;

  __shared__ __attribute__((aligned(16))) unsigned char
      xl[2][kBlockM * kRowBytes];
  // the step's 4 scale bytes of every row; the upper 128 entries only give
  // threads 128 ... 255 somewhere to store, so that no store is predicated
  __shared__ u32 sl[2][2 * kBlockM];

  // panel staging: thread -> rows tid / 8 + 32 i, 16 B chunk tid % 8; scale
  // staging: thread -> row tid % 128
  const unsigned char* xg[4];
  int xo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (tid >> 3) + 32 * i;
    const int src = GATE_UP ? sorted_ids[slot0 + row] : slot0 + row;
    xg[i] = aq + static_cast<int64_t>(src) * K + 16 * (tid & 7);
    xo[i] = row * kRowBytes + 16 * (tid & 7);
  }
  const unsigned char* sg;
  {
    const int row = tid & (kBlockM - 1);
    const int src = GATE_UP ? sorted_ids[slot0 + row] : slot0 + row;
    sg = asc + static_cast<int64_t>(src) * (K / 32);
  }
  // W fragments and their scale bytes: lane -> row r, MX block g of the step
  const unsigned char* wp[4];
  const unsigned char* wsp[4];
  w_frag_ptrs<GATE_UP>(wp, wsp, wq, ws, wrow0, wn, r, g, N, K);
  // x fragment: bytes 16 g ... + 15 and 64 + 16 g ... + 15 of the row's step
  const int xfrag = (wm + r) * kRowBytes + 16 * g;

  floatx4 acc[4][4];  // [n fragment][m fragment]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = floatx4{0.f, 0.f, 0.f, 0.f};

  // two named operand sets: step s computes from set s & 1 while the loads
  // of step s + 1 land in the other one. The panel and its scales are loaded
  // two steps ahead (stage[s & 1] holds step s + 2).
  u32x4 stage[2][4], wv[2][4];
  u32 sstage[2], wsc[2][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    stage[0][i] = *reinterpret_cast<const u32x4*>(xg[i]);
    stage[1][i] = *reinterpret_cast<const u32x4*>(
        xg[i] + min(1, nsteps - 1) * 128);
  }
  sstage[0] = *reinterpret_cast<const u32*>(sg);
  sstage[1] = *reinterpret_cast<const u32*>(sg + min(1, nsteps - 1) * 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wv[0][j] = *reinterpret_cast<const u32x4*>(wp[j]);
    wsc[0][j] = wsp[j][0];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<u32x4*>(&xl[0][xo[i]]) = stage[0][i];
  sl[0][tid] = sstage[0];
  __syncthreads();

  // the 16 MFMAs of one step: operand set and LDS buffers P
  auto mfmas = [&](auto P) {
    constexpr int p = decltype(P)::value;
    const unsigned char* buf = xl[p];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const intx8 xv = lds_read_a8_frag(buf + xfrag + 16 * i * kRowBytes);
      // byte g of the row's dword (one v_bfe_u32)
      const u32 xsc = (sl[p][wm + 16 * i + r] >> (8 * g)) & 0xffu;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j][i] = mfma_w4a8(wv[p][j], wsc[p][j], xv, xsc, acc[j][i]);
    }
  };
  // one full step s of parity P. Past the end the last step is loaded again
  // and stored into the idle buffers: in bounds, never read.
  auto step = [&](auto P, int s) {
    constexpr int p = decltype(P)::value;
    const int sn = min(s + 1, nsteps - 1);
    const int sx = min(s + 2, nsteps - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      stage[p][i] = *reinterpret_cast<const u32x4*>(xg[i] + sx * 128);
    sstage[p] = *reinterpret_cast<const u32*>(sg + sx * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wv[p ^ 1][j] = *reinterpret_cast<const u32x4*>(wp[j] + sn * 64);
      wsc[p ^ 1][j] = wsp[j][sn * 4];
    }
    FI_SCHED_FENCE();  // the loads are issued before the MFMAs ...
    mfmas(P);
    FI_SCHED_FENCE();  // ... and waited for only after them
    // buffers p ^ 1 were last read in step s - 1, before its barrier
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<u32x4*>(&xl[p ^ 1][xo[i]]) = stage[p ^ 1][i];
    sl[p ^ 1][tid] = sstage[p ^ 1];
    __syncthreads();
  };
  // Two steps per trip with no branch between them, so the fences hold both
  // halves in place. An odd last step is peeled: its operands are already in
  // set 0 and buffers 0.
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  for (int s = 0; s + 1 < nsteps; s += 2) {
    step(P0{}, s);
    step(P1{}, s + 1);
  }
  if (nsteps & 1) mfmas(P0{});

  if constexpr (!GATE_UP)
    store_bf16_tile(static_cast<u16*>(out_v), acc, slot0 + wm, wn, r, g, N);
  else
    store_swiglu_mxfp8_tile(static_cast<unsigned char*>(out_v), out_scale, acc,
                            slot0 + wm, wn, r, g, N);
}

// ---------------------------------------------------------------------------
// block_m 32 instance, for 32 ... 256 routed rows per expert: a weight-bound,
// latency-bound regime (the pair reads every expert's weights and does little
// arithmetic per byte), so the tile is narrow in M and the W prefetch deep.
//
// Split: 256 threads, the four waves side by side in N, sharing no W. Down:
// a wave owns 32 slots x 64 columns (2 m-fragments x 4 n-fragments), the
// workgroup 32 x 256. Gate_up: a wave owns 32 slots x 32 act columns (2
// m-fragments x (2 gate + 2 up) n-fragments: one whole MX block of the act
// row), the workgroup 32 x 128 act columns. 32 accumulator registers either
// way, which leaves room for four named W operand sets: the fragments and
// scale bytes of step s + 3 are requested before the MFMAs of step s, and
// every W byte is read once per (m-tile, column tile).
//
// Activation panel: 32 rows x 128 B per step, one 16 B load per thread.
// kStage steps form a group that is staged through registers into LDS (144 B
// padded rows; one dword per row and step carries the row's 4 scale bytes)
// behind one barrier per group, double-buffered by group; the registers hold
// the group after next while the current one is consumed. The loop runs four
// steps per trip without a branch; up to three remaining steps are peeled.
//
// Accumulation order, epilogues, bounds and the early return are those of the
// 128-slot kernel: a (token, expert) row has the same bits in both.

#ifndef FI_MOE_A8_STAGE
#define FI_MOE_A8_STAGE 4
#endif

constexpr int kBlockM32 = 32;                       // slots of an m-tile
constexpr int kStage = FI_MOE_A8_STAGE;             // steps per barrier
constexpr int kPanelBytes = kBlockM32 * kRowBytes;  // one step's LDS panel
static_assert(kStage == 1 || kStage == 2 || kStage == 4,
              "a trip of four steps must hold whole groups");

template <bool GATE_UP>
__global__ __launch_bounds__(256, 2) void moe_mxfp4_mxfp8_gemm32_kernel(
    void* __restrict__ out_v,               // [PM, N] bf16, or e4m3 (GATE_UP)
    unsigned char* __restrict__ out_scale,  // GATE_UP: [PM, N/32] e8m0
    const unsigned char* __restrict__ aq,   // GATE_UP: [T, K]; else [PM, K]
    const unsigned char* __restrict__ asc,  // same rows, [., K/32] e8m0
    const unsigned char* __restrict__ wq,   // [E, NB, K/2]
    const unsigned char* __restrict__ ws,   // [E, NB, K/32]
    const int* __restrict__ sorted_ids,     // [PM] token row per padded slot
    const int* __restrict__ expert_ids,     // [PM/32] local expert per tile
    const int* __restrict__ n_valid,        // device scalar: real tile count
    const int K, const int N) {
  const int mtile = blockIdx.x;
  if (mtile >= *n_valid) return;

  // columns of out per wave and per workgroup
  constexpr int kWaveN = GATE_UP ? 32 : 64;
  constexpr int kTileN = 4 * kWaveN;
  const int tid = threadIdx.x;
  const int lane = tid % kWaveSize;
  const int wave = tid / kWaveSize;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int slot0 = mtile * kBlockM32;
  const int wn = blockIdx.y * kTileN + kWaveN * wave;  // first column
  const int nsteps = K / 128;
  const int NB = GATE_UP ? 2 * N : N;
  const int64_t wrow0 = static_cast<int64_t>(expert_ids[mtile]) * NB;

  __shared__ __attribute__((aligned(16))) unsigned char
      xl[2][kStage * kPanelBytes];
  // [step of the group][row]; entries from 32 kStage on only give the other
  // threads somewhere to store, so that no store is predicated
  __shared__ u32 sl[2][256];

  // panel staging: thread -> row tid / 8, 16 B chunk tid % 8 of every step of
  // the group; scale staging: thread -> row tid % 32 of step tid / 32
  const unsigned char* xg;
  const unsigned char* sg;
  const int xo = (tid >> 3) * kRowBytes + 16 * (tid & 7);
  const int sstep = tid >> 5;
  {
    const int prow = slot0 + (tid >> 3);
    const int srow = slot0 + (tid & 31);
    xg = aq + static_cast<int64_t>(GATE_UP ? sorted_ids[prow] : prow) * K +
         16 * (tid & 7);
    sg = asc + static_cast<int64_t>(GATE_UP ? sorted_ids[srow] : srow) *
                   (K / 32);
  }
  // W fragments and their scale bytes: lane -> row r, MX block g of the step
  const unsigned char* wp[4];
  const unsigned char* wsp[4];
  w_frag_ptrs<GATE_UP>(wp, wsp, wq, ws, wrow0, wn, r, g, N, K);
  // x fragment: bytes 16 g ... + 15 and 64 + 16 g ... + 15 of the row's step
  const int xfrag = r * kRowBytes + 16 * g;

  floatx4 acc[4][2];  // [n fragment][m fragment]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[j][i] = floatx4{0.f, 0.f, 0.f, 0.f};

  // four named W operand sets: step s computes from set s & 3 while the
  // loads of steps s + 1 ... s + 3 are in flight to the other three. Loads
  // past the end read the last step again: in bounds, never used.
  u32x4 wv[4][4];
  u32 wsc[4][4];
  u32x4 stage[kStage];
  u32 sstage;
  auto load_w = [&](auto P, int s) {
    constexpr int p = decltype(P)::value;
    const int sc = min(s, nsteps - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      wv[p][j] = *reinterpret_cast<const u32x4*>(wp[j] + sc * 64);
      wsc[p][j] = wsp[j][sc * 4];
    }
  };
  // the panel group that starts at step s0: global -> registers -> LDS
  auto load_group = [&](int s0) {
#pragma unroll
    for (int q = 0; q < kStage; ++q)
      stage[q] = *reinterpret_cast<const u32x4*>(
          xg + min(s0 + q, nsteps - 1) * 128);
    sstage = *reinterpret_cast<const u32*>(
        sg + min(s0 + sstep, nsteps - 1) * 4);
  };
  auto store_group = [&](int b) {
#pragma unroll
    for (int q = 0; q < kStage; ++q)
      *reinterpret_cast<u32x4*>(&xl[b][q * kPanelBytes + xo]) = stage[q];
    sl[b][tid] = sstage;
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  using P2 = std::integral_constant<int, 2>;
  using P3 = std::integral_constant<int, 3>;
  load_w(P0{}, 0);
  load_w(P1{}, 1);
  load_w(P2{}, 2);
  load_group(0);
  store_group(0);
  load_group(kStage);
  __syncthreads();
  int cur = 0;  // LDS buffers of the group being consumed

  // the 8 MFMAs of one step: operand set P, panel P % kStage of the group
  auto mfmas = [&](auto P) {
    constexpr int p = decltype(P)::value;
    constexpr int q = p % kStage;
    const unsigned char* buf = xl[cur] + q * kPanelBytes + xfrag;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const intx8 xv = lds_read_a8_frag(buf + 16 * i * kRowBytes);
      // byte g of the row's dword (one v_bfe_u32)
      const u32 xsc = (sl[cur][32 * q + 16 * i + r] >> (8 * g)) & 0xffu;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j][i] = mfma_w4a8(wv[p][j], wsc[p][j], xv, xsc, acc[j][i]);
    }
  };
  // one step s of parity P = s & 3
  auto step = [&](auto P, int s) {
    constexpr int p = decltype(P)::value;
    load_w(std::integral_constant<int, (p + 3) & 3>{}, s + 3);
    FI_SCHED_FENCE();  // the loads are issued before the MFMAs ...
    mfmas(P);
    FI_SCHED_FENCE();  // ... and waited for only after them
    if constexpr ((p + 1) % kStage == 0) {
      // the group ends: the next one goes to the buffers last read one group
      // ago, before that group's barrier, and the one after it is requested
      store_group(cur ^ 1);
      load_group(s + 1 + kStage);
      __syncthreads();
      cur ^= 1;
    }
  };
  int s = 0;
  for (; s + 3 < nsteps; s += 4) {
    step(P0{}, s);
    step(P1{}, s + 1);
    step(P2{}, s + 2);
    step(P3{}, s + 3);
  }
  // peeled remainder: same steps, their extra loads clamped to the last one
  const int rem = nsteps - s;
  if (rem >= 1) step(P0{}, s);
  if (rem >= 2) step(P1{}, s + 1);
  if (rem == 3) step(P2{}, s + 2);

  if constexpr (!GATE_UP)
    store_bf16_tile(static_cast<u16*>(out_v), acc, slot0, wn, r, g, N);
  else
    store_swiglu_mxfp8_tile(static_cast<unsigned char*>(out_v), out_scale, acc,
                            slot0, wn, r, g, N);
}

}  // namespace

// K % 128 == 0, N % 16 == 0 (N % 32 == 0 with gate_up), max_mtiles tiles of
// block_m = 128 or 32 slots (checked by the binding). The grid is static and
// tiles at or past *n_valid leave at once.
void launch_moe_gemm_mxfp4_mxfp8(void* out, unsigned char* out_scale,
                                 const unsigned char* aq,
                                 const unsigned char* asc,
                                 const unsigned char* wq,
                                 const unsigned char* ws,
                                 const int* sorted_ids, const int* expert_ids,
                                 const int* n_valid, int max_mtiles, int K,
                                 int N, bool gate_up, int block_m,
                                 hipStream_t stream) {
  if (block_m == kBlockM32) {
    if (gate_up)
      moe_mxfp4_mxfp8_gemm32_kernel<true>
          <<<dim3(max_mtiles, ceil_div(N, 128)), 256, 0, stream>>>(
              out, out_scale, aq, asc, wq, ws, sorted_ids, expert_ids,
              n_valid, K, N);
    else
      moe_mxfp4_mxfp8_gemm32_kernel<false>
          <<<dim3(max_mtiles, ceil_div(N, 256)), 256, 0, stream>>>(
              out, out_scale, aq, asc, wq, ws, sorted_ids, expert_ids,
              n_valid, K, N);
    return;
  }
  if (gate_up)
    moe_mxfp4_mxfp8_gemm_kernel<true>
        <<<dim3(max_mtiles, ceil_div(N, 64)), 256, 0, stream>>>(
            out, out_scale, aq, asc, wq, ws, sorted_ids, expert_ids, n_valid, K,
            N);
  else
    moe_mxfp4_mxfp8_gemm_kernel<false>
        <<<dim3(max_mtiles, ceil_div(N, 128)), 256, 0, stream>>>(
            out, out_scale, aq, asc, wq, ws, sorted_ids, expert_ids, n_valid, K,
            N);
}

}  // namespace fi
