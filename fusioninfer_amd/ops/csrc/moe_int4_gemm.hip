// Grouped W4A16 GEMM for MoE experts stored as int4 group-quantised weights
// (the AWQ / GPTQ format), gfx950.
//
//   out[slot, n] = bf16( f( sum_k A[row(slot), k] * dq(W[e])[n, k] ) )
//   dq(W)[n, k]  = bf16_rne( fp32(q - z) * fp32(s) )
//
// joins the block-aligned grouped-GEMM contract of moe_mxfp4_gemm.hip
// (sorted_ids / expert_ids / the n_valid device scalar, static grid, fused
// SwiGLU epilogue) and the exact int4 group expansion and W4A16 lane mapping
// of int4_common.h. Expert weights use the row format int4_linear reads, per
// expert: w_packed [E, NB, K/2] (k even in the low nibble), w_scale
// [E, NB, K/G] fp16 and w_zero [E, NB, K/G] bytes, G = 32, 64 or 128; NB = 2N
// for gate_up (gate rows first, then up rows), NB = N for down.
// Dequantisation is exact, so the kernel is a bf16 grouped GEMM on dq(W). It
// never forms an index from weight, scale or zero data.
//
// Lane l (column c = l & 15, group g = l >> 4) of k-chunk s (128 k) loads
// the 16 B that hold k = 128 s + 32 g ... + 31 of W row n0 + c and the scale
// and zero of group (4 s + g) >> log2(G / 32) of that row. -z s and s / 16
// (group_scale) are formed once per (row, chunk); dword t expands to B
// fragment t of mfma_f32_16x16x32_bf16, and the A fragment is the matching
// contiguous 16 B of the activation row.
//
// One template, two instances per epilogue, chosen by block_m:
//  * MITER = 1 (block_m 16, decode): a wave owns one 16-column fragment
//    (gate and up rows of it when GATE_UP) over the whole K; four waves side
//    by side in N, no LDS, no barrier. Chunks are issued in pairs (a pair is
//    one 128 B line of every W row) and double-buffered in registers. The
//    scale and zero of a chunk travel in the same buffers as its packed
//    dwords and are issued with them, before the previous pair is consumed.
//  * MITER = 8 (block_m 128, prefill): a wave owns the same column fragment
//    for all eight row fragments, so every dequantised B fragment (18 VALU
//    per dword) is reused from registers eight times; the next chunk's
//    packed W, scale and zero are in flight meanwhile. With LDS_A the
//    workgroup stages each 128 x 128 bf16 chunk of the A panel into LDS once
//    (the sorted_ids gather included) instead of every wave reading it from
//    global memory: 16 B per thread per load, 16 consecutive threads on the
//    256 contiguous bytes of one row's chunk, eight loads per thread. Two
//    32 KB buffers, one barrier per chunk: chunk s + 1 is written after
//    chunk s is consumed, into the buffer whose last readers all passed the
//    previous barrier. LDS_A = false is the direct-read form of
//    moe_mxfp4_gemm_kernel<8, ...>, kept for the A/B in
//    profiles/r20_int4_moe.md.
//
// LDS banks. A panel row is 256 B = 16 units of 16 B, and unit u of row r is
// stored at unit u ^ (r & 15), no padding. A wave's ds_read_b128 for (row
// fragment mi, step t) has lane (r, g) read unit (4 g + t) ^ r of row
// 16 mi + r. Any 16 lanes of one g read 16 different units, i.e. 16 x 16 B
// covering all 64 four-byte banks once; so do the quarter-wave groupings
// that mix g ({r < 4} x all g: r moves the low two bits, g the high two).
// Under the 32-bank, 8-lane model the units are distinct mod 8 too. The
// stage's ds_write_b128 has 16 consecutive threads write the 16 units of one
// row. Neither side has a bank conflict.
//
// Determinism: every accumulator sums its row's K in ascending (chunk,
// fragment) order through the same MFMA in every instance, so the bits of
// a (token, expert) row depend on that row and its expert's weights only:
// not on block_m, the slot, the A path or the other tokens. No atomics, no
// workspace, no K split across waves.
//
// C-fragment map (16x16): row = (lane >> 4) * 4 + r, col = lane & 15.

#include <hip/hip_runtime.h>

#include "int4_common.h"
#include "mx_common.h"  // swiglu, FI_SCHED_FENCE

namespace fi {

namespace {

// NF W rows per lane (gate, up) of one k-chunk: packed run, scale, zero
template <int NF>
struct Int4Chunk {
  u32x4 w[NF];
  u16 s[NF];
  unsigned char z[NF];
};

template <int MITER, bool GATE_UP, bool LDS_A>
__global__ __launch_bounds__(256) void moe_int4_gemm_kernel(
    u16* __restrict__ out,                 // [PM, N] bf16
    const u16* __restrict__ a,             // GATE_UP: x [T, K]; else act [PM, K]
    const unsigned char* __restrict__ wq,  // [E, NB, K/2]
    const u16* __restrict__ ws,            // [E, NB, K/G] fp16 bits
    const unsigned char* __restrict__ wz,  // [E, NB, K/G]
    const int* __restrict__ sorted_ids,    // [PM] token row per padded slot
    const int* __restrict__ expert_ids,    // [PM/BM] local expert per m-tile
    const int* __restrict__ n_valid,       // device scalar: real m-tile count
    const int K, const int N,
    const int gshift) {                    // log2(G / 32)
  static_assert(!LDS_A || MITER == 8, "the LDS panel is 128 rows");
  constexpr int BM = 16 * MITER;
  constexpr int NF = GATE_UP ? 2 : 1;
  using WC = Int4Chunk<NF>;
  const int mtile = blockIdx.x;
  // uniform for the workgroup and ahead of every barrier
  if (mtile >= *n_valid) return;

  const int lane = threadIdx.x % kWaveSize;
  const int wave = threadIdx.x / kWaveSize;
  const int col = lane & 15;
  const int g = lane >> 4;
  const int ntiles = N / 16;
  // this wave's 16-column fragment. Without barriers a wave past N simply
  // leaves; with the LDS panel it stays for the stage and the barriers,
  // reads no W and stores nothing
  const bool wok = blockIdx.y * 4 + wave < ntiles;  // wave-uniform
  if constexpr (!LDS_A) {
    if (!wok) return;
  }
  const int nt = min(static_cast<int>(blockIdx.y) * 4 + wave, ntiles - 1);
  const int e = expert_ids[mtile];
  const int nchunks = K / 128;
  const int ngroups = (K / 32) >> gshift;  // per W row

  const unsigned char* wp[NF];
  const u16* sp[NF];
  const unsigned char* zp[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int64_t n = static_cast<int64_t>(e) * (NF * N) + f * N + nt * 16 + col;
    wp[f] = wq + n * (K / 2) + 16 * g;
    sp[f] = ws + n * ngroups;
    zp[f] = wz + n * ngroups;
  }

  floatx4 acc[MITER][NF];
#pragma unroll
  for (int mi = 0; mi < MITER; ++mi)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[mi][f] = floatx4{0.f, 0.f, 0.f, 0.f};

  auto load_w = [&](WC& d, int c) {
    const int grp = (4 * c + g) >> gshift;  // < ngroups for c < nchunks
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      d.w[f] = *reinterpret_cast<const u32x4*>(wp[f] + c * 64);
      d.s[f] = sp[f][grp];
      d.z[f] = zp[f][grp];
    }
  };

  if constexpr (MITER == 1) {
    // A row: gathered through sorted_ids for gate_up (padding slots carry a
    // valid dummy row), read by slot otherwise
    const int slot = mtile * BM + col;
    const int row = GATE_UP ? sorted_ids[slot] : slot;
    const u16* ap = a + static_cast<int64_t>(row) * K + 32 * g;
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
          wd[q].s[f] = 0;
          wd[q].z[f] = 0;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) xd[q][t] = short8{0, 0, 0, 0, 0, 0, 0, 0};
        if (c < nchunks) {  // wave-uniform
          load_w(wd[q], c);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            xd[q][t] = *reinterpret_cast<const short8*>(ap + c * 128 + 8 * t);
        }
      }
    };
    auto consume = [&](WC (&wv)[2], short8 (&xv)[2][4], int p) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (2 * p + q < nchunks) {  // an absent chunk adds nothing at all
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            const GroupScale gs = group_scale(wv[q].s[f], wv[q].z[f]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
              acc[0][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  xv[q][t], dequant_int4x8(wv[q].w[f][t], gs), acc[0][f], 0, 0,
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
    // this chunk's dequantised fragments serve all MITER row fragments;
    // read_a(mi, xv) fetches the four A fragments of row fragment mi
    auto consume = [&](const WC& wv, auto read_a) {
      short8 b[NF][4];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const GroupScale gs = group_scale(wv.s[f], wv.z[f]);
#pragma unroll
        for (int t = 0; t < 4; ++t) b[f][t] = dequant_int4x8(wv.w[f][t], gs);
      }
#pragma unroll
      for (int mi = 0; mi < MITER; ++mi) {
        short8 xv[4];
        read_a(mi, xv);
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[mi][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                xv[t], b[f][t], acc[mi][f], 0, 0, 0);
      }
    };
    WC wa, wb;
    if constexpr (LDS_A) {
      // [buffer][row][16 B unit], unit u of row r at u ^ (r & 15)
      __shared__ __attribute__((aligned(16))) u32x4 panel[2][BM][16];
      // stage: thread -> unit `sseg` of rows srow + 16 i; all eight rows
      // share r & 15 = srow, hence one swizzled unit
      const int srow = threadIdx.x >> 4;
      const int sseg = threadIdx.x & 15;
      const int sunit = sseg ^ srow;
      const u16* gp[MITER];
#pragma unroll
      for (int i = 0; i < MITER; ++i) {
        const int slot = mtile * BM + 16 * i + srow;
        const int row = GATE_UP ? sorted_ids[slot] : slot;
        gp[i] = a + static_cast<int64_t>(row) * K + 8 * sseg;
      }
      u32x4 st[MITER];
      auto stage_load = [&](int c) {
#pragma unroll
        for (int i = 0; i < MITER; ++i)
          st[i] = *reinterpret_cast<const u32x4*>(gp[i] + c * 128);
      };
      auto stage_store = [&](int buf) {
#pragma unroll
        for (int i = 0; i < MITER; ++i) panel[buf][16 * i + srow][sunit] = st[i];
      };
      auto reader = [&](int buf) {
        return [&, buf](int mi, short8 (&xv)[4]) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            xv[t] = *reinterpret_cast<const short8*>(
                &panel[buf][16 * mi + col][(4 * g + t) ^ col]);
        };
      };
      stage_load(0);
      if (wok) load_w(wa, 0);
      stage_store(0);
      __syncthreads();
      for (int c = 0; c < nchunks; c += 2) {
        const bool n1 = c + 1 < nchunks;  // uniform: K only
        if (n1) {
          stage_load(c + 1);
          if (wok) load_w(wb, c + 1);
        }
        FI_SCHED_FENCE();
        if (wok) consume(wa, reader(0));
        FI_SCHED_FENCE();
        if (n1) stage_store(1);
        __syncthreads();
        if (n1) {
          const bool n2 = c + 2 < nchunks;
          if (n2) {
            stage_load(c + 2);
            if (wok) load_w(wa, c + 2);
          }
          FI_SCHED_FENCE();
          if (wok) consume(wb, reader(1));
          FI_SCHED_FENCE();
          if (n2) stage_store(0);
          __syncthreads();
        }
      }
    } else {
      const u16* ap[MITER];
#pragma unroll
      for (int mi = 0; mi < MITER; ++mi) {
        const int slot = mtile * BM + mi * 16 + col;
        const int row = GATE_UP ? sorted_ids[slot] : slot;
        ap[mi] = a + static_cast<int64_t>(row) * K + 32 * g;
      }
      auto reader = [&](int c) {
        return [&, c](int mi, short8 (&xv)[4]) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            xv[t] = *reinterpret_cast<const short8*>(ap[mi] + c * 128 + 8 * t);
        };
      };
      load_w(wa, 0);
      for (int c = 0; c < nchunks; c += 2) {
        if (c + 1 < nchunks) load_w(wb, c + 1);
        consume(wa, reader(c));
        if (c + 1 < nchunks) {
          if (c + 2 < nchunks) load_w(wa, c + 2);
          consume(wb, reader(c + 1));
        }
      }
    }
  }

  if (!wok) return;  // every barrier is behind us
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

// K % 128 == 0, N % 16 == 0, block_m in {16, 128}, gshift in {0, 1, 2}
// (checked by the binding). Four waves per workgroup, one 16-column fragment
// each; the grid is static (max_mtiles m-tiles) and tiles at or past
// *n_valid leave at once. lds_a picks the A path of the block_m 128 instance
// and has no effect at block_m 16.
void launch_moe_gemm_int4(u16* out, const u16* a, const unsigned char* wq,
                          const u16* ws, const unsigned char* wz,
                          const int* sorted_ids, const int* expert_ids,
                          const int* n_valid, int max_mtiles, int K, int N,
                          int gshift, int block_m, bool gate_up, bool lds_a,
                          hipStream_t stream) {
  decltype(&moe_int4_gemm_kernel<1, true, false>) kernel;
  if (block_m == 16)
    kernel = gate_up ? moe_int4_gemm_kernel<1, true, false>
                     : moe_int4_gemm_kernel<1, false, false>;
  else if (lds_a)
    kernel = gate_up ? moe_int4_gemm_kernel<8, true, true>
                     : moe_int4_gemm_kernel<8, false, true>;
  else
    kernel = gate_up ? moe_int4_gemm_kernel<8, true, false>
                     : moe_int4_gemm_kernel<8, false, false>;
  hipLaunchKernelGGL(kernel, dim3(max_mtiles, ceil_div(N / 16, 4)), dim3(256),
                     0, stream, out, a, wq, ws, wz, sorted_ids, expert_ids,
                     n_valid, K, N, gshift);
}

}  // namespace fi
