// Short-query paged attention for CDNA4 (gfx950): a FEW q rows per sequence
// (a speculative verify chunk of 1 + k tokens, at most 32) against
// a long paged KV cache ([num_blocks, Hk, 16, D], bf16 or OCP e4m3 at scale
// 1.0). Semantics of prefill_attention_paged: with n_s new rows, row j of
// sequence s attends positions 0 .. seq_lens_k[s] - n_s + j.
//
// Work split. Grid (sequence, kv head, partition x query group): the
// context is cut into 512-token partitions like the decode kernel (count
// from the block-table width), and the (row j, group head g) PAIRS
// r = j*G + g of one kv head are cut into query groups of 16*NT pairs
// (count from the host bound max_q). Every launch dimension is a function
// of shapes and max_q: no host sync. A workgroup is 4 waves; wave w takes
// the partition's chunk pairs w, w+4, w+8, w+12 (a chunk pair = two
// 16-token cache blocks = one 32-deep PV MFMA step). Each K/V element is
// read once for all 16*NT pairs; further query groups re-read from L2.
//
// QK^T, swapped: S^T = mfma_f32_16x16x32_bf16(A = K block, B = Q), one per
// 32-dim slice. A: lane holds K[token = lane&15][slice + (lane>>4)*8 .. +8];
// B: lane holds Q'[pair = lane&15][same dims], Q' = bf16(q * (scale*log2e))
// built once and kept in registers. C: lane holds scores of pair lane&15
// for tokens (lane>>4)*4 + 0..3, so a pair's 16 scores sit in 4 lanes x 4
// registers: max and sum are two xor shuffles (16, 32), and m, l, alpha are
// lane-local for the pair. e4m3 K is converted to bf16 in registers (exact)
// in front of the same MFMAs. Softmax is base 2 on v_exp_f32. Invalid
// scores (causal limit, missing pair, pad) are REPLACED by select, so a NaN
// in a pad slot cannot survive.
//
// PV, swapped too: O^T[d][pair] += mfma(A = V^T, B = P^T). B is the packed
// bf16 P straight from the score registers: the lane's 8 k-slots
// k = (lane>>4)*8 + e are tokens (lane>>4)*4 + (e&3) of block e>>2 — the
// token order inside the 32-deep step is free as long as V uses the same
// one. C: lane holds O^T[d = 16*nb + (lane>>4)*4 + 0..3][pair = lane&15]:
// the pair is again lane&15, so the alpha rescale needs no shuffle.
//
// V through LDS. A = V^T needs 8 token-contiguous values of one dim per
// lane, the cache has dims contiguous. Each wave owns a private V^T tile
// [D rows (dims)][32 tokens in k order] bf16, row stride 80 B (64 B of
// data + 16 B pad). In: a lane loads the dim pair {2i, 2i+1} of all 16
// tokens of a block (each load instruction reads whole contiguous cache
// rows), packs four tokens of one dim into 8 B and writes them to row
// dim at byte 16*(t>>2) + 8*block. V rows at or past seq_lens_k are
// zeroed here, so 0 * NaN cannot occur. Out: one ds_read_b128 per 16-dim
// block at row 16*nb + (lane&15), byte 16*(lane>>4).
// Banks (64 x 4 B): row r starts at bank 20*r mod 64. For the 16 lanes
// of one lane>>4 value, 20*r mod 64 over r = 0..15 is the 16 distinct
// multiples of 4 {0,20,40,60,16,36,56,12,32,52,8,28,48,4,24,44}; each lane
// covers 4 consecutive banks from there (plus the common 4*(lane>>4)), so
// the 16 lanes tile the 64 banks exactly once: conflict-free b128 reads.
// (The staging writes of even rows collide 8 lanes to a bank pair; there
// are 16 per chunk pair against 2*D/16 MFMAs and 16 KB of HBM traffic.)
// The tile is private to its wave: no barrier in the K loop.
//
// End: per pair tile, the 4 waves park (m, l, acc) in LDS (the V^T area is
// reused) and merge in wave order. One partition writes out; several
// write fp32 partials [T, Hq, P, 2 | D] and shortq_reduce_kernel merges
// them in ascending partition order. A pair whose partition is entirely
// masked publishes m = -1e30, l = 0 and is skipped. No atomics.
//
// A row's bits depend on its q row, its sequence's cache, table, length
// and n_s only: a pair is one MFMA column, the chunk-to-wave map depends
// on the position alone, and NT / the query group only choose the column.

#include "common.h"

#include <type_traits>

namespace fi {

namespace {

constexpr int kSqBlock = 16;       // cache block size (tokens)
constexpr int kSqPartChunks = 32;  // 512 tokens per partition
constexpr int kSqWaves = 4;
constexpr int kSqVtRowB = 80;      // V^T LDS row: 32 tokens bf16 + 16 B pad
constexpr float kSqNegInf = -1e30f;
constexpr float kSqLog2e = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(8))) short sq_short8;
typedef __attribute__((ext_vector_type(4))) float sq_floatx4;
typedef __attribute__((ext_vector_type(4))) unsigned int sq_u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int sq_u32x2;

FI_DEV u32 sq_pack_bf16x2(float lo, float hi) {
  return static_cast<u32>(f32_to_bf16(lo)) |
         (static_cast<u32>(f32_to_bf16(hi)) << 16);
}

// the 8 K elements a lane feeds one MFMA: 16 B of bf16 or 8 B of e4m3
template <bool FP8>
struct SqKRaw {
  using T = typename std::conditional<FP8, sq_u32x2, sq_u32x4>::type;
  static FI_DEV T zero() {
    if constexpr (FP8) return T{0u, 0u};
    else return T{0u, 0u, 0u, 0u};
  }
  static FI_DEV sq_short8 frag(T raw) {
    if constexpr (FP8) {
      float f[8];
      unpack_fp8x4(raw[0], f);
      unpack_fp8x4(raw[1], f + 4);
      const sq_u32x4 w = {sq_pack_bf16x2(f[0], f[1]), sq_pack_bf16x2(f[2], f[3]),
                          sq_pack_bf16x2(f[4], f[5]), sq_pack_bf16x2(f[6], f[7])};
      return __builtin_bit_cast(sq_short8, w);
    } else {
      return __builtin_bit_cast(sq_short8, raw);
    }
  }
};

// Two tokens (a, b) of one dim pair -> the two bf16x2 words {dim0 of a, b}
// and {dim1 of a, b}. bf16: a word is {dim0, dim1} of one token. e4m3: the
// low 16 bits are the two bytes of one token.
template <bool FP8>
FI_DEV void sq_pair_words(u32 a, u32 b, u32& d0, u32& d1) {
  if constexpr (FP8) {
    float f[4];
    unpack_fp8x4(a | (b << 16), f);
    d0 = sq_pack_bf16x2(f[0], f[2]);
    d1 = sq_pack_bf16x2(f[1], f[3]);
  } else {
    d0 = (a & 0xffffu) | (b << 16);
    d1 = (a >> 16) | (b & 0xffff0000u);
  }
}

}  // namespace

// 2 waves/SIMD: without the bound the two-tile D=128 variants take 264
// registers and drop to one workgroup per CU
template <int D, bool FP8, int NT>
__global__ __launch_bounds__(kSqWaves * kWaveSize, 2) void shortq_attn_kernel(
    u16* __restrict__ out,            // [T, Hq, D] (written when 1 partition)
    float* __restrict__ ml_ws,        // [T, Hq, P, 2] (multi-partition)
    float* __restrict__ acc_ws,       // [T, Hq, P, D]
    const u16* __restrict__ q,        // [T] rows, stride q_stride, Hq*D elems
    const void* __restrict__ k_cache_p,  // [B, Hk, 16, D]
    const void* __restrict__ v_cache_p,
    const int* __restrict__ block_tables,  // [S, max_blocks]
    const int* __restrict__ cu_seqlens_q,  // [S+1]
    const int* __restrict__ seq_lens_k,    // [S] total context
    const int64_t q_stride, const int max_blocks, const int num_kv_heads,
    const int group, const int num_parts, const int max_q,
    const int total_rows, const float scale) {
  using CT = typename std::conditional<FP8, unsigned char, u16>::type;
  using KRaw = SqKRaw<FP8>;
  constexpr int KK = D / 32;   // QK^T MFMAs per block (32-dim slices)
  constexpr int NB = D / 16;   // PV MFMAs per chunk pair (16-dim blocks)
  constexpr int LPB = D / 2;   // lanes that cover one V row in dim pairs
  constexpr int NVB = D / 64;  // V blocks a lane stages per chunk pair
  const CT* k_cache = static_cast<const CT*>(k_cache_p);
  const CT* v_cache = static_cast<const CT*>(v_cache_p);

  const int seq = blockIdx.x;
  const int kv_head = blockIdx.y;
  const int part = blockIdx.z % num_parts;
  const int qgroup = blockIdx.z / num_parts;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWaveSize);
  const int lane = tid % kWaveSize;
  const int col = lane & 15;  // pair within a tile / token within a block
  const int q4 = lane >> 4;

  const int q_start = cu_seqlens_q[seq];
  const int n_s = cu_seqlens_q[seq + 1] - q_start;
  // rows past max_q of a malformed sequence are ignored, never indexed
  const int num_pairs = min(n_s, max_q) * group;
  const int pair_base = qgroup * (16 * NT);
  if (pair_base >= num_pairs) return;  // also n_s == 0: nothing to do

  const int ctx = seq_lens_k[seq];
  const int num_chunks = min((ctx + kSqBlock - 1) / kSqBlock, max_blocks);
  const int chunk_lo = part * kSqPartChunks;
  const int chunk_hi = min(num_chunks, chunk_lo + kSqPartChunks);
  const int num_heads = num_kv_heads * group;

  // pair index -> (q row, head); row < 0 when the pair does not exist
  auto pair_row_head = [&](int p, int& row, int& head) {
    const int j = p / group;
    head = kv_head * group + (p - j * group);
    row = q_start + j;
    if (p >= num_pairs || row >= total_rows) row = -1;
    return j;
  };

  // empty partition: publish "nothing" and leave
  if (chunk_lo >= chunk_hi) {
    if (num_parts > 1 && tid < 16 * NT) {
      int row, head;
      pair_row_head(pair_base + tid, row, head);
      if (row >= 0) {
        float* ml = ml_ws + ((static_cast<int64_t>(row) * num_heads + head) *
                                 num_parts + part) * 2;
        ml[0] = kSqNegInf;
        ml[1] = 0.f;
      }
    }
    return;
  }

  // per-wave V^T tiles; reused by the cross-wave merge ([wave][16][D] fp32)
  __shared__ __attribute__((aligned(16))) char smem[kSqWaves * D * kSqVtRowB];
  __shared__ float mrg_m[kSqWaves][16];
  __shared__ float mrg_l[kSqWaves][16];
  static_assert(kSqWaves * 16 * D * 4 <= kSqWaves * D * kSqVtRowB);
  char* vt = smem + wave * (D * kSqVtRowB);

  // ---- Q fragments (B operand), prescaled, resident for the kernel ----
  sq_short8 qf[NT][KK];
  int limit[NT];  // last position this lane's pair attends; -1: no pair
  {
    const float qs = scale * kSqLog2e;
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      int row, head;
      const int j = pair_row_head(pair_base + ti * 16 + col, row, head);
      limit[ti] = row >= 0 ? ctx - n_s + j : -1;
      const u16* qrow = q + static_cast<int64_t>(max(row, 0)) * q_stride +
                        static_cast<int64_t>(head) * D;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        bf16x8 h = {};
        if (row >= 0) {
          h = *reinterpret_cast<const bf16x8*>(qrow + kk * 32 + q4 * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            h.h[e] = f32_to_bf16(bf16_to_f32(h.h[e]) * qs);
        }
        qf[ti][kk] = __builtin_bit_cast(sq_short8, h);
      }
    }
  }

  float m[NT], l[NT];
  sq_floatx4 acc[NT][NB];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    m[ti] = kSqNegInf;
    l[ti] = 0.f;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[ti][nb] = sq_floatx4{0.f, 0.f, 0.f, 0.f};
  }

  const int* bt_row = block_tables + static_cast<int64_t>(seq) * max_blocks;
  auto kv_base_of = [&](int chunk) -> int64_t {
    return ((static_cast<int64_t>(bt_row[chunk]) * num_kv_heads + kv_head) *
            kSqBlock) * D;
  };
  // K of a chunk pair; a block at or past chunk_hi is not read
  typename KRaw::T kraw[2][KK];
  int64_t base[2] = {0, 0};
  auto load_k = [&](int c0) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      if (c0 + b < chunk_hi) {
        base[b] = kv_base_of(c0 + b);
        const CT* k_row = k_cache + base[b] + col * D + q4 * 8;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
          kraw[b][kk] =
              *reinterpret_cast<const typename KRaw::T*>(k_row + kk * 32);
      } else {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) kraw[b][kk] = KRaw::zero();
      }
    }
  };
  const int c_first = chunk_lo + 2 * wave;
  if (c_first < chunk_hi) load_k(c_first);

  const int dp = lane % LPB;  // this lane's V dim pair {2dp, 2dp+1}
  for (int c0 = c_first; c0 < chunk_hi; c0 += 2 * kSqWaves) {
    // ---- this chunk pair's V rows, in flight under QK^T + softmax ----
    u32 vw[NVB][kSqBlock];
#pragma unroll
    for (int bi = 0; bi < NVB; ++bi) {
      const int b = D == 128 ? bi : (lane >> 5);
      if (c0 + b < chunk_hi) {
        const CT* v_rows = v_cache + (b ? base[1] : base[0]) + 2 * dp;
#pragma unroll
        for (int t = 0; t < kSqBlock; ++t)
          vw[bi][t] = FP8
              ? static_cast<u32>(
                    *reinterpret_cast<const u16*>(v_rows + t * D))
              : *reinterpret_cast<const u32*>(v_rows + t * D);
      } else {
#pragma unroll
        for (int t = 0; t < kSqBlock; ++t) vw[bi][t] = 0u;
      }
    }

    // ---- swapped QK^T: s[ti][b][r] = score(token 4*q4 + r, pair col) ----
    sq_floatx4 s[NT][2];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
      s[ti][0] = s[ti][1] = sq_floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int kk = 0; kk < KK; ++kk) {
        const sq_short8 kf = KRaw::frag(kraw[b][kk]);
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
          s[ti][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kf, qf[ti][kk], s[ti][b], 0, 0, 0);
      }
    // next chunk pair's K lands under softmax + PV
    if (c0 + 2 * kSqWaves < chunk_hi) load_k(c0 + 2 * kSqWaves);

    // ---- base-2 online softmax, masked by select; P packed to bf16 ----
    const int pos0 = c0 * kSqBlock + q4 * 4;
    // a missing second block holds no valid token
    const int pair_end = (c0 + 1 < chunk_hi ? c0 + 2 : c0 + 1) * kSqBlock - 1;
    sq_short8 pf[NT];
#pragma unroll
    for (int ti = 0; ti < NT; ++ti) {
      const int lim = min(limit[ti], pair_end);
      float sv[8];
      float cm = kSqNegInf;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int pos = pos0 + (e >> 2) * kSqBlock + (e & 3);
        sv[e] = pos <= lim ? s[ti][e >> 2][e & 3] : kSqNegInf;
        cm = fmaxf(cm, sv[e]);
      }
      cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
      cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
      const float m_new = fmaxf(m[ti], cm);
      const float alpha = __builtin_amdgcn_exp2f(m[ti] - m_new);
      m[ti] = m_new;
      float psum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int pos = pos0 + (e >> 2) * kSqBlock + (e & 3);
        sv[e] = pos <= lim ? __builtin_amdgcn_exp2f(sv[e] - m_new) : 0.f;
        psum += sv[e];
      }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      l[ti] = l[ti] * alpha + psum;
      const sq_u32x4 pw = {sq_pack_bf16x2(sv[0], sv[1]),
                           sq_pack_bf16x2(sv[2], sv[3]),
                           sq_pack_bf16x2(sv[4], sv[5]),
                           sq_pack_bf16x2(sv[6], sv[7])};
      pf[ti] = __builtin_bit_cast(sq_short8, pw);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[ti][nb] *= alpha;
    }

    // ---- V -> V^T tile (k order: token t of block b at 8*(t>>2)+4*b+(t&3))
#pragma unroll
    for (int bi = 0; bi < NVB; ++bi) {
      const int b = D == 128 ? bi : (lane >> 5);
      const int tok0 = (c0 + b) * kSqBlock;
      if (tok0 + kSqBlock > ctx) {  // last block: zero the pad rows
#pragma unroll
        for (int t = 0; t < kSqBlock; ++t)
          if (tok0 + t >= ctx) vw[bi][t] = 0u;
      }
      char* row0 = vt + (2 * dp) * kSqVtRowB + b * 8;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        sq_u32x2 d0, d1;
        u32 a0, a1, b0, b1;
        sq_pair_words<FP8>(vw[bi][4 * qd], vw[bi][4 * qd + 1], a0, a1);
        sq_pair_words<FP8>(vw[bi][4 * qd + 2], vw[bi][4 * qd + 3], b0, b1);
        d0[0] = a0; d0[1] = b0;
        d1[0] = a1; d1[1] = b1;
        *reinterpret_cast<sq_u32x2*>(row0 + qd * 16) = d0;
        *reinterpret_cast<sq_u32x2*>(row0 + kSqVtRowB + qd * 16) = d1;
      }
    }
    // the wave's own LDS traffic executes in order; the fence keeps the
    // compiler from moving the fragment reads above the staging writes
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- swapped PV: O^T[16 dims x 16 pairs] += V^T[16 x 32] P^T ----
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const sq_u32x4 vf = *reinterpret_cast<const sq_u32x4*>(
          vt + (nb * 16 + col) * kSqVtRowB + q4 * 16);
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
        acc[ti][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(sq_short8, vf), pf[ti], acc[ti][nb], 0, 0, 0);
    }
    // ... and the next staging writes below these reads
    asm volatile("" ::: "memory");
  }

  // ---- cross-wave flash merge, one pair tile at a time ----
  constexpr int DS = D / 16;  // dims per merge thread
  float* mrg = reinterpret_cast<float*>(smem);
  const int mp = tid >> 4;        // merge thread: pair in the tile
  const int md = (tid & 15) * DS; // ... and its first dim
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    __syncthreads();  // V^T reads (or the previous tile's merge) are done
    if (q4 == 0) {
      mrg_m[wave][col] = m[ti];
      mrg_l[wave][col] = l[ti];
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      *reinterpret_cast<sq_floatx4*>(
          mrg + (wave * 16 + col) * D + nb * 16 + q4 * 4) = acc[ti][nb];
    __syncthreads();

    int row, head;
    pair_row_head(pair_base + ti * 16 + mp, row, head);
    if (row < 0) continue;
    float gm = kSqNegInf;
#pragma unroll
    for (int w = 0; w < kSqWaves; ++w) gm = fmaxf(gm, mrg_m[w][mp]);
    float L = 0.f, o[DS];
#pragma unroll
    for (int i = 0; i < DS; ++i) o[i] = 0.f;
#pragma unroll
    for (int w = 0; w < kSqWaves; ++w) {
      const float f = __builtin_amdgcn_exp2f(mrg_m[w][mp] - gm);
      L += mrg_l[w][mp] * f;
      const float* a = mrg + (w * 16 + mp) * D + md;
#pragma unroll
      for (int i = 0; i < DS; ++i) o[i] = fmaf(a[i], f, o[i]);
    }
    const int64_t rh = static_cast<int64_t>(row) * num_heads + head;
    if (num_parts == 1) {
      const float inv = L > 0.f ? 1.f / L : 0.f;
      u32* orow = reinterpret_cast<u32*>(out + rh * D + md);
#pragma unroll
      for (int i = 0; i < DS; i += 2)
        orow[i / 2] = sq_pack_bf16x2(o[i] * inv, o[i + 1] * inv);
    } else {
      const int64_t slot = rh * num_parts + part;
      if ((tid & 15) == 0) {
        ml_ws[slot * 2] = gm;
        ml_ws[slot * 2 + 1] = L;
      }
      float* arow = acc_ws + slot * D + md;
#pragma unroll
      for (int i = 0; i < DS; ++i) arow[i] = o[i];
    }
  }
}

// merge partials in ascending partition order: grid (T, Hq), one wave;
// lane covers dims {2l, 2l+1}. A row no workgroup served (past max_q of a
// malformed sequence) merges whatever the workspace holds, in bounds.
template <int D>
__global__ __launch_bounds__(kWaveSize) void shortq_reduce_kernel(
    u16* __restrict__ out,             // [T, Hq, D]
    const float* __restrict__ ml_ws,   // [T, Hq, P, 2]
    const float* __restrict__ acc_ws,  // [T, Hq, P, D]
    const int num_parts) {
  const int lane = threadIdx.x;
  if (lane >= D / 2) return;
  const int64_t rh = static_cast<int64_t>(blockIdx.x) * gridDim.y + blockIdx.y;
  const int64_t base = rh * num_parts;
  float gm = kSqNegInf;
  for (int p = 0; p < num_parts; ++p) gm = fmaxf(gm, ml_ws[(base + p) * 2]);
  float L = 0.f, o0 = 0.f, o1 = 0.f;
  for (int p = 0; p < num_parts; ++p) {
    const float mp = ml_ws[(base + p) * 2];
    if (!(mp > kSqNegInf)) continue;  // empty or fully masked: weight 0
    const float f = __builtin_amdgcn_exp2f(mp - gm);
    L += ml_ws[(base + p) * 2 + 1] * f;
    const float2 a =
        reinterpret_cast<const float2*>(acc_ws + (base + p) * D)[lane];
    o0 = fmaf(a.x, f, o0);
    o1 = fmaf(a.y, f, o1);
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  reinterpret_cast<u32*>(out + rh * D)[lane] =
      sq_pack_bf16x2(o0 * inv, o1 * inv);
}

void launch_shortq_attn(u16* out, float* ml_ws, float* acc_ws, const u16* q,
                        const void* k_cache, const void* v_cache,
                        const int* block_tables, const int* cu_seqlens_q,
                        const int* seq_lens_k, int num_seqs, int total_rows,
                        int64_t q_stride, int max_blocks, int num_kv_heads,
                        int head_dim, int group, int num_parts, int max_q,
                        float scale, bool fp8, hipStream_t stream) {
  if (num_seqs == 0 || total_rows == 0) return;
  // one 16-pair tile when max_q * G fits it, else two per workgroup; the
  // query groups cover the rest
  const int pairs = max_q * group;
  const int nt = pairs <= 16 ? 1 : 2;
  const int qgroups = ceil_div(pairs, 16 * nt);
  const dim3 grid(num_seqs, num_kv_heads, num_parts * qgroups);
  const dim3 block(kSqWaves * kWaveSize);
  auto launch = [&](auto d, auto f8, auto t) {
    constexpr int D = decltype(d)::value, NT = decltype(t)::value;
    constexpr bool F8 = decltype(f8)::value;
    hipLaunchKernelGGL((shortq_attn_kernel<D, F8, NT>), grid, block, 0, stream,
                       out, ml_ws, acc_ws, q, k_cache, v_cache, block_tables,
                       cu_seqlens_q, seq_lens_k, q_stride, max_blocks,
                       num_kv_heads, group, num_parts, max_q, total_rows,
                       scale);
    if (num_parts > 1) {
      const dim3 rgrid(total_rows, num_kv_heads * group);
      hipLaunchKernelGGL((shortq_reduce_kernel<D>), rgrid, dim3(kWaveSize), 0,
                         stream, out, ml_ws, acc_ws, num_parts);
    }
  };
  auto launch_nt = [&](auto d, auto f8) {
    if (nt == 1) launch(d, f8, std::integral_constant<int, 1>{});
    else launch(d, f8, std::integral_constant<int, 2>{});
  };
  auto launch_fp8 = [&](auto d) {
    if (fp8) launch_nt(d, std::true_type{});
    else launch_nt(d, std::false_type{});
  };
  if (head_dim == 128) launch_fp8(std::integral_constant<int, 128>{});
  else if (head_dim == 64) launch_fp8(std::integral_constant<int, 64>{});
  // unreachable: check_attn_head_dim() in ops.hip, called by the binding
  else abort();
}

}  // namespace fi
