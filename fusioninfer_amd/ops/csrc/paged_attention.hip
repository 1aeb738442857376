// Paged-attention DECODE kernels for CDNA4 (gfx950) — flash-decoding.
//
// One-token attention per sequence against the paged KV cache
// ([num_blocks, Hk, 16, D], bf16 or OCP e4m3 at scale 1.0). Memory-bound:
// stream each sequence's K/V once at near-HBM rate, reusing every K/V read
// across the GQA group (G q-heads per kv-head).
//
// Grid: (num_seqs, num_kv_heads, num_partitions) — the context is split
// into 512-token partitions so small decode batches still fill 256 CUs;
// partial (m, l, acc) go to an fp32 workspace and a second kernel merges
// partitions. num_partitions == 1 writes output directly.
//
// ONE skeleton, paged_attn_decode_kernel: kNWaves waves in HS head-groups
// of G/HS heads; a head-group's waves stream interleaved 16-token chunks
// (1 chunk == 1 cache block, so its K/V are contiguous). Per chunk: scores
// (phase A), base-2 online softmax (m, l per head, wave-uniform), probs
// parked in per-wave LDS, PV (phase B: lane = dim pair, V rows coalesced,
// fp32 acc). Next K prefetched and this V preloaded under the softmax; a
// cross-wave flash-merge through LDS ends the workgroup.
// THREE score policies supply phase A and own what differs: ScalarScores
// (bf16 or fp8 K, per-lane FMAs against fp32 q in LDS), MfmaScoresBf16 and
// MfmaScoresFp8 (QK^T on the matrix cores). decode_plan() alone decides
// which policy, wave count and head split run; only those are instantiated.
//
// Known gap (the engine never sends it: padding rows use length 1):
// seq_lens[s] == 0 with a one-partition table takes the empty-partition
// branch, which writes to the workspace — null when there is one partition.
//
// Known gap (pad slots must hold finite V): phase B multiplies all 16 V
// rows of a sequence's last block by p and relies on p == 0 for the pad
// rows, so a NaN or Inf in a V pad slot reaches the output as 0 * NaN.
// The engine zero-initialises the cache and the fp8 writers saturate; such
// a value can only be a non-finite bf16 activation left by a previous
// owner of the block. Finite pad contents of any size are harmless
// (tests/test_attention_adversarial_gpu.py fills them with poison). A
// select on vball in the hot loop would close the gap; its cost has not
// been measured.
//
// Capability parity: the paged-attention decode the reference delegates to
// its vLLM containers (SURVEY.md §2.3 "Paged-attention decode kernel").

#include "common.h"

#include <type_traits>

namespace fi {

constexpr int kBlockSz = 16;     // cache block size (tokens)
constexpr int kPartChunks = 32;  // 512 tokens per partition
constexpr float kNegInf = -1e30f;
// q is pre-scaled by scale*log2e: scores land in base-2 units so the
// softmax uses bare v_exp_f32 (exp2) with no argument multiply
constexpr float kLog2e = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float floatx4;

// ---- score policies -------------------------------------------------------
// Scores<D, G, HS> serves one wave carrying G2 = G/HS heads (head-group
// `hsplit`) of the kv-head whose G query rows start at q_row. All static:
//   CT, KTile, load_k()  cache element type, one chunk's K registers
//   Q, init()     the Q state and its builder. init() may declare
//                 __shared__ storage and __syncthreads(): every thread of
//                 the block calls it, after the early return
//   dot()         phase A: s[G2] for the chunk
//   kTokLo/kTokHi lanes differing in xor bits [kTokLo, kTokHi) hold the 16
//                 tokens; a token's kTokLo lanes hold partial dot products

// Scalar FMA path. lane = token*4 + quad; the lane reads the quad-th
// quarter of K[token] (64 B bf16 / 32 B fp8). xor-1,2 shuffles finish the
// dot, xor 4..32 spans the 16 token groups.
template <typename CT_, int D, int G, int HS>
struct ScalarScores {
  using CT = CT_;
  static constexpr int G2 = G / HS, kTokLo = 4, kTokHi = 64;
  static constexpr int DPQ = D / 4;                  // dims per lane
  static constexpr int KQ4 = DPQ * sizeof(CT) / 16;  // 16-B K loads per lane
  static constexpr int EPG = 16 / sizeof(CT);        // elems per 16-B group
  struct KTile { uint4 v[KQ4]; };
  struct Q { const float (*heads)[D]; };  // this wave's G2 rows of q_lds

  static FI_DEV void init(Q& qs, const u16* q_row, float scale, int tid,
                          int nthreads, int, int hsplit) {
    // stage q (G heads) into LDS as fp32 (pre-scaled)
    __shared__ float q_lds[G][D];
    for (int e = tid; e < G * D; e += nthreads)
      q_lds[e / D][e % D] = bf16_to_f32(q_row[e]) * scale * kLog2e;
    __syncthreads();
    qs.heads = &q_lds[hsplit * G2];
  }

  static FI_DEV void load_k(const CT* k_block, int lane, KTile& k) {
    const CT* k_row = k_block + (lane / 4) * D + (lane % 4) * DPQ;
#pragma unroll
    for (int j8 = 0; j8 < KQ4; ++j8)
      k.v[j8] = reinterpret_cast<const uint4*>(k_row)[j8];
  }

  // streaming convert+FMA: per 16-B K group, convert its elements and
  // fold them into all G2 head accumulators immediately — kf[8] live
  // instead of kf[32] (round-2 register diet: the G=4/D=128 variant
  // was 218 VGPR -> 2 waves/SIMD; PMC showed WAIT-dominant)
  static FI_DEV void dot(const Q& qs, const KTile& k, int lane,
                         float (&s)[G2]) {
    const int quad = lane % 4;
#pragma unroll
    for (int g = 0; g < G2; ++g) s[g] = 0.f;
#pragma unroll
    for (int j8 = 0; j8 < KQ4; ++j8) {
      float kf8[EPG];
      if constexpr (sizeof(CT) == 1) {
        const u32 w[4] = {k.v[j8].x, k.v[j8].y, k.v[j8].z, k.v[j8].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) unpack_fp8x4(w[i], &kf8[i * 4]);
      } else {
        const bf16x8 kv8 = __builtin_bit_cast(bf16x8, k.v[j8]);
#pragma unroll
        for (int j = 0; j < 8; ++j) kf8[j] = bf16_to_f32(kv8.h[j]);
      }
#pragma unroll
      for (int g = 0; g < G2; ++g) {
#pragma unroll
        for (int j4 = 0; j4 < EPG / 4; ++j4) {
          // float4 -> ds_read_b128 (4x fewer LDS cycles than scalar)
          const float4 qv = *reinterpret_cast<const float4*>(
              &qs.heads[g][quad * DPQ + j8 * EPG + j4 * 4]);
          s[g] = fmaf(kf8[j4 * 4 + 0], qv.x, s[g]);
          s[g] = fmaf(kf8[j4 * 4 + 1], qv.y, s[g]);
          s[g] = fmaf(kf8[j4 * 4 + 2], qv.z, s[g]);
          s[g] = fmaf(kf8[j4 * 4 + 3], qv.w, s[g]);
        }
      }
    }
  }
};
template <int D, int G, int HS>
using ScalarScoresBf16 = ScalarScores<u16, D, G, HS>;
template <int D, int G, int HS>
using ScalarScoresFp8 = ScalarScores<unsigned char, D, G, HS>;

// The two MFMA policies run QK^T on the MATRIX CORES instead of per-lane
// FMAs + 6-7-deep shfl_xor reduction chains (PMC showed the scalar phase A
// WAIT-dominant on those serial permlanes). One mfma_f32_16x16x32 per
// 32-dim slice: A = Q fragment with the G2 head rows REPLICATED over all 16
// rows (row i carries head i % G2), B = K fragment (lane reads
// K[tok = l&15][(l>>4)*8 .. +8]: same bytes as the scalar path, different
// pattern, block stays L2-resident). The K-dim reduction happens INSIDE the
// MFMA, c[row = g][col = lane&15], so every 16-lane col group holds a full
// copy of the scores: the softmax reductions are 4-deep within a group and
// wave-uniform by construction — alpha needs no broadcast, and each token
// is counted once.
// Frag = the 8 K elements a lane feeds one MFMA: 16 B of bf16, 8 B of e4m3.
template <typename CT_, typename Frag, int D>
struct MfmaScoresBase {
  using CT = CT_;
  static constexpr int kTokLo = 1, kTokHi = 16;
  struct KTile { Frag v[D / 32]; };
  static FI_DEV void load_k(const CT* k_block, int lane, KTile& k) {
    const CT* k_row = k_block + (lane & 15) * D;
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk)
      k.v[kk] = *reinterpret_cast<const Frag*>(
          k_row + kk * 32 + (lane >> 4) * 8);
  }
};

template <int D, int G, int HS>
struct MfmaScoresBf16 : MfmaScoresBase<u16, uint4, D> {
  using KTile = typename MfmaScoresBase<u16, uint4, D>::KTile;
  static constexpr int G2 = G / HS;
  // per-wave Q fragments, built once (Q is fixed for the whole kernel),
  // pre-scaled by scale*log2e and re-rounded to bf16 (same trick as the
  // prefill kernel's pre-scaled Q)
  struct Q { short8 a[D / 32]; };

  static FI_DEV void init(Q& qs, const u16* q_row, float scale, int, int,
                          int lane, int hsplit) {
    const int head = hsplit * G2 + ((lane & 15) % G2);
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
      const int d0 = kk * 32 + (lane >> 4) * 8;
      u16 tmp[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        tmp[e] = f32_to_bf16(bf16_to_f32(q_row[head * D + d0 + e]) *
                             scale * kLog2e);
      qs.a[kk] = *reinterpret_cast<short8*>(tmp);
    }
  }

  static FI_DEV void dot(const Q& qs, const KTile& k, int, float (&s)[G2]) {
    floatx4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk)
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          qs.a[kk], __builtin_bit_cast(short8, k.v[kk]), c, 0, 0, 0);
#pragma unroll
    for (int g = 0; g < G2; ++g) s[g] = c[g];
  }
};

template <int D, int G, int HS>
struct MfmaScoresFp8 : MfmaScoresBase<unsigned char, long long, D> {
  using KTile = typename MfmaScoresBase<unsigned char, long long, D>::KTile;
  static constexpr int G2 = G / HS;
  // Q quantized to e4m3 per HEAD; the dequant scale folds into the
  // post-MFMA per-head scalar together with scale*log2e (the model
  // already folded the cache's k_scale into `scale`)
  struct Q {
    long long a[D / 32];
    float sc[G2];
  };

  static FI_DEV void init(Q& qs, const u16* q_row, float scale, int tid, int,
                          int lane, int hsplit) {
    __shared__ float qsc_lds[G];
    if (tid < G) {
      float mx = 1e-8f;
      for (int d = 0; d < D; ++d)
        mx = fmaxf(mx, fabsf(bf16_to_f32(q_row[tid * D + d])));
      qsc_lds[tid] = mx / 448.f;
    }
    __syncthreads();
    const int head = hsplit * G2 + ((lane & 15) % G2);
    const float inv_qs = 1.f / qsc_lds[head];
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk) {
      const int d0 = kk * 32 + (lane >> 4) * 8;
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        f[e] = bf16_to_f32(q_row[head * D + d0 + e]) * inv_qs;
      u32 w[2];
      pack_fp8x8(f, w);
      qs.a[kk] = static_cast<long long>(
          (static_cast<unsigned long long>(w[1]) << 32) | w[0]);
    }
#pragma unroll
    for (int g = 0; g < G2; ++g)
      qs.sc[g] = qsc_lds[hsplit * G2 + g] * scale * kLog2e;
  }

  static FI_DEV void dot(const Q& qs, const KTile& k, int, float (&s)[G2]) {
    floatx4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < D / 32; ++kk)
      c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(qs.a[kk], k.v[kk], c, 0,
                                                     0, 0);
#pragma unroll
    for (int g = 0; g < G2; ++g) s[g] = c[g] * qs.sc[g];
  }
};

// one output row's dim pair {2*lane, 2*lane+1} as packed bf16x2
FI_DEV void store_out_pair(u16* o_row, int lane, float o0, float o1) {
  const u32 obits = static_cast<u32>(f32_to_bf16(o0)) |
                    (static_cast<u32>(f32_to_bf16(o1)) << 16);
  *reinterpret_cast<u32*>(o_row + 2 * lane) = obits;
}

// ---- the skeleton ---------------------------------------------------------
// HS (head split): waves are partitioned into HS head-groups of G/HS
// heads each; a wave streams chunks at stride kNWaves/HS for ITS head
// slice only. G=8 runs HS=2 so the per-wave state is the G=4 footprint —
// the monolithic G=8 variant spilled ~500 B/lane (8 waves) or sat at
// occupancy 1 (4 waves).
template <template <int, int, int> class ScoresT, int D, int G, int kNWaves,
          int HS>
__global__ __launch_bounds__(kNWaves * kWaveSize) void paged_attn_decode_kernel(
    u16* __restrict__ out,            // [S, Hq, D] (written when 1 partition)
    float* __restrict__ ml_ws,        // [S, Hq, P, 2] (multi-partition)
    float* __restrict__ acc_ws,       // [S, Hq, P, D]
    const u16* __restrict__ q,        // [S] rows, stride q_stride, Hq*D elems
    const void* __restrict__ k_cache_p,  // [B, Hk, 16, D] of Scores::CT
    const void* __restrict__ v_cache_p,
    const int* __restrict__ block_tables,  // [S, max_blocks]
    const int* __restrict__ seq_lens,      // [S]
    const int64_t q_stride, const int max_blocks, const int num_kv_heads,
    const float scale) {
  static_assert(HS <= G && G % HS == 0 && kNWaves % HS == 0);
  using Scores = ScoresT<D, G, HS>;
  using CT = typename Scores::CT;
  constexpr bool kFp8 = sizeof(CT) == 1;
  const CT* k_cache = static_cast<const CT*>(k_cache_p);
  const CT* v_cache = static_cast<const CT*>(v_cache_p);
  const int seq = blockIdx.x;
  const int kv_head = blockIdx.y;
  const int part = blockIdx.z;
  const int num_parts = gridDim.z;
  const int tid = threadIdx.x;
  const int wave = tid / kWaveSize;
  const int lane = tid % kWaveSize;
  // head-split decomposition: wave = cwave * HS + hsplit
  constexpr int G2 = G / HS;             // heads this wave carries
  constexpr int kCWaves = kNWaves / HS;  // waves streaming chunks together
  const int hsplit = wave % HS;
  const int cwave = wave / HS;

  const int ctx = seq_lens[seq];
  const int num_chunks = (ctx + kBlockSz - 1) / kBlockSz;
  const int chunk_lo = part * kPartChunks;
  const int chunk_hi = min(num_chunks, chunk_lo + kPartChunks);
  const int num_heads = num_kv_heads * G;

  // empty partition: publish "nothing" and leave
  if (chunk_lo >= num_chunks) {
    if (tid < G) {
      const int h = kv_head * G + tid;
      float* ml = ml_ws + ((static_cast<int64_t>(seq) * num_heads + h) *
                               num_parts + part) * 2;
      ml[0] = kNegInf;
      ml[1] = 0.f;
    }
    return;
  }

  __shared__ float p_lds[kNWaves][kBlockSz][G2];
  __shared__ float merge_m[kNWaves][G2];
  __shared__ float merge_l[kNWaves][G2];
  __shared__ float merge_acc[kNWaves][G2][D];

  typename Scores::Q qs;
  Scores::init(qs, q + seq * q_stride + static_cast<int64_t>(kv_head) * G * D,
               scale, tid, kNWaves * kWaveSize, lane, hsplit);

  // online-softmax state, wave-uniform (every lane holds the same copy)
  float m[G2], l[G2], acc[G2][2];
#pragma unroll
  for (int g = 0; g < G2; ++g) {
    m[g] = kNegInf;
    l[g] = 0.f;
    acc[g][0] = acc[g][1] = 0.f;
  }

  // software-prefetch: this wave's NEXT chunk's K flies while the current
  // chunk's softmax + PV run (the phases were serialized on K latency)
  auto kv_base_of = [&](int chunk) -> int64_t {
    const int block_id = block_tables[seq * max_blocks + chunk];
    return ((static_cast<int64_t>(block_id) * num_kv_heads + kv_head) *
            kBlockSz) * D;
  };
  typename Scores::KTile kraw;
  int64_t kv_base = 0;
  if (chunk_lo + cwave < chunk_hi) {
    kv_base = kv_base_of(chunk_lo + cwave);
    Scores::load_k(k_cache + kv_base, lane, kraw);
  }

  // the lane holds the score of chunk token `tok`; one lane per token
  // parks its p in LDS for phase B
  constexpr int kTokLo = Scores::kTokLo, kTokHi = Scores::kTokHi;
  const int tok = (lane % kTokHi) / kTokLo;
  const bool parks_p = lane % kTokLo == 0 && lane < kTokHi;
  for (int chunk = chunk_lo + cwave; chunk < chunk_hi; chunk += kCWaves) {
    const int token_pos = chunk * kBlockSz + tok;
    const int64_t kv_base_cur = kv_base;

    // ---- phase A: scores for 16 tokens x G2 heads ----
    float s[G2];
    Scores::dot(qs, kraw, lane, s);
    // preload THIS chunk's V before the softmax so its latency hides
    // under the reductions (it was serialized behind phase A before)
    u32 vball[kBlockSz];
    const CT* v_rows = v_cache + kv_base_cur;
    if (lane < D / 2) {
#pragma unroll
      for (int t = 0; t < kBlockSz; ++t)
        vball[t] = kFp8
            ? static_cast<u32>(*reinterpret_cast<const u16*>(
                  v_rows + t * D + 2 * lane))
            : *reinterpret_cast<const u32*>(v_rows + t * D + 2 * lane);
    }
    // issue next chunk's K now; it lands under softmax + PV
    if (chunk + kCWaves < chunk_hi) {
      kv_base = kv_base_of(chunk + kCWaves);
      Scores::load_k(k_cache + kv_base, lane, kraw);
    }
    // fence: stop the scheduler from hoisting phase-B work (and its live
    // ranges) above the softmax — cross-phase overlap doubled VGPRs
    // (G2 is always <= 4: G=8 is head-split)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      // sum the token's kTokLo partial dot products (kTokLo is 1 or 4)
      if constexpr (kTokLo > 1) s[g] += __shfl_xor(s[g], 1, 64);
      if constexpr (kTokLo > 2) s[g] += __shfl_xor(s[g], 2, 64);
      if (token_pos >= ctx) s[g] = kNegInf;
    }

    // chunk max over tokens
    float alpha[G2];
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      float cm = s[g];
#pragma unroll
      for (int off = kTokLo; off < kTokHi; off <<= 1)
        cm = fmaxf(cm, __shfl_xor(cm, off, 64));
      const float m_new = fmaxf(m[g], cm);
      alpha[g] = __builtin_amdgcn_exp2f(m[g] - m_new);
      if (m[g] <= kNegInf && m_new <= kNegInf) alpha[g] = 0.f;
      m[g] = m_new;
    }

    // probs + row-sum
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      float p = (s[g] <= kNegInf) ? 0.f
                : __builtin_amdgcn_exp2f(s[g] - m[g]);
      if (parks_p) p_lds[wave][tok][g] = p;
      // a token's p is replicated on kTokLo lanes -> scale by 1/kTokLo
      float psum = p;
#pragma unroll
      for (int off = 1; off < kTokHi; off <<= 1)
        psum += __shfl_xor(psum, off, 64);
      l[g] = l[g] * alpha[g] + psum * (1.f / kTokLo);
    }

    __builtin_amdgcn_sched_barrier(0);
    // ---- phase B: PV accumulate; lane covers dims {2l, 2l+1} ----
    // (vball preloaded before the softmax; p is 0 for padding tokens —
    // phase A masks every invalid position — so the full block is safe)
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      acc[g][0] *= alpha[g];
      acc[g][1] *= alpha[g];
    }
    if (lane < D / 2) {
      for (int t = 0; t < kBlockSz; ++t) {
        float v0, v1;
        if (kFp8) {
          float vf[4];
          unpack_fp8x4(vball[t], vf);
          v0 = vf[0];
          v1 = vf[1];
        } else {
          v0 = bf16_to_f32(static_cast<u16>(vball[t] & 0xffff));
          v1 = bf16_to_f32(static_cast<u16>(vball[t] >> 16));
        }
#pragma unroll
        for (int g = 0; g < G2; ++g) {
          const float p = p_lds[wave][t][g];
          acc[g][0] = fmaf(p, v0, acc[g][0]);
          acc[g][1] = fmaf(p, v1, acc[g][1]);
        }
      }
    }
  }

  // ---- cross-wave flash merge (within each head-group) ----
  if (lane < G2) {
    merge_m[wave][lane] = m[lane];
    merge_l[wave][lane] = l[lane];
  }
  if (lane < D / 2) {
#pragma unroll
    for (int g = 0; g < G2; ++g) {
      merge_acc[wave][g][2 * lane] = acc[g][0];
      merge_acc[wave][g][2 * lane + 1] = acc[g][1];
    }
  }
  __syncthreads();

  // head-group hsplit's G2 heads are distributed over its kCWaves waves
#pragma unroll
  for (int g = 0; g < G2; ++g) {
    if ((g % kCWaves) != cwave || lane >= D / 2) continue;
    float gm = kNegInf;
#pragma unroll
    for (int c = 0; c < kCWaves; ++c)
      gm = fmaxf(gm, merge_m[c * HS + hsplit][g]);
    float L = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
    for (int c = 0; c < kCWaves; ++c) {
      const int w = c * HS + hsplit;
      const float mw = merge_m[w][g];
      const float f = (mw <= kNegInf) ? 0.f
                      : __builtin_amdgcn_exp2f(mw - gm);
      L += merge_l[w][g] * f;
      o0 = fmaf(merge_acc[w][g][2 * lane], f, o0);
      o1 = fmaf(merge_acc[w][g][2 * lane + 1], f, o1);
    }
    const int h = kv_head * G + hsplit * G2 + g;
    if (num_parts == 1) {
      const float inv = 1.f / L;
      store_out_pair(out + (static_cast<int64_t>(seq) * num_heads + h) * D,
                     lane, o0 * inv, o1 * inv);
    } else {
      const int64_t slot = (static_cast<int64_t>(seq) * num_heads + h) *
                               gridDim.z + part;
      if (lane == 0) {
        ml_ws[slot * 2] = gm;
        ml_ws[slot * 2 + 1] = L;
      }
      float2* arow = reinterpret_cast<float2*>(acc_ws + slot * D);
      arow[lane] = make_float2(o0, o1);
    }
  }
}

// merge partials: grid (S, Hq), one wave; lane covers dims {2l, 2l+1}
template <int D>
__global__ __launch_bounds__(kWaveSize) void paged_attn_reduce_kernel(
    u16* __restrict__ out,            // [S, Hq, D]
    const float* __restrict__ ml_ws,  // [S, Hq, P, 2]
    const float* __restrict__ acc_ws, // [S, Hq, P, D]
    const int num_parts) {
  const int seq = blockIdx.x;
  const int h = blockIdx.y;
  const int num_heads = gridDim.y;
  const int lane = threadIdx.x;
  if (lane >= D / 2) return;
  const int64_t base = (static_cast<int64_t>(seq) * num_heads + h) * num_parts;

  float gm = kNegInf;
  for (int p = 0; p < num_parts; ++p)
    gm = fmaxf(gm, ml_ws[(base + p) * 2]);
  float L = 0.f, o0 = 0.f, o1 = 0.f;
  for (int p = 0; p < num_parts; ++p) {
    const float mp = ml_ws[(base + p) * 2];
    if (mp <= kNegInf) continue;
    const float f = __builtin_amdgcn_exp2f(mp - gm);
    L += ml_ws[(base + p) * 2 + 1] * f;
    const float2 a =
        reinterpret_cast<const float2*>(acc_ws + (base + p) * D)[lane];
    o0 = fmaf(a.x, f, o0);
    o1 = fmaf(a.y, f, o1);
  }
  const float inv = 1.f / L;
  store_out_pair(out + (static_cast<int64_t>(seq) * num_heads + h) * D, lane,
                 o0 * inv, o1 * inv);
}

// ---- dispatch -------------------------------------------------------------
namespace {

struct DecodePlan {
  int nwaves, head_split;
  bool mfma_scores;
};

// The whole dispatch policy: (group, wide, fp8, mfma_enabled) -> variant.
// A/B'd on hardware (2026-09-14 kbench):
// - 8 waves when the grid underfills the chip ("wide": small decode
//   batches, measured +46% at batch<=8), 4 when it is full (~5% faster).
// - G=8 always runs HS=2 (monolithic spilled; HS=4 measured a wash at
//   full grids and -12% wide).
// - G=4 runs HS=2 only at FULL grids (4-wave blocks): the G2=2 state
//   compiles to 149 VGPR = 3 waves/SIMD, measured +2.5% bf16 / +8% fp8
//   at b256; at WIDE grids the halved chunk parallelism lost 12-19%, so
//   wide keeps the monolithic G=4 shape.
// - bf16 takes the MFMA scores at every G. The fp8 MFMA scores are
//   G=8-only: kbench showed +41-43% there (G2=4 after head-split) but
//   -21% at G=4 fp8, where the scalar HS=2 path with halved KV bytes was
//   already latency-optimal.
constexpr DecodePlan decode_plan(int group, bool wide, bool fp8, bool mfma) {
  return {wide ? 8 : 4, (group == 8 || (group == 4 && !wide)) ? 2 : 1,
          mfma && (!fp8 || group == 8)};
}

// launches the one kernel decode_plan() names; inputs with the same plan
// (fp8 below G=8, MFMA on or off) share its instantiation
template <int D, int G, bool kWide, bool kFp8, bool kMfma, class... Args>
void launch_variant(dim3 grid, hipStream_t stream, Args... args) {
  constexpr DecodePlan p = decode_plan(G, kWide, kFp8, kMfma);
  constexpr int NW = p.nwaves, HS = p.head_split;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(NW * kWaveSize), 0, stream, args...);
  };
  if constexpr (p.mfma_scores && kFp8)
    launch(paged_attn_decode_kernel<MfmaScoresFp8, D, G, NW, HS>);
  else if constexpr (p.mfma_scores)
    launch(paged_attn_decode_kernel<MfmaScoresBf16, D, G, NW, HS>);
  else if constexpr (kFp8)
    launch(paged_attn_decode_kernel<ScalarScoresFp8, D, G, NW, HS>);
  else
    launch(paged_attn_decode_kernel<ScalarScoresBf16, D, G, NW, HS>);
}

// runtime key (wide << 2 | fp8 << 1 | mfma) -> compile-time plan inputs
template <int D, int G, int kKey = 0, class... Args>
void launch_decode(int key, Args... args) {
  if constexpr (kKey < 8) {
    if (key != kKey) return launch_decode<D, G, kKey + 1>(key, args...);
    launch_variant<D, G, (kKey & 4) != 0, (kKey & 2) != 0, (kKey & 1) != 0>(
        args...);
  }
}

}  // namespace

void launch_paged_attn_decode(u16* out, float* ml_ws, float* acc_ws,
                              const u16* q, const void* k_cache,
                              const void* v_cache, const int* block_tables,
                              const int* seq_lens, int num_seqs,
                              int64_t q_stride, int max_blocks,
                              int num_kv_heads, int head_dim, int group,
                              int num_parts, float scale, bool fp8,
                              hipStream_t stream) {
  const bool wide = num_seqs * num_kv_heads * num_parts < 256;
  // FI_DECODE_MFMA=0 falls back to the scalar-FMA scores (both dtypes)
  static const bool mfma = [] {
    const char* e = getenv("FI_DECODE_MFMA");
    return !(e && e[0] == '0');
  }();
  const dim3 grid(num_seqs, num_kv_heads, num_parts);
  auto launch = [&](auto d, auto g) {
    constexpr int D = decltype(d)::value, G = decltype(g)::value;
    launch_decode<D, G>(wide << 2 | fp8 << 1 | mfma, grid, stream, out, ml_ws,
                        acc_ws, q, k_cache, v_cache, block_tables, seq_lens,
                        q_stride, max_blocks, num_kv_heads, scale);
    if (num_parts > 1) {
      dim3 rgrid(num_seqs, num_kv_heads * G), rblock(kWaveSize);
      hipLaunchKernelGGL((paged_attn_reduce_kernel<D>), rgrid, rblock, 0,
                         stream, out, ml_ws, acc_ws, num_parts);
    }
  };
  auto launch_group = [&](auto d) {
    switch (group) {
      case 1: return launch(d, std::integral_constant<int, 1>{});
      case 2: return launch(d, std::integral_constant<int, 2>{});
      case 4: return launch(d, std::integral_constant<int, 4>{});
      case 8: return launch(d, std::integral_constant<int, 8>{});
      default: abort();
    }
  };
  if (head_dim == 128) launch_group(std::integral_constant<int, 128>{});
  else if (head_dim == 64) launch_group(std::integral_constant<int, 64>{});
  else abort();
}

}  // namespace fi
