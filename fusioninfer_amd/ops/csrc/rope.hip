// Fused per-head RMSNorm (Qwen3 qk-norm) + NeoX rotary embedding, in-place.
//
// One wave per (token, head): D/2 lanes hold 2 bf16 each; the rotate-half
// partner lives exactly shfl_xor(D/4) away, so RoPE needs one cross-lane
// exchange and zero LDS. cos/sin are precomputed on host (f32 [P, D],
// cos | sin) — on-device trig would turn this memory-bound op VALU-bound
// (guide Appendix B).
//
// Capability parity: RoPE/qk-norm epilogue the reference delegates to vLLM
// (SURVEY.md §2.3).

#include "common.h"

namespace fi {

template <int D>
__global__ void rope_qk_norm_kernel(
    u16* __restrict__ q,             // [T, Hq*D] rows, stride q_stride
    u16* __restrict__ k,             // [T, Hk*D] rows, stride k_stride
    const int64_t q_stride, const int64_t k_stride,
    const u16* __restrict__ q_weight,  // [D] or nullptr
    const u16* __restrict__ k_weight,  // [D] or nullptr
    const float* __restrict__ cos_sin,  // [P, D]
    const int* __restrict__ positions,  // [T]
    const int num_q_heads, const float eps) {
  constexpr int kHalfLanes = D / 4;   // lanes holding x1 pairs
  constexpr int kActive = D / 2;
  const int lane = threadIdx.x;
  if (lane >= kActive) return;

  const int token = blockIdx.x;
  const int head = blockIdx.y;
  const bool is_q = head < num_q_heads;
  u16* base = is_q ? q + token * q_stride + static_cast<int64_t>(head) * D
                   : k + token * k_stride +
                         static_cast<int64_t>(head - num_q_heads) * D;
  const u16* w = is_q ? q_weight : k_weight;

  // element offset of this lane's pair within the head
  const int e = 2 * lane;
  u32 bits = *reinterpret_cast<const u32*>(base + e);
  float a = bf16_to_f32(static_cast<u16>(bits & 0xffff));
  float b = bf16_to_f32(static_cast<u16>(bits >> 16));

  if (w != nullptr) {
    float sumsq = a * a + b * b;
#pragma unroll
    for (int off = kActive / 2; off > 0; off >>= 1)
      sumsq += __shfl_xor(sumsq, off, 64);
    const float inv_rms = rsqrtf(sumsq / D + eps);
    const u32 wbits = *reinterpret_cast<const u32*>(w + e);
    a *= inv_rms * bf16_to_f32(static_cast<u16>(wbits & 0xffff));
    b *= inv_rms * bf16_to_f32(static_cast<u16>(wbits >> 16));
  }

  // rotate-half partner exchange
  const float pa = __shfl_xor(a, kHalfLanes, 64);
  const float pb = __shfl_xor(b, kHalfLanes, 64);

  const bool is_x1 = lane < kHalfLanes;
  const int pair = is_x1 ? e : e - D / 2;  // rotary pair index in [0, D/2)
  const int pos = positions[token];
  const float2 c = *reinterpret_cast<const float2*>(
      cos_sin + static_cast<int64_t>(pos) * D + pair);
  const float2 s = *reinterpret_cast<const float2*>(
      cos_sin + static_cast<int64_t>(pos) * D + D / 2 + pair);

  float oa, ob;
  if (is_x1) {  // x1' = x1*cos - x2*sin
    oa = a * c.x - pa * s.x;
    ob = b * c.y - pb * s.y;
  } else {  // x2' = x2*cos + x1*sin
    oa = a * c.x + pa * s.x;
    ob = b * c.y + pb * s.y;
  }
  u32 obits = static_cast<u32>(f32_to_bf16(oa)) |
              (static_cast<u32>(f32_to_bf16(ob)) << 16);
  *reinterpret_cast<u32*>(base + e) = obits;
}

void launch_rope_qk_norm(u16* q, u16* k, int64_t q_stride, int64_t k_stride,
                         const u16* q_weight, const u16* k_weight,
                         const float* cos_sin, const int* positions,
                         int tokens, int num_q_heads, int num_kv_heads,
                         int head_dim, float eps, hipStream_t stream) {
  dim3 grid(tokens, num_q_heads + num_kv_heads), block(64);
  if (head_dim == 128) {
    hipLaunchKernelGGL((rope_qk_norm_kernel<128>), grid, block, 0, stream, q,
                       k, q_stride, k_stride, q_weight, k_weight, cos_sin,
                       positions, num_q_heads, eps);
  } else if (head_dim == 64) {
    hipLaunchKernelGGL((rope_qk_norm_kernel<64>), grid, block, 0, stream, q, k,
                       q_stride, k_stride, q_weight, k_weight, cos_sin,
                       positions, num_q_heads, eps);
  } else {
    abort();  // head_dim ∈ {64, 128}
  }
}

// ---------------------------------------------------------------------
// rope_qk_norm_cache: qk-norm + RoPE + paged-cache write in one pass.
//
// q gets norm + rope in place; K gets norm + rope and goes STRAIGHT to
// k_cache[slot] (never back to the qkv buffer: attention only ever reads
// K from the paged cache, so the write-back + re-read of the two-kernel
// path is an HBM round trip for nothing); V is copied to v_cache[slot].
//
// 16 B per lane: D/8 lanes per head, 256-thread workgroups covering
// 2048/D heads of one token, grid (T, ceil((Hq + 2 Hk) / heads per wg)).
// The rotate-half partner of a lane's 8 elements sits D/16 lanes away:
// one shfl_xor per element, no LDS.
//
// Results are bit-for-bit those of rope_qk_norm_kernel followed by
// reshape_and_cache_kernel. What the compiler makes of the expressions
// in rope_qk_norm_kernel (which products it contracts into FMAs) depends
// on how it vectorizes them, so the arithmetic here is pinned down with
// contraction off and explicit fmaf, to the operations that kernel
// compiles to:
//   pair sum      a*a + b*b, both products rounded;
//   sum of squares over the head: that kernel holds one pair per lane and
//                 adds across lanes at xor D/4 ... 1. With four pairs
//                 p0..p3 per lane here, its levels D/4 ... 4 are this
//                 kernel's cross-lane levels D/16 ... 1 on each p_j
//                 separately, its level 2 is p0+p2 | p1+p3 and its level
//                 1 is (p0+p2) + (p1+p3);
//   inv_rms       rsqrtf(fmaf(sumsq, 1/D, eps));
//   norm          x * (inv_rms * w);
//   rope          fmaf(x, cos, -+(partner * sin)).
// tests/test_rope_cache_fused_gpu.py holds the two paths to torch.equal.

// 8 bf16 as one 16 B value (a vector type, so that it stays one register
// quad and one load / store instruction through the branches below)
typedef u32 u32x4 __attribute__((ext_vector_type(4)));

// one row of 8 bf16 -> cache, as reshape_and_cache_kernel
template <bool FP8>
FI_DEV void store_cache_row(void* __restrict__ cache, const int64_t dst,
                            const u32x4 row, const float inv_scale) {
  if (FP8) {
    const u32 w[4] = {row[0], row[1], row[2], row[3]};
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const u16 h = static_cast<u16>(j & 1 ? w[j / 2] >> 16 : w[j / 2] & 0xffff);
      // saturate at e4m3 max: v_cvt_pk_fp8_f32 has no hardware clamp
      f[j] = fminf(fmaxf(bf16_to_f32(h) * inv_scale, -448.f), 448.f);
    }
    u32 p[2];
    pack_fp8x8(f, p);
    *reinterpret_cast<uint2*>(static_cast<unsigned char*>(cache) + dst) =
        make_uint2(p[0], p[1]);
  } else {
    *reinterpret_cast<u32x4*>(static_cast<u16*>(cache) + dst) = row;
  }
}

template <int D, bool FP8>
__global__ __launch_bounds__(256) void rope_qk_norm_cache_kernel(
    u16* __restrict__ q,              // [T, Hq*D] rows, stride q_stride
    const u16* __restrict__ k,        // [T, Hk*D] rows, stride k_stride
    const u16* __restrict__ v,        // [T, Hk*D] rows, stride v_stride
    const int64_t q_stride, const int64_t k_stride, const int64_t v_stride,
    const u16* __restrict__ q_weight,  // [D] or nullptr
    const u16* __restrict__ k_weight,  // [D] or nullptr
    const float* __restrict__ cos_sin,  // [P, D]
    const int* __restrict__ positions,  // [T]
    void* __restrict__ k_cache,  // [B, Hk, 16, D] bf16 (FP8: e4m3 bytes)
    void* __restrict__ v_cache,
    const int* __restrict__ slot_mapping,  // [T], < 0 = padding row
    const int num_q_heads, const int num_kv_heads, const float eps,
    const float k_inv_scale, const float v_inv_scale) {
#pragma clang fp contract(off)
  constexpr int kLanes = D / 8;  // lanes per head, 8 bf16 each
  constexpr int kHeadsPerBlock = 256 / kLanes;
  constexpr int kCacheBlock = 16;

  const int token = blockIdx.x;
  const int head = blockIdx.y * kHeadsPerBlock + threadIdx.x / kLanes;
  const int sub = threadIdx.x % kLanes;
  const int e = sub * 8;  // element offset of this lane within the head
  // whole heads leave together, so every shuffle below has its partner
  if (head >= num_q_heads + 2 * num_kv_heads) return;

  const bool is_q = head < num_q_heads;
  const bool is_v = head >= num_q_heads + num_kv_heads;
  const int kv_head =
      is_q ? 0 : (head - num_q_heads) % num_kv_heads;  // K then V heads
  int64_t dst = 0;
  if (!is_q) {
    const int slot = slot_mapping[token];
    if (slot < 0) return;  // padding token: no cache write
    dst = ((static_cast<int64_t>(slot / kCacheBlock) * num_kv_heads +
            kv_head) * kCacheBlock + slot % kCacheBlock) * D + e;
  }

  u16* qrow = q + token * q_stride + static_cast<int64_t>(head) * D + e;
  const int64_t kv_off = static_cast<int64_t>(kv_head) * D + e;
  const u16* src = is_q ? qrow
                        : (is_v ? v + token * v_stride : k + token * k_stride) +
                              kv_off;
  u32x4 row = *reinterpret_cast<const u32x4*>(src);

  if (!is_v) {  // V is a straight copy
    const u32 iw[4] = {row[0], row[1], row[2], row[3]};
    float x[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = bf16_to_f32(static_cast<u16>(iw[j] & 0xffff));
      x[2 * j + 1] = bf16_to_f32(static_cast<u16>(iw[j] >> 16));
    }

    const u16* w = is_q ? q_weight : k_weight;
    if (w != nullptr) {
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        p[j] = x[2 * j] * x[2 * j] + x[2 * j + 1] * x[2 * j + 1];
#pragma unroll
      for (int off = kLanes / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] += __shfl_xor(p[j], off, 64);
      }
      const float sumsq = (p[0] + p[2]) + (p[1] + p[3]);
      const float inv_rms = rsqrtf(__builtin_fmaf(sumsq, 1.0f / D, eps));
      const bf16x8 wv = *reinterpret_cast<const bf16x8*>(w + e);
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] *= inv_rms * bf16_to_f32(wv.h[j]);
    }

    // rotate-half partner exchange
    float px[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) px[j] = __shfl_xor(x[j], kLanes / 2, 64);

    const bool is_x1 = sub < kLanes / 2;
    const int pair = is_x1 ? e : e - D / 2;  // rotary pair index in [0, D/2)
    const float* cs =
        cos_sin + static_cast<int64_t>(positions[token]) * D + pair;
    const float4 c0 = *reinterpret_cast<const float4*>(cs);
    const float4 c1 = *reinterpret_cast<const float4*>(cs + 4);
    const float4 s0 = *reinterpret_cast<const float4*>(cs + D / 2);
    const float4 s1 = *reinterpret_cast<const float4*>(cs + D / 2 + 4);
    const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
    const float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};

    u32 ow[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      // x1' = x1*cos - x2*sin ; x2' = x2*cos + x1*sin
      const float m0 = px[j] * s[j];
      const float m1 = px[j + 1] * s[j + 1];
      const float o0 = __builtin_fmaf(x[j], c[j], is_x1 ? -m0 : m0);
      const float o1 = __builtin_fmaf(x[j + 1], c[j + 1], is_x1 ? -m1 : m1);
      ow[j / 2] = static_cast<u32>(f32_to_bf16(o0)) |
                  (static_cast<u32>(f32_to_bf16(o1)) << 16);
    }
    row = u32x4{ow[0], ow[1], ow[2], ow[3]};
  }

  if (is_q) {
    *reinterpret_cast<u32x4*>(qrow) = row;
  } else {
    // fp8: K is already rounded to bf16 here, as the qkv write-back was
    store_cache_row<FP8>(is_v ? v_cache : k_cache, dst, row,
                         is_v ? v_inv_scale : k_inv_scale);
  }
}

void launch_rope_qk_norm_cache(
    u16* q, const u16* k, const u16* v, int64_t q_stride, int64_t k_stride,
    int64_t v_stride, const u16* q_weight, const u16* k_weight,
    const float* cos_sin, const int* positions, void* k_cache, void* v_cache,
    const int* slot_mapping, int tokens, int num_q_heads, int num_kv_heads,
    int head_dim, float eps, bool fp8, float k_inv_scale, float v_inv_scale,
    hipStream_t stream) {
  if (tokens == 0) return;
  const int heads = num_q_heads + 2 * num_kv_heads;
  const dim3 grid(tokens, ceil_div(heads, 2048 / head_dim)), block(256);
#define FI_ROPE_CACHE(D_, FP8_)                                             \
  hipLaunchKernelGGL((rope_qk_norm_cache_kernel<D_, FP8_>), grid, block, 0, \
                     stream, q, k, v, q_stride, k_stride, v_stride,         \
                     q_weight, k_weight, cos_sin, positions, k_cache,       \
                     v_cache, slot_mapping, num_q_heads, num_kv_heads, eps, \
                     k_inv_scale, v_inv_scale)
  if (head_dim == 128) {
    if (fp8) FI_ROPE_CACHE(128, true); else FI_ROPE_CACHE(128, false);
  } else if (head_dim == 64) {
    if (fp8) FI_ROPE_CACHE(64, true); else FI_ROPE_CACHE(64, false);
  } else {
    abort();  // head_dim ∈ {64, 128}, checked by the binding
  }
#undef FI_ROPE_CACHE
}

}  // namespace fi
