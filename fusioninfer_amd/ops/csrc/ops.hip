// PyTorch bindings for the FusionInfer-AMD CDNA4 kernel library.

#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "common.h"

namespace fi {

template <bool FUSED_ADD, bool FP8_OUT>
void launch_rms_norm(void*, float*, const u16*, u16*, const u16*, float, int,
                     int, hipStream_t);
void launch_silu_and_mul(u16*, const u16*, int64_t, int, hipStream_t);
template <bool SILU_MUL>
void launch_row_quant_fp8(unsigned char*, float*, const u16*, int, int,
                          hipStream_t);
void launch_rope_qk_norm(u16*, u16*, int64_t, int64_t, const u16*, const u16*,
                         const float*, const int*, int, int, int, int, float,
                         hipStream_t);
void launch_reshape_and_cache(const u16*, const u16*, void*, void*,
                              const int*, int64_t, int64_t, int, int, int,
                              int, bool, float, float, hipStream_t);
void launch_rope_qk_norm_cache(u16*, const u16*, const u16*, int64_t, int64_t,
                               int64_t, const u16*, const u16*, const float*,
                               const int*, void*, void*, const int*, int, int,
                               int, int, float, bool, float, float,
                               hipStream_t);
template <bool GATHER>
void launch_kv_block_copy(u16*, u16*, u16*, const int*, int, int64_t,
                          hipStream_t);
void launch_paged_attn_decode(u16*, float*, float*, const u16*, const void*,
                              const void*, const int*, const int*, int,
                              int64_t, int, int, int, int, int, float, bool,
                              hipStream_t);
void launch_prefill_attn(u16*, const u16*, const void*, const void*,
                         const int*, const int*, const int*, const int*,
                         const int*, int, int, int64_t, int64_t, int64_t, int,
                         int, int, float, bool, int, bool, hipStream_t);
void launch_moe_gemm(u16*, const u16*, const u16*, const int*, const int*,
                     const int*, int, int, int, int, bool, hipStream_t);
void launch_moe_gemm_fp8(u16*, const unsigned char*, const float*,
                         const unsigned char*, const float*, const int*,
                         const int*, const int*, int, int, int, int, bool,
                         hipStream_t);
void launch_moe_align(const int*, int*, int*, int*, int*, int, int, int,
                      int, int, int, hipStream_t);
void launch_moe_router_topk(const float*, float*, int*, int, int, int,
                            bool, hipStream_t);
void launch_moe_combine(u16*, const u16*, const int*, const float*, int, int,
                        int, hipStream_t);
void launch_lora_apply(u16*, u16*, const u16*, const int*, const u16*,
                       const u16*, const float*, int, int, int, int, int,
                       hipStream_t);
void launch_mxfp4_linear(u16*, const u16*, const unsigned char*,
                         const unsigned char*, const u16*, int, int, int,
                         hipStream_t);
void launch_mxfp4_dequant(u16*, const unsigned char*, const unsigned char*,
                          int64_t, hipStream_t);
void launch_moe_gemm_mxfp4(u16*, const u16*, const unsigned char*,
                           const unsigned char*, const int*, const int*,
                           const int*, int, int, int, int, bool, hipStream_t);
void launch_sample_tokens(int64_t*, const float*, const float*, const int*,
                          const float*, const float*, const int64_t*, int,
                          int, hipStream_t);
void launch_token_logprobs(float*, int*, float*, const float*, const int64_t*,
                           const int*, int, int, int, hipStream_t);
void launch_apply_penalties(float*, const int*, const int*, const float*, int,
                            int, int, hipStream_t);
void launch_penalty_counts_add(int*, const int*, const int64_t*, int, int,
                               int, hipStream_t);
void launch_apply_penalties_spec(float*, const int*, const int*, const float*,
                                 const int64_t*, int, int, int, int,
                                 hipStream_t);
void launch_spec_accept(int64_t*, int*, const int64_t*, const int64_t*,
                        const int*, int, int, int, hipStream_t);
void launch_apply_logit_mods(float*, const int*, const int*, const int*,
                             const int*, const float*, int, int, int, int,
                             int, hipStream_t);

}  // namespace fi

namespace {

using fi::u16;

#define CHECK_BF16_CUDA(t)                                     \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");            \
  TORCH_CHECK((t).scalar_type() == at::kBFloat16, #t " must be bf16")

u16* bf16_ptr(at::Tensor& t) { return reinterpret_cast<u16*>(t.data_ptr()); }
const u16* bf16_cptr(const at::Tensor& t) {
  return reinterpret_cast<const u16*>(t.data_ptr());
}

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// KV caches are bf16 or fp8 (OCP e4m3, scale 1.0)
bool cache_is_fp8(const at::Tensor& t) {
  TORCH_CHECK(
      t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kFloat8_e4m3fn,
      "kv cache must be bf16 or float8_e4m3fn");
  return t.scalar_type() == at::kFloat8_e4m3fn;
}

void rms_norm(at::Tensor out, at::Tensor input, at::Tensor weight, double eps) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(input);
  TORCH_CHECK(input.is_contiguous() && out.is_contiguous());
  const int hidden = input.size(-1);
  const int tokens = input.numel() / hidden;
  fi::launch_rms_norm<false, false>(bf16_ptr(out), nullptr, bf16_cptr(input),
                                    nullptr, bf16_cptr(weight),
                                    static_cast<float>(eps), tokens, hidden,
                                    current_stream());
}

void fused_add_rms_norm(at::Tensor input, at::Tensor residual,
                        at::Tensor weight, double eps) {
  CHECK_BF16_CUDA(input);
  CHECK_BF16_CUDA(residual);
  TORCH_CHECK(input.is_contiguous() && residual.is_contiguous());
  const int hidden = input.size(-1);
  const int tokens = input.numel() / hidden;
  // in-place: residual += input; input = rmsnorm(residual)
  fi::launch_rms_norm<true, false>(bf16_ptr(input), nullptr, bf16_cptr(input),
                                   bf16_ptr(residual), bf16_cptr(weight),
                                   static_cast<float>(eps), tokens, hidden,
                                   current_stream());
}

#define CHECK_FP8_OUT(o, s)                                                  \
  TORCH_CHECK((o).scalar_type() == at::kFloat8_e4m3fn && (o).is_cuda() &&    \
              (o).is_contiguous());                                          \
  TORCH_CHECK((s).scalar_type() == at::kFloat && (s).is_cuda())

void rms_norm_fp8(at::Tensor out, at::Tensor out_scales, at::Tensor input,
                  at::Tensor weight, double eps) {
  CHECK_BF16_CUDA(input);
  CHECK_FP8_OUT(out, out_scales);
  TORCH_CHECK(input.is_contiguous());
  const int hidden = input.size(-1);
  const int tokens = input.numel() / hidden;
  fi::launch_rms_norm<false, true>(
      out.data_ptr(), out_scales.data_ptr<float>(), bf16_cptr(input), nullptr,
      bf16_cptr(weight), static_cast<float>(eps), tokens, hidden,
      current_stream());
}

void fused_add_rms_norm_fp8(at::Tensor out, at::Tensor out_scales,
                            at::Tensor input, at::Tensor residual,
                            at::Tensor weight, double eps) {
  CHECK_BF16_CUDA(input);
  CHECK_BF16_CUDA(residual);
  CHECK_FP8_OUT(out, out_scales);
  TORCH_CHECK(input.is_contiguous() && residual.is_contiguous());
  const int hidden = input.size(-1);
  const int tokens = input.numel() / hidden;
  // residual += input (in place); out = fp8(rmsnorm(residual))
  fi::launch_rms_norm<true, true>(
      out.data_ptr(), out_scales.data_ptr<float>(), bf16_cptr(input),
      bf16_ptr(residual), bf16_cptr(weight), static_cast<float>(eps), tokens,
      hidden, current_stream());
}

void silu_and_mul_fp8(at::Tensor out, at::Tensor out_scales, at::Tensor input) {
  CHECK_BF16_CUDA(input);
  CHECK_FP8_OUT(out, out_scales);
  TORCH_CHECK(input.is_contiguous());
  const int inter = out.size(-1);
  TORCH_CHECK(input.size(-1) == 2 * inter);
  TORCH_CHECK(inter % 8 == 0);
  fi::launch_row_quant_fp8<true>(
      static_cast<unsigned char*>(out.data_ptr()),
      out_scales.data_ptr<float>(), bf16_cptr(input),
      input.numel() / (2 * inter), inter, current_stream());
}

void quant_fp8_rows(at::Tensor out, at::Tensor out_scales, at::Tensor input) {
  CHECK_BF16_CUDA(input);
  CHECK_FP8_OUT(out, out_scales);
  TORCH_CHECK(input.is_contiguous());
  const int cols = input.size(-1);
  TORCH_CHECK(cols % 8 == 0);
  fi::launch_row_quant_fp8<false>(
      static_cast<unsigned char*>(out.data_ptr()),
      out_scales.data_ptr<float>(), bf16_cptr(input), input.numel() / cols,
      cols, current_stream());
}

void silu_and_mul(at::Tensor out, at::Tensor input) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(input);
  TORCH_CHECK(input.is_contiguous() && out.is_contiguous());
  const int inter = out.size(-1);
  TORCH_CHECK(input.size(-1) == 2 * inter);
  TORCH_CHECK(inter % 8 == 0);
  fi::launch_silu_and_mul(bf16_ptr(out), bf16_cptr(input),
                          input.numel() / (2 * inter), inter,
                          current_stream());
}

void rope_qk_norm(at::Tensor q, at::Tensor k,
                  c10::optional<at::Tensor> q_weight,
                  c10::optional<at::Tensor> k_weight, at::Tensor cos_sin,
                  at::Tensor positions, int64_t num_q_heads,
                  int64_t num_kv_heads, int64_t head_dim, double eps) {
  CHECK_BF16_CUDA(q);
  CHECK_BF16_CUDA(k);
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat && cos_sin.is_cuda());
  TORCH_CHECK(positions.scalar_type() == at::kInt && positions.is_cuda());
  // q/k may be row-strided slices of the fused qkv projection output
  TORCH_CHECK(q.dim() == 2 && k.dim() == 2);
  TORCH_CHECK(q.stride(1) == 1 && k.stride(1) == 1);
  const int tokens = q.size(0);
  fi::launch_rope_qk_norm(
      bf16_ptr(q), bf16_ptr(k), q.stride(0), k.stride(0),
      q_weight ? bf16_cptr(*q_weight) : nullptr,
      k_weight ? bf16_cptr(*k_weight) : nullptr, cos_sin.data_ptr<float>(),
      positions.data_ptr<int>(), tokens, num_q_heads, num_kv_heads, head_dim,
      static_cast<float>(eps), current_stream());
}

void reshape_and_cache(at::Tensor k, at::Tensor v, at::Tensor k_cache,
                       at::Tensor v_cache, at::Tensor slot_mapping,
                       double k_inv_scale, double v_inv_scale) {
  CHECK_BF16_CUDA(k);
  CHECK_BF16_CUDA(v);
  const bool fp8 = cache_is_fp8(k_cache);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kInt);
  TORCH_CHECK(k.dim() == 2 && v.dim() == 2);  // [T, Hk*D] (maybe strided rows)
  TORCH_CHECK(k.stride(1) == 1 && v.stride(1) == 1);
  const int kv_heads = k_cache.size(1);
  const int block_size = k_cache.size(2);
  const int head_dim = k_cache.size(3);
  fi::launch_reshape_and_cache(
      bf16_cptr(k), bf16_cptr(v), k_cache.data_ptr(), v_cache.data_ptr(),
      slot_mapping.data_ptr<int>(), k.stride(0), v.stride(0), k.size(0),
      kv_heads, block_size, head_dim, fp8,
      static_cast<float>(k_inv_scale), static_cast<float>(v_inv_scale),
      current_stream());
}

void rope_qk_norm_cache(at::Tensor q, at::Tensor k, at::Tensor v,
                        c10::optional<at::Tensor> q_weight,
                        c10::optional<at::Tensor> k_weight, at::Tensor cos_sin,
                        at::Tensor positions, at::Tensor k_cache,
                        at::Tensor v_cache, at::Tensor slot_mapping,
                        int64_t num_q_heads, int64_t num_kv_heads,
                        int64_t head_dim, double eps, double k_inv_scale,
                        double v_inv_scale) {
  CHECK_BF16_CUDA(q);
  CHECK_BF16_CUDA(k);
  CHECK_BF16_CUDA(v);
  TORCH_CHECK(head_dim == 64 || head_dim == 128,
              "rope_qk_norm_cache: head_dim must be 64 or 128");
  TORCH_CHECK(num_q_heads >= 1 && num_kv_heads >= 1);
  const bool fp8 = cache_is_fp8(k_cache);
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type() &&
              k_cache.is_cuda() && v_cache.is_cuda() &&
              k_cache.is_contiguous() && v_cache.is_contiguous() &&
              k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes());
  TORCH_CHECK(k_cache.size(2) == 16, "cache block_size must be 16");
  TORCH_CHECK(k_cache.size(1) == num_kv_heads && k_cache.size(3) == head_dim,
              "rope_qk_norm_cache: cache must be [B, Hk, 16, D]");
  // q/k/v are row-strided slices of the fused qkv projection output
  const int64_t tokens = q.size(0);
  TORCH_CHECK(q.dim() == 2 && k.dim() == 2 && v.dim() == 2);
  TORCH_CHECK(q.stride(1) == 1 && k.stride(1) == 1 && v.stride(1) == 1);
  TORCH_CHECK(q.size(1) == num_q_heads * head_dim &&
              k.size(1) == num_kv_heads * head_dim &&
              v.size(1) == num_kv_heads * head_dim &&
              k.size(0) == tokens && v.size(0) == tokens);
  TORCH_CHECK(tokens < (1LL << 31));
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat && cos_sin.is_cuda() &&
              cos_sin.is_contiguous() && cos_sin.dim() == 2 &&
              cos_sin.size(1) == head_dim);
  TORCH_CHECK(positions.scalar_type() == at::kInt && positions.is_cuda() &&
              positions.is_contiguous() && positions.numel() == tokens);
  TORCH_CHECK(slot_mapping.scalar_type() == at::kInt &&
              slot_mapping.is_cuda() && slot_mapping.is_contiguous() &&
              slot_mapping.numel() == tokens);
  // every access is 16 B per lane
  auto aligned16 = [](const at::Tensor& t) {
    return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
  };
  TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(v) &&
                  aligned16(cos_sin) && aligned16(k_cache) &&
                  aligned16(v_cache) && q.stride(0) % 8 == 0 &&
                  k.stride(0) % 8 == 0 && v.stride(0) % 8 == 0,
              "rope_qk_norm_cache: q/k/v rows and caches must be 16-byte "
              "aligned");
  auto weight_ptr = [&](const c10::optional<at::Tensor>& w) -> const u16* {
    if (!w) return nullptr;
    CHECK_BF16_CUDA(*w);
    TORCH_CHECK(w->is_contiguous() && w->numel() == head_dim && aligned16(*w));
    return bf16_cptr(*w);
  };
  const u16* qw = weight_ptr(q_weight);
  const u16* kw = weight_ptr(k_weight);
  fi::launch_rope_qk_norm_cache(
      bf16_ptr(q), bf16_cptr(k), bf16_cptr(v), q.stride(0), k.stride(0),
      v.stride(0), qw, kw, cos_sin.data_ptr<float>(),
      positions.data_ptr<int>(), k_cache.data_ptr(), v_cache.data_ptr(),
      slot_mapping.data_ptr<int>(), static_cast<int>(tokens),
      static_cast<int>(num_q_heads), static_cast<int>(num_kv_heads),
      static_cast<int>(head_dim), static_cast<float>(eps), fp8,
      static_cast<float>(k_inv_scale), static_cast<float>(v_inv_scale),
      current_stream());
}

void gather_kv_blocks(at::Tensor staging, at::Tensor k_cache,
                      at::Tensor v_cache, at::Tensor block_ids) {
  TORCH_CHECK(staging.is_cuda() &&
              staging.scalar_type() == k_cache.scalar_type());
  TORCH_CHECK(block_ids.scalar_type() == at::kInt);
  const int n = block_ids.size(0);
  // raw byte mover in u16 units (fp8 blocks are half the bytes)
  const int64_t block_elems = k_cache.size(1) * k_cache.size(2) *
      k_cache.size(3) * k_cache.element_size() / 2;
  fi::launch_kv_block_copy<true>(
      static_cast<fi::u16*>(staging.data_ptr()),
      static_cast<fi::u16*>(k_cache.data_ptr()),
      static_cast<fi::u16*>(v_cache.data_ptr()), block_ids.data_ptr<int>(), n,
      block_elems, current_stream());
}

void scatter_kv_blocks(at::Tensor staging, at::Tensor k_cache,
                       at::Tensor v_cache, at::Tensor block_ids) {
  TORCH_CHECK(staging.is_cuda() &&
              staging.scalar_type() == k_cache.scalar_type());
  TORCH_CHECK(block_ids.scalar_type() == at::kInt);
  const int n = block_ids.size(0);
  const int64_t block_elems = k_cache.size(1) * k_cache.size(2) *
      k_cache.size(3) * k_cache.element_size() / 2;
  fi::launch_kv_block_copy<false>(
      static_cast<fi::u16*>(staging.data_ptr()),
      static_cast<fi::u16*>(k_cache.data_ptr()),
      static_cast<fi::u16*>(v_cache.data_ptr()), block_ids.data_ptr<int>(), n,
      block_elems, current_stream());
}

void paged_attention_decode(at::Tensor out, at::Tensor q, at::Tensor k_cache,
                            at::Tensor v_cache, at::Tensor block_tables,
                            at::Tensor seq_lens,
                            c10::optional<at::Tensor> ml_ws,
                            c10::optional<at::Tensor> acc_ws,
                            int64_t num_parts, double scale) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(q);
  const bool fp8 = cache_is_fp8(k_cache);
  TORCH_CHECK(block_tables.scalar_type() == at::kInt &&
              block_tables.is_contiguous());
  TORCH_CHECK(seq_lens.scalar_type() == at::kInt);
  TORCH_CHECK(q.dim() == 3);  // [S, Hq, D], rows may be strided
  const int num_seqs = q.size(0);
  const int num_heads = q.size(1);
  const int head_dim = q.size(2);
  const int num_kv_heads = k_cache.size(1);
  TORCH_CHECK(k_cache.size(2) == 16, "cache block_size must be 16");
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == head_dim);
  TORCH_CHECK(out.is_contiguous() && out.sizes() == q.sizes(),
              "out must be a contiguous [S, Hq, D] tensor");
  float* ml = nullptr;
  float* acc = nullptr;
  if (num_parts > 1) {
    TORCH_CHECK(ml_ws && acc_ws, "workspace required when num_parts > 1");
    ml = ml_ws->data_ptr<float>();
    acc = acc_ws->data_ptr<float>();
  }
  fi::launch_paged_attn_decode(
      bf16_ptr(out), ml, acc, bf16_cptr(q), k_cache.data_ptr(),
      v_cache.data_ptr(), block_tables.data_ptr<int>(),
      seq_lens.data_ptr<int>(), num_seqs, q.stride(0), block_tables.size(1),
      num_kv_heads, head_dim, num_heads / num_kv_heads,
      static_cast<int>(num_parts), static_cast<float>(scale), fp8,
      current_stream());
}

void prefill_attention(at::Tensor out, at::Tensor q, at::Tensor k,
                       at::Tensor v, at::Tensor tile_seq, at::Tensor tile_row0,
                       at::Tensor cu_seqlens, double scale,
                       int64_t tile_rows, bool heads_adjacent) {
  TORCH_CHECK(tile_rows == 128 || tile_rows == 256,
              "tile_rows must be 128 or 256");
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(q);
  TORCH_CHECK(tile_seq.scalar_type() == at::kInt &&
              tile_row0.scalar_type() == at::kInt &&
              cu_seqlens.scalar_type() == at::kInt);
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3);
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  const int num_kv_heads = k.size(1);
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == head_dim);
  TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == head_dim);
  TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == head_dim);
  TORCH_CHECK(tile_seq.size(0) * q.size(1) < (int64_t{1} << 31),
              "too many (tile, head) workgroups for one grid");
  fi::launch_prefill_attn(
      bf16_ptr(out), bf16_cptr(q), bf16_cptr(k), bf16_cptr(v),
      tile_seq.data_ptr<int>(), tile_row0.data_ptr<int>(),
      cu_seqlens.data_ptr<int>(), nullptr, nullptr, 0, tile_seq.size(0),
      q.stride(0), k.stride(0), v.stride(0), num_q_heads, num_kv_heads,
      head_dim, static_cast<float>(scale), false,
      static_cast<int>(tile_rows / 32), heads_adjacent, current_stream());
}

void prefill_attention_paged(at::Tensor out, at::Tensor q, at::Tensor k_cache,
                             at::Tensor v_cache, at::Tensor tile_seq,
                             at::Tensor tile_row0, at::Tensor cu_seqlens,
                             at::Tensor block_tables, at::Tensor seq_lens_k,
                             double scale, int64_t tile_rows,
                             bool heads_adjacent) {
  TORCH_CHECK(tile_rows == 128 || tile_rows == 256,
              "tile_rows must be 128 or 256");
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(q);
  const bool fp8 = cache_is_fp8(k_cache);
  TORCH_CHECK(tile_seq.scalar_type() == at::kInt &&
              tile_row0.scalar_type() == at::kInt &&
              cu_seqlens.scalar_type() == at::kInt &&
              block_tables.scalar_type() == at::kInt &&
              seq_lens_k.scalar_type() == at::kInt);
  TORCH_CHECK(block_tables.is_contiguous());
  TORCH_CHECK(q.dim() == 3);
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  const int num_kv_heads = k_cache.size(1);
  TORCH_CHECK(k_cache.size(2) == 16, "cache block_size must be 16");
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == head_dim);
  TORCH_CHECK(out.is_contiguous() && out.sizes() == q.sizes(),
              "out must be a contiguous [T, Hq, D] tensor");
  TORCH_CHECK(tile_seq.size(0) * q.size(1) < (int64_t{1} << 31),
              "too many (tile, head) workgroups for one grid");
  fi::launch_prefill_attn(
      bf16_ptr(out), bf16_cptr(q), k_cache.data_ptr(), v_cache.data_ptr(),
      tile_seq.data_ptr<int>(), tile_row0.data_ptr<int>(),
      cu_seqlens.data_ptr<int>(), block_tables.data_ptr<int>(),
      seq_lens_k.data_ptr<int>(), block_tables.size(1), tile_seq.size(0),
      q.stride(0), 0, 0, num_q_heads, num_kv_heads, head_dim,
      static_cast<float>(scale), fp8,
      static_cast<int>(tile_rows / 32), heads_adjacent, current_stream());
}

// Shape checks shared by the bf16 and fp8 grouped GEMMs (dtype checks
// stay with the callers).
struct MoeGemmDims {
  int K, N, max_mtiles;
};

MoeGemmDims check_moe_gemm(const at::Tensor& out, const at::Tensor& a,
                           const at::Tensor& b_packed,
                           const at::Tensor& sorted_ids,
                           const at::Tensor& expert_ids,
                           const at::Tensor& n_valid, int64_t block_m,
                           bool gate_up) {
  TORCH_CHECK(sorted_ids.scalar_type() == at::kInt &&
              expert_ids.scalar_type() == at::kInt &&
              n_valid.scalar_type() == at::kInt);
  TORCH_CHECK(block_m == 16 || block_m == 128, "block_m must be 16 or 128");
  const int K = a.size(1);
  const int N = out.size(1);
  const int PM = out.size(0);
  TORCH_CHECK(PM % block_m == 0, "padded rows must be block_m-aligned");
  TORCH_CHECK(K % 32 == 0, "K must be a multiple of 32");
  TORCH_CHECK(
      N % (block_m == 16 ? 64 : (gate_up ? 64 : 128)) == 0,
      "N tile misalignment");
  // packed B: [E, K/32, NB/16, 64, 8]
  TORCH_CHECK(b_packed.dim() == 5 && b_packed.size(1) == K / 32 &&
              b_packed.size(2) == (gate_up ? 2 * N : N) / 16 &&
              b_packed.size(3) == 64 && b_packed.size(4) == 8,
              "b_packed layout mismatch");
  TORCH_CHECK(expert_ids.size(0) >= PM / block_m);
  if (gate_up) TORCH_CHECK(sorted_ids.size(0) >= PM);
  return {K, N, static_cast<int>(PM / block_m)};
}

void moe_gemm(at::Tensor out, at::Tensor a, at::Tensor b_packed,
              at::Tensor sorted_ids, at::Tensor expert_ids,
              at::Tensor n_valid, int64_t block_m, bool gate_up) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(a);
  CHECK_BF16_CUDA(b_packed);
  TORCH_CHECK(out.is_contiguous() && a.is_contiguous() &&
              b_packed.is_contiguous());
  const MoeGemmDims d = check_moe_gemm(out, a, b_packed, sorted_ids,
                                       expert_ids, n_valid, block_m, gate_up);
  fi::launch_moe_gemm(bf16_ptr(out), bf16_cptr(a),
                      bf16_cptr(b_packed), sorted_ids.data_ptr<int>(),
                      expert_ids.data_ptr<int>(), n_valid.data_ptr<int>(),
                      d.max_mtiles, d.K, d.N, static_cast<int>(block_m),
                      gate_up, current_stream());
}

void moe_gemm_fp8(at::Tensor out, at::Tensor a, at::Tensor a_scales,
                  at::Tensor b_packed, at::Tensor b_scales,
                  at::Tensor sorted_ids, at::Tensor expert_ids,
                  at::Tensor n_valid, int64_t block_m, bool gate_up) {
  CHECK_BF16_CUDA(out);
  TORCH_CHECK(a.scalar_type() == at::kFloat8_e4m3fn && a.is_cuda() &&
              a.is_contiguous());
  TORCH_CHECK(b_packed.scalar_type() == at::kFloat8_e4m3fn &&
              b_packed.is_contiguous());
  TORCH_CHECK(a_scales.scalar_type() == at::kFloat &&
              b_scales.scalar_type() == at::kFloat &&
              b_scales.is_contiguous());
  const MoeGemmDims d = check_moe_gemm(out, a, b_packed, sorted_ids,
                                       expert_ids, n_valid, block_m, gate_up);
  TORCH_CHECK(b_scales.numel() ==
              b_packed.size(0) * (gate_up ? 2 * d.N : d.N));
  fi::launch_moe_gemm_fp8(
      bf16_ptr(out), static_cast<const unsigned char*>(a.data_ptr()),
      a_scales.data_ptr<float>(),
      static_cast<const unsigned char*>(b_packed.data_ptr()),
      b_scales.data_ptr<float>(), sorted_ids.data_ptr<int>(),
      expert_ids.data_ptr<int>(), n_valid.data_ptr<int>(), d.max_mtiles,
      d.K, d.N, static_cast<int>(block_m), gate_up, current_stream());
}

void moe_combine(at::Tensor out, at::Tensor y, at::Tensor pos, at::Tensor w) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(y);
  TORCH_CHECK(out.is_contiguous() && y.is_contiguous());
  TORCH_CHECK(pos.scalar_type() == at::kInt && pos.is_contiguous());
  TORCH_CHECK(w.scalar_type() == at::kFloat && w.is_contiguous());
  const int T = out.size(0);
  const int H = out.size(1);
  TORCH_CHECK(y.size(1) == H && H % 8 == 0);
  const int topk = pos.numel() / T;
  TORCH_CHECK(pos.numel() == T * topk && w.numel() == T * topk);
  fi::launch_moe_combine(bf16_ptr(out), bf16_cptr(y), pos.data_ptr<int>(),
                         w.data_ptr<float>(), T, topk, H, current_stream());
}

void moe_align(at::Tensor topi, at::Tensor sorted_ids, at::Tensor expert_ids,
               at::Tensor n_valid, at::Tensor pos, int64_t topk,
               int64_t e_start, int64_t e_end, int64_t block_m) {
  TORCH_CHECK(topi.is_cuda() && topi.scalar_type() == at::kInt &&
              topi.is_contiguous());
  TORCH_CHECK(sorted_ids.scalar_type() == at::kInt &&
              expert_ids.scalar_type() == at::kInt &&
              n_valid.scalar_type() == at::kInt &&
              pos.scalar_type() == at::kInt);
  const int n = topi.numel();
  const int PM = sorted_ids.numel();
  TORCH_CHECK(e_end - e_start <= 128, "moe_align: E_local > 128");
  TORCH_CHECK(PM % block_m == 0 && expert_ids.numel() == PM / block_m);
  TORCH_CHECK(pos.numel() == n);
  fi::launch_moe_align(topi.data_ptr<int>(), sorted_ids.data_ptr<int>(),
                       expert_ids.data_ptr<int>(), n_valid.data_ptr<int>(),
                       pos.data_ptr<int>(), n, (int)topk, (int)e_start,
                       (int)e_end, (int)block_m, PM, current_stream());
}

void moe_router_topk(at::Tensor logits, at::Tensor topv, at::Tensor topi,
                     int64_t k, bool renorm) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat &&
              logits.is_contiguous());
  TORCH_CHECK(topv.scalar_type() == at::kFloat &&
              topi.scalar_type() == at::kInt);
  const int T = logits.size(0);
  const int E = logits.size(1);
  TORCH_CHECK(E <= 128 && k <= E);
  TORCH_CHECK(topv.numel() == T * k && topi.numel() == T * k);
  fi::launch_moe_router_topk(logits.data_ptr<float>(),
                             topv.data_ptr<float>(), topi.data_ptr<int>(),
                             T, E, (int)k, renorm, current_stream());
}

void lora_apply(at::Tensor out, at::Tensor y_ws, at::Tensor x,
                at::Tensor slot_ids, at::Tensor a_stack, at::Tensor b_stack,
                at::Tensor scales) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(y_ws);
  CHECK_BF16_CUDA(x);
  CHECK_BF16_CUDA(a_stack);
  CHECK_BF16_CUDA(b_stack);
  TORCH_CHECK(out.is_contiguous() && y_ws.is_contiguous() &&
              x.is_contiguous() && a_stack.is_contiguous() &&
              b_stack.is_contiguous());
  TORCH_CHECK(slot_ids.is_cuda() && slot_ids.scalar_type() == at::kInt &&
              slot_ids.is_contiguous());
  TORCH_CHECK(scales.is_cuda() && scales.scalar_type() == at::kFloat &&
              scales.is_contiguous());
  TORCH_CHECK(out.dim() == 2 && x.dim() == 2 && a_stack.dim() == 3 &&
              b_stack.dim() == 3);
  const int64_t T = x.size(0);
  const int64_t K = x.size(1);
  const int64_t N = out.size(1);
  const int64_t S = a_stack.size(0);
  const int64_t R = a_stack.size(1);
  TORCH_CHECK(T >= 1 && T < (1LL << 31) - 16 && out.size(0) == T &&
              slot_ids.numel() == T);
  TORCH_CHECK(K % 64 == 0 && N % 16 == 0 && R % 16 == 0 && R >= 16 &&
                  R <= 128,
              "lora_apply: need K % 64 == 0, N % 16 == 0, R % 16 == 0, "
              "16 <= R <= 128");
  TORCH_CHECK(a_stack.size(2) == K && b_stack.size(0) == S &&
              b_stack.size(1) == N && b_stack.size(2) == R &&
              scales.numel() == S && S >= 1);
  TORCH_CHECK(y_ws.dim() == 2 && y_ws.size(0) == T && y_ws.size(1) == R);
  fi::launch_lora_apply(bf16_ptr(out), bf16_ptr(y_ws), bf16_cptr(x),
                        slot_ids.data_ptr<int>(), bf16_cptr(a_stack),
                        bf16_cptr(b_stack), scales.data_ptr<float>(),
                        static_cast<int>(T), static_cast<int>(K),
                        static_cast<int>(N), static_cast<int>(R),
                        static_cast<int>(S), current_stream());
}

// shared checks of the MXFP4 ops: weight_packed [N, K/2] uint8 and
// weight_scale [N, K/32] uint8, both contiguous on the GPU
void check_mxfp4_weight(const at::Tensor& w_packed, const at::Tensor& w_scale,
                        int64_t* N, int64_t* K) {
  TORCH_CHECK(w_packed.is_cuda() && w_scale.is_cuda(),
              "mxfp4: weights must be on GPU");
  TORCH_CHECK(w_packed.scalar_type() == at::kByte &&
                  w_scale.scalar_type() == at::kByte,
              "mxfp4: weight_packed and weight_scale must be uint8");
  TORCH_CHECK(w_packed.dim() == 2 && w_scale.dim() == 2 &&
                  w_packed.is_contiguous() && w_scale.is_contiguous(),
              "mxfp4: weights must be 2-D and contiguous");
  *N = w_packed.size(0);
  *K = w_packed.size(1) * 2;
  TORCH_CHECK(*N >= 16 && *N % 16 == 0 && *K >= 128 && *K % 128 == 0 &&
                  *N < (1LL << 31) && *K < (1LL << 31),
              "mxfp4: need K % 128 == 0 and N % 16 == 0");
  TORCH_CHECK(w_scale.size(0) == *N && w_scale.size(1) == *K / 32,
              "mxfp4: weight_scale must be [N, K/32]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(w_packed.data_ptr()) % 16 == 0,
              "mxfp4: weight_packed must be 16-byte aligned");
}

void mxfp4_linear(at::Tensor out, at::Tensor x, at::Tensor w_packed,
                  at::Tensor w_scale, c10::optional<at::Tensor> bias) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(x);
  int64_t N, K;
  check_mxfp4_weight(w_packed, w_scale, &N, &K);
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2 && x.is_contiguous() &&
                  out.is_contiguous(),
              "mxfp4_linear: x and out must be 2-D and contiguous");
  const int64_t M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= 65535 * 16 && x.size(1) == K &&
                  out.size(0) == M && out.size(1) == N,
              "mxfp4_linear: need x [M, K], out [M, N], 1 <= M <= 1048560");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "mxfp4_linear: x must be 16-byte aligned");
  TORCH_CHECK(x.get_device() == out.get_device() &&
                  x.get_device() == w_packed.get_device() &&
                  x.get_device() == w_scale.get_device(),
              "mxfp4_linear: tensors must share one device");
  const u16* bias_p = nullptr;
  if (bias.has_value()) {
    CHECK_BF16_CUDA(*bias);
    TORCH_CHECK(bias->dim() == 1 && bias->numel() == N &&
                    bias->is_contiguous() &&
                    bias->get_device() == x.get_device(),
                "mxfp4_linear: bias must be a contiguous [N] bf16 tensor");
    bias_p = bf16_cptr(*bias);
  }
  fi::launch_mxfp4_linear(
      bf16_ptr(out), bf16_cptr(x),
      static_cast<const unsigned char*>(w_packed.data_ptr()),
      static_cast<const unsigned char*>(w_scale.data_ptr()), bias_p,
      static_cast<int>(M), static_cast<int>(N), static_cast<int>(K),
      current_stream());
}

void mxfp4_dequant(at::Tensor out, at::Tensor w_packed, at::Tensor w_scale) {
  CHECK_BF16_CUDA(out);
  int64_t N, K;
  check_mxfp4_weight(w_packed, w_scale, &N, &K);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == N && out.size(1) == K &&
                  out.is_contiguous() &&
                  out.get_device() == w_packed.get_device() &&
                  out.get_device() == w_scale.get_device(),
              "mxfp4_dequant: out must be a contiguous [N, K] bf16 tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0,
              "mxfp4_dequant: out must be 16-byte aligned");
  const int64_t nblocks = N * (K / 32);
  TORCH_CHECK(nblocks / 256 < (1LL << 31) - 1, "mxfp4_dequant: too large");
  fi::launch_mxfp4_dequant(
      bf16_ptr(out), static_cast<const unsigned char*>(w_packed.data_ptr()),
      static_cast<const unsigned char*>(w_scale.data_ptr()), nblocks,
      current_stream());
}

// grouped W4A16 GEMM: w_packed [E, NB, K/2], w_scale [E, NB, K/32] uint8,
// NB = 2N when gate_up; a = x [T, K] (gate_up) or act [PM, K]
void moe_gemm_mxfp4(at::Tensor out, at::Tensor a, at::Tensor w_packed,
                    at::Tensor w_scale, at::Tensor sorted_ids,
                    at::Tensor expert_ids, at::Tensor n_valid,
                    int64_t block_m, bool gate_up) {
  CHECK_BF16_CUDA(out);
  CHECK_BF16_CUDA(a);
  TORCH_CHECK(out.dim() == 2 && a.dim() == 2 && out.is_contiguous() &&
                  a.is_contiguous(),
              "moe_gemm_mxfp4: out and a must be 2-D and contiguous");
  TORCH_CHECK(w_packed.is_cuda() && w_scale.is_cuda() &&
                  w_packed.scalar_type() == at::kByte &&
                  w_scale.scalar_type() == at::kByte &&
                  w_packed.dim() == 3 && w_scale.dim() == 3 &&
                  w_packed.is_contiguous() && w_scale.is_contiguous(),
              "moe_gemm_mxfp4: weights must be contiguous 3-D uint8 on GPU");
  TORCH_CHECK(sorted_ids.is_cuda() && expert_ids.is_cuda() &&
                  n_valid.is_cuda() && sorted_ids.scalar_type() == at::kInt &&
                  expert_ids.scalar_type() == at::kInt &&
                  n_valid.scalar_type() == at::kInt &&
                  sorted_ids.is_contiguous() && expert_ids.is_contiguous() &&
                  n_valid.numel() == 1,
              "moe_gemm_mxfp4: sorted_ids, expert_ids, n_valid must be "
              "contiguous int32 on GPU");
  TORCH_CHECK(block_m == 16 || block_m == 128,
              "moe_gemm_mxfp4: block_m must be 16 or 128");
  const int64_t K = a.size(1);
  const int64_t N = out.size(1);
  const int64_t PM = out.size(0);
  const int64_t NB = gate_up ? 2 * N : N;
  TORCH_CHECK(K >= 128 && K % 128 == 0 && N >= 16 && N % 16 == 0 &&
                  K < (1LL << 31) && NB < (1LL << 31),
              "moe_gemm_mxfp4: need K % 128 == 0 and N % 16 == 0");
  TORCH_CHECK(PM >= block_m && PM % block_m == 0 && PM < (1LL << 31),
              "moe_gemm_mxfp4: padded rows must be block_m-aligned");
  TORCH_CHECK(w_packed.size(0) >= 1 && w_packed.size(1) == NB &&
                  w_packed.size(2) == K / 2 &&
                  w_scale.size(0) == w_packed.size(0) &&
                  w_scale.size(1) == NB && w_scale.size(2) == K / 32,
              "moe_gemm_mxfp4: need w_packed [E, NB, K/2] and w_scale "
              "[E, NB, K/32]");
  TORCH_CHECK(expert_ids.numel() >= PM / block_m &&
                  sorted_ids.numel() >= PM && a.size(0) >= 1 &&
                  (gate_up || a.size(0) >= PM),
              "moe_gemm_mxfp4: sorted_ids / expert_ids / a too short");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(w_packed.data_ptr()) % 16 == 0,
              "moe_gemm_mxfp4: a and w_packed must be 16-byte aligned");
  const auto dev = out.get_device();
  TORCH_CHECK(a.get_device() == dev && w_packed.get_device() == dev &&
                  w_scale.get_device() == dev &&
                  sorted_ids.get_device() == dev &&
                  expert_ids.get_device() == dev &&
                  n_valid.get_device() == dev,
              "moe_gemm_mxfp4: tensors must share one device");
  fi::launch_moe_gemm_mxfp4(
      bf16_ptr(out), bf16_cptr(a),
      static_cast<const unsigned char*>(w_packed.data_ptr()),
      static_cast<const unsigned char*>(w_scale.data_ptr()),
      sorted_ids.data_ptr<int>(), expert_ids.data_ptr<int>(),
      n_valid.data_ptr<int>(), static_cast<int>(PM / block_m),
      static_cast<int>(K), static_cast<int>(N), static_cast<int>(block_m),
      gate_up, current_stream());
}

void sample_tokens(at::Tensor out, at::Tensor logits, at::Tensor temperature,
                   at::Tensor top_k, at::Tensor top_p, at::Tensor min_p,
                   at::Tensor rng) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat &&
              logits.is_contiguous() && logits.dim() == 2,
              "sample_tokens: logits must be a contiguous [T, V] fp32 GPU "
              "tensor");
  const int64_t T = logits.size(0);
  const int64_t V = logits.size(1);
  TORCH_CHECK(T >= 1 && T < (1LL << 31) && V >= 1 && V < (1LL << 30),
              "sample_tokens: need 1 <= T < 2^31 and 1 <= V < 2^30");
  auto check_row = [&](const at::Tensor& t, at::ScalarType ty, int64_t n,
                       const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() &&
                    t.numel() == n,
                "sample_tokens: bad ", name);
  };
  check_row(out, at::kLong, T, "out");
  check_row(temperature, at::kFloat, T, "temperature");
  check_row(top_k, at::kInt, T, "top_k");
  check_row(top_p, at::kFloat, T, "top_p");
  check_row(min_p, at::kFloat, T, "min_p");
  check_row(rng, at::kLong, 2 * T, "rng");
  fi::launch_sample_tokens(
      out.data_ptr<int64_t>(), logits.data_ptr<float>(),
      temperature.data_ptr<float>(), top_k.data_ptr<int>(),
      top_p.data_ptr<float>(), min_p.data_ptr<float>(),
      rng.data_ptr<int64_t>(), static_cast<int>(T), static_cast<int>(V),
      current_stream());
}

void token_logprobs(at::Tensor chosen, at::Tensor top_ids, at::Tensor top_lp,
                    at::Tensor logits, at::Tensor token_ids,
                    at::Tensor num_top) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat &&
              logits.is_contiguous() && logits.dim() == 2,
              "token_logprobs: logits must be a contiguous [T, V] fp32 GPU "
              "tensor");
  const int64_t T = logits.size(0);
  const int64_t V = logits.size(1);
  TORCH_CHECK(T >= 1 && T < (1LL << 31) && V >= 1 && V < (1LL << 30),
              "token_logprobs: need 1 <= T < 2^31 and 1 <= V < 2^30");
  TORCH_CHECK(top_ids.dim() == 2 && top_ids.size(0) == T,
              "token_logprobs: top_ids must be [T, W]");
  const int64_t W = top_ids.size(1);
  // W bounds the kernel's LDS list
  TORCH_CHECK(W >= 1 && W <= 32, "token_logprobs: need 1 <= W <= 32");
  auto check = [&](const at::Tensor& t, at::ScalarType ty, int64_t n,
                   const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() &&
                    t.numel() == n,
                "token_logprobs: bad ", name);
  };
  check(chosen, at::kFloat, T, "chosen");
  check(top_ids, at::kInt, T * W, "top_ids");
  check(top_lp, at::kFloat, T * W, "top_lp");
  check(token_ids, at::kLong, T, "token_ids");
  check(num_top, at::kInt, T, "num_top");
  fi::launch_token_logprobs(
      chosen.data_ptr<float>(), top_ids.data_ptr<int>(),
      top_lp.data_ptr<float>(), logits.data_ptr<float>(),
      token_ids.data_ptr<int64_t>(), num_top.data_ptr<int>(),
      static_cast<int>(T), static_cast<int>(V), static_cast<int>(W),
      current_stream());
}

void apply_penalties(at::Tensor logits, at::Tensor counts,
                     at::Tensor slot_ids, at::Tensor params) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat &&
              logits.is_contiguous() && logits.dim() == 2,
              "apply_penalties: logits must be a contiguous [T, V] fp32 GPU "
              "tensor");
  const int64_t T = logits.size(0);
  const int64_t V = logits.size(1);
  // T is the grid's y extent
  TORCH_CHECK(T >= 1 && T <= 65535 && V >= 1 && V < (1LL << 30),
              "apply_penalties: need 1 <= T <= 65535 and 1 <= V < 2^30");
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == at::kInt &&
              counts.is_contiguous() && counts.dim() == 2 &&
              counts.size(0) >= 1 && counts.size(0) < (1LL << 31) &&
              counts.size(1) == V,
              "apply_penalties: counts must be a contiguous [S >= 1, V] "
              "int32 GPU tensor");
  TORCH_CHECK(slot_ids.is_cuda() && slot_ids.scalar_type() == at::kInt &&
              slot_ids.is_contiguous() && slot_ids.numel() == T,
              "apply_penalties: bad slot_ids");
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == at::kFloat &&
              params.is_contiguous() && params.numel() == 4 * T,
              "apply_penalties: bad params");
  fi::launch_apply_penalties(
      logits.data_ptr<float>(), counts.data_ptr<int>(),
      slot_ids.data_ptr<int>(), params.data_ptr<float>(),
      static_cast<int>(T), static_cast<int>(V),
      static_cast<int>(counts.size(0)), current_stream());
}

void penalty_counts_add(at::Tensor counts, at::Tensor slot_ids,
                        at::Tensor token_ids) {
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == at::kInt &&
              counts.is_contiguous() && counts.dim() == 2 &&
              counts.size(0) >= 1 && counts.size(0) < (1LL << 31) &&
              counts.size(1) >= 1 && counts.size(1) < (1LL << 30),
              "penalty_counts_add: counts must be a contiguous [S >= 1, "
              "1 <= V < 2^30] int32 GPU tensor");
  const int64_t N = slot_ids.numel();
  TORCH_CHECK(N >= 1 && N < (1LL << 31) - 256,
              "penalty_counts_add: need 1 <= N < 2^31 - 256");
  TORCH_CHECK(slot_ids.is_cuda() && slot_ids.scalar_type() == at::kInt &&
              slot_ids.is_contiguous() && slot_ids.dim() == 1,
              "penalty_counts_add: bad slot_ids");
  TORCH_CHECK(token_ids.is_cuda() && token_ids.scalar_type() == at::kLong &&
              token_ids.is_contiguous() && token_ids.dim() == 1 &&
              token_ids.numel() == N,
              "penalty_counts_add: bad token_ids");
  fi::launch_penalty_counts_add(
      counts.data_ptr<int>(), slot_ids.data_ptr<int>(),
      token_ids.data_ptr<int64_t>(), static_cast<int>(N),
      static_cast<int>(counts.size(1)), static_cast<int>(counts.size(0)),
      current_stream());
}

void apply_penalties_spec(at::Tensor logits, at::Tensor counts,
                          at::Tensor slot_ids, at::Tensor params,
                          at::Tensor extra) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat &&
              logits.is_contiguous() && logits.dim() == 2,
              "apply_penalties_spec: logits must be a contiguous [R, V] fp32 "
              "GPU tensor");
  const int64_t T = logits.size(0);
  const int64_t V = logits.size(1);
  // T is the grid's y extent
  TORCH_CHECK(T >= 1 && T <= 65535 && V >= 1 && V < (1LL << 30),
              "apply_penalties_spec: need 1 <= R <= 65535 and 1 <= V < 2^30");
  TORCH_CHECK(counts.is_cuda() && counts.scalar_type() == at::kInt &&
              counts.is_contiguous() && counts.dim() == 2 &&
              counts.size(0) >= 1 && counts.size(0) < (1LL << 31) &&
              counts.size(1) == V,
              "apply_penalties_spec: counts must be a contiguous [S >= 1, V] "
              "int32 GPU tensor");
  TORCH_CHECK(slot_ids.is_cuda() && slot_ids.scalar_type() == at::kInt &&
              slot_ids.is_contiguous() && slot_ids.numel() == T,
              "apply_penalties_spec: bad slot_ids");
  TORCH_CHECK(params.is_cuda() && params.scalar_type() == at::kFloat &&
              params.is_contiguous() && params.numel() == 4 * T,
              "apply_penalties_spec: bad params");
  // E bounds the kernel's LDS copy of a row's ids
  TORCH_CHECK(extra.is_cuda() && extra.scalar_type() == at::kLong &&
              extra.is_contiguous() && extra.dim() == 2 &&
              extra.size(0) == T && extra.size(1) >= 1 && extra.size(1) <= 16,
              "apply_penalties_spec: extra must be a contiguous [R, 1 <= E "
              "<= 16] int64 GPU tensor");
  fi::launch_apply_penalties_spec(
      logits.data_ptr<float>(), counts.data_ptr<int>(),
      slot_ids.data_ptr<int>(), params.data_ptr<float>(),
      extra.data_ptr<int64_t>(), static_cast<int>(T), static_cast<int>(V),
      static_cast<int>(counts.size(0)), static_cast<int>(extra.size(1)),
      current_stream());
}

void spec_accept(at::Tensor emitted, at::Tensor n_emit, at::Tensor sampled,
                 at::Tensor drafts, at::Tensor span_cu) {
  TORCH_CHECK(emitted.is_cuda() && emitted.scalar_type() == at::kLong &&
              emitted.is_contiguous() && emitted.dim() == 2 &&
              emitted.size(0) >= 1 && emitted.size(0) < (1LL << 24) &&
              emitted.size(1) >= 1 && emitted.size(1) <= 17,
              "spec_accept: emitted must be a contiguous [1 <= S < 2^24, "
              "1 <= W <= 17] int64 GPU tensor");
  const int64_t S = emitted.size(0);
  const int64_t R = sampled.numel();
  TORCH_CHECK(R >= 1 && R < (1LL << 31), "spec_accept: need 1 <= R < 2^31");
  auto check = [&](const at::Tensor& t, at::ScalarType ty, int64_t n,
                   const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() &&
                    t.dim() == 1 && t.numel() == n,
                "spec_accept: bad ", name);
  };
  check(n_emit, at::kInt, S, "n_emit");
  check(sampled, at::kLong, R, "sampled");
  check(drafts, at::kLong, R, "drafts");
  check(span_cu, at::kInt, S + 1, "span_cu");
  fi::launch_spec_accept(
      emitted.data_ptr<int64_t>(), n_emit.data_ptr<int>(),
      sampled.data_ptr<int64_t>(), drafts.data_ptr<int64_t>(),
      span_cu.data_ptr<int>(), static_cast<int>(R), static_cast<int>(S),
      static_cast<int>(emitted.size(1)), current_stream());
}

// Either half may be absent (both of its tensors undefined): mask_ids +
// masks, or bias_cu + bias_ids + bias_vals.
void apply_logit_mods(at::Tensor logits, c10::optional<at::Tensor> mask_ids,
                      c10::optional<at::Tensor> masks,
                      c10::optional<at::Tensor> bias_cu,
                      c10::optional<at::Tensor> bias_ids,
                      c10::optional<at::Tensor> bias_vals) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat &&
              logits.is_contiguous() && logits.dim() == 2,
              "apply_logit_mods: logits must be a contiguous [T, V] fp32 GPU "
              "tensor");
  const int64_t T = logits.size(0);
  const int64_t V = logits.size(1);
  // T is the grid's y extent
  TORCH_CHECK(T >= 1 && T <= 65535 && V >= 1 && V < (1LL << 30),
              "apply_logit_mods: need 1 <= T <= 65535 and 1 <= V < 2^30");
  const int64_t W = (V + 31) / 32;
  const bool has_mask = mask_ids.has_value();
  const bool has_bias = bias_cu.has_value();
  TORCH_CHECK(masks.has_value() == has_mask,
              "apply_logit_mods: mask_ids and masks come together");
  TORCH_CHECK(bias_ids.has_value() == has_bias &&
              bias_vals.has_value() == has_bias,
              "apply_logit_mods: bias_cu, bias_ids and bias_vals come "
              "together");
  TORCH_CHECK(has_mask || has_bias,
              "apply_logit_mods: neither a mask nor a bias given");
  const int* mask_ids_p = nullptr;
  const int* masks_p = nullptr;
  int64_t M = 0;
  if (has_mask) {
    TORCH_CHECK(mask_ids->is_cuda() && mask_ids->scalar_type() == at::kInt &&
                mask_ids->is_contiguous() && mask_ids->dim() == 1 &&
                mask_ids->numel() == T,
                "apply_logit_mods: mask_ids must be a contiguous [T] int32 "
                "GPU tensor");
    TORCH_CHECK(masks->is_cuda() && masks->scalar_type() == at::kInt &&
                masks->is_contiguous() && masks->dim() == 2 &&
                masks->size(0) >= 1 && masks->size(0) < (1LL << 31) &&
                masks->size(1) == W,
                "apply_logit_mods: masks must be a contiguous [M >= 1, "
                "ceil(V / 32)] int32 GPU tensor");
    M = masks->size(0);
    mask_ids_p = mask_ids->data_ptr<int>();
    masks_p = masks->data_ptr<int>();
  }
  const int* bias_cu_p = nullptr;
  const int* bias_ids_p = nullptr;
  const float* bias_vals_p = nullptr;
  int64_t B = 0;
  if (has_bias) {
    TORCH_CHECK(bias_cu->is_cuda() && bias_cu->scalar_type() == at::kInt &&
                bias_cu->is_contiguous() && bias_cu->dim() == 1 &&
                bias_cu->numel() == T + 1,
                "apply_logit_mods: bias_cu must be a contiguous [T + 1] "
                "int32 GPU tensor");
    B = bias_ids->numel();
    // entry indices advance by up to 2^19 * 256 threads per step
    TORCH_CHECK(bias_ids->is_cuda() && bias_ids->scalar_type() == at::kInt &&
                bias_ids->is_contiguous() && bias_ids->dim() == 1 &&
                B < (1LL << 30),
                "apply_logit_mods: bias_ids must be a contiguous [B < 2^30] "
                "int32 GPU tensor");
    TORCH_CHECK(bias_vals->is_cuda() &&
                bias_vals->scalar_type() == at::kFloat &&
                bias_vals->is_contiguous() && bias_vals->dim() == 1 &&
                bias_vals->numel() == B,
                "apply_logit_mods: bias_vals must be a contiguous [B] fp32 "
                "GPU tensor");
    bias_cu_p = bias_cu->data_ptr<int>();
    if (B > 0) {
      bias_ids_p = bias_ids->data_ptr<int>();
      bias_vals_p = bias_vals->data_ptr<float>();
    }
  }
  fi::launch_apply_logit_mods(
      logits.data_ptr<float>(), mask_ids_p, masks_p, bias_cu_p, bias_ids_p,
      bias_vals_p, static_cast<int>(T), static_cast<int>(V),
      static_cast<int>(M), static_cast<int>(W), static_cast<int>(B),
      current_stream());
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rms_norm", &rms_norm, "RMSNorm (bf16, fp32 accum)");
  m.def("fused_add_rms_norm", &fused_add_rms_norm,
        "in-place residual add + RMSNorm");
  m.def("silu_and_mul", &silu_and_mul, "fused SiLU-mul");
  m.def("rms_norm_fp8", &rms_norm_fp8, "RMSNorm with fused fp8 row quant");
  m.def("fused_add_rms_norm_fp8", &fused_add_rms_norm_fp8,
        "residual add + RMSNorm with fused fp8 row quant");
  m.def("silu_and_mul_fp8", &silu_and_mul_fp8,
        "fused SiLU-mul with fp8 row quant");
  m.def("quant_fp8_rows", &quant_fp8_rows, "per-row dynamic fp8 quant");
  m.def("rope_qk_norm", &rope_qk_norm,
        "fused per-head qk RMSNorm + NeoX RoPE (in-place)");
  m.def("reshape_and_cache", &reshape_and_cache, "scatter K/V into paged cache");
  m.def("rope_qk_norm_cache", &rope_qk_norm_cache,
        "fused qk RMSNorm + NeoX RoPE (q in place) + K/V paged-cache write");
  m.def("gather_kv_blocks", &gather_kv_blocks, "pack KV blocks for PD send");
  m.def("scatter_kv_blocks", &scatter_kv_blocks, "unpack KV blocks from PD recv");
  m.def("paged_attention_decode", &paged_attention_decode,
        "paged decode attention");
  m.def("prefill_attention", &prefill_attention, "varlen causal MFMA prefill");
  m.def("prefill_attention_paged", &prefill_attention_paged,
        "varlen causal MFMA prefill over the paged cache (context attention)");
  m.def("moe_gemm", &moe_gemm,
        "grouped MFMA GEMM over block-aligned expert segments "
        "(gate_up=true fuses the SwiGLU epilogue)");
  m.def("moe_gemm_fp8", &moe_gemm_fp8,
        "grouped fp8 (e4m3) MFMA GEMM with per-row/per-channel dequant "
        "epilogue (gate_up=true fuses SwiGLU)");
  m.def("moe_combine", &moe_combine,
        "weighted top-k combine of expert outputs (deterministic)");
  m.def("moe_align", &moe_align,
        "single-kernel block alignment of expert assignments "
        "(vLLM moe_align_block_size analog)");
  m.def("moe_router_topk", &moe_router_topk,
        "fused router tail: softmax + top-k + optional renormalize");
  m.def("mxfp4_linear", &mxfp4_linear,
        "W4A16 linear on MXFP4 weights (bf16 in/out, fp32 accumulation)");
  m.def("mxfp4_dequant", &mxfp4_dequant, "expand MXFP4 weights to bf16");
  m.def("moe_gemm_mxfp4", &moe_gemm_mxfp4,
        "grouped W4A16 GEMM over block-aligned expert segments with MXFP4 "
        "expert weights (gate_up=true fuses the SwiGLU epilogue)");
  m.def("lora_apply", &lora_apply,
        "batched multi-LoRA shrink + expand indexed by per-token slot ids "
        "(in-place on out)");
  m.def("sample_tokens", &sample_tokens,
        "fused temperature / top-k / top-p / min-p sampling with a "
        "counter-based (Philox4x32-10) draw, one workgroup per row");
  m.def("token_logprobs", &token_logprobs,
        "log-softmax value of one token per row plus the top-k (id, "
        "logprob) pairs, one workgroup per row");
  m.def("apply_penalties", &apply_penalties,
        "repetition / presence / frequency penalties from a per-slot token "
        "histogram (in-place on logits)");
  m.def("penalty_counts_add", &penalty_counts_add,
        "counts[slot_ids[i], token_ids[i]] += 1 (integer atomics)");
  m.def("apply_penalties_spec", &apply_penalties_spec,
        "apply_penalties for speculative verification rows: the histogram "
        "plus up to 16 draft ids per row (in-place on logits)");
  m.def("spec_accept", &spec_accept,
        "longest accepted draft prefix plus the corrected token per "
        "verification span");
  m.def("apply_logit_mods", &apply_logit_mods,
        "logit_bias (CSR) and packed grammar masks, bias then mask "
        "(in-place on logits)");
}
