"""Op dispatch: CDNA4 HIP kernels on GPU, PyTorch fp32 reference on CPU.

Policy (required by the build contract): on a GPU box the HIP extension is
the ONLY execution path — if ``_C.so`` is missing or fails to import, any
GPU-tensor call raises immediately instead of silently falling back to
eager PyTorch. CPU tensors (CI containers without a GPU) use the reference
implementations from ``fusioninfer_amd.ops.reference``.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from fusioninfer_amd.ops import reference as ref

_C = None
_C_IMPORT_ERROR: Optional[BaseException] = None
try:
    import importlib

    _C = importlib.import_module("fusioninfer_amd.ops._C")
except Exception as e:  # pragma: no cover - exercised only when build broken
    _C_IMPORT_ERROR = e


def has_native() -> bool:
    return _C is not None


def _require_native():
    if _C is None:
        raise RuntimeError(
            "fusioninfer_amd HIP extension (_C.so) is not available but a GPU "
            "tensor was passed — refusing to fall back to eager PyTorch on "
            "the GPU path. Build it with `python -m fusioninfer_amd.ops.build`."
        ) from _C_IMPORT_ERROR


# ---------------------------------------------------------------- norm ops

def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if x.is_cuda:
        _require_native()
        out = torch.empty_like(x)
        _C.rms_norm(out, x, weight, eps)
        return out
    return ref.rms_norm(x, weight, eps)


def fused_add_rms_norm(x, residual, weight, eps: float):
    """In-place on GPU: residual += x; x = rmsnorm(residual). Returns (x, residual)."""
    if x.is_cuda:
        _require_native()
        _C.fused_add_rms_norm(x, residual, weight, eps)
        return x, residual
    return ref.fused_add_rms_norm(x, residual, weight, eps)


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        _require_native()
        out = torch.empty(
            (*x.shape[:-1], x.shape[-1] // 2), dtype=x.dtype, device=x.device
        )
        _C.silu_and_mul(out, x)
        return out
    return ref.silu_and_mul(x)


# ------------------------------------------------------- fp8 fused epilogues
#
# The fp8 serving mode quantizes activations per-token for torch._scaled_mm;
# done eagerly that costs more than the fp8 GEMM saves, so quantization is
# fused into the producing kernel (norm / SwiGLU) or done in one pass
# (quant_fp8_rows for the attention output).

def rms_norm_fp8(x: torch.Tensor, weight: torch.Tensor, eps: float):
    """Returns (x_fp8 [T, H] e4m3, scales [T] fp32)."""
    if x.is_cuda:
        _require_native()
        out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
        scales = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _C.rms_norm_fp8(out, scales, x, weight, eps)
        return out, scales
    return ref.rms_norm_fp8(x, weight, eps)


def fused_add_rms_norm_fp8(x, residual, weight, eps: float):
    """residual += x in place; returns (x_fp8, scales, residual)."""
    if x.is_cuda:
        _require_native()
        out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
        scales = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _C.fused_add_rms_norm_fp8(out, scales, x, residual, weight, eps)
        return out, scales, residual
    return ref.fused_add_rms_norm_fp8(x, residual, weight, eps)


def silu_and_mul_fp8(x: torch.Tensor):
    """x: [T, 2*I] -> (act_fp8 [T, I] e4m3, scales [T] fp32)."""
    if x.is_cuda:
        _require_native()
        inter = x.shape[-1] // 2
        out = torch.empty(
            (*x.shape[:-1], inter), dtype=torch.float8_e4m3fn, device=x.device
        )
        scales = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _C.silu_and_mul_fp8(out, scales, x)
        return out, scales
    return ref.silu_and_mul_fp8(x)


def quant_fp8_rows(x: torch.Tensor):
    """Per-row dynamic fp8 quant: (x_fp8, scales [T] fp32)."""
    if x.is_cuda:
        _require_native()
        out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
        scales = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _C.quant_fp8_rows(out, scales, x)
        return out, scales
    return ref.quant_fp8_rows(x)


# ---------------------------------------------------------------- rope

def rope_qk_norm_(
    q: torch.Tensor,          # [T, Hq*D] (row-strided slice OK)
    k: torch.Tensor,          # [T, Hk*D]
    positions: torch.Tensor,  # [T] int32
    cos_sin: torch.Tensor,    # [P, D] fp32
    num_q_heads: int,
    num_kv_heads: int,
    head_dim: int,
    q_weight: Optional[torch.Tensor] = None,
    k_weight: Optional[torch.Tensor] = None,
    eps: float = 1e-6,
):
    """Fused optional per-head RMSNorm + NeoX RoPE, in-place. Returns (q, k)."""
    if q.is_cuda:
        _require_native()
        _C.rope_qk_norm(
            q, k, q_weight, k_weight, cos_sin, positions,
            num_q_heads, num_kv_heads, head_dim, eps,
        )
        return q, k
    qv = q.view(-1, num_q_heads, head_dim)
    kv = k.view(-1, num_kv_heads, head_dim)
    qo, ko = ref.rope_qk_norm(qv, kv, positions.long(), cos_sin, q_weight, k_weight, eps)
    q.copy_(qo.reshape(q.shape))
    k.copy_(ko.reshape(k.shape))
    return q, k


# ---------------------------------------------------------------- kv cache

def reshape_and_cache(k, v, k_cache, v_cache, slot_mapping,
                      k_inv_scale: float = 1.0, v_inv_scale: float = 1.0):
    """Scatter K/V rows into the paged cache. For fp8 caches the rows are
    multiplied by the INVERSE per-layer static scales before e4m3
    conversion (vLLM k_scale/v_scale); bf16 caches ignore the scales
    (the read side compensates only on the fp8 path)."""
    if k.is_cuda:
        _require_native()
        _C.reshape_and_cache(k, v, k_cache, v_cache, slot_mapping,
                             k_inv_scale, v_inv_scale)
        return
    H, D = k_cache.shape[1], k_cache.shape[3]
    ref.reshape_and_cache(
        k.view(-1, H, D), v.view(-1, H, D), k_cache, v_cache,
        slot_mapping.long(), k_inv_scale, v_inv_scale,
    )


def rope_qk_norm_cache_(
    q: torch.Tensor,          # [T, Hq*D] (row-strided slice OK)
    k: torch.Tensor,          # [T, Hk*D]
    v: torch.Tensor,          # [T, Hk*D]
    positions: torch.Tensor,  # [T] int32
    cos_sin: torch.Tensor,    # [P, D] fp32
    num_q_heads: int,
    num_kv_heads: int,
    head_dim: int,
    k_cache: torch.Tensor,    # [B, Hk, 16, D] bf16 or float8_e4m3fn
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,  # [T] int32, < 0 = padding row
    q_weight: Optional[torch.Tensor] = None,
    k_weight: Optional[torch.Tensor] = None,
    eps: float = 1e-6,
    k_inv_scale: float = 1.0,
    v_inv_scale: float = 1.0,
):
    """rope_qk_norm_ + reshape_and_cache in one kernel, bit for bit.

    q gets the optional per-head RMSNorm + NeoX RoPE in place. K gets the
    same and is written to k_cache at slot_mapping[t]; it is NOT written
    back, so the contents of `k` after the call are unspecified. V is
    copied to v_cache. Rows with a negative slot skip both cache writes
    (their q is still processed). fp8 caches take the rows times the
    inverse scales, as reshape_and_cache does. Returns q.

    The kernel covers head_dim 64 and 128 and the [B, Hk, 16, D] cache
    layout; anything else raises ValueError on the GPU. On the CPU this is
    the reference composition (ref.rope_qk_norm, ref.reshape_and_cache)."""
    if q.is_cuda:
        _require_native()
        if head_dim not in (64, 128):
            raise ValueError(
                f"rope_qk_norm_cache_: head_dim must be 64 or 128, got "
                f"{head_dim}")
        if (k_cache.dim() != 4 or k_cache.shape != v_cache.shape
                or k_cache.shape[1] != num_kv_heads or k_cache.shape[2] != 16
                or k_cache.shape[3] != head_dim):
            raise ValueError(
                "rope_qk_norm_cache_: caches must both be "
                f"[B, {num_kv_heads}, 16, {head_dim}], got "
                f"{tuple(k_cache.shape)} and {tuple(v_cache.shape)}")
        _C.rope_qk_norm_cache(
            q, k, v, q_weight, k_weight, cos_sin, positions, k_cache,
            v_cache, slot_mapping, num_q_heads, num_kv_heads, head_dim, eps,
            k_inv_scale, v_inv_scale,
        )
        return q
    rope_qk_norm_(q, k, positions, cos_sin, num_q_heads, num_kv_heads,
                  head_dim, q_weight, k_weight, eps)
    reshape_and_cache(k, v, k_cache, v_cache, slot_mapping,
                      k_inv_scale, v_inv_scale)
    return q


def gather_kv_blocks(k_cache, v_cache, block_ids) -> torch.Tensor:
    if k_cache.is_cuda:
        _require_native()
        n = int(block_ids.numel())
        staging = torch.empty(
            (2, n, *k_cache.shape[1:]), dtype=k_cache.dtype, device=k_cache.device
        )
        _C.gather_kv_blocks(staging, k_cache, v_cache, block_ids)
        return staging
    return ref.gather_kv_blocks(k_cache, v_cache, block_ids.long())


def scatter_kv_blocks(staging, k_cache, v_cache, block_ids):
    if k_cache.is_cuda:
        _require_native()
        _C.scatter_kv_blocks(staging, k_cache, v_cache, block_ids)
        return
    ref.scatter_kv_blocks(staging, k_cache, v_cache, block_ids.long())


# ---------------------------------------------------------------- attention

DECODE_PARTITION_TOKENS = 512  # flash-decoding partition size (kernel contract)


def _check_attn_out(out: torch.Tensor, q: torch.Tensor) -> None:
    """`out=` of the attention ops: the kernels index it as a dense
    [n, Hq, D] bf16 array (a row slice of a larger buffer viewed that way
    is fine, a column slice is not)."""
    if (out.shape != q.shape or out.dtype != q.dtype
            or out.device != q.device or not out.is_contiguous()):
        raise ValueError(
            f"out must be a contiguous {tuple(q.shape)} {q.dtype} tensor on "
            f"{q.device}, got {tuple(out.shape)} {out.dtype} strides "
            f"{out.stride()} on {out.device}")


def paged_attention_decode(
    q: torch.Tensor,            # [S, Hq, D]
    k_cache: torch.Tensor,      # [B, Hk, bs, D]
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,  # [S, max_blocks] int32
    seq_lens: torch.Tensor,      # [S] int32
    scale: Optional[float] = None,
    out: Optional[torch.Tensor] = None,  # [S, Hq, D] contiguous, written
) -> torch.Tensor:
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if out is not None:
        _check_attn_out(out, q)
    if q.is_cuda:
        _require_native()
        S, Hq, D = q.shape
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        # partitions from the block-table width: static shape under
        # hipGraph capture (seq_lens vary between replays, width doesn't)
        max_tokens = int(block_tables.shape[1]) * int(k_cache.shape[2])
        num_parts = max(
            (max_tokens + DECODE_PARTITION_TOKENS - 1) // DECODE_PARTITION_TOKENS,
            1,
        )
        ml_ws = acc_ws = None
        if num_parts > 1:
            ml_ws = torch.empty(
                (S, Hq, num_parts, 2), dtype=torch.float32, device=q.device
            )
            acc_ws = torch.empty(
                (S, Hq, num_parts, D), dtype=torch.float32, device=q.device
            )
        _C.paged_attention_decode(
            out, q, k_cache, v_cache, block_tables, seq_lens,
            ml_ws, acc_ws, num_parts, scale,
        )
        return out
    res = ref.paged_attention_decode(q, k_cache, v_cache, block_tables, seq_lens, scale)
    return res if out is None else out.copy_(res)


# q rows per prefill workgroup (NW waves x 32) — kernel contract; the
# FI_PF_NW env selects the 4-wave variant on both sides (see
# prefill_attention.hip launcher)
import os as _os

PREFILL_TILE_ROWS = (4 if _os.environ.get("FI_PF_NW", "8").startswith("4")
                     else 8) * 32


def prefill_tile_rows(seq_lens) -> int:
    """Per-batch workgroup width: 128-row (4-wave) workgroups once any
    sequence is >=4096 new tokens — the narrower shape halves the
    causal-raggedness idle and measured +10% at 1x8192 (it loses ~5% at
    many short sequences, so the default stays 256)."""
    if seq_lens and max(seq_lens) >= 4096:
        return 128
    return PREFILL_TILE_ROWS


# FI_PF_TILE_ORDER=0 restores the prefill schedule as it was before the
# heaviest-first order: the ascending tile table and the (tile, head) grid
# with the tile fastest. Both schedules give the same bits (a tile's
# arithmetic does not depend on when it is dispatched); the switch exists
# for before/after measurements from one build. Read once at import.
PF_TILE_ORDER = _os.environ.get("FI_PF_TILE_ORDER", "1") != "0"

PREFILL_KV_TILE = 64  # kv tokens per K-loop step of the prefill kernel


def build_prefill_tiles(seq_lens, device=None, rows=None, ctx_starts=None,
                        heaviest_first=None):
    """Host-side tile table for the prefill kernel: one workgroup per
    `rows` q-rows of each sequence (rows must be 128 or 256 and MATCH
    the tile_rows passed to the kernel).

    seq_lens: list[int], the NEW tokens per sequence; ctx_starts: list[int],
    the tokens already cached per sequence (default: zeros).
    Returns (tile_seq, tile_row0) int32 tensors.

    Tiles are listed heaviest first: a causal tile walks
    ceil((ctx_start + min(row0 + rows, L)) / 64) KV steps, and the kernel
    hands tiles out in table order, so the long ones start first and the
    short ones fill the tail (ties: ascending (seq, row0), so the table is
    a pure function of its inputs). The kernel accepts any order;
    heaviest_first=False keeps the ascending (seq, row0) one, and None
    takes the process default (on unless FI_PF_TILE_ORDER=0).
    """
    rows = rows or PREFILL_TILE_ROWS
    if heaviest_first is None:
        heaviest_first = PF_TILE_ORDER
    if ctx_starts is None:
        ctx_starts = [0] * len(seq_lens)
    tiles = []
    for s, (L, c) in enumerate(zip(seq_lens, ctx_starts)):
        for r0 in range(0, L, rows):
            cost = -(-(c + min(r0 + rows, L)) // PREFILL_KV_TILE)
            tiles.append((-cost, s, r0))
    if heaviest_first:
        tiles.sort()
    tile_seq = [t[1] for t in tiles]
    tile_row0 = [t[2] for t in tiles]
    return (
        torch.tensor(tile_seq, dtype=torch.int32, device=device),
        torch.tensor(tile_row0, dtype=torch.int32, device=device),
    )


def prefill_attention(
    q: torch.Tensor,           # [T, Hq, D]
    k: torch.Tensor,           # [T, Hk, D]
    v: torch.Tensor,           # [T, Hk, D]
    cu_seqlens: torch.Tensor,  # [S+1] int32
    scale: Optional[float] = None,
    tile_seq: Optional[torch.Tensor] = None,
    tile_row0: Optional[torch.Tensor] = None,
    tile_rows: Optional[int] = None,
) -> torch.Tensor:
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if q.is_cuda:
        _require_native()
        if tile_seq is None:
            lens = (cu_seqlens[1:] - cu_seqlens[:-1]).tolist()
            tile_rows = tile_rows or prefill_tile_rows(lens)
            tile_seq, tile_row0 = build_prefill_tiles(
                lens, device=q.device, rows=tile_rows
            )
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        _C.prefill_attention(out, q, k, v, tile_seq, tile_row0, cu_seqlens,
                             scale, tile_rows or PREFILL_TILE_ROWS,
                             PF_TILE_ORDER)
        return out
    return ref.prefill_attention(q, k, v, cu_seqlens, scale, causal=True)


def prefill_attention_paged(
    q: torch.Tensor,             # [Tnew, Hq, D] new tokens only
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,  # [S, max_blocks] int32
    cu_seqlens_q: torch.Tensor,  # [S+1] int32 over new tokens
    seq_lens_k: torch.Tensor,    # [S] int32 total context length
    scale: Optional[float] = None,
    tile_seq: Optional[torch.Tensor] = None,
    tile_row0: Optional[torch.Tensor] = None,
    tile_rows: Optional[int] = None,
    out: Optional[torch.Tensor] = None,  # [Tnew, Hq, D] contiguous, written
) -> torch.Tensor:
    """Context attention: new tokens attend over the paged cache (their own
    K/V must already be written via reshape_and_cache)."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if out is not None:
        _check_attn_out(out, q)
    if q.is_cuda:
        _require_native()
        if tile_seq is None:
            lens = (cu_seqlens_q[1:] - cu_seqlens_q[:-1]).tolist()
            ctx = [k_len - n for k_len, n in zip(seq_lens_k.tolist(), lens)]
            tile_rows = tile_rows or prefill_tile_rows(lens)
            tile_seq, tile_row0 = build_prefill_tiles(
                lens, device=q.device, rows=tile_rows, ctx_starts=ctx
            )
        if out is None:
            out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        _C.prefill_attention_paged(
            out, q, k_cache, v_cache, tile_seq, tile_row0, cu_seqlens_q,
            block_tables, seq_lens_k, scale,
            tile_rows or PREFILL_TILE_ROWS, PF_TILE_ORDER,
        )
        return out
    res = ref.prefill_attention_paged(
        q, k_cache, v_cache, block_tables, cu_seqlens_q, seq_lens_k, scale
    )
    return res if out is None else out.copy_(res)


# ---------------------------------------------------------------- MoE

def pack_moe_weights(w: torch.Tensor) -> torch.Tensor:
    """Pack per-expert weights [E, K, N] into MFMA B-fragment order
    [E, K/32, N/16, 64, 8] for the grouped GEMM: lane l of a wave reads
    its 8 contiguous bf16 B elements (B[k=(l>>4)*8+e][n=l&15] within a
    32x16 k-by-n subtile) with one 16 B load — one fully-coalesced 1 KiB
    transaction per wave per K-step."""
    E, K, N = w.shape
    assert K % 32 == 0 and N % 16 == 0, (K, N)
    return (
        w.view(E, K // 32, 4, 8, N // 16, 16)
        .permute(0, 1, 4, 2, 5, 3)
        .reshape(E, K // 32, N // 16, 64, 8)
        .contiguous()
    )


def moe_gemm(out, a, b_packed, sorted_ids, expert_ids, n_valid,
             block_m: int, gate_up: bool):
    """Grouped GEMM over block-aligned expert segments.

    out [PM, N] bf16; a = x [T, K] (gate_up, rows gathered via sorted_ids)
    or act [PM, K]; b_packed from pack_moe_weights ([E, K/32, NB/16, 64, 8]
    with NB = 2N when gate_up). n_valid: device int32 scalar tensor with
    the real m-tile count (static grid, dynamic work — hipGraph-safe).
    gate_up=True fuses the SwiGLU epilogue: out = silu(gate) * up."""
    if out.is_cuda:
        _require_native()
        _C.moe_gemm(out, a, b_packed, sorted_ids, expert_ids, n_valid,
                    block_m, gate_up)
        return out
    return ref.moe_gemm(out, a, b_packed, sorted_ids, expert_ids, n_valid,
                        block_m, gate_up)


def moe_gemm_fp8(out, a, a_scales, b_packed, b_scales, sorted_ids,
                 expert_ids, n_valid, block_m: int, gate_up: bool):
    """Grouped fp8 (e4m3) GEMM with dequant epilogue: out[bf16] =
    (A_fp8 @ B_fp8) * a_scale[row] * b_scale[expert, col]; gate_up fuses
    SwiGLU. Same block-aligned layout as moe_gemm; b_packed from
    pack_moe_weights over the [E, K, N] e4m3 weights."""
    if out.is_cuda:
        _require_native()
        _C.moe_gemm_fp8(out, a, a_scales, b_packed, b_scales, sorted_ids,
                        expert_ids, n_valid, block_m, gate_up)
        return out
    return ref.moe_gemm_fp8(out, a, a_scales, b_packed, b_scales,
                            sorted_ids, expert_ids, n_valid, block_m,
                            gate_up)


def moe_align(topi: torch.Tensor, e_start: int, e_end: int, block_m: int):
    """Single-kernel device-side block alignment of expert assignments
    (GPU only; MoEMLP._moe_align's torch composition is the CPU
    reference and the semantic oracle). Within-expert slot order is
    arrival order rather than stable order — downstream results are
    bit-identical either way (each row's K-loop and the pos-gathered
    combine don't depend on the slot). Returns
    (sorted_ids [PM], expert_ids [PM/bm], n_valid [1], pos [T*k], PM)."""
    _require_native()
    T, k = topi.shape
    n = T * k
    E_local = e_end - e_start
    PM = ((n + block_m - 1) // block_m + E_local) * block_m
    dev = topi.device
    sorted_ids = torch.empty(PM, dtype=torch.int32, device=dev)
    expert_ids = torch.empty(PM // block_m, dtype=torch.int32, device=dev)
    n_valid = torch.empty(1, dtype=torch.int32, device=dev)
    pos = torch.empty(n, dtype=torch.int32, device=dev)
    _C.moe_align(topi.reshape(-1).int().contiguous(), sorted_ids,
                 expert_ids, n_valid, pos, k, e_start, e_end, block_m)
    return sorted_ids, expert_ids, n_valid, pos, PM


def moe_router_topk(logits: torch.Tensor, k: int, renorm: bool):
    """Fused router tail (GPU): softmax + top-k + optional top-k
    renormalization in one wave-per-token kernel. logits [T, E] fp32;
    returns (topv [T,k] fp32 weights, topi [T,k] int32 expert ids,
    descending; ties pick the smaller index)."""
    _require_native()
    T, E = logits.shape
    topv = torch.empty(T, k, dtype=torch.float32, device=logits.device)
    topi = torch.empty(T, k, dtype=torch.int32, device=logits.device)
    _C.moe_router_topk(logits.contiguous(), topv, topi, k, renorm)
    return topv, topi


def moe_combine(out, y, pos, w):
    """out[t] = sum_k w[t,k] * y[pos[t,k]] (pos < 0 skipped). Deterministic
    (no atomics) so token-exact tests stay reproducible."""
    if out.is_cuda:
        _require_native()
        _C.moe_combine(out, y, pos, w)
        return out
    return ref.moe_combine(out, y, pos, w)


# ---------------------------------------------------------------- LoRA

LORA_MAX_RANK = 128  # kernel contract: R % 16 == 0 and R <= 128


def lora_shapes_supported(K: int, N: int, R: int) -> bool:
    """Shapes the HIP lora_apply kernels cover (any T >= 1)."""
    return (K % 64 == 0 and N % 16 == 0 and R % 16 == 0
            and 16 <= R <= LORA_MAX_RANK)


def lora_apply(out, x, slot_ids, a_stack, b_stack, scales):
    """Batched multi-LoRA, in place on out:

        out[t] += scales[s] * bf16(x[t] @ a_stack[s].T) @ b_stack[s].T

    with s = slot_ids[t]; an id outside [0, S) (canonically -1) means "no
    adapter" and leaves the row bit-for-bit untouched. out [T, N] bf16,
    x [T, K] bf16, slot_ids [T] int32, a_stack [S, R, K] bf16 and
    b_stack [S, N, R] bf16 (zero-padded beyond each adapter's rank),
    scales [S] fp32. Static shapes, no host sync: hipGraph-capturable.
    Unsupported shapes raise ValueError (no silent fallback)."""
    T, K = x.shape
    N = out.shape[1]
    S, R = a_stack.shape[0], a_stack.shape[1]
    if (out.shape[0] != T or slot_ids.shape != (T,)
            or a_stack.shape != (S, R, K) or b_stack.shape != (S, N, R)
            or scales.shape != (S,)):
        raise ValueError(
            f"lora_apply: inconsistent shapes out={tuple(out.shape)} "
            f"x={tuple(x.shape)} slot_ids={tuple(slot_ids.shape)} "
            f"a_stack={tuple(a_stack.shape)} b_stack={tuple(b_stack.shape)} "
            f"scales={tuple(scales.shape)}"
        )
    if T < 1 or S < 1 or not lora_shapes_supported(K, N, R):
        raise ValueError(
            f"lora_apply: unsupported shape T={T} K={K} N={N} R={R} S={S} "
            "(need T >= 1, K % 64 == 0, N % 16 == 0, R % 16 == 0, "
            f"R <= {LORA_MAX_RANK})"
        )
    if out.is_cuda:
        _require_native()
        if not out.is_contiguous():
            raise ValueError("lora_apply: out must be contiguous")
        y_ws = torch.empty((T, R), dtype=out.dtype, device=out.device)
        _C.lora_apply(out, y_ws, x.contiguous(), slot_ids, a_stack, b_stack,
                      scales)
        return out
    return ref.lora_apply(out, x, slot_ids, a_stack, b_stack, scales)


# ---------------------------------------------------------------- MXFP4

MXFP4_SCALE_MIN = 8    # scale bytes outside [8, 247] could dequantise to a
MXFP4_SCALE_MAX = 247  # subnormal, an infinity or NaN (0xFF): not accepted


def validate_mxfp4_scales(w_scale: torch.Tensor) -> None:
    """Raise ValueError if an e8m0 scale byte lies outside [8, 247]. Reads
    the tensor on the host (synchronises on a GPU tensor): call it when
    weights are converted or loaded, never per forward. The compute ops do
    not scan scale bytes; feeding them a byte this rejects is outside
    their contract."""
    if w_scale.dtype != torch.uint8:
        raise ValueError(
            f"mxfp4: weight_scale must be uint8, got {w_scale.dtype}")
    if w_scale.numel() == 0:
        return
    lo, hi = int(w_scale.min()), int(w_scale.max())
    if lo < MXFP4_SCALE_MIN or hi > MXFP4_SCALE_MAX:
        raise ValueError(
            f"mxfp4: scale bytes span [{lo}, {hi}], outside the supported "
            f"[{MXFP4_SCALE_MIN}, {MXFP4_SCALE_MAX}]")


def _check_mxfp4_weight(op: str, w_packed, w_scale):
    if w_packed.dtype != torch.uint8 or w_scale.dtype != torch.uint8:
        raise ValueError(
            f"{op}: weight_packed and weight_scale must be uint8, got "
            f"{w_packed.dtype} and {w_scale.dtype}")
    if w_packed.dim() != 2 or w_scale.dim() != 2:
        raise ValueError(f"{op}: weight_packed and weight_scale must be 2-D")
    N, K = w_packed.shape[0], w_packed.shape[1] * 2
    if K < 128 or K % 128 != 0 or N < 16 or N % 16 != 0:
        raise ValueError(
            f"{op}: unsupported shape N={N} K={K} "
            "(need K % 128 == 0 and N % 16 == 0)")
    if tuple(w_scale.shape) != (N, K // 32):
        raise ValueError(
            f"{op}: weight_scale must be [N, K/32] = {(N, K // 32)}, got "
            f"{tuple(w_scale.shape)}")
    if w_scale.device != w_packed.device:
        raise ValueError(f"{op}: weight tensors must share one device")
    if not (w_packed.is_contiguous() and w_scale.is_contiguous()):
        raise ValueError(f"{op}: weight tensors must be contiguous")
    return N, K


def _check_mxfp4_out(op: str, out, shape, device):
    if (out.dtype != torch.bfloat16 or tuple(out.shape) != shape
            or out.device != device or not out.is_contiguous()):
        raise ValueError(
            f"{op}: out must be a contiguous bf16 {shape} tensor on {device}")


def mxfp4_linear(x, w_packed, w_scale, bias=None, out=None):
    """W4A16 linear on MXFP4 weights:

        out[m, n] = bf16( sum_k x[m, k] * dq(W)[n, k] (+ bias[n]) )

    with fp32 accumulation and one rounding. x [M, K] bf16 contiguous,
    w_packed [N, K/2] uint8, w_scale [N, K/32] uint8 (bytes in [8, 247],
    see validate_mxfp4_scales), bias [N] bf16 or None. K % 128 == 0,
    N % 16 == 0, any M >= 0. Static grid, no host sync, no workspace:
    hipGraph-capturable. A row's bits depend only on that x row and the
    weights (deterministic, batch-invariant). Unsupported input raises
    ValueError (no silent fallback)."""
    N, K = _check_mxfp4_weight("mxfp4_linear", w_packed, w_scale)
    if x.dtype != torch.bfloat16:
        raise ValueError(f"mxfp4_linear: x must be bf16, got {x.dtype}")
    if x.dim() != 2 or x.shape[1] != K:
        raise ValueError(
            f"mxfp4_linear: x must be [M, {K}], got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError("mxfp4_linear: x must be contiguous")
    if x.device != w_packed.device:
        raise ValueError("mxfp4_linear: x and the weights must share one device")
    if bias is not None and (
            bias.dtype != torch.bfloat16 or tuple(bias.shape) != (N,)
            or bias.device != x.device or not bias.is_contiguous()):
        raise ValueError(
            f"mxfp4_linear: bias must be a contiguous bf16 [{N}] tensor on "
            f"{x.device}")
    M = x.shape[0]
    if out is not None:
        _check_mxfp4_out("mxfp4_linear", out, (M, N), x.device)
    if x.is_cuda:
        _require_native()
        if out is None:
            out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
        if M > 0:
            _C.mxfp4_linear(out, x, w_packed, w_scale, bias)
        return out
    res = ref.mxfp4_linear(x, w_packed, w_scale, bias)
    if out is None:
        return res
    out.copy_(res)
    return out


def mxfp4_dequant(w_packed, w_scale, out=None):
    """Expand MXFP4 weights to bf16 [N, K] (exact; code 8 reads +0.0).
    Same weight contract as mxfp4_linear."""
    N, K = _check_mxfp4_weight("mxfp4_dequant", w_packed, w_scale)
    if out is not None:
        _check_mxfp4_out("mxfp4_dequant", out, (N, K), w_packed.device)
    if w_packed.is_cuda:
        _require_native()
        if out is None:
            out = torch.empty((N, K), dtype=torch.bfloat16,
                              device=w_packed.device)
        _C.mxfp4_dequant(out, w_packed, w_scale)
        return out
    res = ref.mxfp4_dequant(w_packed, w_scale)
    if out is None:
        return res
    out.copy_(res)
    return out


def moe_gemm_mxfp4(out, a, w_packed, w_scale, sorted_ids, expert_ids, n_valid,
                   block_m: int, gate_up: bool):
    """Grouped W4A16 GEMM over block-aligned expert segments (the moe_gemm
    contract) with MXFP4 expert weights and bf16 activations.

    out [PM, N] bf16; a = x [T, K] (gate_up, rows gathered via sorted_ids)
    or act [PM, K]; w_packed [E, NB, K/2] and w_scale [E, NB, K/32] uint8
    hold each expert in the row format of mxfp4_linear (scale bytes in
    [8, 247], see validate_mxfp4_scales), NB = 2N when gate_up (gate rows,
    then up rows), else N. K % 128 == 0, N % 16 == 0, block_m 16 or 128.
    n_valid: device int32 scalar with the real m-tile count; tiles at or
    past it are not touched. gate_up=True fuses silu(gate) * up. Static
    grid, no host sync, no workspace: hipGraph-capturable. A row's bits
    depend only on its A row and its expert's weights, not on block_m, its
    slot or the rest of the batch. Unsupported input raises ValueError
    before any launch (no silent fallback)."""
    op = "moe_gemm_mxfp4"
    if block_m not in (16, 128):
        raise ValueError(f"{op}: block_m must be 16 or 128, got {block_m}")
    if out.dtype != torch.bfloat16 or a.dtype != torch.bfloat16:
        raise ValueError(
            f"{op}: out and a must be bf16, got {out.dtype} and {a.dtype}")
    if w_packed.dtype != torch.uint8 or w_scale.dtype != torch.uint8:
        raise ValueError(
            f"{op}: w_packed and w_scale must be uint8, got "
            f"{w_packed.dtype} and {w_scale.dtype}")
    if (sorted_ids.dtype != torch.int32 or expert_ids.dtype != torch.int32
            or n_valid.dtype != torch.int32):
        raise ValueError(
            f"{op}: sorted_ids, expert_ids and n_valid must be int32")
    if out.dim() != 2 or a.dim() != 2 or w_packed.dim() != 3 \
            or w_scale.dim() != 3 or sorted_ids.dim() != 1 \
            or expert_ids.dim() != 1 or n_valid.numel() != 1:
        raise ValueError(
            f"{op}: need out [PM, N], a [rows, K], w_packed [E, NB, K/2], "
            "w_scale [E, NB, K/32], sorted_ids [PM], expert_ids [PM/block_m] "
            "and a one-element n_valid")
    tensors = (out, a, w_packed, w_scale, sorted_ids, expert_ids, n_valid)
    if any(t.device != out.device for t in tensors):
        raise ValueError(f"{op}: all tensors must share one device")
    if not all(t.is_contiguous() for t in tensors):
        raise ValueError(f"{op}: all tensors must be contiguous")
    PM, N = out.shape
    K = a.shape[1]
    NB = 2 * N if gate_up else N
    if K < 128 or K % 128 != 0 or N < 16 or N % 16 != 0:
        raise ValueError(
            f"{op}: unsupported shape N={N} K={K} "
            "(need K % 128 == 0 and N % 16 == 0)")
    E = w_packed.shape[0]
    if E < 1 or tuple(w_packed.shape) != (E, NB, K // 2) \
            or tuple(w_scale.shape) != (E, NB, K // 32):
        raise ValueError(
            f"{op}: need w_packed [E, {NB}, {K // 2}] and w_scale "
            f"[E, {NB}, {K // 32}], got {tuple(w_packed.shape)} and "
            f"{tuple(w_scale.shape)}")
    if sorted_ids.numel() % block_m != 0 or sorted_ids.numel() != PM \
            or PM < block_m:
        raise ValueError(
            f"{op}: sorted_ids must hold PM = {PM} slots, a positive "
            f"multiple of block_m = {block_m}; got {sorted_ids.numel()}")
    if expert_ids.numel() < PM // block_m:
        raise ValueError(
            f"{op}: expert_ids must cover {PM // block_m} m-tiles, got "
            f"{expert_ids.numel()}")
    if a.shape[0] < 1 or (not gate_up and a.shape[0] != PM):
        raise ValueError(
            f"{op}: a must be [{PM}, {K}] without gate_up and have at least "
            f"one row with it, got {tuple(a.shape)}")
    if out.is_cuda:
        _require_native()
        _C.moe_gemm_mxfp4(out, a, w_packed, w_scale, sorted_ids, expert_ids,
                          n_valid, block_m, gate_up)
        return out
    return ref.moe_gemm_mxfp4(out, a, w_packed, w_scale, sorted_ids,
                              expert_ids, n_valid, block_m, gate_up)


# ---------------------------------------------------------------- sampling

def sample_tokens(logits, temperature, top_k, top_p, min_p, rng):
    """Fused sampling, one token per row: greedy when temperature == 0,
    otherwise temperature scaling, top-k (0 < k < V), top-p (p < 1),
    min-p (> 0) and a Philox4x32-10 draw keyed by rng[t] = (seed, offset).
    Fixed-point integer masses make the result a pure function of the row,
    its parameters and its rng pair (see reference.sample_row).

    logits [T, V] fp32, temperature / top_p / min_p [T] fp32, top_k [T]
    int32, rng [T, 2] int64. Returns [T] int64. One launch, static grid,
    no host sync. Shape or dtype mismatch raises ValueError."""
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(
            f"sample_tokens: logits must be [T >= 1, V >= 1], got "
            f"{tuple(logits.shape)}"
        )
    T = logits.shape[0]
    for name, t, dtype, shape in (
        ("logits", logits, torch.float32, tuple(logits.shape)),
        ("temperature", temperature, torch.float32, (T,)),
        ("top_k", top_k, torch.int32, (T,)),
        ("top_p", top_p, torch.float32, (T,)),
        ("min_p", min_p, torch.float32, (T,)),
        ("rng", rng, torch.int64, (T, 2)),
    ):
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(
                f"sample_tokens: {name} must be {dtype} {shape}, got "
                f"{t.dtype} {tuple(t.shape)}"
            )
        if t.device != logits.device:
            raise ValueError(f"sample_tokens: {name} is on {t.device}, "
                             f"logits on {logits.device}")
    if logits.is_cuda:
        _require_native()
        out = torch.empty(T, dtype=torch.int64, device=logits.device)
        _C.sample_tokens(
            out, logits.contiguous(), temperature.contiguous(),
            top_k.contiguous(), top_p.contiguous(), min_p.contiguous(),
            rng.contiguous(),
        )
        return out
    return ref.sample_tokens(logits, temperature, top_k, top_p, min_p, rng)


# ---------------------------------------------------------------- logprobs

LOGPROBS_MAX_TOP = 32  # kernel contract: the top list lives in LDS


def token_logprobs(logits, token_ids, num_top, width=LOGPROBS_MAX_TOP,
                   out=None):
    """Per row: the log-softmax value of one token and the top-k (id,
    logprob) pairs, with no host involvement.

    logits [T, V] fp32 contiguous, token_ids [T] int64, num_top [T] int32.
    Returns (chosen [T] fp32, top_ids [T, W] int32, top_lp [T, W] fp32)
    with W = width, 1 <= W <= LOGPROBS_MAX_TOP. Row t with num_top[t] < 0
    is skipped: its logits are not read and its outputs not written. For
    the others, with lp(i) = x_i - (m + log(sum(exp(x - m)))), m = max x:

        chosen[t] = lp(token_ids[t]), NaN for an id outside [0, V) (the id
            is range-checked before it is used as an index)
        k = min(num_top[t], W, V)
        top_ids[t, :k] = indices of the k largest logits in the order
            (logit descending, index ascending), -0.0 equal to +0.0: an
            exact function of the inputs
        top_lp[t, :k] = their logprobs; columns >= k get id -1 and -inf

    -inf logits are ordinary values (lp = -inf); a row without a finite
    entry gives -inf everywhere. NaN / +inf logits are outside the
    contract. The sum of exponentials runs in a fixed order: a row's bits
    depend only on the row and V.

    out = (chosen, top_ids, top_lp) writes into existing tensors, e.g.
    views of one buffer; `width` is then taken from top_ids. Without out=
    the outputs of skipped rows are uninitialised. One launch, static grid,
    no host sync. Shape, dtype, device or contiguity mismatch raises
    ValueError. On the CPU this is reference.token_logprobs."""
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(
            f"token_logprobs: logits must be [T >= 1, V >= 1], got "
            f"{tuple(logits.shape)}"
        )
    T, V = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError(
            "token_logprobs: logits must be contiguous fp32, got "
            f"{logits.dtype} strides {logits.stride()}"
        )
    if V >= 1 << 30:
        raise ValueError(f"token_logprobs: need V < 2^30, got {V}")
    if out is not None:
        if len(out) != 3 or out[1].dim() != 2:
            raise ValueError(
                "token_logprobs: out must be (chosen [T], top_ids [T, W], "
                "top_lp [T, W])"
            )
        width = out[1].shape[1]
    if not 1 <= width <= LOGPROBS_MAX_TOP:
        raise ValueError(
            f"token_logprobs: need 1 <= width <= {LOGPROBS_MAX_TOP}, got "
            f"{width}"
        )
    if out is None:
        out = (
            torch.empty(T, dtype=torch.float32, device=logits.device),
            torch.empty(T, width, dtype=torch.int32, device=logits.device),
            torch.empty(T, width, dtype=torch.float32, device=logits.device),
        )
    for name, t, dtype, shape in (
        ("token_ids", token_ids, torch.int64, (T,)),
        ("num_top", num_top, torch.int32, (T,)),
        ("chosen", out[0], torch.float32, (T,)),
        ("top_ids", out[1], torch.int32, (T, width)),
        ("top_lp", out[2], torch.float32, (T, width)),
    ):
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(
                f"token_logprobs: {name} must be {dtype} {shape}, got "
                f"{t.dtype} {tuple(t.shape)}"
            )
        if t.device != logits.device:
            raise ValueError(f"token_logprobs: {name} is on {t.device}, "
                             f"logits on {logits.device}")
        if not t.is_contiguous():
            raise ValueError(f"token_logprobs: {name} must be contiguous, "
                             f"got strides {t.stride()}")
    if logits.is_cuda:
        _require_native()
        _C.token_logprobs(out[0], out[1], out[2], logits, token_ids, num_top)
        return tuple(out)
    return ref.token_logprobs(logits, token_ids, num_top, tuple(out))


# ---------------------------------------------------------------- penalties

PENALTY_MAX_ROWS = 65535  # kernel contract: T is a grid extent


def _check_penalty_counts(op: str, counts) -> None:
    if (counts.dim() != 2 or counts.dtype != torch.int32
            or counts.shape[0] < 1 or counts.shape[1] < 1
            or not counts.is_contiguous()):
        raise ValueError(
            f"{op}: counts must be a contiguous [S >= 1, V >= 1] int32 "
            f"tensor, got {counts.dtype} {tuple(counts.shape)}"
        )


def apply_penalties(logits, counts, slot_ids, params):
    """Repetition / presence / frequency penalties, in place on logits.

    logits [T, V] fp32 contiguous, counts [S, V] int32 (row s = token
    histogram of the sequence that owns slot s), slot_ids [T] int32,
    params [T, 4] fp32 = (rp, inv_rp, presence, frequency) per row, with
    inv_rp = fp32(1 / rp), the quotient taken in double
    (engine.sampler.penalty_params). For a row with s = slot_ids[t] in
    [0, S) and every v with c = counts[s, v] > 0:

        x = x * inv_rp if x > 0 else x * rp     (rp != 1)
        x = x - presence                        (presence != 0)
        x = x - frequency * float(c)            (frequency != 0)

    each step rounded to fp32, the operation sequence of
    Sampler._apply_penalties (with the torch build this was tested on, the
    GPU division by a scalar multiplies by that reciprocal; see
    penalty_params). Rows with a slot outside [0, S) (canonically
    -1) and elements with count 0 are left bit-for-bit untouched. One
    launch, static grid, no host sync. Shape or dtype mismatch raises
    ValueError. On the CPU this runs the torch ops of the sampler."""
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(
            f"apply_penalties: logits must be [T >= 1, V >= 1], got "
            f"{tuple(logits.shape)}"
        )
    T, V = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError(
            "apply_penalties: logits must be contiguous fp32 (the op works "
            f"in place), got {logits.dtype} strides {logits.stride()}"
        )
    if T > PENALTY_MAX_ROWS or V >= 1 << 30:
        raise ValueError(
            f"apply_penalties: need T <= {PENALTY_MAX_ROWS} and V < 2^30, "
            f"got T={T} V={V}"
        )
    _check_penalty_counts("apply_penalties", counts)
    if counts.shape[1] != V:
        raise ValueError(
            f"apply_penalties: counts has {counts.shape[1]} columns, logits "
            f"{V}"
        )
    for name, t, dtype, shape in (
        ("slot_ids", slot_ids, torch.int32, (T,)),
        ("params", params, torch.float32, (T, 4)),
    ):
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(
                f"apply_penalties: {name} must be {dtype} {shape}, got "
                f"{t.dtype} {tuple(t.shape)}"
            )
    for name, t in (("counts", counts), ("slot_ids", slot_ids),
                    ("params", params)):
        if t.device != logits.device:
            raise ValueError(f"apply_penalties: {name} is on {t.device}, "
                             f"logits on {logits.device}")
    if logits.is_cuda:
        _require_native()
        _C.apply_penalties(logits, counts, slot_ids.contiguous(),
                           params.contiguous())
        return logits
    return ref.apply_penalties(logits, counts, slot_ids, params)


def penalty_counts_add(counts, slot_ids, token_ids):
    """counts[slot_ids[i], token_ids[i]] += 1 for every i, in place.

    counts [S, V] int32, slot_ids [N] int32, token_ids [N] int64. An entry
    whose slot is outside [0, S) or whose token is outside [0, V) is
    skipped (never used as an index). Integer atomics: duplicate tokens and
    slots count exactly, in any order. One launch, no host sync. Shape or
    dtype mismatch raises ValueError."""
    _check_penalty_counts("penalty_counts_add", counts)
    if counts.shape[1] >= 1 << 30:
        raise ValueError("penalty_counts_add: need V < 2^30")
    N = slot_ids.numel()
    if (slot_ids.dim() != 1 or N < 1 or slot_ids.dtype != torch.int32
            or token_ids.dtype != torch.int64
            or tuple(token_ids.shape) != (N,)):
        raise ValueError(
            "penalty_counts_add: slot_ids must be int32 [N >= 1] and "
            f"token_ids int64 [N], got {slot_ids.dtype} "
            f"{tuple(slot_ids.shape)} and {token_ids.dtype} "
            f"{tuple(token_ids.shape)}"
        )
    for name, t in (("slot_ids", slot_ids), ("token_ids", token_ids)):
        if t.device != counts.device:
            raise ValueError(f"penalty_counts_add: {name} is on {t.device}, "
                             f"counts on {counts.device}")
    if counts.is_cuda:
        _require_native()
        _C.penalty_counts_add(counts, slot_ids.contiguous(),
                              token_ids.contiguous())
        return counts
    return ref.penalty_counts_add(counts, slot_ids, token_ids)


# ------------------------------------------------- speculative verification

SPEC_MAX_DRAFT = 16  # kernel contract: draft ids per row live in LDS


def apply_penalties_spec(logits, counts, slot_ids, params, extra):
    """apply_penalties for the rows of speculative verification spans, in
    place on logits: row r also counts the draft tokens that precede it
    inside its span.

    logits [R, V] fp32 contiguous, counts [S, V] int32, slot_ids [R] int32,
    params [R, 4] fp32 as in apply_penalties, extra [R, E] int64 with
    1 <= E <= SPEC_MAX_DRAFT, padded with -1. The effective count of
    column v in row r is

        c = counts[slot_ids[r], v] + #{e : extra[r, e] == v}

    and an element with c > 0 is penalised exactly as in apply_penalties
    (same operations, same order, each rounded to fp32). Elements with
    c == 0 and rows whose slot is outside [0, S) are left bit-for-bit
    untouched; extra ids outside [0, V) (-1, V, 1 << 40) are ignored and
    never used as an index. counts is only read. One launch, static grid,
    no workspace, no host sync. Shape or dtype mismatch raises ValueError.
    On the CPU this is reference.apply_penalties_spec."""
    op = "apply_penalties_spec"
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(
            f"{op}: logits must be [R >= 1, V >= 1], got "
            f"{tuple(logits.shape)}"
        )
    T, V = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError(
            f"{op}: logits must be contiguous fp32 (the op works in place), "
            f"got {logits.dtype} strides {logits.stride()}"
        )
    if T > PENALTY_MAX_ROWS or V >= 1 << 30:
        raise ValueError(
            f"{op}: need R <= {PENALTY_MAX_ROWS} and V < 2^30, got R={T} "
            f"V={V}"
        )
    _check_penalty_counts(op, counts)
    if counts.shape[1] != V:
        raise ValueError(
            f"{op}: counts has {counts.shape[1]} columns, logits {V}"
        )
    if (extra.dim() != 2 or extra.dtype != torch.int64
            or extra.shape[0] != T
            or not 1 <= extra.shape[1] <= SPEC_MAX_DRAFT):
        raise ValueError(
            f"{op}: extra must be int64 [{T}, 1 <= E <= {SPEC_MAX_DRAFT}], "
            f"got {extra.dtype} {tuple(extra.shape)}"
        )
    for name, t, dtype, shape in (
        ("slot_ids", slot_ids, torch.int32, (T,)),
        ("params", params, torch.float32, (T, 4)),
    ):
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(
                f"{op}: {name} must be {dtype} {shape}, got {t.dtype} "
                f"{tuple(t.shape)}"
            )
    for name, t in (("counts", counts), ("slot_ids", slot_ids),
                    ("params", params), ("extra", extra)):
        if t.device != logits.device:
            raise ValueError(f"{op}: {name} is on {t.device}, logits on "
                             f"{logits.device}")
    if logits.is_cuda:
        _require_native()
        _C.apply_penalties_spec(logits, counts, slot_ids.contiguous(),
                                params.contiguous(), extra.contiguous())
        return logits
    return ref.apply_penalties_spec(logits, counts, slot_ids, params, extra)


def spec_accept_sections(buf: torch.Tensor, S: int, W: int):
    """(emitted [S, W] int64, n_emit [S] int32) as views of one int64
    buffer of spec_accept_words(S, W) elements."""
    return (
        buf[:S * W].view(S, W),
        buf[S * W:].view(torch.int32)[:S],
    )


def spec_accept_words(S: int, W: int) -> int:
    return S * W + (S + 1) // 2


def spec_accept(sampled, drafts, span_cu, width, out=None):
    """Draft acceptance for one verification pass, without the host.

    sampled [R] int64: the token drawn from the target distribution at each
    verification row. drafts [R] int64: the draft token checked at that
    row, -1 at the last (bonus) row of a span. span_cu [S + 1] int32: span
    s owns rows [cu[s], cu[s + 1]). width = W with 1 <= W <=
    SPEC_MAX_DRAFT + 1. Per span, with m the longest prefix on which
    sampled == drafts (the last row of a span always ends it):

        emitted[s, :m + 1] = sampled[cu[s] : cu[s] + m + 1], rest -1
        n_emit[s] = m + 1

    A span that is empty, longer than W rows or not inside [0, R) gets
    n_emit 0 and a row of -1, and indexes nothing. Returns (emitted [S, W]
    int64, n_emit [S] int32): two sections of ONE int64 buffer
    (spec_accept_sections), so that a single copy brings both to the host.
    out = that buffer (contiguous int64, spec_accept_words(S, W) elements)
    writes into an existing one. One launch, no host sync. Shape, dtype or
    device mismatch raises ValueError. On the CPU this is
    reference.spec_accept."""
    if (sampled.dim() != 1 or sampled.numel() < 1
            or sampled.dtype != torch.int64):
        raise ValueError(
            f"spec_accept: sampled must be int64 [R >= 1], got "
            f"{sampled.dtype} {tuple(sampled.shape)}"
        )
    R = sampled.numel()
    if R >= 1 << 31:
        raise ValueError("spec_accept: need R < 2^31")
    if drafts.dtype != torch.int64 or tuple(drafts.shape) != (R,):
        raise ValueError(
            f"spec_accept: drafts must be int64 ({R},), got {drafts.dtype} "
            f"{tuple(drafts.shape)}"
        )
    if (span_cu.dim() != 1 or span_cu.dtype != torch.int32
            or span_cu.numel() < 2):
        raise ValueError(
            f"spec_accept: span_cu must be int32 [S + 1 >= 2], got "
            f"{span_cu.dtype} {tuple(span_cu.shape)}"
        )
    S = span_cu.numel() - 1
    W = int(width)
    if not 1 <= W <= SPEC_MAX_DRAFT + 1:
        raise ValueError(
            f"spec_accept: need 1 <= width <= {SPEC_MAX_DRAFT + 1}, got {W}"
        )
    if S >= 1 << 24:
        raise ValueError("spec_accept: need S < 2^24")
    words = spec_accept_words(S, W)
    if out is None:
        out = torch.empty(words, dtype=torch.int64, device=sampled.device)
    elif (out.dtype != torch.int64 or tuple(out.shape) != (words,)
            or not out.is_contiguous()):
        raise ValueError(
            f"spec_accept: out must be a contiguous int64 ({words},) "
            f"tensor, got {out.dtype} {tuple(out.shape)}"
        )
    for name, t in (("drafts", drafts), ("span_cu", span_cu), ("out", out)):
        if t.device != sampled.device:
            raise ValueError(f"spec_accept: {name} is on {t.device}, "
                             f"sampled on {sampled.device}")
    emitted, n_emit = spec_accept_sections(out, S, W)
    if sampled.is_cuda:
        _require_native()
        _C.spec_accept(emitted, n_emit, sampled.contiguous(),
                       drafts.contiguous(), span_cu.contiguous())
        return emitted, n_emit
    return ref.spec_accept(sampled, drafts, span_cu, emitted, n_emit)


# ------------------------------------------------ logit_bias / grammar masks

def apply_logit_mods(logits, mask_ids=None, masks=None, bias_cu=None,
                     bias_ids=None, bias_vals=None):
    """logit_bias and packed grammar masks, in place on logits: bias, then
    mask (the order of the engine's host path).

    logits [T, V] fp32 contiguous. Either half may be absent (all of its
    arguments None); with both absent nothing is launched.

    Mask half: masks [M, W] int32 contiguous with W = ceil(V / 32); bit
    (v & 31) of word (v >> 5) set means token v is allowed; bits at
    positions >= V are ignored. mask_ids [T] int32 names each row's mask; an
    id outside [0, M) (canonically -1) means no mask and is never used as
    an index. Every disallowed element of a masked row becomes exactly -inf,
    whatever it held (NaN included) and whatever its bias.

    Bias half, CSR: bias_cu [T + 1] int32, bias_ids [B] int32, bias_vals [B]
    fp32. Row t does x = x + bias_vals[e] (one fp32 add, the host path's
    indexed add) for e in [bias_cu[t], bias_cu[t + 1]), clamped to [0, B).
    An id outside [0, V) is skipped and never used as an index. Ids within a
    row must be distinct; the host guarantees that (they are dict keys), the
    kernel does not check it, and a duplicate would make two threads race on
    one element.

    Allowed elements without a bias entry and rows with neither a mask nor
    a bias are left bit-for-bit untouched (not stored to). No element has
    two writers, so the result does not depend on workgroup order. One
    launch, static grid, no workspace, no host sync. Shape, dtype, device or
    contiguity mismatch raises ValueError. On the CPU this is
    reference.apply_logit_mods."""
    op = "apply_logit_mods"
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(
            f"{op}: logits must be [T >= 1, V >= 1], got "
            f"{tuple(logits.shape)}"
        )
    T, V = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError(
            f"{op}: logits must be contiguous fp32 (the op works in place), "
            f"got {logits.dtype} strides {logits.stride()}"
        )
    if T > PENALTY_MAX_ROWS or V >= 1 << 30:
        raise ValueError(
            f"{op}: need T <= {PENALTY_MAX_ROWS} and V < 2^30, got T={T} "
            f"V={V}"
        )
    has_mask = mask_ids is not None or masks is not None
    has_bias = any(x is not None for x in (bias_cu, bias_ids, bias_vals))
    if has_mask and (mask_ids is None or masks is None):
        raise ValueError(f"{op}: mask_ids and masks come together")
    if has_bias and any(x is None for x in (bias_cu, bias_ids, bias_vals)):
        raise ValueError(
            f"{op}: bias_cu, bias_ids and bias_vals come together")
    checks = []
    if has_mask:
        W = (V + 31) // 32
        if (masks.dim() != 2 or masks.dtype != torch.int32
                or masks.shape[0] < 1 or masks.shape[1] != W):
            raise ValueError(
                f"{op}: masks must be int32 [M >= 1, ceil(V / 32) = {W}], "
                f"got {masks.dtype} {tuple(masks.shape)}"
            )
        checks += [("mask_ids", mask_ids, torch.int32, (T,)),
                   ("masks", masks, torch.int32, tuple(masks.shape))]
    if has_bias:
        if bias_ids.dim() != 1 or bias_ids.numel() >= 1 << 30:
            raise ValueError(
                f"{op}: bias_ids must be [B < 2^30], got "
                f"{tuple(bias_ids.shape)}"
            )
        B = bias_ids.numel()
        checks += [("bias_cu", bias_cu, torch.int32, (T + 1,)),
                   ("bias_ids", bias_ids, torch.int32, (B,)),
                   ("bias_vals", bias_vals, torch.float32, (B,))]
    for name, t, dtype, shape in checks:
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise ValueError(
                f"{op}: {name} must be {dtype} {shape}, got {t.dtype} "
                f"{tuple(t.shape)}"
            )
        if t.device != logits.device:
            raise ValueError(f"{op}: {name} is on {t.device}, logits on "
                             f"{logits.device}")
        if not t.is_contiguous():
            raise ValueError(f"{op}: {name} must be contiguous, got strides "
                             f"{t.stride()}")
    if not checks:
        return logits
    if logits.is_cuda:
        _require_native()
        _C.apply_logit_mods(logits, mask_ids, masks, bias_cu, bias_ids,
                            bias_vals)
        return logits
    return ref.apply_logit_mods(logits, mask_ids, masks, bias_cu, bias_ids,
                                bias_vals)


compute_cos_sin_cache = ref.compute_cos_sin_cache
