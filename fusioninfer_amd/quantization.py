"""Quantized linear paths: FP8 (OCP e4m3, W8A8) and MXFP4 (W4A16, below).

gfx950 runs OCP fp8 MFMA at ~2x the bf16 rate and halves weight-read
bytes — decode-time GEMMs are weight-bandwidth-bound, so fp8 weights pay
there directly. Enabled per-engine with `--quantization fp8`: projection
weights are stored fp8 with per-output-channel scales; activations are
dynamically quantized per-token; the GEMM is hipBLASLt fp8 via
torch._scaled_mm with bf16 output. The flagship benchmark stays bf16
(BASELINE dtype contract); fp8 is an opt-in serving mode.

Note: gfx950 fp8 is OCP e4m3fn — NOT the MI300X fnuz variant
(guide cdna_hip_programming.md §4).
"""

from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from fusioninfer_amd.distributed import parallel_state as ps

FP8_DTYPE = torch.float8_e4m3fn
FP8_MAX = 448.0  # e4m3fn max normal


def quantize_weight_fp8(w: torch.Tensor):
    """Per-output-channel symmetric quantization: returns (w_fp8 [O, I],
    scale [O] fp32) with w ~= w_fp8 * scale[:, None]."""
    absmax = w.abs().amax(dim=1, keepdim=True).float().clamp(min=1e-8)
    scale = absmax / FP8_MAX
    w_fp8 = (w.float() / scale).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
    return w_fp8, scale.squeeze(1)


def quantize_activation_fp8(x: torch.Tensor):
    """Per-token dynamic quantization: (x_fp8 [T, I], scale [T] fp32)."""
    absmax = x.abs().amax(dim=1, keepdim=True).float().clamp(min=1e-8)
    scale = absmax / FP8_MAX
    x_fp8 = (x.float() / scale).clamp(-FP8_MAX, FP8_MAX).to(FP8_DTYPE)
    return x_fp8, scale.squeeze(1)


def fp8_linear(x, w_fp8: torch.Tensor, w_scale: torch.Tensor):
    """y[T, O] = x @ W^T with fp8 operands, bf16 output.

    `x` is either a bf16 tensor (quantized here, one fused HIP kernel on
    GPU) or an (x_fp8, x_scale) tuple already produced by a fused epilogue
    (rms_norm_fp8 / silu_and_mul_fp8 / quant_fp8_rows)."""
    if isinstance(x, tuple):
        x_fp8, x_scale = x
    elif x.is_cuda:
        from fusioninfer_amd import ops

        x_fp8, x_scale = ops.quant_fp8_rows(x)
    else:
        x_fp8, x_scale = None, None  # CPU: keep the bf16 tensor
    if x_fp8 is not None and x_fp8.is_cuda:
        return torch._scaled_mm(
            x_fp8,
            w_fp8.t(),  # [I, O], column-major view of the row-major weight
            scale_a=x_scale.unsqueeze(1),
            scale_b=w_scale.unsqueeze(0),
            out_dtype=torch.bfloat16,
        )
    # CPU reference path (tests): dequantize and matmul in fp32
    if x_fp8 is not None:  # tuple input on CPU
        x = x_fp8.float() * x_scale.unsqueeze(1).float()
    w = w_fp8.float() * w_scale.unsqueeze(1).float()
    return (x.float() @ w.t()).to(torch.bfloat16)


def convert_linear_to_fp8(module: nn.Module) -> int:
    """Convert every projection Linear in a CausalLM to fp8 storage.
    Returns the number of converted layers. lm_head/embedding stay bf16
    (vocab-scale accuracy)."""
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )

    converted = 0
    for m in module.modules():
        if isinstance(m, (MergedColumnParallelLinear, RowParallelLinear)):
            w_fp8, scale = quantize_weight_fp8(m.weight.data)
            m.weight = nn.Parameter(w_fp8, requires_grad=False)
            m.register_buffer("weight_scale", scale, persistent=False)
            m.forward = _make_fp8_forward(m)
            converted += 1
    return converted


# ------------------------------------------------------------------ MXFP4
#
# Weight-only 4-bit mode (`--quantization mxfp4`): projection weights are
# stored as OCP Microscaling MXFP4 along K — e2m1 elements (1 sign, 2
# exponent, 1 mantissa bit; magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6}), two per
# byte with k even in the low nibble, and one e8m0 scale byte 2^(s - 127) per
# 32 consecutive k of an output row: 4.25 bits per weight. Activations stay
# bf16. Scale bytes are confined to [8, 247] — the quantiser clamps to it and
# validate_mxfp4_scales rejects anything else, 0xFF (NaN) included — so every
# dequantised value is zero or a normal bf16 and dequantisation is exact: the
# W4A16 GEMM is "a bf16 GEMM with fp32 accumulation on dequant(W)".

MXFP4_BLOCK = 32
# Largest M served by the weight-streaming HIP GEMM (ops.mxfp4_linear);
# larger batches expand the weight into the shared bf16 scratch and call the
# library GEMM. The streaming kernel re-reads x once per column tile, so it
# loses once x traffic outweighs the 4x smaller weight read. Measured on
# the Qwen3-8B shapes (profiles/r12_mxfp4.md): it beats dequant + F.linear
# on all four up to M = 32; at M = 64 it loses on down_proj (K = 12288).
MXFP4_MAX_M = int(os.environ.get("FI_MXFP4_MAX_M", "32"))


def validate_mxfp4_scales(weight_scale: torch.Tensor) -> None:
    """Raise ValueError on an e8m0 scale byte outside [8, 247]. Host-side
    (synchronises on a GPU tensor); runs at conversion or load time only."""
    from fusioninfer_amd import ops

    ops.validate_mxfp4_scales(weight_scale)


def quantize_weight_mxfp4(w: torch.Tensor):
    """[N, K] -> (packed [N, K/2] uint8, scale [N, K/32] uint8). Per 32-k
    block: amax in fp32; s = 127 for an all-zero block, else
    clamp(floor(log2(amax)) - 2 + 127, 8, 247) (2 = e2m1's emax, as in the
    OCP spec); elements are w / 2^(s - 127) rounded to the nearest grid
    point, ties to the code with even mantissa bit, saturating at +-6.
    Zeros are stored as code 0, never as negative zero."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK != 0:
        raise ValueError(
            f"quantize_weight_mxfp4: need [N, K] with K % 32 == 0, got "
            f"{tuple(w.shape)}")
    wf = w.float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_weight_mxfp4: non-finite weight")
    N, K = wf.shape
    blocks = wf.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = blocks.abs().amax(dim=-1)
    # amax = m * 2^e with m in [0.5, 1): floor(log2(amax)) = e - 1, exactly
    _, e = torch.frexp(amax)
    s = (e.to(torch.int32) - 1 - 2 + 127).clamp(8, 247)
    s = torch.where(amax == 0, torch.full_like(s, 127), s)
    # 2^(127 - s) from its bit pattern: the scaling below is exact
    inv = ((254 - s) << 23).view(torch.float32)
    a = (blocks * inv.unsqueeze(-1)).abs()
    # midpoints of the grid; a tie goes to the neighbour with mantissa bit 0
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8)
            + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
            + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
            + (a > 5.0).to(torch.uint8))
    code = code | (((blocks < 0) & (code > 0)).to(torch.uint8) << 3)
    code = code.view(N, K // 2, 2)
    packed = code[..., 0] | (code[..., 1] << 4)
    return packed.contiguous(), s.to(torch.uint8).contiguous()


def dequantize_mxfp4(packed: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """Exact inverse map of the format: bf16 [N, K]."""
    from fusioninfer_amd.ops import reference

    return reference.mxfp4_dequant(packed, scale)


class _Mxfp4Scratch:
    """One bf16 buffer shared by every converted layer of a model, sized to
    the largest of them, for the large-M path (dequant, then library GEMM).
    Allocated once at conversion, so its address is stable for captured
    graphs and the KV-cache sizing sees it. Sharing it assumes all model
    forwards run on one stream: a layer's GEMM must finish reading the
    buffer before the next layer's dequant overwrites it, which stream
    order gives and concurrent streams would not."""

    def __init__(self):
        self.buf = None

    def reserve(self, numel: int, device) -> None:
        self.buf = torch.empty(numel, dtype=torch.bfloat16, device=device)

    def view(self, n: int, k: int) -> torch.Tensor:
        return self.buf[: n * k].view(n, k)


def convert_linear_to_mxfp4(module: nn.Module) -> int:
    """Convert every projection Linear in a CausalLM to MXFP4 storage:
    `weight` is replaced by the buffers `weight_packed` [N, K/2] and
    `weight_scale` [N, K/32] and the bf16 tensor is freed. Returns the
    number of converted layers. lm_head/embedding stay bf16."""
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )

    layers = [
        m for m in module.modules()
        if isinstance(m, (MergedColumnParallelLinear, RowParallelLinear))
    ]
    for m in layers:  # reject before anything is converted
        N, K = m.weight.shape
        if K % 128 != 0 or N % 16 != 0:
            what = ("in_per_rank" if isinstance(m, RowParallelLinear)
                    else "in_features")
            raise ValueError(
                f"mxfp4: {type(m).__name__} shard [{N}, {K}] is unsupported: "
                f"{what} must be a multiple of 128 and the output rows a "
                "multiple of 16")
    scratch = _Mxfp4Scratch()
    if layers and layers[0].weight.is_cuda:
        scratch.reserve(max(m.weight.numel() for m in layers),
                        layers[0].weight.device)
    for m in layers:
        w = m.weight.data
        packed, scale = quantize_weight_mxfp4(w)
        validate_mxfp4_scales(scale)
        del m.weight
        m.register_buffer("weight_packed", packed, persistent=False)
        m.register_buffer("weight_scale", scale, persistent=False)
        m.forward = _make_mxfp4_forward(m, scratch)
    return len(layers)


def convert_moe_experts_to_mxfp4(module: nn.Module) -> int:
    """Convert the experts of every MoEMLP in a CausalLM to MXFP4 storage.

    Each expert is quantised on its [O, I] view (the transpose of
    gate_up_t[e] / down_t[e]), one expert at a time, into the buffers
    gate_up_packed [E, 2I, H/2], gate_up_scale [E, 2I, H/32], down_packed
    [E, H, I/2] and down_scale [E, H, I/32] (gate rows first, then up rows:
    the order of cat([gate, up])). The bf16 parameters become zero-expert
    stand-ins that keep shape[1:], the MFMA pack cache is dropped, and
    `mlp.mxfp4` is set: nothing bf16 of the experts stays resident. Returns
    the number of converted layers."""
    from fusioninfer_amd.models.model import MoEMLP

    mlps = [m for m in module.modules() if isinstance(m, MoEMLP)]
    for m in mlps:  # reject before anything is converted
        if m.fp8 or m.mxfp4:
            raise ValueError(
                f"mxfp4: the experts of layer {m.layer_idx} are not bf16")
        H, inter = m.gate_up_t.shape[1], m.down_t.shape[1]
        if H % 128 != 0 or inter % 128 != 0:
            raise ValueError(
                f"mxfp4: MoE layer {m.layer_idx} experts [hidden_size={H}, "
                f"moe_intermediate_size={inter}] are unsupported: both must "
                "be multiples of 128")
    for m in mlps:
        m.ensure_unpacked()
        E, H, inter2 = m.gate_up_t.shape
        inter = inter2 // 2
        dev = m.gate_up_t.device

        def new(*shape):
            return torch.empty(shape, dtype=torch.uint8, device=dev)

        gu_p, gu_s = new(E, inter2, H // 2), new(E, inter2, H // 32)
        dn_p, dn_s = new(E, H, inter // 2), new(E, H, inter // 32)
        for e in range(E):
            gu_p[e], gu_s[e] = quantize_weight_mxfp4(
                m.gate_up_t.data[e].t().contiguous())
            dn_p[e], dn_s[e] = quantize_weight_mxfp4(
                m.down_t.data[e].t().contiguous())
        validate_mxfp4_scales(gu_s)
        validate_mxfp4_scales(dn_s)
        m._pack_cache = None
        m._pack_version = None
        for p in (m.gate_up_t, m.down_t):
            p.data = p.data.new_empty((0,) + tuple(p.shape[1:]))
        m.register_buffer("gate_up_packed", gu_p, persistent=False)
        m.register_buffer("gate_up_scale", gu_s, persistent=False)
        m.register_buffer("down_packed", dn_p, persistent=False)
        m.register_buffer("down_scale", dn_s, persistent=False)
        m.mxfp4 = True
    return len(mlps)


def _make_mxfp4_forward(m, scratch):
    from fusioninfer_amd import ops

    is_row_parallel = hasattr(m, "in_per_rank")
    bias = getattr(m, "bias", None)
    N, K = m.weight_packed.shape[0], m.weight_packed.shape[1] * 2

    def fwd(x):
        x = x.contiguous()
        if x.is_cuda and x.shape[0] > MXFP4_MAX_M:
            w = ops.mxfp4_dequant(m.weight_packed, m.weight_scale,
                                  out=scratch.view(N, K))
            out = F.linear(x, w, bias)
        else:
            out = ops.mxfp4_linear(x, m.weight_packed, m.weight_scale, bias)
        if is_row_parallel:
            out = ps.tp_all_reduce(out)
        return out

    return fwd


def _make_fp8_forward(m):
    is_row_parallel = hasattr(m, "in_per_rank")
    bias = getattr(m, "bias", None)

    def fwd(x):
        out = fp8_linear(x, m.weight, m.weight_scale)
        if bias is not None:
            out = out + bias
        if is_row_parallel:
            out = ps.tp_all_reduce(out)
        return out

    return fwd
