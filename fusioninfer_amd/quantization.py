"""Quantized linear paths: FP8 (OCP e4m3, W8A8), MXFP4 and int4 (W4A16, below).

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
from fusioninfer_amd.ops import INT4_GROUP_SIZES, validate_int4_scales

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
#
# `--mxfp4-activations mxfp8` (opt-in) changes only the batches above
# MXFP4_MAX_M rows: activations are quantised to MXFP8 (e4m3, one e8m0 scale
# per 32 k) and multiplied with the packed weights by the scaled-MFMA HIP
# GEMM (ops.mxfp4_mxfp8_linear), instead of dequant + library GEMM.

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


MXFP4_ACTIVATIONS = ("bf16", "mxfp8")
# the experts also take "mxfp8-wide": the scaled-MFMA GEMM from
# MXFP4_MOE_WIDE_LO routed rows per expert on, at block_m 32 below
# MXFP4_MOE_WIDE_HI (models/model.py)
MXFP4_MOE_ACTIVATIONS = MXFP4_ACTIVATIONS + ("mxfp8-wide",)


def convert_linear_to_mxfp4(module: nn.Module, activations: str = "bf16") -> int:
    """Convert every projection Linear in a CausalLM to MXFP4 storage:
    `weight` is replaced by the buffers `weight_packed` [N, K/2] and
    `weight_scale` [N, K/32] and the bf16 tensor is freed. Returns the
    number of converted layers. lm_head/embedding stay bf16.

    `activations` picks the path of batches above MXFP4_MAX_M rows: "bf16"
    expands the layer into the shared bf16 scratch and calls the library
    GEMM; "mxfp8" quantises the activations to MXFP8 and runs the
    scaled-MFMA HIP GEMM on the packed weights, so no scratch is reserved."""
    if activations not in MXFP4_ACTIVATIONS:
        raise ValueError(
            f"mxfp4: activations must be one of {MXFP4_ACTIVATIONS}, got "
            f"{activations!r}")
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
    if activations == "bf16" and layers and layers[0].weight.is_cuda:
        scratch.reserve(max(m.weight.numel() for m in layers),
                        layers[0].weight.device)
    for m in layers:
        w = m.weight.data
        packed, scale = quantize_weight_mxfp4(w)
        validate_mxfp4_scales(scale)
        del m.weight
        m.register_buffer("weight_packed", packed, persistent=False)
        m.register_buffer("weight_scale", scale, persistent=False)
        m.forward = _make_mxfp4_forward(m, scratch, activations)
    return len(layers)


def convert_moe_experts_to_mxfp4(module: nn.Module,
                                 activations: str = "bf16") -> int:
    """Convert the experts of every MoEMLP in a CausalLM to MXFP4 storage.

    `activations` is recorded on each MoEMLP (`mlp.mxfp4_activations`) and
    picks the path of batches routed at block_m 128: "bf16" is the grouped
    W4A16 GEMM, "mxfp8" the grouped scaled-MFMA GEMM on MXFP8 activations
    (ops.moe_gemm_mxfp4_mxfp8), which needs hidden_size and
    moe_intermediate_size to be multiples of 128 like the storage itself.
    "mxfp8-wide" runs that GEMM on mid-size batches too, at block_m 32
    (MoEMLP._forward_mxfp4_grouped has the rule).

    Each expert is quantised on its [O, I] view (the transpose of
    gate_up_t[e] / down_t[e]), one expert at a time, into the buffers
    gate_up_packed [E, 2I, H/2], gate_up_scale [E, 2I, H/32], down_packed
    [E, H, I/2] and down_scale [E, H, I/32] (gate rows first, then up rows:
    the order of cat([gate, up])). The bf16 parameters become zero-expert
    stand-ins that keep shape[1:], the MFMA pack cache is dropped, and
    `mlp.mxfp4` is set: nothing bf16 of the experts stays resident. Returns
    the number of converted layers."""
    from fusioninfer_amd.models.model import MoEMLP

    if activations not in MXFP4_MOE_ACTIVATIONS:
        raise ValueError(
            "mxfp4: MoE activations must be one of "
            f"{MXFP4_MOE_ACTIVATIONS}, got "
            f"{activations!r}")
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
        m.mxfp4_activations = activations
    return len(mlps)


def _make_mxfp4_forward(m, scratch, activations="bf16"):
    from fusioninfer_amd import ops

    is_row_parallel = hasattr(m, "in_per_rank")
    bias = getattr(m, "bias", None)
    N, K = m.weight_packed.shape[0], m.weight_packed.shape[1] * 2

    def fwd(x):
        x = x.contiguous()
        if activations == "mxfp8" and x.shape[0] > MXFP4_MAX_M:
            # GPU: two HIP kernels; CPU: their reference ops
            x_q, x_scale = ops.quant_mxfp8_rows(x)
            out = ops.mxfp4_mxfp8_linear(x_q, x_scale, m.weight_packed,
                                         m.weight_scale, bias)
        elif x.is_cuda and x.shape[0] > MXFP4_MAX_M:
            w = ops.mxfp4_dequant(m.weight_packed, m.weight_scale,
                                  out=scratch.view(N, K))
            out = F.linear(x, w, bias)
        else:
            out = ops.mxfp4_linear(x, m.weight_packed, m.weight_scale, bias)
        if is_row_parallel:
            out = ps.tp_all_reduce(out)
        return out

    return fwd


# ------------------------------------------------------------------- int4
#
# Weight-only 4-bit mode for AWQ / GPTQ style weights (`--quantization
# int4`): unsigned 4-bit codes q along K, two per byte with k even in the low
# nibble (the MXFP4 nibble convention, so shards concatenate and slice the
# same way), and per group of G = 32, 64 or 128 consecutive k of an output
# row one fp16 scale s and one zero point z in 0..15:
#
#     dq(W)[n, k] = bf16_rne( fp32(q - z) * fp32(s) )
#
# The fp32 product is exact, so dq has exactly one rounding, and the W4A16
# GEMM is "a bf16 GEMM with fp32 accumulation on dq(W)". Scales stay fp16
# because checkpoints store fp16. 4 + 24 / G bits per weight.

# Largest M served by the weight-streaming HIP GEMM (ops.int4_linear);
# larger batches expand the weight into the shared bf16 scratch and call the
# library GEMM. Measured on the Qwen3-8B shapes (profiles/r19_int4.md): it
# beats dequant + F.linear on all four in every repetition up to M = 16; at
# M = 32 it loses on down_proj (K = 12288: 71 us against 57 us), where the
# M <= 32 instance fills only 64 workgroups. mxfp4's threshold is 32: the
# integer expansion costs 18 VALU per 8 codes against 4 converts.
INT4_MAX_M = int(os.environ.get("FI_INT4_MAX_M", "16"))


def quantize_weight_int4(w: torch.Tensor, group_size: int = 128):
    """[N, K] -> (packed [N, K/2] uint8, scale [N, K/G] fp16, zero [N, K/G]
    uint8): asymmetric, per group of G consecutive k, all in fp32:

        wmin = min(group, 0), wmax = max(group, 0)
        s = fp16(max(wmax - wmin, tiny) / 15), clamped to fp16's normal range
            [2^-14, 65504], with tiny = 15 * 2^-14
        z = clamp(round(-wmin / s), 0, 15)
        q = clamp(round(w / s) + z, 0, 15)

    where s in the last two lines is the stored fp16 value and round is to
    nearest, ties to even. The range is widened to contain 0, so a group of
    one sign (a constant group included) is covered by the grid instead of
    saturating, and 0 itself is always exact (q == z). Within a group
    |w - dq| <= s / 2, plus 15 s 2^-11 for the fp16 rounding of s (the top
    code can clamp from 16) and the bf16 rounding of dq. An all-zero group
    gets the smallest normal scale and q == z == 0."""
    if group_size not in INT4_GROUP_SIZES:
        raise ValueError(
            f"quantize_weight_int4: group_size must be one of "
            f"{INT4_GROUP_SIZES}, got {group_size!r}")
    if w.dim() != 2 or w.shape[1] % group_size != 0:
        raise ValueError(
            f"quantize_weight_int4: need [N, K] with K % {group_size} == 0, "
            f"got {tuple(w.shape)}")
    wf = w.float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_weight_int4: non-finite weight")
    N, K = wf.shape
    groups = wf.view(N, K // group_size, group_size)
    wmin = groups.amin(dim=-1).clamp(max=0.0)
    wmax = groups.amax(dim=-1).clamp(min=0.0)
    tiny = 15.0 * 2.0 ** -14
    s16 = ((wmax - wmin).clamp(min=tiny) / 15.0).clamp(
        2.0 ** -14, 65504.0).to(torch.float16)
    s = s16.float()
    z = torch.round(-wmin / s).clamp(0, 15)
    q = (torch.round(groups / s.unsqueeze(-1)) + z.unsqueeze(-1)).clamp(0, 15)
    q = q.to(torch.uint8).view(N, K // 2, 2)
    packed = q[..., 0] | (q[..., 1] << 4)
    return (packed.contiguous(), s16.contiguous(),
            z.to(torch.uint8).contiguous())


def dequantize_int4(packed: torch.Tensor, scale: torch.Tensor,
                    zero: torch.Tensor, group_size: int) -> torch.Tensor:
    """The format's dq: bf16 [N, K]."""
    from fusioninfer_amd.ops import reference

    return reference.int4_dequant(packed, scale, zero, group_size)


def _unpack_int32_nibbles(t: torch.Tensor, order) -> torch.Tensor:
    """[R, C] int32 -> [R, 8 C] uint8: output column 8 c + order[i] is nibble
    i (bits 4 i ... + 3) of t[:, c]."""
    shifts = torch.arange(0, 32, 4, dtype=torch.int32)
    nib = ((t.unsqueeze(-1) >> shifts) & 0xF).to(torch.uint8)  # [R, C, 8]
    out = torch.empty_like(nib)
    out[..., list(order)] = nib
    return out.reshape(t.shape[0], -1)


def _pack_rows(codes_nk: torch.Tensor) -> torch.Tensor:
    N, K = codes_nk.shape
    c = codes_nk.reshape(N, K // 2, 2)
    return (c[..., 0] | (c[..., 1] << 4)).contiguous()


def _check_ckpt(name, qweight, qzeros, scales):
    if qweight.dtype != torch.int32 or qzeros.dtype != torch.int32:
        raise ValueError(f"{name}: qweight and qzeros must be int32")
    if scales.dtype != torch.float16:
        raise ValueError(f"{name}: scales must be float16")
    if qweight.dim() != 2 or qzeros.dim() != 2 or scales.dim() != 2:
        raise ValueError(f"{name}: qweight, qzeros and scales must be 2-D")


AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)


def int4_from_awq(qweight, qzeros, scales):
    """AWQ (GEMM layout) -> (weight_packed, weight_scale, weight_zero).
    qweight [K, N/8] int32, qzeros [K/G, N/8] int32, scales [K/G, N] fp16;
    nibble i of a word holds output column 8 c + (0, 2, 4, 6, 1, 3, 5, 7)[i].
    Pure torch on the CPU, exact."""
    _check_ckpt("int4_from_awq", qweight, qzeros, scales)
    K, N = qweight.shape[0], qweight.shape[1] * 8
    ng = scales.shape[0]
    if (ng == 0 or K % ng != 0 or tuple(scales.shape) != (ng, N)
            or tuple(qzeros.shape) != (ng, N // 8)):
        raise ValueError(
            f"int4_from_awq: inconsistent shapes qweight "
            f"{tuple(qweight.shape)}, qzeros {tuple(qzeros.shape)}, scales "
            f"{tuple(scales.shape)}")
    codes = _unpack_int32_nibbles(qweight.cpu(), AWQ_ORDER)  # [K, N]
    zeros = _unpack_int32_nibbles(qzeros.cpu(), AWQ_ORDER)   # [K/G, N]
    return (_pack_rows(codes.t().contiguous()),
            scales.cpu().t().contiguous(), zeros.t().contiguous())


def check_trivial_g_idx(g_idx, group_size: int, what: str) -> None:
    """Raise ValueError unless g_idx[k] == k // group_size for every k."""
    g = g_idx.cpu().to(torch.int64).view(-1)
    if not torch.equal(g, torch.arange(g.numel()) // group_size):
        raise ValueError(
            f"{what}: g_idx is not k // group_size: act-order (desc_act) "
            "checkpoints are not supported")


def int4_from_gptq(qweight, qzeros, scales, g_idx=None):
    """GPTQ (v1) -> (weight_packed, weight_scale, weight_zero). qweight
    [K/8, N] int32 with nibble i of word r holding k = 8 r + i, qzeros
    [K/G, N/8] int32 sequential along N and stored as z - 1, scales [K/G, N]
    fp16. `g_idx` must be None or the trivial k // G: act-order checkpoints
    are refused. A stored zero of 15 (z = 16) is not representable and raises.
    Pure torch on the CPU, exact."""
    _check_ckpt("int4_from_gptq", qweight, qzeros, scales)
    K, N = qweight.shape[0] * 8, qweight.shape[1]
    ng = scales.shape[0]
    if (ng == 0 or K % ng != 0 or tuple(scales.shape) != (ng, N) or N % 8 != 0
            or tuple(qzeros.shape) != (ng, N // 8)):
        raise ValueError(
            f"int4_from_gptq: inconsistent shapes qweight "
            f"{tuple(qweight.shape)}, qzeros {tuple(qzeros.shape)}, scales "
            f"{tuple(scales.shape)}")
    if g_idx is not None:
        check_trivial_g_idx(g_idx, K // ng, "int4_from_gptq")
    seq = tuple(range(8))
    # [N, K/8] words along K -> codes [N, K]
    codes = _unpack_int32_nibbles(qweight.cpu().t().contiguous(), seq)
    zeros = _unpack_int32_nibbles(qzeros.cpu(), seq).to(torch.int32) + 1
    if int(zeros.max()) > 15:
        raise ValueError(
            "int4_from_gptq: a stored zero point of 15 means z = 16, which "
            "the int4 format cannot hold")
    return (_pack_rows(codes), scales.cpu().t().contiguous(),
            zeros.to(torch.uint8).t().contiguous())


def _int4_layers(module: nn.Module, group_size: int):
    """The projection layers of a CausalLM, after checking every shard."""
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )

    if group_size not in INT4_GROUP_SIZES:
        raise ValueError(
            f"int4: group_size must be one of {INT4_GROUP_SIZES}, got "
            f"{group_size!r}")
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
                f"int4: {type(m).__name__} shard [{N}, {K}] is unsupported: "
                f"{what} must be a multiple of 128 and the output rows a "
                "multiple of 16")
    return layers


def convert_linear_to_int4(module: nn.Module, group_size: int = 128,
                           quantize: bool = True) -> int:
    """Convert every projection Linear in a CausalLM to int4 storage:
    `weight` is replaced by the buffers `weight_packed` [N, K/2],
    `weight_scale` [N, K/G] fp16 and `weight_zero` [N, K/G] and the bf16
    tensor is freed. Returns the number of converted layers.
    lm_head/embedding stay bf16. One bf16 scratch, sized to the largest
    layer, is reserved for the batches above INT4_MAX_M rows.

    With quantize=False the buffers are allocated but left unfilled, for a
    loader that copies pre-quantised checkpoint tensors into them
    (models/weight_loader.py)."""
    layers = _int4_layers(module, group_size)
    scratch = _Mxfp4Scratch()
    if layers and layers[0].weight.is_cuda:
        scratch.reserve(max(m.weight.numel() for m in layers),
                        layers[0].weight.device)
    for m in layers:
        w = m.weight.data
        N, K = w.shape
        if quantize:
            packed, scale, zero = quantize_weight_int4(w, group_size)
            validate_int4_scales(scale, zero)
        else:
            packed = torch.zeros((N, K // 2), dtype=torch.uint8,
                                 device=w.device)
            scale = torch.ones((N, K // group_size), dtype=torch.float16,
                               device=w.device)
            zero = torch.zeros((N, K // group_size), dtype=torch.uint8,
                               device=w.device)
        del m.weight
        m.register_buffer("weight_packed", packed, persistent=False)
        m.register_buffer("weight_scale", scale, persistent=False)
        m.register_buffer("weight_zero", zero, persistent=False)
        m.int4_group_size = group_size
        m.forward = _make_int4_forward(m, scratch, group_size)
    return len(layers)


def convert_moe_experts_to_int4(module: nn.Module,
                                group_size: int = 128) -> int:
    """Convert the experts of every MoEMLP in a CausalLM to int4 storage, the
    int4 counterpart of convert_moe_experts_to_mxfp4.

    Each expert is quantised on its [O, I] view (the transpose of
    gate_up_t[e] / down_t[e]) with quantize_weight_int4, one expert at a
    time, into the buffers gate_up_packed [E, 2I, H/2], gate_up_scale and
    gate_up_zero [E, 2I, H/G], down_packed [E, H, I/2], down_scale and
    down_zero [E, H, I/G] (gate rows first, then up rows). hidden_size and
    moe_intermediate_size must be multiples of 128. The bf16 parameters
    become zero-expert stand-ins that keep shape[1:], the MFMA pack cache is
    dropped, and `mlp.int4` / `mlp.int4_group_size` are set: nothing bf16 of
    the experts stays resident. Returns the number of converted layers."""
    from fusioninfer_amd.models.model import MoEMLP

    if group_size not in INT4_GROUP_SIZES:
        raise ValueError(
            f"int4: group_size must be one of {INT4_GROUP_SIZES}, got "
            f"{group_size!r}")
    mlps = [m for m in module.modules() if isinstance(m, MoEMLP)]
    for m in mlps:  # reject before anything is converted
        if m.fp8 or m.mxfp4 or m.int4:
            raise ValueError(
                f"int4: the experts of layer {m.layer_idx} are not bf16")
        H, inter = m.gate_up_t.shape[1], m.down_t.shape[1]
        if H % 128 != 0 or inter % 128 != 0:
            raise ValueError(
                f"int4: MoE layer {m.layer_idx} experts [hidden_size={H}, "
                f"moe_intermediate_size={inter}] are unsupported: both must "
                "be multiples of 128")
    for m in mlps:
        m.ensure_unpacked()
        E = m.gate_up_t.shape[0]
        for name, p in (("gate_up", m.gate_up_t), ("down", m.down_t)):
            parts = [quantize_weight_int4(p.data[e].t().contiguous(),
                                          group_size) for e in range(E)]
            packed, scale, zero = (torch.stack(t) for t in zip(*parts))
            validate_int4_scales(scale, zero)
            m.register_buffer(f"{name}_packed", packed, persistent=False)
            m.register_buffer(f"{name}_scale", scale, persistent=False)
            m.register_buffer(f"{name}_zero", zero, persistent=False)
        m._pack_cache = None
        m._pack_version = None
        for p in (m.gate_up_t, m.down_t):
            p.data = p.data.new_empty((0,) + tuple(p.shape[1:]))
        m.int4 = True
        m.int4_group_size = group_size
    return len(mlps)


def _make_int4_forward(m, scratch, group_size):
    from fusioninfer_amd import ops

    is_row_parallel = hasattr(m, "in_per_rank")
    bias = getattr(m, "bias", None)
    N, K = m.weight_packed.shape[0], m.weight_packed.shape[1] * 2

    def fwd(x):
        x = x.contiguous()
        if x.is_cuda and x.shape[0] > INT4_MAX_M:
            w = ops.int4_dequant(m.weight_packed, m.weight_scale,
                                 m.weight_zero, group_size,
                                 out=scratch.view(N, K))
            out = F.linear(x, w, bias)
        else:
            out = ops.int4_linear(x, m.weight_packed, m.weight_scale,
                                  m.weight_zero, group_size, bias)
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
