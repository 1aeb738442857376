"""MXFP4 weight-only mode: format, quantiser, conversion, CPU engine, CLI.

Dequantisation is exact in bf16 (a 3-bit significand times a power of two
with scale bytes in [8, 247]), so every check here is an equality."""

import math

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q

GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


# ------------------------------------------------------------------ layout

def test_hand_written_byte_low_nibble_first():
    packed = torch.tensor([[0x21] + [0] * 15], dtype=torch.uint8)
    scale = torch.tensor([[127]], dtype=torch.uint8)
    dq = Q.dequantize_mxfp4(packed, scale)
    assert dq.dtype == torch.bfloat16 and dq.shape == (1, 32)
    assert dq[0, :2].tolist() == [0.5, 1.0]
    assert torch.equal(dq, ref.mxfp4_dequant(packed, scale))


@pytest.mark.parametrize("s", [8, 126, 127, 128, 247])
def test_all_codes_times_scale_exact(s):
    # byte j = code j in the low nibble, code 15 - j in the high nibble
    row = [c | ((15 - c) << 4) for c in range(16)]
    packed = torch.tensor([row], dtype=torch.uint8)
    scale = torch.tensor([[s]], dtype=torch.uint8)
    dq = Q.dequantize_mxfp4(packed, scale)[0].double()
    for c in range(16):
        for code, got in ((c, dq[2 * c]), (15 - c, dq[2 * c + 1])):
            mag = GRID[code & 7] * 2.0 ** (s - 127)
            want = -mag if (code & 8) and mag else mag
            assert got.item() == want, (s, code)
    # exact in bf16: the fp32 product survives the cast unchanged
    lut = torch.tensor(ref.MXFP4_TABLE, dtype=torch.float64)
    codes = torch.tensor([[c, 15 - c] for c in range(16)]).flatten()
    assert torch.equal(dq, lut[codes] * 2.0 ** (s - 127))


def test_code_8_is_positive_zero():
    packed = torch.full((1, 16), 0x88, dtype=torch.uint8)
    dq = Q.dequantize_mxfp4(packed, torch.tensor([[200]], dtype=torch.uint8))
    assert torch.equal(dq.view(torch.int16), torch.zeros(1, 32, dtype=torch.int16))


@pytest.mark.parametrize("validate",
                         [Q.validate_mxfp4_scales, ops.validate_mxfp4_scales])
def test_validate_scales(validate):
    ok = torch.arange(8, 248, dtype=torch.uint8).view(16, 15)
    validate(ok)
    for bad in (7, 248, 255):
        t = ok.clone()
        t[3, 4] = bad
        with pytest.raises(ValueError):
            validate(t)


# --------------------------------------------------------------- quantiser

def _brute_force(w):
    """float64 quantiser straight from the format's definition."""
    N, K = w.shape
    packed = torch.zeros(N, K // 2, dtype=torch.uint8)
    scale = torch.zeros(N, K // 32, dtype=torch.uint8)
    wl = w.double().tolist()
    for n in range(N):
        for b in range(K // 32):
            blk = wl[n][32 * b: 32 * b + 32]
            amax = max(abs(v) for v in blk)
            if amax == 0:
                s = 127
            else:
                m, e = math.frexp(amax)  # amax = m 2^e, 0.5 <= m < 1
                s = min(max(e - 1 - 2 + 127, 8), 247)
            scale[n, b] = s
            for i, v in enumerate(blk):
                a = abs(v) / 2.0 ** (s - 127)
                best, best_d = 0, None
                for code, gpt in enumerate(GRID):
                    d = abs(a - gpt)
                    # nearest; on a tie the code with even mantissa bit
                    if (best_d is None or d < best_d
                            or (d == best_d and code % 2 == 0)):
                        best, best_d = code, d
                if v < 0 and best:
                    best |= 8
                k = 32 * b + i
                packed[n, k // 2] |= best << (4 * (k % 2))
    return packed, scale


def _check(w):
    p, s = Q.quantize_weight_mxfp4(w)
    bp, bs = _brute_force(w)
    assert torch.equal(s, bs)
    assert torch.equal(p, bp)
    return p, s


def test_quantiser_random_blocks():
    torch.manual_seed(0)
    w = (torch.randn(8, 128) * 0.02).to(torch.bfloat16)
    _check(w)
    _check(torch.randn(4, 64) * 0.02)  # fp32 input


def test_quantiser_zero_block():
    w = torch.zeros(2, 64)
    w[1, 40] = 0.3
    p, s = _check(w)
    assert s[0].tolist() == [127, 127] and s[1, 0].item() == 127
    assert int(p[0].max()) == 0 and int(p[1, :16].max()) == 0


def test_quantiser_power_of_two_amax():
    torch.manual_seed(1)
    w = torch.rand(4, 32) * 0.001
    w[:, 0] = torch.tensor([0.25, -0.25, 2.0 ** -7, 8.0])
    p, s = _check(w)
    # amax = 2^e gives 4.0 after scaling: s = e - 2 + 127, code 6
    assert s[:, 0].tolist() == [123, 123, 118, 128]
    assert (p[:, 0] & 0xF).tolist() == [6, 14, 6, 6]


def test_quantiser_saturates_just_under_eight():
    w = torch.zeros(1, 32)
    w[0, :4] = torch.tensor([7.96875, -7.5, 6.5, 5.5])  # scale 1
    p, s = _check(w)
    assert s.item() == 127
    assert p[0, :2].tolist() == [0x7 | (0xF << 4), 0x7 | (0x7 << 4)]


def test_quantiser_exact_ties():
    w = torch.zeros(1, 32)
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    w[0, :7] = torch.tensor(ties)
    w[0, 7:14] = -torch.tensor(ties)
    w[0, 31] = 6.0  # pins the scale to 1
    p, s = _check(w)
    assert s.item() == 127
    dq = Q.dequantize_mxfp4(p, s)[0].tolist()
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert dq[:7] == want
    assert dq[7:14] == [-v if v else 0.0 for v in want]


def test_quantiser_clamps_scale_range():
    w = torch.zeros(2, 32)
    w[0, :3] = torch.tensor([2.0 ** -130, 2.0 ** -120, -(2.0 ** -119)])
    w[1, :3] = torch.tensor([2.0 ** 125, -(2.0 ** 121), 2.0 ** 119])
    p, s = _check(w)
    assert s.flatten().tolist() == [8, 247]
    Q.validate_mxfp4_scales(s)
    dq = Q.dequantize_mxfp4(p, s).double()
    # s = 8: grid step 0.5 * 2^-119; s = 247: saturation at 6 * 2^120
    assert dq[0, :3].tolist() == [0.0, 2.0 ** -120, -(2.0 ** -119)]
    assert dq[1, :3].tolist() == [6 * 2.0 ** 120, -(2.0 ** 121), 2.0 ** 119]


def test_quantiser_idempotent():
    torch.manual_seed(2)
    w = (torch.randn(16, 256) * 0.02).to(torch.bfloat16)
    p, s = Q.quantize_weight_mxfp4(w)
    p2, s2 = Q.quantize_weight_mxfp4(Q.dequantize_mxfp4(p, s))
    assert torch.equal(p, p2) and torch.equal(s, s2)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_quantiser_rejects_non_finite(bad):
    w = torch.zeros(2, 32)
    w[1, 5] = bad
    with pytest.raises(ValueError):
        Q.quantize_weight_mxfp4(w)


# ------------------------------------------------------------------ CPU ops

def test_cpu_ops_dispatch_and_validation():
    torch.manual_seed(3)
    w = torch.randn(16, 128) * 0.02
    p, s = Q.quantize_weight_mxfp4(w)
    x = torch.randn(3, 128).to(torch.bfloat16)
    bias = torch.randn(16).to(torch.bfloat16)
    dq = ops.mxfp4_dequant(p, s)
    assert torch.equal(dq, Q.dequantize_mxfp4(p, s))
    want = (x.float() @ dq.float().t() + bias.float()).to(torch.bfloat16)
    assert torch.equal(ops.mxfp4_linear(x, p, s, bias), want)
    out = torch.empty(3, 16, dtype=torch.bfloat16)
    assert ops.mxfp4_linear(x, p, s, bias, out=out) is out
    assert torch.equal(out, want)
    assert ops.mxfp4_linear(x[:0], p, s).shape == (0, 16)
    with pytest.raises(ValueError):  # K = 96
        ops.mxfp4_linear(x[:, :96].contiguous(), p[:, :48].contiguous(),
                         s[:, :3].contiguous())
    with pytest.raises(ValueError):  # N = 8
        ops.mxfp4_linear(x, p[:8], s[:8])
    with pytest.raises(ValueError):
        ops.mxfp4_linear(x.to(torch.float16), p, s)
    with pytest.raises(ValueError):  # non-contiguous x
        ops.mxfp4_linear(torch.randn(128, 3).to(torch.bfloat16).t(), p, s)
    with pytest.raises(ValueError):  # wrong scale shape
        ops.mxfp4_linear(x, p, s[:, :3].contiguous())
    with pytest.raises(ValueError):
        ops.mxfp4_dequant(p, s.to(torch.int8))


# --------------------------------------------------------------- conversion

def _tiny_model(seed=0):
    from fusioninfer_amd.models.model import CausalLM
    from fusioninfer_amd.models.registry import get_model_config

    torch.manual_seed(seed)
    return CausalLM(get_model_config("tiny-qwen3")).eval()


def test_convert_tiny_qwen3():
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )

    model = _tiny_model()
    lm_head = model.lm_head.weight.clone()
    shapes = {
        name: tuple(m.weight.shape) for name, m in model.named_modules()
        if isinstance(m, (MergedColumnParallelLinear, RowParallelLinear))
    }
    n = Q.convert_linear_to_mxfp4(model)
    assert n == len(shapes) > 0
    for name, m in model.named_modules():
        if name not in shapes:
            continue
        N, K = shapes[name]
        assert not hasattr(m, "weight")
        assert m.weight_packed.shape == (N, K // 2)
        assert m.weight_scale.shape == (N, K // 32)
        tensors = [t for k, t in list(m.named_parameters())
                   + list(m.named_buffers()) if k != "bias"]
        nbytes = sum(t.numel() * t.element_size() for t in tensors)
        assert nbytes == N * K // 2 + N * K // 32
        assert not any(t.requires_grad for t in tensors)
    assert model.lm_head.weight.dtype == torch.bfloat16
    assert torch.equal(model.lm_head.weight, lm_head)


def test_convert_rejects_row_shard_not_multiple_of_128():
    from fusioninfer_amd.distributed.layers import RowParallelLinear

    holder = torch.nn.Module()
    holder.ok = RowParallelLinear(256, 32)
    holder.bad = RowParallelLinear(192, 32)  # e.g. K = 384 split over TP = 2
    assert holder.bad.in_per_rank % 128 != 0
    with pytest.raises(ValueError, match="in_per_rank"):
        Q.convert_linear_to_mxfp4(holder)
    assert hasattr(holder.ok, "weight")  # nothing was half-converted


# --------------------------------------------------------------- CPU engine

def _engine(quant, enable_lora=False, model="tiny-qwen3"):
    from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config(model)
    mc.quantization = quant
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=64),
        scheduler=SchedulerConfig(
            max_num_seqs=4, max_num_batched_tokens=256, max_model_len=128
        ),
        seed=11,
        enable_lora=enable_lora,
    )
    return LLMEngine(cfg, device="cpu")


def test_cpu_engine_matches_bf16_engine_on_dequantised_weights():
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )
    from fusioninfer_amd.engine.sequence import SamplingParams

    prompts = [[3, 1, 4] * 6, [2, 7, 1, 8, 2, 8] * 2, list(range(5, 30))]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)

    mx = _engine("mxfp4")
    got = [o.output_token_ids for o in mx.generate(prompts, sp)]
    assert all(len(t) == 16 for t in got)

    bf = _engine(None)  # same seed, same random weights
    for m in bf.runner.model.modules():
        if isinstance(m, (MergedColumnParallelLinear, RowParallelLinear)):
            p, s = Q.quantize_weight_mxfp4(m.weight.data)
            m.weight.data.copy_(Q.dequantize_mxfp4(p, s))
    want = [o.output_token_ids for o in bf.generate(prompts, sp)]
    assert got == want


# --------------------------------------------------------------- rejections

def test_unknown_quantization_still_raises():
    with pytest.raises(ValueError, match="unknown quantization"):
        _engine("int3")


def test_moe_with_mxfp4_raises():
    with pytest.raises(ValueError, match="mxfp4 does not cover MoE experts yet"):
        _engine("mxfp4", model="tiny-qwen3-moe")


def test_lora_rejected_in_mxfp4_mode():
    eng = _engine("mxfp4")
    with pytest.raises(AssertionError, match="mxfp4"):
        eng.add_lora("a", rank=4)
    # the slot table is not built either, as in fp8 mode
    assert _engine("mxfp4", enable_lora=True).runner.lora_slots is None


def test_cli_accepts_mxfp4():
    from fusioninfer_amd.server.__main__ import parse_args

    assert parse_args(["--quantization", "mxfp4"]).quantization == "mxfp4"
    assert parse_args([]).quantization is None
