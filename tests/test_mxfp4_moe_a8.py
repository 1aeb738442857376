"""`mxfp4_moe_activations` on the CPU: the flag, its validation, and the
reference definition of moe_gemm_mxfp4_mxfp8 against a plain float64 loop."""

import pytest
import torch
import torch.nn.functional as F

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q
from tests.test_mxfp4_moe import _engine, _moe_mlps


def test_flag_and_validation():
    from fusioninfer_amd.server.__main__ import build_engine_config, parse_args

    assert parse_args([]).mxfp4_moe_activations == "bf16"
    args = parse_args(["--model", "tiny-qwen3-moe", "--quantization", "mxfp4",
                       "--mxfp4-moe-experts", "--mxfp4-moe-activations", "mxfp8"])
    assert build_engine_config(args).model.mxfp4_moe_activations == "mxfp8"
    with pytest.raises(SystemExit):
        parse_args(["--mxfp4-moe-activations", "fp8"])
    with pytest.raises(ValueError, match="mxfp4_moe_activations"):
        _engine("mxfp4", False, mxfp4_moe_activations="mxfp8")
    with pytest.raises(ValueError, match="mxfp4_moe_activations"):
        _engine("mxfp4", True, mxfp4_moe_activations="fp8")
    with pytest.raises(ValueError, match="moe_intermediate_size=64"):
        _engine("mxfp4", True, mxfp4_moe_activations="mxfp8",
                moe_intermediate_size=64)
    assert all(m.mxfp4_activations == "bf16"
               for m in _moe_mlps(_engine("mxfp4", True).runner.model))
    mlps = _moe_mlps(
        _engine("mxfp4", True, mxfp4_moe_activations="mxfp8").runner.model)
    assert mlps and all(m.mxfp4_activations == "mxfp8" for m in mlps)


def test_reference_op_against_float64_loop():
    """Gate_up (gather, SwiGLU, quantiser): two valid tiles (experts 1 and
    0) and a sentinel tail tile, through the public op on CPU tensors."""
    g = torch.Generator().manual_seed(3)
    E, K, N, T, PM = 2, 128, 32, 5, 384
    w = torch.randn(E, 2 * N, K, generator=g) * 0.05
    ps = [Q.quantize_weight_mxfp4(w[e]) for e in range(E)]
    packed, scale = (torch.stack(t) for t in zip(*ps))
    x_q, x_s = ref.mxfp8_quant_rows(
        (4 * torch.randn(T, K, generator=g)).to(torch.bfloat16))
    sorted_ids = torch.randint(0, T, (PM,), generator=g).int()
    expert_ids = torch.tensor([1, 0, 0], dtype=torch.int32)
    raw = torch.full((PM, N), 0x55, dtype=torch.uint8)
    osc = torch.full((PM, 1), 0x55, dtype=torch.uint8)
    out = raw.view(torch.float8_e4m3fn)
    ops.moe_gemm_mxfp4_mxfp8(out, x_q, x_s, packed, scale, sorted_ids,
                             expert_ids, torch.tensor([2], dtype=torch.int32),
                             True, osc)
    x = ref.mxfp8_dequant(x_q, x_s).double()
    for slot in range(256):
        wd = ref.mxfp4_dequant(*ps[int(expert_ids[slot // 128])]).double()
        acc = wd @ x[int(sorted_ids[slot])]
        act = (F.silu(acc[:N]) * acc[N:]).to(torch.bfloat16)[None]
        got = ref.mxfp8_dequant(out[slot:slot + 1], osc[slot:slot + 1])
        # e4m3 rounds within 2^-4 relative; the op's fp32 sums against these
        # float64 ones may move a value across a midpoint (one more step,
        # 2^-3) or the amax across a power of two (scale byte +-1)
        assert abs(int(osc[slot]) - int(ref.mxfp8_quant_rows(act)[1])) <= 1
        assert torch.allclose(got.double(), act.double(),
                              rtol=2.0 ** -4 + 2.0 ** -3, atol=2.0 ** -12)
    assert bool((raw[256:] == 0x55).all()) and bool((osc[256:] == 0x55).all())
