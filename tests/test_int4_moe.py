"""int4 MoE experts on the CPU: reference op, conversion, engine, CLI."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q
from tests.test_mxfp4_moe import _align, _engine, _moe_cfg, _moe_mlps

G = 64


def _moe_engine(quant, flag):
    return _engine(quant, int4_moe_experts=flag, int4_group_size=G)


@pytest.mark.parametrize("block_m", [16, 128])
@pytest.mark.parametrize("group", [32, 64, 128])
def test_reference_equals_float64_rows(group, block_m):
    """Scale 1.0, random codes and zeros, integer activations in [-4, 4]:
    |sum| <= 4 * 15 * 384 < 2^24, so the fp32 sums are exact and the result
    is the float64 product on dq(W) rounded to bf16 once."""
    gen = torch.Generator().manual_seed(group + block_m)
    E, K, N, T = 4, 384, 16, 24
    sorted_ids, expert_ids, n_valid, real = _align([0, 1, 17, 30], block_m, T,
                                                   2, gen)
    PM = sorted_ids.numel()
    packed = torch.randint(0, 256, (E, N, K // 2), generator=gen).to(torch.uint8)
    zero = torch.randint(0, 16, (E, N, K // group), generator=gen).to(torch.uint8)
    scale = torch.ones(E, N, K // group, dtype=torch.float16)
    a = torch.randint(-4, 5, (PM, K), generator=gen).to(torch.bfloat16)
    out = torch.full((PM, N), -7.0, dtype=torch.bfloat16)
    assert ops.moe_gemm_int4(out, a, packed, scale, zero, group, sorted_ids,
                             expert_ids, n_valid, block_m, False) is out
    for slot, tok, e in real:
        w = ref.int4_dequant(packed[e], scale[e], zero[e], group).double()
        want = (w @ a[slot].double()).to(torch.bfloat16)
        assert torch.equal(out[slot], want), (slot, tok, e)
    assert bool((out[int(n_valid) * block_m:] == -7.0).all())


def test_conversion_refuses_fp8_and_a_second_conversion():
    from fusioninfer_amd.models.model import CausalLM

    torch.manual_seed(3)
    with pytest.raises(ValueError, match="layer 0 are not bf16"):
        Q.convert_moe_experts_to_int4(
            CausalLM(_moe_cfg(quantization="fp8")).eval(), G)
    model = CausalLM(_moe_cfg()).eval()
    assert Q.convert_moe_experts_to_int4(model, G) == 2
    for m in _moe_mlps(model):
        assert m.int4 and m.int4_group_size == G
        assert m.gate_up_t.numel() == 0 and m.down_t.numel() == 0
        with pytest.raises(RuntimeError, match="int4"):
            m.ensure_unpacked()
    with pytest.raises(ValueError, match="layer 0 are not bf16"):
        Q.convert_moe_experts_to_int4(model, G)


def test_cpu_engine_matches_bf16_engine_on_dequantised_weights():
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )
    from fusioninfer_amd.engine.sequence import SamplingParams

    def dq(w):
        return Q.dequantize_int4(*Q.quantize_weight_int4(w, G), G)

    prompts = [[3, 1, 4] * 6, [2, 7, 1, 8, 2, 8] * 2, list(range(5, 30))]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    q = _moe_engine("int4", True)
    assert all(m.int4 for m in _moe_mlps(q.runner.model))
    got = [o.output_token_ids for o in q.generate(prompts, sp)]
    bf = _moe_engine(None, False)  # same seed, same random weights
    for m in bf.runner.model.modules():
        if isinstance(m, (MergedColumnParallelLinear, RowParallelLinear)):
            m.weight.data.copy_(dq(m.weight.data))
    for m in _moe_mlps(bf.runner.model):
        for p in (m.gate_up_t, m.down_t):
            for e in range(p.shape[0]):
                p.data[e].copy_(dq(p.data[e].t().contiguous()).t())
    want = [o.output_token_ids for o in bf.generate(prompts, sp)]
    assert got == want and all(len(t) == 16 for t in got)


def test_flag_needs_int4_and_cli_sets_it():
    from fusioninfer_amd.server.__main__ import build_engine_config, parse_args

    for quant in (None, "mxfp4"):
        with pytest.raises(ValueError, match="int4_moe_experts needs"):
            _moe_engine(quant, True)
    assert parse_args([]).int4_moe_experts is False
    args = parse_args(["--model", "tiny-qwen3-moe", "--quantization", "int4",
                       "--int4-moe-experts"])
    assert build_engine_config(args).model.int4_moe_experts is True
