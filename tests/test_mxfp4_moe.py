"""MXFP4 MoE experts: reference op, conversion, CPU engine, rejections, CLI.

Dequantisation is exact in bf16, so the engine check is an equality against
a bf16 engine that runs on the dequantised weights."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q

SENTINEL = -7.0


def _align(counts, block_m, T, top_k, gen):
    """Block-aligned routing with counts[e] rows for expert e, plus two
    spare tiles past n_valid. Returns sorted_ids, expert_ids, n_valid, and
    the (slot, token, expert) triple of every real assignment."""
    sorted_ids, expert_ids, real = [], [], []
    for e, c in enumerate(counts):
        toks = torch.randint(0, T, (c,), generator=gen).tolist()
        tiles = (c + block_m - 1) // block_m
        base = len(sorted_ids)
        for i, t in enumerate(toks):
            real.append((base + i, t, e))
        sorted_ids += toks + [0] * (tiles * block_m - c)
        expert_ids += [e] * tiles
    n_valid = len(expert_ids)
    sorted_ids += [0] * (2 * block_m)
    expert_ids += [len(counts) - 1] * 2
    return (torch.tensor(sorted_ids, dtype=torch.int32),
            torch.tensor(expert_ids, dtype=torch.int32),
            torch.tensor([n_valid], dtype=torch.int32), real)


def _experts(E, NB, K, gen):
    w = torch.randn(E, NB, K, generator=gen) * 0.05
    packed = torch.empty(E, NB, K // 2, dtype=torch.uint8)
    scale = torch.empty(E, NB, K // 32, dtype=torch.uint8)
    for e in range(E):
        packed[e], scale[e] = Q.quantize_weight_mxfp4(w[e])
    return packed, scale


# ------------------------------------------------------------ reference op

@pytest.mark.parametrize("gate_up", [True, False])
@pytest.mark.parametrize("block_m", [16, 128])
def test_reference_equals_per_assignment_loop(gate_up, block_m):
    gen = torch.Generator().manual_seed(5)
    E, K, N, T = 4, 128, 32, 24
    counts = [0, 1, 17, 30]
    sorted_ids, expert_ids, n_valid, real = _align(counts, block_m, T, 2, gen)
    PM = sorted_ids.numel()
    NB = 2 * N if gate_up else N
    packed, scale = _experts(E, NB, K, gen)
    rows = T if gate_up else PM
    a = (torch.randn(rows, K, generator=gen)).to(torch.bfloat16)
    out = torch.full((PM, N), SENTINEL, dtype=torch.bfloat16)
    got = ops.moe_gemm_mxfp4(out, a, packed, scale, sorted_ids, expert_ids,
                             n_valid, block_m, gate_up)
    assert got is out
    assert real
    # the same reference with an fp32 out shows its values before the one
    # rounding: the bf16 result must be exactly their rounding, and they
    # must match a float64 per-assignment loop to fp32 accuracy (K = 128
    # products of magnitude <= ~1: 1e-5 relative, 1e-6 near cancellation)
    out32 = torch.full((PM, N), SENTINEL, dtype=torch.float32)
    ref.moe_gemm_mxfp4(out32, a, packed, scale, sorted_ids, expert_ids,
                       n_valid, block_m, gate_up)
    assert torch.equal(out, out32.to(torch.bfloat16))
    for slot, tok, e in real:
        w = Q.dequantize_mxfp4(packed[e], scale[e]).double()  # [NB, K]
        src = a[tok if gate_up else slot].double()
        acc = w @ src
        if gate_up:
            acc = torch.nn.functional.silu(acc[:N]) * acc[N:]
        assert torch.allclose(out32[slot].double(), acc,
                              rtol=1e-5, atol=1e-6), (slot, tok, e)
    # tiles at or past n_valid are never touched
    tail = out[int(n_valid) * block_m:]
    assert tail.numel() and bool((tail == SENTINEL).all())
    assert bool(torch.isfinite(out.float()).all())


# ---------------------------------------------------------------- rejections

def _good_args(gate_up=True, block_m=16):
    gen = torch.Generator().manual_seed(1)
    E, K, N, T = 2, 128, 16, 4
    sorted_ids, expert_ids, n_valid, _ = _align([3, 2], block_m, T, 2, gen)
    PM = sorted_ids.numel()
    packed, scale = _experts(E, 2 * N if gate_up else N, K, gen)
    a = torch.zeros(T if gate_up else PM, K, dtype=torch.bfloat16)
    out = torch.zeros(PM, N, dtype=torch.bfloat16)
    return dict(out=out, a=a, w_packed=packed, w_scale=scale,
                sorted_ids=sorted_ids, expert_ids=expert_ids,
                n_valid=n_valid, block_m=block_m, gate_up=gate_up)


def test_op_accepts_the_good_arguments():
    ops.moe_gemm_mxfp4(**_good_args(True))
    ops.moe_gemm_mxfp4(**_good_args(False))


@pytest.mark.parametrize("change", [
    lambda k: k.update(a=k["a"].float()),
    lambda k: k.update(out=k["out"].float()),
    lambda k: k.update(w_packed=k["w_packed"].to(torch.int8)),
    lambda k: k.update(w_scale=k["w_scale"].to(torch.int32)),
    lambda k: k.update(sorted_ids=k["sorted_ids"].long()),
    lambda k: k.update(expert_ids=k["expert_ids"].long()),
    lambda k: k.update(n_valid=k["n_valid"].long()),
    lambda k: k.update(block_m=32),
    lambda k: k.update(sorted_ids=k["sorted_ids"][:-1]),
    lambda k: k.update(out=k["out"][:-1]),
    lambda k: k.update(out=k["out"].t().contiguous().t()),
    lambda k: k.update(a=k["a"][:, :64].contiguous()),
    lambda k: k.update(w_packed=k["w_packed"][:, :16].contiguous()),
    lambda k: k.update(w_scale=k["w_scale"][:, :, :3].contiguous()),
    lambda k: k.update(w_packed=k["w_packed"][0]),
    lambda k: k.update(expert_ids=k["expert_ids"][:1]),
    lambda k: k.update(out=torch.zeros(k["out"].shape[0], 24,
                                       dtype=torch.bfloat16)),
])
def test_op_rejects_bad_dtypes_and_shapes(change):
    kw = _good_args()
    change(kw)
    with pytest.raises(ValueError, match="moe_gemm_mxfp4"):
        ops.moe_gemm_mxfp4(**kw)


def test_op_rejects_short_act_without_gate_up():
    kw = _good_args(gate_up=False)
    kw["a"] = kw["a"][:-1]
    with pytest.raises(ValueError, match="moe_gemm_mxfp4"):
        ops.moe_gemm_mxfp4(**kw)


# ---------------------------------------------------------------- conversion

def _moe_cfg(**over):
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config("tiny-qwen3-moe")
    for k, v in over.items():
        setattr(mc, k, v)
    return mc


def _moe_mlps(model):
    from fusioninfer_amd.models.model import MoEMLP

    return [m for m in model.modules() if isinstance(m, MoEMLP)]


def test_conversion_drops_bf16_and_stores_4_25_bits():
    from fusioninfer_amd.models.model import CausalLM

    torch.manual_seed(3)
    model = CausalLM(_moe_cfg()).eval()
    mlps = _moe_mlps(model)
    before = [(m.gate_up_t.data.clone(), m.down_t.data.clone()) for m in mlps]
    assert Q.convert_moe_experts_to_mxfp4(model) == len(mlps) == 2
    for m, (gu, dn) in zip(mlps, before):
        assert m.mxfp4
        assert m.gate_up_t.numel() == 0 and m.down_t.numel() == 0
        assert tuple(m.gate_up_t.shape[1:]) == tuple(gu.shape[1:])
        assert tuple(m.down_t.shape[1:]) == tuple(dn.shape[1:])
        E, H, I2 = gu.shape
        assert m.gate_up_packed.shape == (E, I2, H // 2)
        assert m.gate_up_scale.shape == (E, I2, H // 32)
        assert m.down_packed.shape == (E, H, I2 // 4)
        assert m.down_scale.shape == (E, H, I2 // 64)
        stored = sum(t.numel() * t.element_size() for t in (
            m.gate_up_packed, m.gate_up_scale, m.down_packed, m.down_scale))
        bf16_bytes = 2 * (gu.numel() + dn.numel())
        assert stored * 16 == bf16_bytes * 4.25
        assert getattr(m, "_pack_cache", None) is None
        # expert by expert on the [O, I] view, gate rows first
        for e in (0, E - 1):
            p, s = Q.quantize_weight_mxfp4(gu[e].t().contiguous())
            assert torch.equal(m.gate_up_packed[e], p)
            assert torch.equal(m.gate_up_scale[e], s)
            p, s = Q.quantize_weight_mxfp4(dn[e].t().contiguous())
            assert torch.equal(m.down_packed[e], p)
            assert torch.equal(m.down_scale[e], s)
        with pytest.raises(RuntimeError, match="MXFP4"):
            m.ensure_unpacked()
        with pytest.raises(RuntimeError, match="MXFP4"):
            m.invalidate_packed()
        m.release_unpacked()  # a no-op
        assert m.gate_up_packed.shape[0] == E


def test_conversion_rejects_intermediate_64():
    from fusioninfer_amd.models.model import CausalLM

    torch.manual_seed(3)
    model = CausalLM(_moe_cfg(moe_intermediate_size=64)).eval()
    with pytest.raises(ValueError, match=r"layer 0.*moe_intermediate_size=64"):
        Q.convert_moe_experts_to_mxfp4(model)
    assert not any(m.mxfp4 for m in _moe_mlps(model))
    assert all(m.gate_up_t.numel() for m in _moe_mlps(model))


# --------------------------------------------------------------- CPU engine

def _engine(quant, experts=False, model="tiny-qwen3-moe", **over):
    from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config(model)
    mc.quantization = quant
    mc.mxfp4_moe_experts = experts
    for k, v in over.items():
        setattr(mc, k, v)
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=64),
        scheduler=SchedulerConfig(
            max_num_seqs=4, max_num_batched_tokens=256, max_model_len=128
        ),
        seed=11,
    )
    return LLMEngine(cfg, device="cpu")


def _dq(w):
    return Q.dequantize_mxfp4(*Q.quantize_weight_mxfp4(w))


def test_cpu_engine_matches_bf16_engine_on_dequantised_weights():
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )
    from fusioninfer_amd.engine.sequence import SamplingParams

    prompts = [[3, 1, 4] * 6, [2, 7, 1, 8, 2, 8] * 2, list(range(5, 30))]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)

    mx = _engine("mxfp4", experts=True)
    assert all(m.mxfp4 for m in _moe_mlps(mx.runner.model))
    got = [o.output_token_ids for o in mx.generate(prompts, sp)]
    assert all(len(t) == 16 for t in got)

    bf = _engine(None)  # same seed, same random weights
    for m in bf.runner.model.modules():
        if isinstance(m, (MergedColumnParallelLinear, RowParallelLinear)):
            m.weight.data.copy_(_dq(m.weight.data))
    for m in _moe_mlps(bf.runner.model):
        for p in (m.gate_up_t, m.down_t):
            for e in range(p.shape[0]):
                p.data[e].copy_(_dq(p.data[e].t().contiguous()).t())
    want = [o.output_token_ids for o in bf.generate(prompts, sp)]
    assert got == want


def test_switch_without_mxfp4_raises():
    for quant in (None, "fp8"):
        with pytest.raises(ValueError, match="mxfp4_moe_experts"):
            _engine(quant, experts=True)


def test_switch_off_keeps_the_refusal():
    with pytest.raises(ValueError, match="mxfp4 does not cover MoE experts yet"):
        _engine("mxfp4", experts=False)


def test_engine_rejects_intermediate_64():
    with pytest.raises(ValueError, match="moe_intermediate_size=64"):
        _engine("mxfp4", experts=True, moe_intermediate_size=64)


def test_switch_has_no_effect_on_a_dense_model():
    eng = _engine("mxfp4", experts=True, model="tiny-qwen3")
    assert not _moe_mlps(eng.runner.model)
    from fusioninfer_amd.engine.sequence import SamplingParams

    sp = SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True)
    got = eng.generate([[3, 1, 4, 1, 5]], sp)[0].output_token_ids
    want = _engine("mxfp4", model="tiny-qwen3").generate(
        [[3, 1, 4, 1, 5]], sp)[0].output_token_ids
    assert got == want


def test_cli_parses_the_flag():
    from fusioninfer_amd.server.__main__ import build_engine_config, parse_args

    assert parse_args([]).mxfp4_moe_experts is False
    args = parse_args(["--model", "tiny-qwen3-moe", "--quantization", "mxfp4",
                       "--mxfp4-moe-experts"])
    assert args.mxfp4_moe_experts is True
    cfg = build_engine_config(args)
    assert cfg.model.mxfp4_moe_experts is True
    assert cfg.model.quantization == "mxfp4"
