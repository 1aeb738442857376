"""Int4 group-quantised weight-only mode (AWQ / GPTQ format): quantiser,
reference dequant, checkpoint converters, loader and CPU engine."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q
from fusioninfer_amd.models import weight_loader as WL
from int4_cases import engine, pack, prefill_logits

GS = (32, 64, 128)


def random_format(N, K, G, seed=0):
    """Random codes, zeros and full-significand fp16 scales: (q [N, K], z, s)."""
    g = torch.Generator().manual_seed(seed + N + K + G)
    q = torch.randint(0, 16, (N, K), generator=g).to(torch.uint8)
    z = torch.randint(0, 16, (N, K // G), generator=g).to(torch.uint8)
    s = (torch.rand(N, K // G, generator=g) * 0.03 + 1e-3).to(torch.float16)
    return q, z, s


@pytest.mark.parametrize("G", GS)
def test_quantiser_round_trip(G):
    torch.manual_seed(G)
    w = torch.randn(8, 256) * 0.02
    w[0, :G] = 0.0125           # constant group
    w[1, :G] = 0.0              # zeros only
    w[2, :G] = w[2, :G].abs()   # one sign
    w[3, :G] = -w[3, :G].abs() - 0.01
    p, s, z = Q.quantize_weight_int4(w, G)
    Q.validate_int4_scales(s, z)
    dq = Q.dequantize_int4(p, s, z, G).double()
    sg = s.double().repeat_interleave(G, dim=1)
    # half a step, the fp16 rounding of s over 15 steps, bf16 rounding of dq
    bound = sg / 2 + 15 * sg * 2.0 ** -11 + dq.abs() * 2.0 ** -8
    assert bool(((w.double() - dq).abs() <= bound).all())
    assert torch.equal(dq[1, :G], torch.zeros(G, dtype=torch.float64))
    assert s[1, 0].item() == 2.0 ** -14


@pytest.mark.parametrize("G", GS)
def test_reference_dequant_matches_definition(G):
    q, z, s = random_format(16, 256, G)
    want = ((q.double() - z.double().repeat_interleave(G, dim=1))
            * s.double().repeat_interleave(G, dim=1)).to(torch.bfloat16)
    got = ref.int4_dequant(pack(q), s, z, G)
    assert torch.equal(got, want)
    assert torch.equal(ops.int4_dequant(pack(q), s, z, G), want)
    x = torch.randn(3, 256).to(torch.bfloat16)
    bias = torch.randn(16).to(torch.bfloat16)
    y = (x.float() @ want.float().t() + bias.float()).to(torch.bfloat16)
    assert torch.equal(ops.int4_linear(x, pack(q), s, z, G, bias), y)
    assert ops.int4_linear(x[:0], pack(q), s, z, G).shape == (0, 16)


def words(nib, order):
    """[R, 8 C] nibbles -> [R, C] int32; nibble i of a word is column order[i]."""
    r = nib.view(nib.shape[0], -1, 8)[..., list(order)].to(torch.int64)
    w = (r << (4 * torch.arange(8))).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def awq_layout(q, z, s):
    return (words(q.t().contiguous(), Q.AWQ_ORDER),
            words(z.t().contiguous(), Q.AWQ_ORDER), s.t().contiguous())


def gptq_layout(q, z, s):
    return (words(q, range(8)).t().contiguous(),
            words(z.t().contiguous() - 1, range(8)), s.t().contiguous())


@pytest.mark.parametrize("G", GS)
def test_checkpoint_converters_exact(G):
    q, z, s = random_format(32, 256, G, seed=1)
    want = (pack(q), s, z)
    for got in (Q.int4_from_awq(*awq_layout(q, z, s)),
                Q.int4_from_gptq(*gptq_layout(q, z.clamp(min=1), s))):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(Q.int4_from_awq(*awq_layout(q, z, s))[2], z)
    zg = z.clamp(min=1)
    trivial = torch.arange(256) // G
    assert torch.equal(
        Q.int4_from_gptq(*gptq_layout(q, zg, s), g_idx=trivial)[2], zg)
    with pytest.raises(ValueError, match="act-order"):
        Q.int4_from_gptq(*gptq_layout(q, zg, s), g_idx=trivial.flip(0))


def test_rejections():
    q, z, s = random_format(16, 128, 32)
    for bad in (0.0, -1.0, 2.0 ** -15, float("inf"), float("nan")):
        t = s.clone()
        t[3, 1] = bad
        with pytest.raises(ValueError):
            ops.validate_int4_scales(t, z)
    with pytest.raises(ValueError):
        ops.validate_int4_scales(s, z + 16)
    x = torch.ones(2, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError):  # group size
        ops.int4_linear(x, pack(q), s, z, 16)
    with pytest.raises(ValueError):  # scale shape belongs to G = 32
        ops.int4_linear(x, pack(q), s, z, 64)
    qc = {"quant_method": "gptq", "bits": 4, "group_size": 128}
    assert WL.int4_quantization_config(qc) == ("gptq", 128)
    for field, value in (("bits", 8), ("desc_act", True), ("group_size", -1),
                         ("checkpoint_format", "gptq_v2")):
        with pytest.raises(ValueError, match=field):
            WL.int4_quantization_config({**qc, field: value})
    for field, value in (("version", "gemv"), ("zero_point", False)):
        with pytest.raises(ValueError, match=field):
            WL.int4_quantization_config(
                {**qc, "quant_method": "awq", field: value})


def _projections(model):
    return [m for m in model.modules() if type(m).__name__ in (
        "MergedColumnParallelLinear", "RowParallelLinear")]


def _tokens(eng):
    from fusioninfer_amd.engine.sequence import SamplingParams

    prompts = [[3, 1, 4] * 6, [2, 7, 1, 8, 2, 8] * 2, list(range(5, 30))]
    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    return [o.output_token_ids for o in eng.generate(prompts, sp)]


@pytest.fixture(scope="module")
def int4_engine_and_tokens():
    eng = engine("int4")
    for m in _projections(eng.runner.model):
        m.weight_zero.clamp_(min=1)  # GPTQ stores z - 1: keep z >= 1
    return eng, _tokens(eng)


def test_cpu_engine_matches_bf16_engine_on_dequantised_weights(
        int4_engine_and_tokens):
    """Two bf16 GEMM implementations on the same numbers: greedy tokens can
    part at a near-tie, so prefill logits are compared. Each evaluation lies
    within the floor measured between a bf16 and an fp32 evaluation of this
    model (7.85e-3, tests/test_mxfp4_gpu.py) of the fp32 one: bound 2x that."""
    eng, got = int4_engine_and_tokens
    bf = engine(None)  # same seed, same random weights
    for m, mq in zip(_projections(bf.runner.model),
                     _projections(eng.runner.model)):
        assert not hasattr(mq, "weight")
        m.weight.data.copy_(Q.dequantize_int4(
            mq.weight_packed, mq.weight_scale, mq.weight_zero, 64))
    a, b = (prefill_logits(e, list(range(5, 45))) for e in (eng, bf))
    assert bool(torch.isfinite(a).all())
    err = ((a - b).norm(dim=-1) / b.norm(dim=-1)).max().item()
    print(f"int4 CPU prefill logits row_rel_err {err:.3e}")
    assert err < 2 * 7.85e-3


@pytest.mark.parametrize("method", ["awq", "gptq"])
def test_checkpoint_dir_loads(method, int4_engine_and_tokens, tmp_path):
    """A checkpoint directory of separately quantised HF projections: int4 and
    G come from config.json; a load with a projection missing is refused."""
    import json

    from safetensors.torch import save_file

    src, want = int4_engine_and_tokens
    layout = awq_layout if method == "awq" else gptq_layout
    sd = {}
    for k, w in WL.export_hf_state_dict(engine(None).runner.model).items():
        if not k.endswith("_proj.weight"):
            sd[k] = w
            continue
        p, s, z = Q.quantize_weight_int4(w, 64)
        q = torch.stack((p & 0xF, p >> 4), dim=-1).reshape(p.shape[0], -1)
        for kind, t in zip(("qweight", "qzeros", "scales"),
                           layout(q, z.clamp(min=1), s)):
            sd[k[:-len("weight")] + kind] = t
    qc = {"quant_method": method, "bits": 4, "group_size": 64}
    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": qc}))
    save_file(sd, str(tmp_path / "model.safetensors"))
    eng = engine(None, G=128, model_path=str(tmp_path))
    assert eng.cfg.model.quantization == "int4"
    for a, b in zip(_projections(eng.runner.model),
                    _projections(src.runner.model)):
        for name in ("weight_packed", "weight_scale", "weight_zero"):
            assert torch.equal(getattr(a, name), getattr(b, name))
    assert _tokens(eng) == want
    sd = {k: v for k, v in sd.items() if "layers.1.mlp.up_proj" not in k}
    with pytest.raises(ValueError, match=r"layers \[1\]"):
        WL.load_hf_state_dict(eng.runner.model, sd.items(), int4_method=method)


def test_moe_refused_and_cli():
    from fusioninfer_amd.server.__main__ import parse_args

    with pytest.raises(ValueError, match="int4 does not cover MoE experts"):
        engine("int4", model="tiny-qwen3-moe")
    args = parse_args(["--quantization", "int4", "--int4-group-size", "64"])
    assert args.quantization == "int4" and args.int4_group_size == 64
    eng = engine("int4")
    with pytest.raises(AssertionError, match="int4"):
        eng.add_lora("a", rank=4)
