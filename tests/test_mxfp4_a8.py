"""MXFP8 activation format, the mxfp4 layer dispatch in both activation
modes, and flag/config validation, on the CPU (reference ops)."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q


def _quant(block):
    """One row holding one 32-k block (padded to K = 128 with zero blocks)."""
    x = torch.zeros(1, 128)
    x[0, :len(block)] = torch.tensor(block, dtype=torch.float32)
    x = x.to(torch.bfloat16)
    q, s = ref.mxfp8_quant_rows(x)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.uint8
    assert q.shape == (1, 128) and s.shape == (1, 4)
    assert s[0, 1:].tolist() == [127] * 3  # all-zero blocks
    assert int(q.view(torch.uint8)[0, 32:].max()) == 0
    return x, q, s


@pytest.mark.parametrize("block,scale,elems", [
    ([0.0] * 32, 127, [0.0, 0.0]),
    # amax = 2^e scales to 256: s = e - 8 + 127
    ([0.25, -0.125], 117, [256.0, -128.0]),
    ([8.0, 3.0], 122, [256.0, 96.0]),
    # 480 = 1.875 * 2^8 stays 480 after scaling, above 448: saturates
    ([480.0, -500.0, 1.0], 127, [448.0, -448.0, 1.0]),
    # e4m3 spacing is 32 in [256, 512): 272 and 304 are ties -> even mantissa
    ([272.0, 304.0, -272.0, 336.0], 127, [256.0, 320.0, -256.0, 320.0]),
    # tiny amax: the scale clamps at 8 and the block sits low in e4m3's range
    ([2.0 ** -130, 2.0 ** -120], 8, [0.0, 0.5]),
    # the largest finite bf16 binade gives 246: the clamp at 247 bounds the
    # formula, no finite input reaches it
    ([2.0 ** 127, -(2.0 ** 120), 2.0 ** 112], 246, [256.0, -2.0, 2.0 ** -7]),
    # a negative value that rounds to zero is stored as +0
    ([256.0, -(2.0 ** -11)], 127, [256.0, 0.0]),
])
def test_quant_hand_made_blocks(block, scale, elems):
    x, q, s = _quant(block)
    assert s[0, 0].item() == scale
    assert not q.float().isnan().any()
    assert q.float()[0, :len(elems)].tolist() == elems
    assert 0x80 not in q.view(torch.uint8).flatten().tolist()
    dq = ref.mxfp8_dequant(q, s)
    assert dq.dtype == torch.bfloat16
    want = [e * 2.0 ** (scale - 127) for e in elems]
    assert dq.double()[0, :len(elems)].tolist() == want


@pytest.mark.parametrize("mode", ["bf16", "mxfp8"])
def test_layer_dispatch(mode, monkeypatch):
    from fusioninfer_amd.distributed.layers import MergedColumnParallelLinear

    torch.manual_seed(2)
    holder = torch.nn.Module()
    holder.up = MergedColumnParallelLinear(128, [32, 16], bias=True)
    holder.up.bias.data.normal_()
    bias = holder.up.bias.data.clone()
    p, s = Q.quantize_weight_mxfp4(holder.up.weight.data)
    assert Q.convert_linear_to_mxfp4(holder, activations=mode) == 1
    calls = []
    for name in ("quant_mxfp8_rows", "mxfp4_mxfp8_linear"):
        real = getattr(ops, name)
        monkeypatch.setattr(
            ops, name,
            lambda *a, _r=real, _n=name, **k: calls.append(_n) or _r(*a, **k))
    for M in (Q.MXFP4_MAX_M, Q.MXFP4_MAX_M + 8):
        calls.clear()
        x = torch.randn(M, 128).to(torch.bfloat16)
        got = holder.up(x)
        if mode == "mxfp8" and M > Q.MXFP4_MAX_M:
            assert calls == ["quant_mxfp8_rows", "mxfp4_mxfp8_linear"]
            xq, xs = ref.mxfp8_quant_rows(x)
            want = ref.mxfp4_mxfp8_linear(xq, xs, p, s, bias)
        else:  # today's output
            assert calls == []
            want = ref.mxfp4_linear(x, p, s, bias)
        assert torch.equal(got, want)


def test_config_and_flag_validation():
    from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config
    from fusioninfer_amd.server.__main__ import parse_args

    assert parse_args([]).mxfp4_activations == "bf16"
    args = parse_args(["--quantization", "mxfp4", "--mxfp4-activations", "mxfp8"])
    assert args.mxfp4_activations == "mxfp8"
    with pytest.raises(SystemExit):
        parse_args(["--mxfp4-activations", "fp8"])

    def engine(quant, act):
        mc = get_model_config("tiny-qwen3")
        assert mc.mxfp4_activations == "bf16"
        mc.quantization, mc.mxfp4_activations = quant, act
        cfg = EngineConfig(
            model=mc, cache=CacheConfig(num_gpu_blocks=64),
            scheduler=SchedulerConfig(max_num_seqs=4, max_num_batched_tokens=256,
                                      max_model_len=128), seed=11)
        return LLMEngine(cfg, device="cpu")

    for quant in (None, "fp8"):
        with pytest.raises(ValueError, match="mxfp4_activations"):
            engine(quant, "mxfp8")
    with pytest.raises(ValueError, match="mxfp4_activations"):
        engine("mxfp4", "fp8")
    with pytest.raises(ValueError):
        Q.convert_linear_to_mxfp4(torch.nn.Module(), activations="fp8")
    engine("mxfp4", "mxfp8")
