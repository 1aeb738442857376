"""MXFP8 quantiser and MXFP4 x MXFP8 scaled-MFMA GEMM on the GPU. Both
dequantisations are exact, so the oracle is float64 on the dequantised
operands. K: one step, fill and drain of the double buffer, an odd step
count, a long loop; N: one fragment, one and three 128-wide column tiles with
tails; M: tile tails and a second and third 128-row block."""

import pytest
import torch
import torch.nn.functional as F

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q

pytestmark = pytest.mark.gpu

KS = (128, 256, 384, 1152)
NS = (16, 144, 272)
MS = (1, 17, 64, 129, 257)
DEV = "cuda:0"
E4M3 = torch.float8_e4m3fn
# exact result rounded to bf16 is within 2^-9 per element; 4x margin for
# the accumulation order (docs/kernels.md convention)
ROW_REL_BOUND = 2.0 ** -7
LOGITS_BOUND = 3.14e-2  # 4x the bf16-vs-fp32 floor, profiles/r12_mxfp4.md

_cache = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def weights(N, K, lo=None, hi=None):
    """GPU (packed, scale, dq(W) bf16): random codes with scale bytes in
    [lo, hi], or quantised Gaussian weights when lo is None."""
    key = (N, K, lo, hi)
    if key not in _cache:
        g = _gen(N * 7919 + K)
        if lo is None:
            p, s = Q.quantize_weight_mxfp4(torch.randn(N, K, generator=g) * 0.02)
        else:
            p = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
            s = torch.randint(lo, hi + 1, (N, K // 32), generator=g).to(torch.uint8)
        _cache[key] = (p.to(DEV), s.to(DEV), ref.mxfp4_dequant(p, s).to(DEV))
    return _cache[key]


def row_rel_err(got, want64):
    num = (got.double() - want64).norm(dim=-1)
    return (num / want64.norm(dim=-1)).max().item()


@pytest.mark.parametrize("hot_scale", [127, 125, 130])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_one_hot_readout_exact(K, N, hot_scale):
    """A single 1.0 per x_q row reads one column of dq(W) back, times its own
    block's scale: pins nibble and byte order, the k-to-lane map, both scale
    selections (all other activation scales are random) and orientation."""
    packed, scale, dq = weights(N, K, 119, 135)
    ks = [k for k in (0, 1, 3, 4, 15, 16, 31, 32, 33, 63, 64, 95, 96, 127, 128)
          if k < K] + [K - 1]
    g = _gen(K + N)
    for M in MS:
        km = torch.tensor([ks[(5 * m + 3) % len(ks)] for m in range(M)])
        x = torch.zeros(M, K)
        x[torch.arange(M), km] = 1.0
        xs = torch.randint(119, 136, (M, K // 32), generator=g).to(torch.uint8)
        xs[torch.arange(M), km // 32] = hot_scale
        out = ops.mxfp4_mxfp8_linear(x.to(E4M3).to(DEV), xs.to(DEV), packed, scale)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16
        want = (dq[:, km.to(DEV)].t().float() * 2.0 ** (hot_scale - 127))
        assert torch.equal(out, want.to(torch.bfloat16)), (K, N, M)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_integer_gemm_exact(K, N, with_bias):
    """x_q in [-4, 4], all scale bytes in {126, 127, 128}: every product is a
    multiple of 2^-3 and |sum| <= 1152 * 8 * 12 = 110592 < 2^24 * 2^-3, so
    fp32 accumulation is exact in any order, the hardware's 128-wide dot
    included, and the result must equal float64 rounded to bf16."""
    packed, scale, dq = weights(N, K, 126, 128)
    g = _gen(K + N)
    bias = None
    if with_bias:
        bias = torch.randint(-8, 9, (N,), generator=g).to(torch.bfloat16).to(DEV)
    for M in MS:
        xq = torch.randint(-4, 5, (M, K), generator=g).float().to(E4M3).to(DEV)
        xs = torch.randint(126, 129, (M, K // 32), generator=g).to(torch.uint8)
        xs = xs.to(DEV)
        want = ref.mxfp8_dequant(xq, xs).double() @ dq.double().t()
        if with_bias:
            want = want + bias.double()
        out = ops.mxfp4_mxfp8_linear(xq, xs, packed, scale, bias)
        assert torch.equal(out, want.to(torch.bfloat16)), (K, N, M)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_data_row_error(K, N):
    packed, scale, dq = weights(N, K)
    g = _gen(3 * K + N)
    worst = 0.0
    for M in MS:
        x = torch.randn(M, K, generator=g).to(torch.bfloat16)
        xq, xs = (t.to(DEV) for t in ref.mxfp8_quant_rows(x))
        want = ref.mxfp8_dequant(xq, xs).double() @ dq.double().t()
        err = row_rel_err(ops.mxfp4_mxfp8_linear(xq, xs, packed, scale), want)
        worst = max(worst, err)
    print(f"mxfp4_mxfp8_linear K={K} N={N} max row_rel_err {worst:.3e}")
    assert worst < ROW_REL_BOUND


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K", KS)
def test_quantiser_bit_for_bit(K, M):
    g = _gen(K + M)
    mag = 2.0 ** (torch.rand(M, K // 32, 1, generator=g) * 40 - 20)
    x = (torch.randn(M, K // 32, 32, generator=g) * mag)
    x[-1, -1] = 0.0  # subnormal amax: scale clamp at 8, 2^-127 -> 2^-8
    x[-1, -1, :3] = torch.tensor([2.0 ** -127, -(2.0 ** -130), 2.0 ** -120])
    x[0, 0] = 0.0                       # all zeros
    x[0, 1] = 0.0
    x[0, 1, 7] = -0.375                 # a single nonzero
    x[0, 2:4] *= 2.0 ** -30             # planted values set the block amax
    x[0, 2, :3] = torch.tensor([480.0, -500.0, 1.0])          # saturates
    x[0, 3, :4] = torch.tensor([272.0, 304.0, -272.0, 336.0])  # ties
    x = x.view(M, K).to(torch.bfloat16)
    want_q, want_s = ref.mxfp8_quant_rows(x)
    got_q, got_s = ops.quant_mxfp8_rows(x.to(DEV))
    assert got_q.dtype == E4M3 and got_s.dtype == torch.uint8
    assert torch.equal(got_s.cpu(), want_s)
    assert torch.equal(got_q.cpu().view(torch.uint8), want_q.view(torch.uint8))
    got_s.zero_()  # out= returns the given tensors, refilled
    assert ops.quant_mxfp8_rows(x.to(DEV), out=(got_q, got_s))[1] is got_s
    assert torch.equal(got_s.cpu(), want_s)


def test_batch_invariance_bitwise():
    K, N = 1152, 272
    packed, scale, _ = weights(N, K)
    g = _gen(99)
    x = torch.randn(257, K, generator=g).to(torch.bfloat16)
    x[200] = x[5]  # third row block, another position in its tile
    xq, xs = (t.to(DEV) for t in ref.mxfp8_quant_rows(x))
    alone = ops.mxfp4_mxfp8_linear(xq[5:6].contiguous(), xs[5:6].contiguous(),
                                   packed, scale)
    full = ops.mxfp4_mxfp8_linear(xq, xs, packed, scale)
    assert torch.equal(full[5], alone[0])
    assert torch.equal(full[200], alone[0])
    assert torch.equal(ops.mxfp4_mxfp8_linear(xq, xs, packed, scale), full)


def test_validation():
    packed, scale, _ = weights(16, 128, 126, 128)
    x = torch.ones(4, 128, dtype=torch.bfloat16, device=DEV)
    xq, xs = ops.quant_mxfp8_rows(x)
    for bad in (
        lambda: ops.quant_mxfp8_rows(x.float()),
        lambda: ops.quant_mxfp8_rows(x[:, :96].contiguous()),
        lambda: ops.quant_mxfp8_rows(
            torch.ones(128, 4, dtype=torch.bfloat16, device=DEV).t()),
        lambda: ops.quant_mxfp8_rows(x, out=(xq, xs[:, :3].contiguous())),
        lambda: ops.mxfp4_mxfp8_linear(x, xs, packed, scale),  # x not e4m3
        lambda: ops.mxfp4_mxfp8_linear(xq, xs[:, :3].contiguous(), packed, scale),
        lambda: ops.mxfp4_mxfp8_linear(xq, xs, packed[:8], scale[:8]),  # N = 8
        lambda: ops.mxfp4_mxfp8_linear(xq, xs, packed.cpu(), scale.cpu()),
        lambda: ops.mxfp4_mxfp8_linear(xq.t().contiguous().t(), xs, packed, scale),
        lambda: ops.mxfp4_mxfp8_linear(
            xq, xs, packed, scale,
            out=torch.empty(4, 16, dtype=torch.float16, device=DEV)),
    ):
        with pytest.raises(ValueError):
            bad()
    out = ops.mxfp4_mxfp8_linear(xq[:0], xs[:0], packed, scale)
    assert out.shape == (0, 16) and out.dtype == torch.bfloat16


def test_layer_mxfp8_mode(monkeypatch):
    """M = 8 is bit-equal to mxfp4_linear; M = 40 meets the random-data bound
    on dq(W) and dq(quant(x)); the bf16 scratch is neither reserved nor used."""
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear,
        RowParallelLinear,
    )

    used = []
    monkeypatch.setattr(Q._Mxfp4Scratch, "reserve",
                        lambda *a, **k: used.append("reserve"))
    monkeypatch.setattr(ops, "mxfp4_dequant",
                        lambda *a, **k: used.append("dequant"))
    torch.manual_seed(5)
    holder = torch.nn.Module()
    with torch.device(DEV):
        holder.up = MergedColumnParallelLinear(256, [384, 128], bias=True)
        holder.down = RowParallelLinear(512, 256)
    holder.up.bias.data.normal_()
    w = {}
    for name in ("up", "down"):
        w[name] = Q.quantize_weight_mxfp4(getattr(holder, name).weight.data)
    assert Q.convert_linear_to_mxfp4(holder, activations="mxfp8") == 2
    bias = holder.up.bias
    x = torch.randn(8, 256, device=DEV).to(torch.bfloat16)
    y_up = holder.up(x)
    assert torch.equal(y_up, ops.mxfp4_linear(x, *w["up"], bias))
    assert torch.equal(holder.down(y_up), ops.mxfp4_linear(y_up, *w["down"]))
    x = torch.randn(40, 256, device=DEV).to(torch.bfloat16)
    y_up = holder.up(x)
    y_down = holder.down(y_up)
    for name, src, got, b in (("up", x, y_up, bias), ("down", y_up, y_down, None)):
        dqx = ref.mxfp8_dequant(*ref.mxfp8_quant_rows(src)).double()
        want = dqx @ ref.mxfp4_dequant(*w[name]).double().t()
        if b is not None:
            want = want + b.double()
        assert row_rel_err(got, want) < ROW_REL_BOUND
    assert used == []


# ------------------------------------------------------------------ engine

PROMPTS = [[3, 1, 4] * 6, [2, 7, 1, 8, 2, 8] * 4, list(range(5, 45))]


def _engine(enforce_eager):
    from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config("tiny-qwen3")  # K = 256 and 512
    mc.quantization = "mxfp4"
    mc.mxfp4_activations = "mxfp8"
    sched = SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=512,
                            max_model_len=256)
    cfg = EngineConfig(model=mc, cache=CacheConfig(num_gpu_blocks=128),
                       scheduler=sched, seed=13, enforce_eager=enforce_eager)
    return LLMEngine(cfg, device=DEV)


def test_engine_graph_decode_matches_eager():
    from fusioninfer_amd.engine.sequence import SamplingParams

    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    eager = _engine(True).generate(PROMPTS, sp)
    graphed = _engine(False).generate(PROMPTS, sp)
    for a, b in zip(eager, graphed):
        assert len(a.output_token_ids) == 16
        assert a.output_token_ids == b.output_token_ids


def prefill_logits(eng, prompt):
    from fusioninfer_amd.engine.block_manager import BlockManager
    from fusioninfer_amd.engine.sequence import SamplingParams, Sequence

    bm = BlockManager(eng.runner.num_gpu_blocks, eng.cfg.cache.block_size)
    seq = Sequence("s", list(prompt), SamplingParams())
    bm.allocate(seq)
    return eng.runner.execute_prefill([seq], bm).double().cpu()


def test_engine_prefill_logits_close_to_reference_ops(monkeypatch):
    """The 40-token prefill (M = 40) against the same engine with both new
    ops replaced by the reference functions on the GPU tensors: the same
    quantisation, the GEMM as F.linear on the dequantised bf16 operands."""
    eng = _engine(True)
    got = prefill_logits(eng, PROMPTS[2])
    monkeypatch.setattr(ops, "quant_mxfp8_rows",
                        lambda x, out=None: ref.mxfp8_quant_rows(x))
    monkeypatch.setattr(
        ops, "mxfp4_mxfp8_linear",
        lambda xq, xs, wp, ws, bias=None, out=None: F.linear(
            ref.mxfp8_dequant(xq, xs), ref.mxfp4_dequant(wp, ws), bias))
    want = prefill_logits(eng, PROMPTS[2])
    err = row_rel_err(got, want)
    print(f"mxfp8-mode prefill logits row_rel_err {err:.3e} (bound {LOGITS_BOUND})")
    assert err < LOGITS_BOUND
