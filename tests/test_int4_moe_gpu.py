"""Grouped W4A16 GEMM on int4 experts (moe_int4_gemm.hip) and the engine mode
on the GPU.

Dequantisation is exact in bf16, so the oracle everywhere is a float64
product on dq(W) from reference.int4_dequant. Shapes, routing and sentinel
are those of test_mxfp4_moe_gpu.py (its docstring has the reasons)."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
import tests.test_mxfp4_moe_gpu as mx_gpu
from fusioninfer_amd import quantization as Q
from int4_cases import prefill_logits
from tests.test_mxfp4_moe_gpu import (BLOCK_MS, DEV, KS, LONG_PROMPT, NS,
                                      PROMPTS, SENTINEL, TOPK, E, T, _gen,
                                      bf16_moe_gemm, by_slot, routing,
                                      row_rel_err)

pytestmark = pytest.mark.gpu

GS = (32, 64, 128)
_cache = {}


def experts(NB, K, G, kind):
    """((packed, scale, zero), dq(W) [E, NB, K] bf16), on the GPU. "codes":
    random codes, zeros with 0 and 15 and fp16 scales with 2^-14 and 2^8 in
    every expert; "unit": scale 1.0; "gauss": quantised Gaussian weights."""
    key = (NB, K, G, kind)
    if key not in _cache:
        g = _gen(NB * 7919 + K + G)
        if kind == "gauss":
            w = torch.randn(E, NB, K, generator=g) * 0.05
            p, s, z = (torch.stack(t) for t in zip(
                *(Q.quantize_weight_int4(w[e], G) for e in range(E))))
        else:
            p = torch.randint(0, 256, (E, NB, K // 2), generator=g).to(torch.uint8)
            z = torch.randint(0, 16, (E, NB, K // G), generator=g).to(torch.uint8)
            z[:, 0, 0], z[:, -1, -1] = 0, 15
            s = torch.exp2(torch.randint(-14, 9, z.shape, generator=g).float())
            s *= 1 + torch.randint(0, 1024, z.shape, generator=g) / 1024
            s[:, 0, -1], s[:, -1, 0] = 2.0 ** -14, 2.0 ** 8
            s = torch.ones_like(s).half() if kind == "unit" else s.half()
        ops.validate_int4_scales(s, z)
        dq = torch.stack([ref.int4_dequant(p[e], s[e], z[e], G)
                          for e in range(E)])
        _cache[key] = (p.to(DEV), s.to(DEV), z.to(DEV)), dq.to(DEV)
    return _cache[key]


def run(a, w, G, block_m, gate_up, N, route=None):
    """One launch over a sentinel-filled out; checks the untouched tail."""
    _, s, e, n, pos, PM = route or routing(block_m)
    out = torch.full((PM, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
    assert ops.moe_gemm_int4(out, a, *w, G, s, e, n, block_m, gate_up) is out
    tail = out[int(n) * block_m:]
    assert tail.numel() >= 2 * block_m * N
    assert bool((tail == SENTINEL).all()), "a tile >= n_valid was written"
    return out


@pytest.mark.parametrize("block_m", BLOCK_MS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("G", GS)
def test_column_readout_exact(G, K, N, block_m):
    """One-hot act rows read single columns of dq(W[e]) back, bit for bit:
    nibble order, group indexing at every G, the expert stride, the
    zero/scale pairing and the LDS panel's addressing at block_m 128."""
    w, dq = experts(N, K, G, "codes")
    topi, _, _, _, pos, _ = routing(block_m)
    ks = [k for k in (0, 1, 7, 8, 31, 32, 33, 63, 64, 127, 128, 255, 256)
          if k < K] + [K - 1]
    km = torch.tensor([ks[(5 * i + 3) % len(ks)] for i in range(T * TOPK)])
    rows = torch.zeros(T * TOPK, K, dtype=torch.bfloat16)
    rows[torch.arange(T * TOPK), km] = 1.0
    out = run(by_slot(rows, block_m), w, G, block_m, False, N)
    want = dq[topi.reshape(-1).long().to(DEV), :, km.to(DEV)]  # [80, N]
    assert torch.equal(out[pos.long()], want), (G, K, N, block_m)


@pytest.mark.parametrize("block_m", BLOCK_MS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_integer_gemm_exact(K, N, block_m):
    """Scale 1.0 and act in [-4, 4]: every product is an integer and
    |sum| <= 4 * 15 * 384 = 23040 < 2^24, so fp32 accumulation is exact in
    any order."""
    w, dq = experts(N, K, G := 64, "unit")
    topi, s, e, n, pos, PM = routing(block_m)
    rows = torch.randint(-4, 5, (T * TOPK, K), generator=_gen(K + N)).to(
        torch.bfloat16)
    act = by_slot(rows, block_m)
    out = run(act, w, G, block_m, False, N)
    want = torch.full((PM, N), SENTINEL, dtype=torch.bfloat16)
    ref.moe_gemm_int4(want, act.cpu(), *(t.cpu() for t in w), G, s.cpu(),
                      e.cpu(), n.cpu(), block_m, False)
    assert torch.equal(out.cpu(), want), (K, N, block_m)
    w64 = dq[topi.reshape(-1).long().to(DEV)].double()  # [80, N, K]
    want64 = torch.einsum("ink,ik->in", w64, rows.to(DEV).double())
    assert torch.equal(out[pos.long()], want64.to(torch.bfloat16))


def inputs(K, N, gate_up, block_m, seed):
    """(a, per-assignment rows [80, K] on the GPU) for either epilogue."""
    g = _gen(seed)
    if gate_up:
        x = (torch.randn(T, K, generator=g) * 4).to(torch.bfloat16).to(DEV)
        return x, x.repeat_interleave(TOPK, dim=0)
    rows = torch.randn(T * TOPK, K, generator=g).to(torch.bfloat16)
    return by_slot(rows, block_m), rows.to(DEV)


@pytest.mark.parametrize("gate_up", [False, True])
@pytest.mark.parametrize("block_m", BLOCK_MS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_data_row_error(K, N, block_m, gate_up):
    """Against an fp64 product on dq(W), row by row: at most twice the error
    of the bf16 grouped GEMM on the same inputs (another K order) plus one
    bf16 ulp of the row's largest element (the final rounding)."""
    w, dq = experts(2 * N if gate_up else N, K, 128, "gauss")
    topi, _, _, _, pos, _ = routing(block_m)
    a, rows = inputs(K, N, gate_up, block_m, 3 * K + N + gate_up)
    want = torch.einsum("ink,ik->in", dq[topi.reshape(-1).long().to(DEV)]
                        .double(), rows.double())
    if gate_up:
        want = torch.nn.functional.silu(want[:, :N]) * want[:, N:]
    got = run(a, w, 128, block_m, gate_up, N)[pos.long()]
    base = bf16_moe_gemm(a, dq, block_m, gate_up, N)[pos.long()]
    err = (got.double() - want).norm(dim=-1)
    err_bf = (base.double() - want).norm(dim=-1)
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().amax(dim=-1))) - 7)
    print(f"moe_gemm_int4 K={K} N={N} block_m={block_m} gate_up={gate_up} "
          f"row_rel_err int4 {row_rel_err(got, want):.3e} "
          f"bf16 moe_gemm {row_rel_err(base, want):.3e}")
    assert bool((err <= 2 * err_bf + ulp).all()), (
        (err - 2 * err_bf - ulp).max().item())


@pytest.mark.parametrize("gate_up", [False, True])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_bitwise_invariance(K, N, gate_up):
    """The bits of a (token, expert) row do not depend on block_m, on the
    slot, on the other tokens in the batch or on the call."""
    w, _ = experts(2 * N if gate_up else N, K, 128, "gauss")
    outs = {}
    for block_m in BLOCK_MS:
        a, rows = inputs(K, N, gate_up, block_m, K + 5 * N + gate_up)
        pos = routing(block_m)[4].long()
        outs[block_m] = run(a, w, 128, block_m, gate_up, N)[pos]
        again = run(a, w, 128, block_m, gate_up, N)[pos]
        assert torch.equal(outs[block_m], again), "two calls differ"
    assert torch.equal(outs[16], outs[128]), "block_m 16 and 128 differ"
    topi = routing(16)[0]
    for t in (0, 17, 39):  # alone: one token, its two assignments
        for block_m in BLOCK_MS:
            route = (topi[t:t + 1],) + ops.moe_align(
                topi[t:t + 1].to(DEV), 0, E, block_m)
            pos, PM = route[4].long(), route[5]
            a = torch.zeros(PM, K, dtype=torch.bfloat16, device=DEV)
            a[pos] = rows[TOPK * t:TOPK * (t + 1)]
            if gate_up:
                a = rows[TOPK * t:TOPK * t + 1].contiguous()
            alone = run(a, w, 128, block_m, gate_up, N, route)[pos]
            assert torch.equal(alone, outs[16][TOPK * t:TOPK * (t + 1)]), (
                t, block_m)


@pytest.mark.parametrize("bad", [
    lambda k: k.update(a=k["a"].half()),
    lambda k: k.update(block_m=64),
    lambda k: k.update(w_packed=k["w_packed"].cpu()),
    lambda k: k.update(a=k["a"][:, :96].contiguous()),
    lambda k: k.update(sorted_ids=k["sorted_ids"][:-1]),
    lambda k: k.update(group_size=48),
    lambda k: k.update(w_zero=k["w_zero"][:, :, :1].contiguous()),
])
def test_op_rejects_before_launch(bad):
    (p, s, z), _ = experts(16, 128, 32, "codes")
    _, sid, eid, n, _, PM = routing(16)
    kw = dict(out=torch.zeros(PM, 16, dtype=torch.bfloat16, device=DEV),
              a=torch.zeros(PM, 128, dtype=torch.bfloat16, device=DEV),
              w_packed=p, w_scale=s, w_zero=z, group_size=32, sorted_ids=sid,
              expert_ids=eid, n_valid=n, block_m=16, gate_up=False)
    bad(kw)
    with pytest.raises(ValueError, match="moe_gemm_int4"):
        ops.moe_gemm_int4(**kw)


G_ENGINE = 64


def _engine(quant, enforce_eager, device=DEV):
    """The limits of test_mxfp4_moe_gpu._engine: 1024 tokens are block_m 128."""
    from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config("tiny-qwen3-moe")
    mc.quantization, mc.int4_group_size = quant, G_ENGINE
    mc.int4_moe_experts = quant == "int4"
    cfg = EngineConfig(
        model=mc, cache=CacheConfig(num_gpu_blocks=128),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=1024, max_model_len=1088),
        seed=13, enforce_eager=enforce_eager)
    return LLMEngine(cfg, device=device)


def test_engine_graph_decode_matches_eager():
    from fusioninfer_amd.engine.sequence import SamplingParams
    from fusioninfer_amd.models.model import MoEMLP

    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    eng = _engine("int4", True)
    mlps = [m for m in eng.runner.model.modules() if isinstance(m, MoEMLP)]
    assert mlps and all(m.int4 and m.gate_up_t.numel() == 0 for m in mlps)
    eager = eng.generate(PROMPTS, sp)
    graphed = _engine("int4", False).generate(PROMPTS, sp)
    assert all(len(o.output_token_ids) == 16 for o in eager)
    assert [o.output_token_ids for o in eager] == [
        o.output_token_ids for o in graphed]


def _dq(w):
    return Q.dequantize_int4(*Q.quantize_weight_int4(w, G_ENGINE), G_ENGINE)


def dequantised_engine():
    """test_mxfp4_moe_gpu.dequantised_engine on this module's engine and dq:
    a bf16 GPU engine whose projections and experts are dq(quantize(w))."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(mx_gpu, "_engine", _engine)
        mp.setattr(mx_gpu, "_dq", _dq)
        return mx_gpu.dequantised_engine()


# Two bf16 implementations are compared, so the bound is 4x a measured floor,
# per prompt: the max-abs difference of the prefill logits between the
# dequantised bf16 engine on the GPU and the same weights on the CPU
# reference ops (neither is code under test; tools/mxfp4_moe_logits_floor.py
# test_int4_moe_gpu, profiles/r20_int4_moe.md). Measured 7.8125e-3 at 40
# tokens and 3.4668e-1 at 1024, where one row differs grossly between the two
# bf16 engines, so that bound says little. The int4 engine itself measured
# 3.906e-3 against the dequantised bf16 engine on both prompts.
LOGITS_FLOOR = {40: 7.82e-3, 1024: 3.47e-1}


def test_engine_prefill_logits_close_to_dequantised_bf16(monkeypatch):
    want_eng, got_eng = dequantised_engine(), _engine("int4", True)
    seen, real = set(), ops.moe_gemm_int4
    monkeypatch.setattr(
        ops, "moe_gemm_int4", lambda *a, **k: seen.add(a[9]) or real(*a, **k))
    for prompt in (PROMPTS[2], LONG_PROMPT):
        bound = 4 * LOGITS_FLOOR[len(prompt)]
        want = prefill_logits(want_eng, prompt)
        err = (prefill_logits(got_eng, prompt) - want).abs().max().item()
        print(f"int4 MoE prefill logits, {len(prompt)} tokens: max abs diff "
              f"{err:.3e} (bound {bound}, max |logit| "
              f"{want.abs().max().item():.3f})")
        assert err < bound, len(prompt)
    assert seen == {16, 128}, seen  # both instances ran inside the engine
