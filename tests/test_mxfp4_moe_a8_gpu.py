"""Grouped MXFP4 x MXFP8 scaled-MFMA GEMM for MoE experts
(moe_mxfp8_gemm.hip) and `mxfp4_moe_activations="mxfp8"` on the GPU.

The oracle is float64 on the (exactly) dequantised operands. E = 4, 100
tokens, top-2, routed 0 / 1 / 17 / 182: an empty expert, a one-row tile, a
full tile plus a partial one. K: one step (peeled), an even and an odd count;
N: masked and partial column tiles. Rows are compared through `pos`; outputs
start as sentinels and tiles at or past n_valid must keep them."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q
from tests.test_mxfp4_moe_gpu import LONG_PROMPT, PROMPTS, _gen, prefill_logits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E4M3 = torch.float8_e4m3fn
E, T, TOPK, BM = 4, 100, 2, 128
A = T * TOPK
SENTINEL = 0x55
# bf16 rounding is within 2^-9; 4x for the order (docs/kernels.md convention)
ROW_REL_BOUND = 2.0 ** -7
LOGITS_BOUND = 3.14e-2  # as tests/test_mxfp4_a8_gpu.py
shapes = lambda ns: pytest.mark.parametrize(  # noqa: E731
    "K,N", [(K, N) for K in (128, 256, 384) for N in ns])
down_shapes, gate_up_shapes = shapes((16, 144)), shapes((32, 96))

_cache = {}


def routing():
    """(topi CPU, sorted_ids, expert_ids, n_valid, pos, PM)"""
    if "route" not in _cache:
        flat = torch.tensor([1] * 1 + [2] * 17 + [3] * 182)
        topi = flat[torch.randperm(A, generator=_gen(7))].view(T, TOPK).int()
        s, e, n, pos, PM = ops.moe_align(topi.to(DEV), 0, E, BM)
        assert int(n) == 4 and PM // BM >= 6
        _cache["route"] = (topi, s, e, n, pos.long(), PM)
    return _cache["route"]


def experts(NB, K, lo=None, hi=None):
    """GPU (packed, scale, dq(W) [E, NB, K]): random codes with scale bytes
    in [lo, hi], or quantised Gaussian weights when lo is None."""
    key = (NB, K, lo, hi)
    if key not in _cache:
        g = _gen(NB * 7919 + K)
        if lo is None:
            w = torch.randn(E, NB, K, generator=g) * 0.05
            p, s = (torch.stack(t) for t in zip(
                *(Q.quantize_weight_mxfp4(w[e]) for e in range(E))))
        else:
            p = torch.randint(0, 256, (E, NB, K // 2), generator=g).to(torch.uint8)
            s = torch.randint(lo, hi + 1, (E, NB, K // 32), generator=g).to(torch.uint8)
        _cache[key] = (p.to(DEV), s.to(DEV), dequant(p, s))
    return _cache[key]


def dequant(p, s):
    """dq(W) gathered per assignment: [A, NB, K] float64 on the GPU."""
    dq = torch.stack([ref.mxfp4_dequant(p[e], s[e]) for e in range(E)])
    return dq.to(DEV)[routing()[0].reshape(-1).long().to(DEV)].double()


def by_slot(q, s, route=None):
    """Per-assignment rows -> act [PM, .]; pad slots zero with scale 127."""
    _, _, _, _, pos, PM = route or routing()
    aq = torch.zeros(PM, q.shape[1], dtype=torch.uint8, device=DEV)
    asc = torch.full((PM, s.shape[1]), 127, dtype=torch.uint8, device=DEV)
    aq[pos] = q.view(torch.uint8).to(DEV)
    asc[pos] = s.to(DEV)
    return aq.view(E4M3), asc


def run(aq, asc, packed, scale, N, gate_up, route=None):
    """One launch over sentinel-filled outputs; checks the untouched tail.
    Returns the rows by assignment: bf16, or [bytes | scale bytes] uint8."""
    _, s, e, n, pos, PM = route or routing()
    raw = torch.full((PM, N * (1 if gate_up else 2)), SENTINEL,
                     dtype=torch.uint8, device=DEV)
    out = raw.view(E4M3 if gate_up else torch.bfloat16)
    osc = torch.full((PM, N // 32), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.moe_gemm_mxfp4_mxfp8(out, aq.to(DEV), asc.to(DEV), packed, scale, s, e,
                             n, gate_up, osc if gate_up else None)
    tail = int(n) * BM
    assert PM - tail >= BM
    assert bool((raw[tail:] == SENTINEL).all()), "a tile >= n_valid was written"
    assert bool((osc[tail:] == SENTINEL).all())
    return torch.cat([raw, osc], 1)[pos] if gate_up else out[pos]


def row_rel_err(got, want64):
    return (got.double() - want64).norm(dim=-1) / want64.norm(dim=-1)


@down_shapes
def test_down_one_hot_readout_exact(K, N):
    """A single 1.0 per act row reads one column of dq(W[e]) back, times its
    own block's scale: nibble order, both fragment layouts, scale routing
    (every other activation scale is random), expert stride, slot -> row."""
    packed, scale, dq = experts(N, K, 119, 135)
    ks = [k for k in (0, 1, 15, 16, 31, 32, 63, 64, 127, 128) if k < K] + [K - 1]
    i = torch.arange(A)
    km = torch.tensor([ks[(5 * j + 3) % len(ks)] for j in range(A)])
    hot = torch.tensor([127, 125, 130])[i % 3]
    x = torch.zeros(A, K)
    x[i, km] = 1.0
    xs = torch.randint(119, 136, (A, K // 32), generator=_gen(K + N))
    xs[i, km // 32] = hot
    out = run(*by_slot(x.to(E4M3), xs.to(torch.uint8)), packed, scale, N, False)
    want = dq[i, :, km] * torch.exp2(hot.double() - 127).to(DEV)[:, None]
    assert torch.equal(out, want.to(torch.bfloat16))


@down_shapes
def test_down_integer_gemm_exact(K, N):
    """act in [-4, 4] is exact under mxfp8_quant_rows and the weight scale
    byte is 127: products are multiples of 0.5, |sum| <= 384 * 4 * 6, so
    fp32 accumulation is exact in any order."""
    packed, scale, dq = experts(N, K, 127, 127)
    rows = torch.randint(-4, 5, (A, K), generator=_gen(K + N)).to(torch.bfloat16)
    q, s = ref.mxfp8_quant_rows(rows)
    assert torch.equal(ref.mxfp8_dequant(q, s), rows)
    out = run(*by_slot(q, s), packed, scale, N, False)
    want = torch.einsum("ink,ik->in", dq, rows.to(DEV).double())
    assert torch.equal(out, want.to(torch.bfloat16))


@gate_up_shapes
def test_gate_up_fused_epilogue_exact(K, N):
    """g = 64 everywhere (x[:, k0] = 1 against one 4.0 code at scale byte
    131) and swiglu(64, u) = 64 u in fp32; u is an exact integer GEMM. Bytes
    and scale bytes must be mxfp8_quant_rows(bf16(64 u)): the gather, the
    gate/up pairing, the cross-lane amax, scale rule, clamp, packing, -0."""
    k0, g = 37, _gen(K + N)
    codes = torch.randint(0, 16, (E, 2 * N, K), generator=g).to(torch.uint8)
    codes[:, :N] = 0
    codes[:, :N, k0] = 6  # e2m1 4.0
    codes[:, N:, k0] = 0
    packed = (codes[..., 0::2] | (codes[..., 1::2] << 4)).contiguous()
    scale = torch.full((E, 2 * N, K // 32), 127, dtype=torch.uint8)
    scale[:, :N] = 131
    x = torch.randint(-4, 5, (T, K), generator=g).to(torch.bfloat16)
    x[:, k0] = 1
    xq, xs = ref.mxfp8_quant_rows(x)
    assert torch.equal(ref.mxfp8_dequant(xq, xs), x)
    got = run(xq, xs, packed.to(DEV), scale.to(DEV), N, True)
    rows = x.repeat_interleave(TOPK, dim=0).to(DEV).double()
    acc = torch.einsum("ink,ik->in", dequant(packed, scale), rows)
    assert bool((acc[:, :N] == 64).all())
    want_q, want_s = ref.mxfp8_quant_rows((64 * acc[:, N:]).to(torch.bfloat16))
    assert torch.equal(got, torch.cat([want_q.view(torch.uint8), want_s], 1))


@down_shapes
def test_down_random_data_row_error(K, N):
    packed, scale, dq = experts(N, K)
    rows = torch.randn(A, K, generator=_gen(3 * K + N)).to(torch.bfloat16)
    q, s = ref.mxfp8_quant_rows(rows)
    out = run(*by_slot(q, s), packed, scale, N, False)
    want = torch.einsum("ink,ik->in", dq,
                        ref.mxfp8_dequant(q, s).to(DEV).double())
    err = row_rel_err(out, want).max().item()
    print(f"moe_gemm_mxfp4_mxfp8 down K={K} N={N} max row_rel_err {err:.3e}")
    assert err < ROW_REL_BOUND


@gate_up_shapes
def test_gate_up_random_data_row_error(K, N):
    """Dequantised act row against float64: at most the reference quantiser's
    own error on bf16(act64) plus 2^-6 (a code moves only across a rounding
    midpoint: twice the act perturbation, itself <= 2^-7), at equal scale
    bytes. Rows with a block amax within 2^-7 of a power of two are left out
    (at most 20 %); derivation in docs/kernels.md."""
    packed, scale, dq = experts(2 * N, K)
    x = (4 * torch.randn(T, K, generator=_gen(3 * K + N + 1))).to(torch.bfloat16)
    xq, xs = ref.mxfp8_quant_rows(x)
    got = run(xq, xs, packed, scale, N, True)
    got_q, got_s = got[:, :N].contiguous().view(E4M3), got[:, N:]
    rows = ref.mxfp8_dequant(xq, xs).repeat_interleave(TOPK, dim=0).to(DEV)
    acc = torch.einsum("ink,ik->in", dq, rows.double())
    act64 = torch.nn.functional.silu(acc[:, :N]) * acc[:, N:]
    ref_q, ref_s = ref.mxfp8_quant_rows(act64.to(torch.bfloat16))
    e_ref = row_rel_err(ref.mxfp8_dequant(ref_q, ref_s), act64)
    amax = act64.view(A, N // 32, 32).abs().amax(dim=-1)
    frac = amax / torch.exp2(torch.floor(torch.log2(amax)))  # [1, 2)
    near = ((frac < 1 + 2.0 ** -7) | (frac > 2 * (1 - 2.0 ** -7))).any(dim=-1)
    keep = ~near
    err = row_rel_err(ref.mxfp8_dequant(got_q, got_s), act64)
    print(f"moe_gemm_mxfp4_mxfp8 gate_up K={K} N={N} left out "
          f"{near.float().mean().item():.3f}, e_ref max {e_ref.max().item():.3e}, "
          f"max (err - e_ref) {(err - e_ref)[keep].max().item():.3e}")
    assert near.float().mean().item() <= 0.20
    assert torch.equal(got_s[keep], ref_s[keep])
    assert bool((err[keep] <= e_ref[keep] + 2.0 ** -6).all())


@pytest.mark.parametrize("K", (128, 256, 384))
def test_bitwise_invariance(K):
    """Two calls agree; a token alone equals its rows in the batch; a down
    row equals mxfp4_mxfp8_linear on that row and its expert's weights."""
    NG, ND = 96, 144
    gu_p, gu_s, _ = experts(2 * NG, K)
    dn_p, dn_s, _ = experts(ND, K)
    topi = routing()[0]
    g = _gen(K + 5)
    xq, xs = ref.mxfp8_quant_rows(
        (4 * torch.randn(T, K, generator=g)).to(torch.bfloat16))
    q, s = ref.mxfp8_quant_rows(torch.randn(A, K, generator=g).to(torch.bfloat16))
    gu = run(xq, xs, gu_p, gu_s, NG, True)
    dn = run(*by_slot(q, s), dn_p, dn_s, ND, False)
    assert torch.equal(run(xq, xs, gu_p, gu_s, NG, True), gu)
    assert torch.equal(run(*by_slot(q, s), dn_p, dn_s, ND, False), dn)
    for t in (0, 17, 99):
        one = slice(TOPK * t, TOPK * (t + 1))
        route = (topi[t:t + 1],) + ops.moe_align(topi[t:t + 1].to(DEV), 0, E, BM)
        route = route[:4] + (route[4].long(), route[5])
        alone = run(xq[t:t + 1], xs[t:t + 1], gu_p, gu_s, NG, True, route)
        assert torch.equal(alone, gu[one])
        alone = run(*by_slot(q[one], s[one], route), dn_p, dn_s, ND, False, route)
        assert torch.equal(alone, dn[one])
    for e in range(1, E):
        sel = (topi.reshape(-1) == e).nonzero().flatten()
        rows = q.view(torch.uint8)[sel].view(E4M3).to(DEV)
        want = ops.mxfp4_mxfp8_linear(rows, s[sel].to(DEV), dn_p[e], dn_s[e])
        assert torch.equal(dn[sel.to(DEV)], want), e


def test_op_rejects_before_launch():
    packed, scale, _ = experts(64, 128, 127, 127)
    _, s, e, n, _, PM = routing()
    aq = torch.zeros(PM, 128, dtype=E4M3, device=DEV)
    asc = torch.full((PM, 4), 127, dtype=torch.uint8, device=DEV)
    out = torch.zeros(PM, 64, dtype=torch.bfloat16, device=DEV)
    base = dict(out=out, a_q=aq, a_scale=asc, w_packed=packed, w_scale=scale,
                sorted_ids=s, expert_ids=e, n_valid=n, gate_up=False)
    ops.moe_gemm_mxfp4_mxfp8(**base)
    q48 = torch.zeros(PM, 48, dtype=E4M3, device=DEV)
    s1 = torch.zeros(PM, 1, dtype=torch.uint8, device=DEV)
    for bad in (
        dict(a_q=aq.view(torch.uint8)),                       # wrong dtype
        dict(a_q=aq[:, :96].contiguous(), a_scale=asc[:, :3].contiguous(),
             w_packed=packed[:, :, :48].contiguous(),
             w_scale=scale[:, :, :3].contiguous()),           # K = 96
        dict(out=q48, out_scale=s1, gate_up=True),            # gate_up N = 48
        dict(out=q48[:, :32].contiguous(), gate_up=True),     # no out_scale
        dict(sorted_ids=s[:-1]),                              # PM not % 128
        dict(w_packed=packed.cpu()),                          # CPU weight
    ):
        with pytest.raises(ValueError, match="moe_gemm_mxfp4_mxfp8"):
            ops.moe_gemm_mxfp4_mxfp8(**{**base, **bad})


def _engine(moe_activations):
    from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config("tiny-qwen3-moe")  # H 256, I 128, E 8, top-2
    mc.quantization, mc.mxfp4_moe_experts = "mxfp4", True
    mc.mxfp4_moe_activations = moe_activations
    sched = SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=1024,
                            max_model_len=1088)
    cfg = EngineConfig(model=mc, cache=CacheConfig(num_gpu_blocks=128),
                       scheduler=sched, seed=13, enforce_eager=True)
    return LLMEngine(cfg, device=DEV)


def test_engine_prefill_mxfp8_experts(monkeypatch):
    """1024 tokens (256 * E_local assignments: block_m 128) run both instances
    inside the engine and match the same engine on the reference op; 40
    tokens never reach the op and are bit-equal to an engine without the
    flag."""
    eng, seen, real = _engine("mxfp8"), [], ops.moe_gemm_mxfp4_mxfp8
    monkeypatch.setattr(ops, "moe_gemm_mxfp4_mxfp8",
                        lambda *a, **k: seen.append(a[8]) or real(*a, **k))
    short = prefill_logits(eng, PROMPTS[2])
    assert seen == []
    assert torch.equal(short, prefill_logits(_engine("bf16"), PROMPTS[2]))
    got = prefill_logits(eng, LONG_PROMPT)
    assert set(seen) == {True, False}
    monkeypatch.setattr(ops, "moe_gemm_mxfp4_mxfp8", ref.moe_gemm_mxfp4_mxfp8)
    err = row_rel_err(got, prefill_logits(eng, LONG_PROMPT)).max().item()
    print(f"mxfp8 MoE prefill logits row_rel_err {err:.3e} (bound {LOGITS_BOUND})")
    assert err < LOGITS_BOUND
