"""moe_mxfp4_mxfp8_gemm32_kernel (block_m 32) and `mxfp8-wide` on the GPU,
against float64 on the dequantised operands. E = 4, 100 tokens, top-2, routed
0 / 1 / 33 / 166: an empty expert, a one-row tile, a full tile plus one row,
five tiles plus a partial one. K: 1, 2, 3 and 5 steps (prefetch depth 3, trip
4). Outputs start as sentinels; tiles at or past n_valid must keep them."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q
from tests.test_mxfp4_moe_a8_gpu import (DEV, E4M3, LOGITS_BOUND,
                                         ROW_REL_BOUND, SENTINEL, _engine,
                                         by_slot, row_rel_err)
from tests.test_mxfp4_moe_gpu import PROMPTS, _gen, prefill_logits

pytestmark = pytest.mark.gpu

E, T, TOPK = 4, 100, 2
A = T * TOPK
KS = (128, 256, 384, 640)
shapes = lambda ns: pytest.mark.parametrize(  # noqa: E731
    "K,N", [(K, N) for K in KS for N in ns])
down_shapes, gate_up_shapes = shapes((16, 272)), shapes((32, 160))
_cache = {}


def routing(bm=32, topi=None):
    """(topi CPU, sorted_ids, expert_ids, n_valid, pos, PM); PM / bm ids"""
    if topi is not None:
        s, e, n, pos, PM = ops.moe_align(topi.to(DEV), 0, E, bm)
        return (topi, s, e, n, pos.long(), PM)
    if bm not in _cache:
        flat = torch.tensor([1] * 1 + [2] * 33 + [3] * 166)
        topi = flat[torch.randperm(A, generator=_gen(7))].view(T, TOPK).int()
        _cache[bm] = routing(bm, topi)
        assert int(_cache[bm][3]) == (9 if bm == 32 else 4)
    return _cache[bm]


def dequant(p, s):
    """dq(W) gathered per assignment: [A, NB, K] float64 on the GPU."""
    dq = torch.stack([ref.mxfp4_dequant(p[e], s[e]) for e in range(E)])
    return dq.to(DEV)[routing()[0].reshape(-1).long().to(DEV)].double()


def experts(NB, K, lo=None, hi=None):
    """GPU (packed, scale, dequant): random codes with scale bytes in [lo,
    hi], or quantised Gaussian weights when lo is None."""
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


def run(aq, asc, packed, scale, N, gate_up, route=None):
    """One launch over sentinel-filled outputs; checks the untouched tail.
    Returns the rows by assignment: bf16, or [bytes | scale bytes] uint8."""
    _, s, e, n, pos, PM = route or routing()
    bm = PM // e.numel()
    raw = torch.full((PM, N * (1 if gate_up else 2)), SENTINEL,
                     dtype=torch.uint8, device=DEV)
    out = raw.view(E4M3 if gate_up else torch.bfloat16)
    osc = torch.full((PM, N // 32), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.moe_gemm_mxfp4_mxfp8(out, aq.to(DEV), asc.to(DEV), packed, scale, s, e,
                             n, gate_up, osc if gate_up else None, block_m=bm)
    tail = int(n) * bm
    assert PM - tail >= bm
    assert bool((raw[tail:] == SENTINEL).all()), "a tile >= n_valid was written"
    assert bool((osc[tail:] == SENTINEL).all())
    return torch.cat([raw, osc], 1)[pos] if gate_up else out[pos]


@down_shapes
def test_down(K, N):
    """One-hot rows read single columns of dq(W[e]) back times their own
    block's scale; an integer GEMM whose fp32 sums are exact in any order
    (|sum| <= 640 * 4 * 6, steps of 0.5); random data within 2^-7 row-wise."""
    packed, scale, dq = experts(N, K, 119, 135)
    ks = [k for k in (0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 511, 512)
          if k < K] + [K - 1]
    i = torch.arange(A)
    km = torch.tensor([ks[(5 * j + 3) % len(ks)] for j in range(A)])
    hot = torch.tensor([127, 125, 130])[i % 3]
    x = torch.zeros(A, K)
    x[i, km] = 1.0
    xs = torch.randint(119, 136, (A, K // 32), generator=_gen(K + N))
    xs[i, km // 32] = hot
    out = run(*by_slot(x.to(E4M3), xs.to(torch.uint8), routing()), packed,
              scale, N, False)
    want = dq[i, :, km] * torch.exp2(hot.double() - 127).to(DEV)[:, None]
    assert torch.equal(out, want.to(torch.bfloat16))
    packed, scale, dq = experts(N, K, 127, 127)
    rows = torch.randint(-4, 5, (A, K), generator=_gen(K + N)).to(torch.bfloat16)
    q, s = ref.mxfp8_quant_rows(rows)
    assert torch.equal(ref.mxfp8_dequant(q, s), rows)
    out = run(*by_slot(q, s, routing()), packed, scale, N, False)
    want = torch.einsum("ink,ik->in", dq, rows.to(DEV).double())
    assert torch.equal(out, want.to(torch.bfloat16))
    packed, scale, dq = experts(N, K)
    rows = torch.randn(A, K, generator=_gen(3 * K + N)).to(torch.bfloat16)
    q, s = ref.mxfp8_quant_rows(rows)
    out = run(*by_slot(q, s, routing()), packed, scale, N, False)
    want = torch.einsum("ink,ik->in", dq,
                        ref.mxfp8_dequant(q, s).to(DEV).double())
    err = row_rel_err(out, want).max().item()
    print(f"block_m 32 down K={K} N={N} max row_rel_err {err:.3e}")
    assert err < ROW_REL_BOUND


@gate_up_shapes
def test_gate_up_fused_epilogue_exact(K, N):
    """g = 64 everywhere (x[:, k0] = 1 against one 4.0 code at scale byte
    131) and swiglu(64, u) = 64 u in fp32; u is an exact integer GEMM. Bytes
    and scale bytes must be mxfp8_quant_rows(bf16(64 u))."""
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


@gate_up_shapes
def test_gate_up_random_data_row_error(K, N):
    """The rule of tests/test_mxfp4_moe_a8_gpu.py: at most the reference
    quantiser's own error on bf16(act64) plus 2^-6, at equal scale bytes;
    rows with a block amax within 2^-7 of a power of two are left out (at
    most 20 %; derivation in docs/kernels.md)."""
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
    keep = ~((frac < 1 + 2.0 ** -7) | (frac > 2 * (1 - 2.0 ** -7))).any(dim=-1)
    err = row_rel_err(ref.mxfp8_dequant(got_q, got_s), act64)
    out = 1 - keep.float().mean().item()
    print(f"block_m 32 gate_up K={K} N={N} left out {out:.3f}, e_ref max "
          f"{e_ref.max().item():.3e}, max (err - e_ref) "
          f"{(err - e_ref)[keep].max().item():.3e}")
    assert out <= 0.20
    assert torch.equal(got_s[keep], ref_s[keep])
    assert bool((err[keep] <= e_ref[keep] + 2.0 ** -6).all())


@pytest.mark.parametrize("K", KS)
def test_bitwise_invariance(K):
    """A (token, expert) row has the bits of the block_m 128 instance; a
    token alone equals its rows in the batch; a down row equals
    mxfp4_mxfp8_linear on that row and its expert's weights."""
    NG, ND = 160, 272
    (gu_p, gu_s, _), (dn_p, dn_s, _) = experts(2 * NG, K), experts(ND, K)
    r32, r128, g = routing(), routing(128), _gen(K + 5)
    topi = r32[0]
    xq, xs = ref.mxfp8_quant_rows(
        (4 * torch.randn(T, K, generator=g)).to(torch.bfloat16))
    q, s = ref.mxfp8_quant_rows(torch.randn(A, K, generator=g).to(torch.bfloat16))
    gu = run(xq, xs, gu_p, gu_s, NG, True)
    dn = run(*by_slot(q, s, r32), dn_p, dn_s, ND, False)
    assert torch.equal(run(xq, xs, gu_p, gu_s, NG, True, r128), gu)
    assert torch.equal(run(*by_slot(q, s, r128), dn_p, dn_s, ND, False, r128), dn)
    for t in (0, 17, 99):
        one, route = slice(TOPK * t, TOPK * (t + 1)), routing(32, topi[t:t + 1])
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
                sorted_ids=s, expert_ids=e, n_valid=n, gate_up=False,
                block_m=32)
    ops.moe_gemm_mxfp4_mxfp8(**base)
    q48 = torch.zeros(PM, 48, dtype=E4M3, device=DEV)
    s1 = torch.zeros(PM, 1, dtype=torch.uint8, device=DEV)
    for bad in (
        dict(block_m=16),
        dict(block_m=64),
        dict(out=out[:-16], a_q=aq[:-16], a_scale=asc[:-16],
             sorted_ids=s[:-16]),                             # PM % 32 == 16
        dict(out=q48, out_scale=s1, gate_up=True),            # gate_up N = 48
        dict(out=q48[:, :32].contiguous(), gate_up=True),     # no out_scale
    ):
        with pytest.raises(ValueError, match="moe_gemm_mxfp4_mxfp8"):
            ops.moe_gemm_mxfp4_mxfp8(**{**base, **bad})


def test_engine_mid_size_prefill(monkeypatch):
    """40 tokens on E 8, top-2 are 10 rows per expert: with LO = 4 and HI =
    64 both GEMMs run at block_m 32 and the logits match the same engine on
    the reference op; mxfp8 still equals the default mode bit for bit."""
    import fusioninfer_amd.models.model as M

    monkeypatch.setattr(M, "MXFP4_MOE_WIDE_LO", 4)
    monkeypatch.setattr(M, "MXFP4_MOE_WIDE_HI", 64)
    eng, seen, real = _engine("mxfp8-wide"), [], ops.moe_gemm_mxfp4_mxfp8
    monkeypatch.setattr(
        ops, "moe_gemm_mxfp4_mxfp8",
        lambda *a, **k: seen.append((a[8], k["block_m"])) or real(*a, **k))
    got = prefill_logits(eng, PROMPTS[2])
    assert set(seen) == {(True, 32), (False, 32)}
    monkeypatch.setattr(ops, "moe_gemm_mxfp4_mxfp8", ref.moe_gemm_mxfp4_mxfp8)
    err = row_rel_err(got, prefill_logits(eng, PROMPTS[2])).max().item()
    print(f"mxfp8-wide prefill logits row_rel_err {err:.3e} < {LOGITS_BOUND}")
    assert err < LOGITS_BOUND
    assert torch.equal(prefill_logits(_engine("mxfp8"), PROMPTS[2]),
                       prefill_logits(_engine("bf16"), PROMPTS[2]))
