"""The adversarial attention inputs can see the mistakes (CPU, references only).

Each mutant below is one way an attention kernel goes subtly wrong. It is
expressed as the float64 reference run on mutated bookkeeping (lengths,
tables, causal positions), and on the inputs of tests/attention_cases.py it
must move the needle head by at least 10x the tolerance the GPU tests give
the kernels. This is a condition on the inputs: if a seed misses it, the
inputs change, not the factor.
"""

import math

import pytest
import torch

import attention_cases as ac
from fusioninfer_amd.ops import reference as ref

BS, PART = ac.BLOCK, ac.PARTITION


def _round_up(n, m):
    return (n + m - 1) // m * m


def _sequential_tables(tables, num_blocks):
    """bt[s, 0] + arange, clamped to valid block ids."""
    width = tables.shape[1]
    seq = tables[:, :1].long() + torch.arange(width).unsqueeze(0)
    return seq.clamp(max=num_blocks - 1).to(torch.int32)


# ------------------------------------------------------------------ decode

# name -> mutated length of a sequence of L tokens (None: cannot alter it)
DECODE_LEN_MUTANTS = {
    "ctx_minus_1": lambda L: L - 1 if L > 1 else None,
    "ctx_rounded_up_to_block": lambda L: (
        _round_up(L, BS) if L % BS else None),
    # a one-chunk row with its only chunk dropped has no defined output
    "last_chunk_dropped": lambda L: (
        (L - 1) // BS * BS if L > BS else None),
    "past_first_512_dropped": lambda L: PART if L > PART else None,
    "last_partition_dropped": lambda L: (
        (L - 1) // PART * PART if L > PART else None),
}


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("group", [1, 4, 8])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_decode_inputs_expose_every_mutant(head_dim, group, fp8):
    lens, table_blocks = ac.DECODE_GRIDS["wide"]
    q, kc, vc, bt, sl = ac.build_decode_case(
        lens, head_dim, group, fp8, table_blocks, seed=11)
    scale = 1.0 / math.sqrt(head_dim)
    want = ac.ref64_decode(q, kc, vc, bt, sl, scale)
    worst = {}

    def check(name, s, got_row):
        err = float(ac.row_rel_err(got_row, want[s]).max())
        worst[name] = min(worst.get(name, math.inf), err)
        assert err >= ac.MUTANT_MIN_ERR, (name, lens[s], err)

    for name, mutate in DECODE_LEN_MUTANTS.items():
        altered = [s for s, L in enumerate(lens) if mutate(L) is not None]
        assert altered, name
        idx = torch.tensor(altered)
        mlens = torch.tensor([mutate(lens[s]) for s in altered],
                             dtype=torch.int32)
        got = ac.ref64_decode(q[idx], kc, vc, bt[idx], mlens, scale)
        for j, s in enumerate(altered):
            check(name, s, got[j])

    seq_bt = _sequential_tables(bt, kc.shape[0])
    got = ac.ref64_decode(q, kc, vc, seq_bt, sl, scale)
    altered = [s for s, L in enumerate(lens)
               if not torch.equal(seq_bt[s, :(L + BS - 1) // BS],
                                  bt[s, :(L + BS - 1) // BS])]
    # every sequence of more than one block must have a scattered table
    assert altered == [s for s, L in enumerate(lens) if L > BS]
    for s in altered:
        check("table_sequential", s, got[s])
    print(f"D={head_dim} G={group} fp8={fp8} min mutant error:",
          {k: round(v, 3) for k, v in worst.items()})


def test_decode_case_structure():
    lens, table_blocks = ac.DECODE_GRIDS["full"]
    q, kc, vc, bt, sl = ac.build_decode_case(lens, 64, 4, False, table_blocks,
                                             seed=3)
    assert bt.shape == (33, 97) and sl.tolist() == lens
    assert int(bt.min()) >= 1 and int(bt.max()) < kc.shape[0]
    owned = torch.cat([bt[s, :(L + BS - 1) // BS] for s, L in enumerate(lens)])
    assert owned.unique().numel() == owned.numel()     # no block shared
    assert not torch.equal(owned, owned.sort().values)  # not ascending
    unowned = sorted(set(range(kc.shape[0])) - set(owned.tolist()))
    assert 0 in unowned and len(unowned) == 1 + len(lens)
    # everything unowned is poisoned and finite
    assert bool((vc[unowned].float() == ac.POISON_V).all())
    assert bool((kc[unowned].float().abs() == ac.POISON_GAIN).all())
    for s, L in enumerate(lens):
        nblk = (L + BS - 1) // BS
        assert set(bt[s, nblk:].tolist()) <= set(unowned)
        if L % BS:
            pad = vc[int(bt[s, nblk - 1]), :, L % BS:].float()
            assert bool((pad == ac.POISON_V).all())
    assert bool(torch.isfinite(kc.float()).all())
    assert bool(torch.isfinite(vc.float()).all())


# ----------------------------------------------------------------- prefill

def _prefill_mutant(case, scale, *, mask_shift=0, round_k_len=False,
                    ctx_start_zero=False, sequential=False):
    """Per-sequence outputs of one prefill mutant, None where the mutant
    cannot alter the sequence."""
    q, kc, vc, bt, cu, slk = case
    tables = _sequential_tables(bt, kc.shape[0]) if sequential else bt
    outs = []
    for s in range(slk.numel()):
        qs, qe = int(cu[s]), int(cu[s + 1])
        k_len, new = int(slk[s]), qe - qs
        nblk = (k_len + BS - 1) // BS
        n = _round_up(k_len, BS) if round_k_len else k_len
        ctx_start = 0 if ctx_start_zero else n - new
        altered = (
            mask_shift != 0 and new > 1 or
            (round_k_len and n != k_len) or
            (ctx_start_zero and k_len != new) or
            (sequential and not torch.equal(tables[s, :nblk], bt[s, :nblk])))
        if not altered:
            outs.append(None)
            continue
        q_pos = ctx_start + mask_shift + torch.arange(new)
        outs.append(ac.attend64(
            q[qs:qe], ac.gather_kv64(kc, tables[s], n),
            ac.gather_kv64(vc, tables[s], n), q_pos, scale))
    return outs


PREFILL_MUTANTS = {
    "causal_mask_shifted_by_1": dict(mask_shift=1),
    "k_len_rounded_up_to_block": dict(round_k_len=True),
    "ctx_start_taken_as_0": dict(ctx_start_zero=True),
    "table_sequential": dict(sequential=True),
}


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_prefill_inputs_expose_every_mutant(head_dim, fp8):
    ctx_lens, new_lens = ac.PREFILL_PAGED
    case = ac.build_prefill_paged_case(ctx_lens, new_lens, head_dim, 8, 2,
                                       fp8, seed=5)
    q, kc, vc, bt, cu, slk = case
    scale = 1.0 / math.sqrt(head_dim)
    want = ac.ref64_prefill_paged(q, kc, vc, bt, cu, slk, scale)
    for name, kwargs in PREFILL_MUTANTS.items():
        outs = _prefill_mutant(case, scale, **kwargs)
        assert any(o is not None for o in outs), name
        for s, got in enumerate(outs):
            if got is None:
                continue
            err = float(ac.row_rel_err(
                got, want[int(cu[s]):int(cu[s + 1])]).max())
            print(f"D={head_dim} fp8={fp8} {name} ctx={ctx_lens[s]} "
                  f"new={new_lens[s]}: {err:.3f}")
            assert err >= ac.MUTANT_MIN_ERR, (name, ctx_lens[s], err)


def test_prefill_mutants_alter_what_they_should():
    """(65, 1) is one row on the diagonal: only the k_len, ctx_start and
    table mutants can touch it; every longer sequence is altered by all."""
    case = ac.build_prefill_paged_case(*ac.PREFILL_PAGED, 64, 8, 2, False,
                                       seed=5)
    hit = {name: [o is not None for o in _prefill_mutant(case, 0.125, **kw)]
           for name, kw in PREFILL_MUTANTS.items()}
    assert hit["causal_mask_shifted_by_1"] == [False, True, True, True, True]
    assert hit["k_len_rounded_up_to_block"] == [True] * 5
    assert hit["ctx_start_taken_as_0"] == [True] * 5
    assert hit["table_sequential"] == [True] * 5


# ------------------------------------------------- the references themselves

def test_ref64_matches_reference_on_float32_inputs():
    q, kc, vc, bt, sl = ac.build_decode_case([1, 17, 255, 513], 64, 4, False,
                                             40, seed=1)
    q, kc, vc = q.float(), kc.float(), vc.float()
    got = ac.ref64_decode(q, kc, vc, bt, sl, 0.125)
    want = ref.paged_attention_decode(q, kc, vc, bt, sl, 0.125)
    assert float(ac.row_rel_err(want, got).max()) < 1e-6

    q, kc, vc, bt, cu, slk = ac.build_prefill_paged_case(
        [65, 81, 300], [1, 64, 283], 64, 8, 2, False, seed=2)
    q, kc, vc = q.float(), kc.float(), vc.float()
    got = ac.ref64_prefill_paged(q, kc, vc, bt, cu, slk, 0.125)
    want = ref.prefill_attention_paged(q, kc, vc, bt, cu, slk, 0.125)
    assert float(ac.row_rel_err(want, got).max()) < 1e-6


def _scores(q, keys, scale, q_rounding, prescale="split"):
    """The scores attend64 uses, up to a constant per (row, head): with
    V = I its output is the softmax itself, whose log is score - lse."""
    n = keys.shape[1]
    eye = torch.eye(n, dtype=torch.float64).expand(keys.shape[0], n, n)
    p = ac.attend64(q, keys, eye, torch.full((q.shape[0],), n - 1), scale,
                    q_rounding, prescale)
    return p.log()


@pytest.mark.parametrize("head_dim", [64, 128])
def test_q_rounding_stays_within_its_quantum(head_dim):
    """bf16_prescaled moves a score by at most 2^-9 of sum|q_i k_i| * scale
    (half an ulp of bf16 per element; the two fp32 products add 2^-23
    each). e4m3_per_head moves element i by at most 2^-4 |q_i| (half an ulp
    of a 3-bit mantissa) or, below the e4m3 normal range, 2^-10 qs (half
    the smallest subnormal), so a score by scale * sum|k_i| * that."""
    gen = torch.Generator().manual_seed(9)
    hk, group, n = 2, 4, 24
    q = torch.randn(3, hk * group, head_dim, generator=gen).to(torch.bfloat16)
    keys = torch.randn(hk, n, head_dim, generator=gen).to(torch.float64)
    scale = 1.0 / math.sqrt(head_dim)
    q64 = q.to(torch.float64).view(3, hk, group, head_dim)
    absdot = torch.einsum("rkgd,knd->rkgn", q64.abs(), keys.abs())
    qs = q64.abs().amax(dim=-1, keepdim=True).clamp(min=1e-8) / 448.0
    step8 = torch.maximum(q64.abs() * 2.0 ** -4, qs * 2.0 ** -10)
    bound = {
        "bf16_prescaled": absdot * scale * (2.0 ** -9 + 2.0 ** -21),
        "e4m3_per_head": torch.einsum("rkgd,knd->rkgn", step8, keys.abs())
        * scale * (1 + 2.0 ** -20),
    }
    base = _scores(q, keys, scale, None)
    for mode, prescales in (("bf16_prescaled", ("split", "folded")),
                            ("e4m3_per_head", ("split",))):
        for prescale in prescales:
            got = _scores(q, keys, scale, mode, prescale)
            delta = (got - base).view(3, hk, group, n)
            # scores are known up to a constant per (row, head): compare
            # differences between tokens, bounded by the sum of two bounds
            d = delta.unsqueeze(-1) - delta.unsqueeze(-2)
            b = bound[mode].unsqueeze(-1) + bound[mode].unsqueeze(-2)
            assert bool((d.abs() <= b + 1e-12).all()), (mode, prescale)
            assert float(d.abs().max()) > 0.0  # the mode does round


def test_row_rel_err_and_bf16_floor():
    want = torch.randn(7, 4, 128, dtype=torch.float64)
    assert float(ac.row_rel_err(want, want).max()) == 0.0
    floor = ac.row_rel_err(want.to(torch.bfloat16), want)
    assert floor.shape == (7, 4)
    assert float(floor.max()) <= 2.0 ** -8 < ac.KERNEL_TOL
