"""CPU checks of tests/rowwise_cases.py: the bounds are satisfiable, the
cases catch the defects they were built for, and the unclamped e4m3
conversion cannot overflow.

No kernel runs here. `emulate` is a float32 model of the kernels; it must
pass every checker on every case (so a correct kernel can), and each of its
switchable defects must fail a checker for every op it can touch.
"""

import pytest
import torch

import rowwise_cases as rc


@pytest.fixture(scope="module")
def cases():
    return list(rc.all_cases())


def test_every_width_and_op_has_cases(cases):
    seen = {(c["op"], c["name"]) for c in cases}
    for op in rc.OPS:
        for w in rc.widths_for(op):
            assert (op, f"random-{w}") in seen and (op, f"exact-{w}") in seen
            if op in rc.NORM_OPS:
                assert (op, f"needle-sumsq-{w}") in seen
            if op in rc.FP8_OPS:
                assert (op, f"needle-amax-{w}") in seen
    # quant.hip's wide kernel is reached by both of its ops
    assert all(w > 16384 for w in rc.WIDE_WIDTHS)


def test_emulation_passes_every_checker(cases):
    worst = {}
    for case in cases:
        for key, ratio in rc.check_case(case, rc.emulate(case)).items():
            k = (case["op"], key)
            worst[k] = max(worst.get(k, 0.0), ratio)
    stride = rc.silu_stride_case()
    rc.check_case(stride, rc.emulate(stride))
    for k, ratio in sorted(worst.items()):
        print(f"emulation {k[0]:>24} {k[1]:>8}: worst error/bound {ratio:.3f}")


@pytest.mark.parametrize("mutant", rc.MUTANTS)
def test_mutant_is_caught(cases, mutant):
    for op in rc.MUTANT_OPS[mutant]:
        caught = []
        for case in cases:
            if case["op"] != op:
                continue
            try:
                rc.check_case(case, rc.emulate(case, mutant))
            except AssertionError:
                caught.append(case["name"])
        assert caught, f"{mutant} passes every {op} case"


def test_exact_cases_are_exact_in_float64():
    """The expected bits of the exact cases are what float64 gives too."""
    for op in rc.OPS:
        case = rc.exact_case(op, 2056)
        y, res = rc.oracle(case)
        ex = case["exact"]
        if "out_bits" in ex:
            assert torch.equal(rc.bits16(y.to(torch.bfloat16)), ex["out_bits"])
        if "residual_bits" in ex:
            assert torch.equal(rc.bits16(res.to(torch.bfloat16)),
                               ex["residual_bits"])
        if "out_bytes" in ex:
            s = y.abs().amax(dim=1, keepdim=True) / 448.0
            q = (y / s).to(torch.float32).to(torch.float8_e4m3fn)
            assert torch.equal(q.view(torch.uint8), ex["out_bytes"])


def test_needles_carry_the_row_statistic():
    for op in rc.FP8_OPS:
        case = rc.needle_amax_case(op, 6152)
        y, _ = rc.oracle(case)
        for r, cols in enumerate(case["needles"]):
            assert int(y[r].abs().argmax()) in cols
            assert (y[r, cols] == y[r].abs().max()).all()
    cols = rc.needle_columns(6152)
    assert (6144,) in cols and (6151,) in cols and (2047,) in cols


def test_scaled_row_maximum_stays_below_e4m3_overflow():
    """The kernels convert v * (1 / scale) without clamping. For every
    positive finite bf16 amax, fl(amax * fl(1 / fl(amax / 448))) must stay
    below 464, the midpoint between 448 and the next e4m3 step, and at or
    above 432, so that it converts to exactly 448."""
    amax = rc.positive_finite_bf16()
    assert amax.numel() == 0x7F7F and torch.isfinite(amax).all()
    p = rc.scaled_amax_f32(amax)
    live = amax >= 1e-8
    assert (p < 464.0).all()
    assert (p[live] >= 432.0).all()
    # the fused ops reduce fp32 values, not bf16 ones: a dense fp32 sample
    g = torch.Generator().manual_seed(5)
    mant = 1.0 + torch.rand(1 << 20, generator=g)
    expo = torch.randint(-26, 100, (1 << 20,), generator=g)
    f = (mant * torch.exp2(expo.float())).to(torch.float32)
    p = rc.scaled_amax_f32(f)
    assert (p < 464.0).all() and (p >= 432.0).all()


def test_ulp8():
    z = torch.tensor([448.0, 256.0, 255.9999, 1.0, 2.0 ** -6, 2.0 ** -7, 0.0],
                     dtype=torch.float64)
    want = torch.tensor([32.0, 32.0, 32.0, 0.125, 2.0 ** -9, 2.0 ** -9,
                         2.0 ** -9], dtype=torch.float64)
    assert torch.equal(rc.ulp8(z), want)


def test_cache_case_exceeds_the_grid_cap_by_one_token():
    case = rc.cache_case()
    vec = case["kv_heads"] * case["head_dim"] // 8
    assert (case["tokens"] - 1) * vec <= rc.CACHE_GRID_CAP_VECS
    assert case["tokens"] * vec > rc.CACHE_GRID_CAP_VECS
    live = case["slots"][case["slots"] >= 0]
    assert live.unique().numel() == live.numel()
    assert (case["slots"] < 0).sum() == 4
    t, w = rc.SILU_STRIDE_SHAPE
    assert t * (w // 8) > 2048 * 256
