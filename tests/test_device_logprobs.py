"""Device-side logprobs on the CPU: reference.token_logprobs (the CPU
implementation of ops.token_logprobs and the oracle of the GPU tests)
against plain torch, the contract's edge cases, and the engine wiring (tiny
model, fused backend). The case builder is shared with the GPU tests."""

import math

import numpy as np
import pytest
import torch

import fusioninfer_amd.ops as ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sampler import Sampler
from fusioninfer_amd.engine.sequence import SamplingParams
from fusioninfer_amd.models.registry import get_model_config

NINF = float("-inf")
# row i of a case asks for NUM_TOP[i % 6] entries: a one-row case is not
# skipped, a three-row case compares all of its rows
NUM_TOP = (5, 20, 32, -1, 0, 1)
SENTINEL_F, SENTINEL_I = 1234.5, -77
_CASES = {}


def logprobs_case(T, V):
    """Inputs (CPU) and reference outputs for one shape, built once and
    never modified: logits randn * 4 with one all-negative row and one row
    with 30 % -inf (as test_fused_sampler_gpu.make_case), in-range token
    ids, num_top cycling through NUM_TOP. The reference ran on outputs
    pre-filled with the sentinels, so skipped rows hold them."""
    if (T, V) in _CASES:
        return _CASES[(T, V)]
    g = torch.Generator().manual_seed(977 * T + V)
    logits = torch.randn(T, V, generator=g) * 4
    if T >= 3:
        logits[1] = -logits[1].abs() - 0.5
        logits[2, torch.rand(V, generator=g) < 0.3] = NINF
    token_ids = torch.randint(0, V, (T,), generator=g)
    num_top = torch.tensor([NUM_TOP[i % len(NUM_TOP)] for i in range(T)],
                           dtype=torch.int32)
    want = ops.token_logprobs(logits, token_ids, num_top,
                              out=sentinel_out(T, 32))
    _CASES[(T, V)] = (logits, token_ids, num_top), want
    return _CASES[(T, V)]


def sentinel_out(T, W, device="cpu"):
    return (
        torch.full((T,), SENTINEL_F, device=device),
        torch.full((T, W), SENTINEL_I, dtype=torch.int32, device=device),
        torch.full((T, W), SENTINEL_F, device=device),
    )


def check_against(got, want, num_top, tol=1e-4):
    """Every non-skipped row: ids equal, values within tol where the
    reference is finite and equal where it is -inf; skipped rows equal
    (both sides started from the sentinels)."""
    chosen, ids, lp = (x.cpu() for x in got)
    w_chosen, w_ids, w_lp = want
    assert torch.equal(ids, w_ids)
    for a, b in ((chosen, w_chosen), (lp, w_lp)):
        fin = torch.isfinite(b)
        assert torch.equal(a[~fin], b[~fin])
        err = (a[fin].double() - b[fin].double()).abs().max().item() \
            if fin.any() else 0.0
        print(f"max |err| {err:.3e} over {int(fin.sum())} finite values")
        assert err <= tol
    skipped = num_top < 0
    assert (chosen[skipped] == SENTINEL_F).all()
    assert (ids[skipped] == SENTINEL_I).all()
    assert (lp[skipped] == SENTINEL_F).all()


# ------------------------------------------------------------- reference

@pytest.mark.parametrize("T,V", [(1, 5), (3, 50), (33, 1000), (257, 4099)])
def test_reference_against_plain_torch(T, V):
    (logits, token_ids, num_top), (chosen, ids, lp) = logprobs_case(T, V)
    full = torch.log_softmax(logits.double(), dim=-1)
    x = (logits + 0.0).numpy()
    compared = 0
    for t in range(T):
        want = int(num_top[t])
        if want < 0:
            assert chosen[t] == SENTINEL_F and (ids[t] == SENTINEL_I).all()
            continue
        # logit descending, then index ascending
        order = np.lexsort((np.arange(V), -x[t].astype(np.float64)))
        k = min(want, 32, V)
        assert ids[t, :k].tolist() == order[:k].tolist()
        assert (ids[t, k:] == -1).all() and (lp[t, k:] == NINF).all()
        ref_vals = torch.cat([full[t, token_ids[t]].view(1),
                              full[t, ids[t, :k].long()]])
        got_vals = torch.cat([chosen[t].view(1), lp[t, :k]]).double()
        fin = torch.isfinite(ref_vals)
        assert torch.equal(got_vals[~fin], ref_vals[~fin])
        assert (got_vals[fin] - ref_vals[fin]).abs().max() <= 1e-4
        compared += 1
    assert compared >= T - T // 6 - 1


def _run(logits, tok, num_top, W=32):
    return ops.token_logprobs(
        torch.tensor(logits, dtype=torch.float32),
        torch.tensor(tok, dtype=torch.int64),
        torch.tensor(num_top, dtype=torch.int32),
        out=sentinel_out(len(tok), W),
    )


def test_skipped_row_is_left_untouched():
    chosen, ids, lp = _run([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]], [0, 0],
                           [-1, 2], W=4)
    assert chosen[0] == SENTINEL_F
    assert (ids[0] == SENTINEL_I).all() and (lp[0] == SENTINEL_F).all()
    assert ids[1].tolist() == [0, 1, -1, -1]
    assert lp[1, 2:].tolist() == [NINF, NINF]
    z = math.log(sum(math.exp(v) for v in (1.0, 2.0, 3.0)))
    assert abs(float(chosen[1]) - (3.0 - z)) < 1e-6


def test_k_zero_writes_the_chosen_value_and_the_fill():
    chosen, ids, lp = _run([[0.5, 0.25, -1.0]], [1], [0], W=3)
    assert torch.isfinite(chosen[0])
    assert ids[0].tolist() == [-1, -1, -1]
    assert lp[0].tolist() == [NINF] * 3


def test_k_beyond_the_vocabulary():
    chosen, ids, lp = _run([[0.0, 3.0, -1.0, 3.0, 2.0]], [4], [20])
    assert ids[0, :5].tolist() == [1, 3, 4, 0, 2]
    assert (ids[0, 5:] == -1).all() and (lp[0, 5:] == NINF).all()
    assert chosen[0] == lp[0, 2]


@pytest.mark.parametrize("tok", [-1, 5, 1 << 40, -(1 << 40)])
def test_out_of_range_token_gives_nan(tok):
    chosen, ids, lp = _run([[0.0, 3.0, -1.0, 3.0, 2.0]], [tok], [2])
    assert math.isnan(float(chosen[0]))
    assert ids[0, :2].tolist() == [1, 3]
    assert torch.isfinite(lp[0, :2]).all()


def test_row_without_a_finite_entry():
    chosen, ids, lp = _run([[NINF] * 6], [3], [4], W=5)
    assert chosen[0] == NINF
    assert ids[0].tolist() == [0, 1, 2, 3, -1]
    assert lp[0].tolist() == [NINF] * 5  # and no NaN


def test_fewer_finite_entries_than_k():
    chosen, ids, lp = _run([[NINF, 1.0, NINF, 2.0, NINF, NINF]], [0], [5])
    # the finite ones by value, then -inf entries in index order
    assert ids[0, :5].tolist() == [3, 1, 0, 2, 4]
    assert torch.isfinite(lp[0, :2]).all()
    assert lp[0, 2:5].tolist() == [NINF] * 3
    assert chosen[0] == NINF


def test_zero_signs_compare_equal():
    chosen, ids, lp = _run([[-5.0, -0.0, 0.0, -5.0]], [1], [1])
    assert ids[0, 0] == 1


def test_dispatch_rejects_bad_arguments():
    logits = torch.randn(4, 64)
    tok = torch.zeros(4, dtype=torch.int64)
    num_top = torch.full((4,), 3, dtype=torch.int32)
    assert ops.LOGPROBS_MAX_TOP == 32
    chosen, ids, lp = ops.token_logprobs(logits, tok, num_top)
    assert ids.shape == lp.shape == (4, 32) and chosen.shape == (4,)
    assert ops.token_logprobs(logits, tok, num_top, width=3)[1].shape == (4, 3)
    for bad in (
        (logits.double(), tok, num_top),
        (logits.t(), tok, num_top),
        (logits[0], tok, num_top),
        (logits, tok.int(), num_top),
        (logits, tok[:3], num_top),
        (logits, tok, num_top.long()),
        (logits, tok, num_top[:3]),
    ):
        with pytest.raises(ValueError):
            ops.token_logprobs(*bad)
    for width in (0, 33):
        with pytest.raises(ValueError):
            ops.token_logprobs(logits, tok, num_top, width=width)
    good = sentinel_out(4, 8)
    ops.token_logprobs(logits, tok, num_top, out=good)
    for bad in (
        (good[0].double(), good[1], good[2]),
        (good[0], good[1].long(), good[2]),
        (good[0], good[1], good[2][:, :7]),
        (good[0][:3], good[1], good[2]),
        (good[0], sentinel_out(4, 16)[1][:, ::2], good[2]),
        (good[0], sentinel_out(4, 33)[1], sentinel_out(4, 33)[2]),
    ):
        with pytest.raises(ValueError):
            ops.token_logprobs(logits, tok, num_top, out=bad)


# ---------------------------------------------------------------- engine

PROMPTS = [[5, 3, 8, 1] * 10, [11, 13, 17] * 8]


def make_engine(**kw):
    cfg = EngineConfig(
        model=get_model_config("tiny-qwen3"),
        cache=CacheConfig(num_gpu_blocks=256),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=1024, max_model_len=256
        ),
        seed=3,
        sampler_backend="fused",
        **kw,
    )
    torch.manual_seed(0)
    return LLMEngine(cfg, device="cpu")


def generate(eng, samplings, prompts=PROMPTS):
    """Final RequestOutput per prompt; `samplings` is one dict for all or
    a list with one per prompt."""
    if isinstance(samplings, dict):
        samplings = [samplings] * len(prompts)
    ids = [eng.add_request(p, SamplingParams(**sp))
           for p, sp in zip(prompts, samplings)]
    done = {}
    while eng.has_unfinished():
        for o in eng.step():
            if o.finished:
                done[o.request_id] = o
    return [done[i] for i in ids]


def tokens(outs):
    return [o.output_token_ids for o in outs]


def assert_entries_agree(got, want, k, tol=2e-4):
    """Chosen values and sorted top values of two runs of one request."""
    assert len(got.logprobs) == len(want.logprobs) == len(
        got.output_token_ids)
    for (c0, top0), (c1, top1) in zip(got.logprobs, want.logprobs):
        assert len(top0) == len(top1) == k
        assert abs(c0 - c1) <= tol
        for a, b in zip(sorted(top0.values()), sorted(top1.values())):
            assert abs(a - b) <= tol


@pytest.mark.parametrize("extra", [
    {},
    dict(temperature=0.8, top_k=50, top_p=0.9, seed=1234),
])
def test_engine_keeps_logprobs_requests_on_the_chain(extra):
    sampling = dict(max_tokens=12, logprobs=3, **extra)
    eng = make_engine()
    assert eng._async_decode and eng.sampler.device_logprobs
    first = generate(eng, sampling)
    assert eng.num_async_steps > 0

    host = make_engine(device_logprobs=False)
    assert not host.sampler.device_logprobs
    want = generate(host, sampling)
    assert host.num_async_steps == 0
    assert tokens(first) == tokens(want)

    plain = generate(make_engine(), dict(max_tokens=12, **extra))
    assert tokens(plain) == tokens(first)
    assert all(o.logprobs == [] for o in plain)

    for got, ref_out in zip(first, want):
        assert len(got.output_token_ids) == 12
        assert_entries_agree(got, ref_out, 3)
        if not extra:
            # greedy: the chosen token is the top-1 entry
            for tok, (c, top) in zip(got.output_token_ids, got.logprobs):
                assert top[tok] == c == max(top.values())


def test_stop_token_inside_the_chain_keeps_one_entry_per_token():
    """A sequence that ends on a stop token while pipelined is still in
    the batch of the step already launched: its late token is discarded
    and so is that step's logprobs entry."""
    free_run = tokens(generate(make_engine(), dict(max_tokens=12,
                                                   logprobs=2)))
    first = free_run[0]
    pos = next(i for i in range(3, 12) if first[i] not in first[:i])
    sampling = dict(max_tokens=12, ignore_eos=False, logprobs=2,
                    stop_token_ids=[first[pos]])
    eng = make_engine()
    host = make_engine(device_logprobs=False)
    outs = generate(eng, sampling)
    want = generate(host, sampling)
    assert eng.num_async_steps > 0 and host.num_async_steps == 0
    assert outs[0].output_token_ids == first[:pos + 1]
    assert tokens(outs) == tokens(want)
    assert len(outs[1].output_token_ids) > pos + 1
    for got, ref_out in zip(outs, want):
        assert_entries_agree(got, ref_out, 2)


def test_mixed_batch():
    prompts = PROMPTS + [[7, 9] * 12, [2, 4, 6, 8] * 6]
    mix = [dict(max_tokens=10, logprobs=2), dict(max_tokens=10, logprobs=0),
           dict(max_tokens=10), dict(max_tokens=10, logprobs=40)]

    eng = make_engine()
    three = generate(eng, mix[:3], prompts[:3])
    assert eng.num_async_steps > 0

    eng = make_engine()
    four = generate(eng, mix, prompts)
    # the request beyond LOGPROBS_MAX_TOP keeps the batch synchronous
    assert eng.num_async_steps == 0
    assert tokens(four[:3]) == tokens(three)
    host = generate(make_engine(device_logprobs=False), mix, prompts)
    assert tokens(host) == tokens(four)

    for outs in (three, four):
        assert [len(t) for _, t in outs[0].logprobs] == [2] * 10
        assert [len(t) for _, t in outs[1].logprobs] == [0] * 10
        assert outs[2].logprobs == []
        assert all(math.isfinite(c) for o in outs[:2] for c, _ in o.logprobs)
    assert [len(t) for _, t in four[3].logprobs] == [40] * 10
    for k, got, ref_out in zip((2, 0), four, host):
        assert_entries_agree(got, ref_out, k)
    assert_entries_agree(four[3], host[3], 40)


def test_eligibility_follows_backend_switch_and_size():
    from fusioninfer_amd.engine.sequence import Sequence

    def seq(**kw):
        return Sequence("s", PROMPTS[0], SamplingParams(**kw))

    eng = make_engine()
    assert eng._seq_async_ok(seq(logprobs=0))
    assert eng._seq_async_ok(seq(logprobs=32))
    assert not eng._seq_async_ok(seq(logprobs=33))
    assert not eng._seq_async_ok(seq(logprobs=3, prompt_logprobs=1))
    assert not make_engine(device_logprobs=False)._seq_async_ok(
        seq(logprobs=3))
    assert not Sampler(backend="torch").device_logprobs
    assert Sampler(backend="fused").device_logprobs


def test_no_requesting_row_launches_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("token_logprobs launched")

    monkeypatch.setattr(ops, "token_logprobs", boom)
    eng = make_engine()
    generate(eng, dict(max_tokens=6))
    generate(eng, dict(max_tokens=6, temperature=0.8, seed=5))
    # beyond the kernel's width: the host path, still no launch
    outs = generate(eng, dict(max_tokens=3, logprobs=40))
    assert [len(t) for _, t in outs[0].logprobs] == [40] * 3
    assert eng.num_async_steps > 0


def test_config_defaults_and_cli_flag():
    from fusioninfer_amd.server.__main__ import (
        build_engine_config, parse_args,
    )

    assert EngineConfig().device_logprobs is True
    cfg = build_engine_config(parse_args(["--model", "Qwen3-0.6B"]))
    assert cfg.device_logprobs is True
    cfg = build_engine_config(parse_args(
        ["--model", "Qwen3-0.6B", "--no-device-logprobs"]))
    assert cfg.device_logprobs is False
