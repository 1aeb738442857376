"""Fused sampler on the CPU: Philox known answers, the sample_tokens
reference against the torch sampler's filtering, Sampler(backend="fused")
behaviour, config / CLI plumbing and a deterministic distribution check."""

import itertools
import math

import pytest
import torch

from fusioninfer_amd import ops
from fusioninfer_amd.config import EngineConfig
from fusioninfer_amd.engine.sampler import Sampler
from fusioninfer_amd.engine.sequence import SamplingParams, Sequence
from fusioninfer_amd.ops import reference as ref

GRID = list(itertools.product([0, 1, 7], [1.0, 0.9, 0.1], [0.0, 0.3]))


def _seq(n_out=0, **kw):
    s = Sequence("s", [1, 2, 3], SamplingParams(**kw))
    s.output_token_ids = [0] * n_out
    return s


def _hex(words):
    return " ".join(f"{w:08x}" for w in words)


def test_philox_known_answers():
    assert _hex(ref.philox4x32_10((0, 0, 0, 0), (0, 0))) == (
        "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    )
    ones = 0xFFFFFFFF
    assert _hex(ref.philox4x32_10((ones,) * 4, (ones,) * 2)) == (
        "408f276d 41c83b0e a20bc7c6 6d5451fd"
    )


@pytest.mark.parametrize("V", [50, 1000])
def test_reference_kept_set_matches_torch_sampler(V, monkeypatch):
    """On tie-free rows the reference keeps exactly the tokens the torch
    sampler's top-k / top-p / min-p filtering leaves finite (read off the
    probabilities it hands to multinomial)."""
    g = torch.Generator().manual_seed(1234 + V)
    seen = []
    real = torch.multinomial

    def spy(probs, *a, **kw):
        seen.append(probs.clone())
        return real(probs, *a, **kw)

    monkeypatch.setattr(torch, "multinomial", spy)
    for row, (k, p, mp) in enumerate(GRID):
        x = torch.randn(V, generator=g) * 4
        assert x.unique().numel() == V  # tie-free
        s = _seq(temperature=0.8, top_k=k, top_p=p, min_p=mp, seed=row)
        seen.clear()
        Sampler().sample(x.clone().unsqueeze(0), [s])
        torch_kept = seen[0].flatten() > 0
        _, _, kept = ref.sample_row(x, 0.8, k, p, mp, seed=row, offset=0)
        assert torch.equal(kept, torch_kept), (k, p, mp)


def test_dispatch_rejects_bad_arguments():
    T, V = 2, 8
    good = dict(
        logits=torch.zeros(T, V), temperature=torch.ones(T),
        top_k=torch.zeros(T, dtype=torch.int32), top_p=torch.ones(T),
        min_p=torch.zeros(T), rng=torch.zeros(T, 2, dtype=torch.int64),
    )
    assert ops.sample_tokens(**good).shape == (T,)
    for name, bad in (
        ("logits", torch.zeros(T, V, dtype=torch.bfloat16)),
        ("top_k", torch.zeros(T, dtype=torch.int64)),
        ("top_p", torch.ones(T + 1)),
        ("rng", torch.zeros(T, dtype=torch.int64)),
    ):
        with pytest.raises(ValueError):
            ops.sample_tokens(**{**good, name: bad})


def test_fused_top_k_limits_support():
    logits = torch.tensor([[10.0, 9.0, -1.0, -2.0]])
    sampler = Sampler(backend="fused")
    picks = set()
    for n in range(64):
        s = _seq(n, temperature=1.0, top_k=2, seed=7)
        picks.add(int(sampler.sample(logits.clone(), [s])[0]))
    assert picks == {0, 1}


def test_fused_min_p_filters_tail():
    logits = torch.tensor([[5.0, 4.9, 0.0, -2.0, -50.0]])
    sampler = Sampler(backend="fused")
    picks = {
        int(sampler.sample(
            logits, [_seq(temperature=1.0, min_p=0.5, seed=i)])[0])
        for i in range(50)
    }
    assert picks == {0, 1}
    picks = {
        int(sampler.sample(
            logits, [_seq(temperature=10.0, min_p=0.0, seed=i)])[0])
        for i in range(200)
    }
    assert len(picks) >= 3


def test_fused_seed_and_offset():
    logits = torch.randn(1, 100, generator=torch.Generator().manual_seed(0))

    def draw(seed, n_out):
        s = _seq(n_out, temperature=1.0, seed=seed)
        return int(Sampler(backend="fused").sample(logits.clone(), [s])[0])

    assert draw(123, 0) == draw(123, 0)
    assert draw(123, 5) == draw(123, 5)
    # the offset (tokens emitted so far) moves the stream
    assert len({draw(123, n) for n in range(32)}) > 1
    assert len({draw(seed, 0) for seed in range(32)}) > 1


def test_fused_unseeded_rows_advance_the_engine_stream():
    logits = torch.randn(1, 100, generator=torch.Generator().manual_seed(0))
    a, b = Sampler(seed=3, backend="fused"), Sampler(seed=3, backend="fused")
    sa = [int(a.sample(logits.clone(), [_seq(temperature=1.0)])[0])
          for _ in range(32)]
    sb = [int(b.sample(logits.clone(), [_seq(temperature=1.0)])[0])
          for _ in range(32)]
    assert sa == sb and len(set(sa)) > 1
    assert a.num_unseeded_draws == 32


def test_fused_mixed_batch_and_degenerate_filters():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(6, 50, generator=g)
    logits[5] = float("-inf")
    seqs = [
        _seq(),                                     # greedy
        _seq(temperature=1.0, seed=5),
        _seq(temperature=0.7, top_k=1, seed=1),     # k = 1
        _seq(temperature=0.7, top_p=1e-9, seed=2),  # p -> 0
        _seq(temperature=0.7, min_p=1.0, seed=3),   # only the max survives
        _seq(temperature=0.9, top_p=0.9, seed=4),   # nothing finite
    ]
    out = Sampler(backend="fused").sample(logits.clone(), seqs)
    assert out.dtype == torch.int64
    for i in (0, 2, 3, 4):
        assert int(out[i]) == int(logits[i].argmax()), i
    assert int(out[5]) == 0


def test_fused_greedy_ties_take_the_lowest_index():
    logits = torch.tensor([[1.0, 3.0, 3.0, 0.0]])
    assert Sampler(backend="fused").sample(logits, [_seq()]).tolist() == [1]


def test_fused_ties_at_the_top_k_boundary_are_kept():
    logits = torch.tensor([[4.0, 3.0, 3.0, 1.0, 0.0]])
    _, _, kept = ref.sample_row(logits[0], 1.0, 2, 1.0, 0.0, 0, 0)
    assert kept.tolist() == [True, True, True, False, False]


def test_unknown_backend_rejected():
    with pytest.raises(ValueError):
        Sampler(backend="triton")


def test_config_default_and_cli_flag():
    from fusioninfer_amd.server.__main__ import build_engine_config, parse_args

    assert EngineConfig().sampler_backend == "torch"
    assert parse_args([]).sampler_backend == "torch"
    args = parse_args(["--model", "Qwen3-0.6B", "--sampler-backend", "fused"])
    assert args.sampler_backend == "fused"
    assert build_engine_config(args).sampler_backend == "fused"
    with pytest.raises(SystemExit):
        parse_args(["--sampler-backend", "other"])


def distribution_case():
    """One 64-token row drawn N = 8192 times at offsets 0 .. N-1 of one
    seed. Returns (logits [N, 64], params..., exact probabilities)."""
    N, V, seed = 8192, 64, 2024
    x = torch.randn(V, generator=torch.Generator().manual_seed(11))
    e = torch.exp(x - x.max())
    w = torch.floor(e.double() * 2.0**32)
    probs = (w / w.sum()).tolist()
    logits = x.unsqueeze(0).expand(N, V).contiguous()
    rng = torch.stack(
        [torch.full((N,), seed, dtype=torch.int64), torch.arange(N)], dim=1
    )
    return (
        logits, torch.ones(N), torch.zeros(N, dtype=torch.int32),
        torch.ones(N), torch.zeros(N), rng, probs,
    )


def check_distribution(tokens, probs):
    N = tokens.numel()
    counts = torch.bincount(tokens.cpu(), minlength=len(probs)).tolist()
    for c, p in zip(counts, probs):
        bound = 5 * math.sqrt(N * p * (1 - p)) + 1
        assert abs(c - N * p) <= bound, (c, N * p, bound)


def test_distribution_of_counter_based_draws():
    """Deterministic (counter-based RNG): the seed in distribution_case is
    one for which the reference passes."""
    *args, probs = distribution_case()
    check_distribution(ops.sample_tokens(*args), probs)
