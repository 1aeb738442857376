"""Fused sampling kernel (sampling.hip) on the GPU: against the integer
reference, ties, determinism, row independence, distribution, and the
engine with sampler_backend="fused" (4-layer Qwen3-0.6B as in
test_lora_engine_gpu)."""

import pytest
import torch

from fusioninfer_amd import ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sequence import SamplingParams
from fusioninfer_amd.models.registry import get_model_config
from fusioninfer_amd.ops import reference as ref
from tests.test_fused_sampler import (
    GRID, check_distribution, distribution_case,
)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# A sampled row is compared token-for-token only when every comparison the
# reference made is further than DELTA (relative to the mass involved) from
# flipping: the GPU and CPU expf differ by 1-2 ulp, which moves a
# fixed-point prefix mass by about 2^-22 * Z.
DELTA = 2.0 ** -20
SHAPES = [(1, 5), (3, 50), (33, 1000), (257, 4099), (4, 151936)]
DATA_SEED = 0
_CASES = {}


def make_case(T, V):
    """Inputs (CPU) and reference results for one shape, built once."""
    if (T, V) in _CASES:
        return _CASES[(T, V)]
    g = torch.Generator().manual_seed(DATA_SEED + 131 * T + V)
    logits = torch.randn(T, V, generator=g) * 4
    if T >= 3:
        logits[1] = -logits[1].abs() - 0.5            # all negative
        logits[2, torch.rand(V, generator=g) < 0.3] = float("-inf")
    rows = list(range(T))
    temperature = torch.tensor(
        [0.0 if i % 5 == 4 else 0.8 for i in rows], dtype=torch.float32
    )
    top_k = torch.tensor([GRID[i % len(GRID)][0] for i in rows],
                         dtype=torch.int32)
    top_p = torch.tensor([GRID[i % len(GRID)][1] for i in rows],
                         dtype=torch.float32)
    min_p = torch.tensor([GRID[i % len(GRID)][2] for i in rows],
                         dtype=torch.float32)
    rng = torch.tensor([[1000 + i, 7 * i] for i in rows], dtype=torch.int64)
    args = (logits, temperature, top_k, top_p, min_p, rng)
    tokens, margins = ref.sample_tokens(*args, return_margin=True)
    wide = [
        ref.sample_row(logits[i], temperature[i], top_k[i], top_p[i],
                       min_p[i], int(rng[i, 0]), int(rng[i, 1]),
                       slack=DELTA)[2]
        for i in rows
    ]
    _CASES[(T, V)] = (args, tokens, margins, wide)
    return _CASES[(T, V)]


def on_gpu(args):
    return tuple(a.to(DEV) for a in args)


@pytest.mark.parametrize("T,V", SHAPES)
def test_kernel_matches_reference(T, V):
    args, tokens, margins, wide = make_case(T, V)
    out = ops.sample_tokens(*on_gpu(args)).cpu()
    temperature = args[1]
    sampled = temperature != 0
    compared = ~sampled | (margins > DELTA)
    skipped = int((sampled & ~compared).sum())
    print(f"T={T} V={V}: sampled rows {int(sampled.sum())}, skipped "
          f"{skipped}, mismatches among compared "
          f"{int((out != tokens)[compared].sum())}")
    # the reference alone guarantees this (DATA_SEED chosen on the CPU)
    assert skipped <= 0.02 * int(sampled.sum())
    assert torch.equal(out[compared], tokens[compared])
    for i in range(T):
        if wide[i] is not None:
            assert bool(wide[i][out[i]]), (i, int(out[i]))


def test_ties_at_the_top_k_boundary():
    """k-th and (k+1)-th values equal: both kept and drawn, nothing below."""
    V, N, k = 1000, 4096, 3
    x = torch.linspace(-6.0, -1.0, V)
    x[17], x[400], x[401], x[900] = 2.0, 1.5, 1.0, 1.0  # 3rd == 4th
    logits = x.unsqueeze(0).expand(N, V).contiguous()
    rng = torch.stack(
        [torch.full((N,), 5, dtype=torch.int64), torch.arange(N)], dim=1
    )
    out = ops.sample_tokens(*on_gpu((
        logits, torch.ones(N), torch.full((N,), k, dtype=torch.int32),
        torch.ones(N), torch.zeros(N), rng,
    ))).cpu()
    assert set(out.tolist()) == {17, 400, 401, 900}


def test_same_call_twice_is_bit_identical():
    args = on_gpu(make_case(257, 4099)[0])
    assert torch.equal(ops.sample_tokens(*args), ops.sample_tokens(*args))


def test_row_is_independent_of_its_batch():
    args = on_gpu(make_case(33, 1000)[0])
    full = ops.sample_tokens(*args)
    alone = ops.sample_tokens(*(a[5:6].contiguous() for a in args))
    assert int(alone[0]) == int(full[5])


def test_distribution_in_one_launch():
    *args, probs = distribution_case()
    check_distribution(ops.sample_tokens(*on_gpu(args)), probs)


# ---------------------------------------------------------------- engine

PROMPTS = [list(range(50, 120)), [11, 13, 17] * 20]


def make_engine(backend):
    mc = get_model_config("Qwen3-0.6B")
    mc.num_layers = 4
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=512),
        scheduler=SchedulerConfig(
            max_num_seqs=16, max_num_batched_tokens=2048, max_model_len=512,
        ),
        seed=7,
        sampler_backend=backend,
    )
    torch.manual_seed(0)
    return LLMEngine(cfg, device=DEV)


def generate(eng, sampling):
    ids = [eng.add_request(p, SamplingParams(**sampling)) for p in PROMPTS]
    done = {}
    while eng.has_unfinished():
        for o in eng.step():
            if o.finished:
                done[o.request_id] = o.output_token_ids
    return [done[i] for i in ids]


def test_engine_fused_backend():
    seeded = dict(max_tokens=16, temperature=0.8, top_k=50, top_p=0.9,
                  seed=1234)
    greedy = dict(max_tokens=16)

    eng = make_engine("fused")
    assert eng._async_decode
    first = generate(eng, seeded)
    assert all(len(t) == 16 for t in first)
    # seeded sampled sequences stay on the pipelined-decode chain
    assert eng.num_async_steps > 0
    greedy_fused = generate(eng, greedy)

    # a fresh engine with pipelining off: same tokens
    sync = make_engine("fused")
    sync._async_decode = False
    assert generate(sync, seeded) == first
    assert sync.num_async_steps == 0

    base = make_engine("torch")
    assert generate(base, greedy) == greedy_fused
