"""Device-side sampling penalties on the GPU (penalties.hip): the kernel
bit for bit against Sampler._apply_penalties, untouched elements and guard
rows, the histogram update, and the pipelined fused engine against the host
path (4-layer Qwen3-0.6B as in test_fused_sampler_gpu)."""

import pytest
import torch

from fusioninfer_amd import ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sampler import Sampler
from fusioninfer_amd.engine.sequence import SamplingParams
from fusioninfer_amd.models.registry import get_model_config
from tests.test_device_penalties import penalty_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 4096), (5, 4099), (33, 32000)]


def as_bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("T,V", SHAPES)
def test_kernel_equals_the_sampler(T, V):
    logits, seqs, counts, slot_ids, params = penalty_case(
        T, V, big_count=1100)
    assert int(counts.max()) > 1000 and int(counts[counts > 0].min()) == 1
    if T > 1:
        assert (slot_ids == -1).any() and (slot_ids >= 0).any()
    want = Sampler(device=DEV)._apply_penalties(logits.to(DEV), seqs)
    got = ops.apply_penalties(
        logits.to(DEV), counts.to(DEV), slot_ids.to(DEV), params.to(DEV))
    diff = as_bits(got) != as_bits(want)
    rep = torch.tensor(
        [s.sampling.repetition_penalty != 1.0 for s in seqs], device=DEV)
    print(f"T={T} V={V}: differing elements {int(diff.sum())}, of them in "
          f"repetition-penalised rows {int(diff[rep].sum())}")
    assert torch.equal(as_bits(got), as_bits(want))
    assert not torch.equal(as_bits(got), as_bits(logits.to(DEV)))


@pytest.mark.parametrize("T,V", SHAPES)
def test_untouched_elements_and_guard_rows(T, V):
    logits, _, counts, slot_ids, params = penalty_case(T, V, first=3)
    S = counts.shape[0]
    live = slot_ids >= 0
    # a NaN payload pattern wherever the kernel must not write
    payload = (0x7FC00000 + 1 + torch.arange(T * V, dtype=torch.int32)
               % 0x1FFFFF).view(T, V).view(torch.float32)
    hit = torch.zeros(T, V, dtype=torch.bool)
    hit[live] = counts[slot_ids[live].long()] > 0
    logits = torch.where(hit, logits, payload)

    # one guard row on each side of both arrays
    big_l = torch.full((T + 2, V), float("nan"))
    big_l.view(torch.int32)[0] = 0x7FC01234
    big_l.view(torch.int32)[-1] = 0x7FC04321
    big_l[1:-1] = logits
    big_c = torch.full((S + 2, V), 5, dtype=torch.int32)
    big_c[1:-1] = counts
    dl, dc = big_l.to(DEV), big_c.to(DEV)
    ops.apply_penalties(dl[1:-1], dc[1:-1], slot_ids.to(DEV), params.to(DEV))
    out = dl.cpu()
    assert torch.equal(dc.cpu(), big_c)
    assert torch.equal(as_bits(out[0]), as_bits(big_l[0]))
    assert torch.equal(as_bits(out[-1]), as_bits(big_l[-1]))
    inner = out[1:-1]
    assert torch.equal(as_bits(inner)[~hit], as_bits(logits)[~hit])
    assert not torch.isnan(inner[hit]).any()
    changed = as_bits(inner) != as_bits(logits)
    assert changed.any() and not changed[~live].any()


def test_counts_add_is_exact():
    S, V, N = 4, 4099, 4096
    g = torch.Generator().manual_seed(0)
    hist = torch.randint(0, V, (N,), generator=g)
    hist[torch.randperm(N, generator=g)[:1000]] = 77
    big = torch.full((S + 2, V), 9, dtype=torch.int32, device=DEV)
    counts = big[1:-1]
    counts.zero_()
    ops.penalty_counts_add(
        counts, torch.full((N,), 2, dtype=torch.int32, device=DEV),
        hist.to(DEV))
    want = torch.zeros(S, V, dtype=torch.int32)
    want[2] = torch.bincount(hist, minlength=V).int()
    assert int(want[2, 77]) >= 1000
    assert torch.equal(counts.cpu(), want)

    # out-of-range tokens and slots are ignored, rows sharing a slot count
    slot_ids = torch.tensor([0, 0, 0, -1, S, 1, 3, 3, 1 << 30, -(1 << 31)],
                            dtype=torch.int32)
    token_ids = torch.tensor([-1, V, 1 << 40, 5, 5, 0, V - 1, V - 1, 6, 6])
    ops.penalty_counts_add(counts, slot_ids.to(DEV), token_ids.to(DEV))
    want[1, 0] += 1
    want[3, V - 1] += 2
    assert torch.equal(counts.cpu(), want)
    guard = big.cpu()
    assert bool((guard[0] == 9).all()) and bool((guard[-1] == 9).all())


# ---------------------------------------------------------------- engine

PROMPTS = [list(range(50, 120)), [11, 13, 17] * 20]
PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.5,
                 frequency_penalty=0.2)
SAMPLINGS = {
    "greedy": dict(max_tokens=24, **PENALTIES),
    "seeded": dict(max_tokens=24, temperature=0.8, top_k=50, top_p=0.9,
                   seed=1234, **PENALTIES),
}
_HOST_TOKENS = {}


def make_engine(**kw):
    mc = get_model_config("Qwen3-0.6B")
    mc.num_layers = 4
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=512),
        scheduler=SchedulerConfig(
            max_num_seqs=16, max_num_batched_tokens=2048, max_model_len=512,
        ),
        seed=7,
        sampler_backend="fused",
        **kw,
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


def host_tokens():
    """Both samplings on one engine with the penalties on the host path."""
    if not _HOST_TOKENS:
        host = make_engine(device_penalties=False)
        for name, sampling in SAMPLINGS.items():
            _HOST_TOKENS[name] = generate(host, sampling)
        assert host.num_async_steps == 0
        assert host.sampler.penalty_table is None
    return _HOST_TOKENS


def test_engine_penalised_sequences_stay_pipelined():
    eng = make_engine()
    assert eng._async_decode
    for name, sampling in SAMPLINGS.items():
        before = eng.num_async_steps
        tokens = generate(eng, sampling)
        assert all(len(t) == 24 for t in tokens)
        assert eng.num_async_steps > before, name
        assert tokens == host_tokens()[name], name
    table = eng.sampler.penalty_table
    assert tuple(table.counts.shape) == (64, eng.cfg.model.vocab_size)
    assert not table._slot_of


def test_engine_stop_token_inside_the_chain_returns_the_slot():
    first = host_tokens()["greedy"][0]
    pos = next(i for i in range(3, 24) if first[i] not in first[:i])
    sampling = dict(SAMPLINGS["greedy"], ignore_eos=False,
                    stop_token_ids=[first[pos]])
    host = make_engine(device_penalties=False)
    eng = make_engine()
    table = eng.sampler.penalty_table
    for _ in range(2):
        before = eng.num_async_steps
        tokens = generate(eng, sampling)
        # a sequence ended on the stop token, not on max_tokens
        assert any(len(t) < 24 and t[-1] == first[pos] for t in tokens)
        assert tokens == generate(host, sampling)
        assert eng.num_async_steps > before
        assert not table._slot_of and len(table._free) == 64


def test_engine_pipelining_does_not_change_tokens():
    sync = make_engine()
    sync._async_decode = False
    for name, sampling in SAMPLINGS.items():
        assert generate(sync, sampling) == host_tokens()[name], name
    assert sync.num_async_steps == 0
    assert sync.sampler.penalty_table.counts is not None


def test_engine_with_one_slot():
    one = make_engine(penalty_slots=1)
    for name, sampling in SAMPLINGS.items():
        assert generate(one, sampling) == host_tokens()[name], name
    assert one.sampler.penalty_table.counts.shape[0] == 1
