"""Speculative decoding for sampled, penalised and logprobs requests on the
GPU: apply_penalties_spec (penalties.hip) bit for bit against
Sampler._apply_penalties on extended histories, untouched elements and
guard rows, spec_accept (spec_verify.hip) against the reference,
Sampler.verify_drafts against the row-by-row sampler on the same device
logits, and the engine (4-layer Qwen3-0.6B as in test_device_penalties_gpu).

Tokens of a speculative and a non-speculative engine are not compared at
temperature > 0: verify rows come from the paged-prefill attention path and
plain decode rows from the decode kernel, their logits differ in the low
bits, and a draw whose threshold falls inside that difference flips. The
same-logits emulation is the exactness check here."""

import pytest
import torch

from fusioninfer_amd import ops
from fusioninfer_amd.engine.sampler import Sampler
from fusioninfer_amd.engine.sequence import SamplingParams
from fusioninfer_amd.engine.spec_decode import SpeculativeConfig
from tests.test_device_penalties_gpu import make_engine
from tests.test_spec_sampled import (
    accept_case, accept_expected, check_verify, random_spans,
    spec_penalty_case,
)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 4096), (5, 4099), (33, 32000)]


def as_bits(t):
    return t.contiguous().view(torch.int32)


# --------------------------------------------------- apply_penalties_spec

@pytest.mark.parametrize("E", [1, 4, 16])
@pytest.mark.parametrize("T,V", SHAPES)
def test_penalties_spec_kernel_equals_the_sampler(T, V, E):
    logits, ahead, counts, slot_ids, params, extra = spec_penalty_case(
        T, V, E, big_count=1100)
    want = Sampler(device=DEV)._apply_penalties(logits.to(DEV), ahead)
    got = ops.apply_penalties_spec(
        logits.to(DEV), counts.to(DEV), slot_ids.to(DEV), params.to(DEV),
        extra.to(DEV))
    diff = as_bits(got) != as_bits(want)
    print(f"T={T} V={V} E={E}: differing elements {int(diff.sum())}")
    assert torch.equal(as_bits(got), as_bits(want))
    plain = ops.apply_penalties(
        logits.to(DEV), counts.to(DEV), slot_ids.to(DEV), params.to(DEV))
    assert not torch.equal(as_bits(plain), as_bits(want))


@pytest.mark.parametrize("E", [1, 4, 16])
@pytest.mark.parametrize("T,V", SHAPES)
def test_penalties_spec_untouched_elements_and_guard_rows(T, V, E):
    logits, _, counts, slot_ids, params, extra = spec_penalty_case(
        T, V, E, first=3)
    S = counts.shape[0]
    live = slot_ids >= 0
    # effective count > 0: histogram or an in-range extra id
    hit = torch.zeros(T, V, dtype=torch.bool)
    hit[live] = counts[slot_ids[live].long()] > 0
    for i in live.nonzero().flatten().tolist():
        ids = extra[i][(extra[i] >= 0) & (extra[i] < V)]
        hit[i, ids] = True
    zero_count_hits = hit.clone()
    zero_count_hits[live] &= counts[slot_ids[live].long()] == 0
    assert zero_count_hits.any()
    # a NaN payload pattern wherever the kernel must not write
    payload = (0x7FC00000 + 1 + torch.arange(T * V, dtype=torch.int32)
               % 0x1FFFFF).view(T, V).view(torch.float32)
    logits = torch.where(hit, logits, payload)

    # one guard row on each side of both arrays
    big_l = torch.full((T + 2, V), float("nan"))
    big_l.view(torch.int32)[0] = 0x7FC01234
    big_l.view(torch.int32)[-1] = 0x7FC04321
    big_l[1:-1] = logits
    big_c = torch.full((S + 2, V), 5, dtype=torch.int32)
    big_c[1:-1] = counts
    dl, dc = big_l.to(DEV), big_c.to(DEV)
    ops.apply_penalties_spec(dl[1:-1], dc[1:-1], slot_ids.to(DEV),
                             params.to(DEV), extra.to(DEV))
    out = dl.cpu()
    assert torch.equal(dc.cpu(), big_c)
    assert torch.equal(as_bits(out[0]), as_bits(big_l[0]))
    assert torch.equal(as_bits(out[-1]), as_bits(big_l[-1]))
    inner = out[1:-1]
    assert torch.equal(as_bits(inner)[~hit], as_bits(logits)[~hit])
    assert not torch.isnan(inner[hit]).any()
    changed = as_bits(inner) != as_bits(logits)
    assert changed.any() and not changed[~live].any()
    assert changed[zero_count_hits].any()


# ------------------------------------------------------------ spec_accept

@pytest.mark.parametrize("S", [1, 7, 64])
def test_spec_accept_kernel_equals_the_reference(S):
    spans = random_spans(S, seed=S)
    W = ops.SPEC_MAX_DRAFT + 1
    sampled, drafts, cu, _ = accept_case(spans, W)
    want = ops.spec_accept(sampled, drafts, cu, W)
    rows, n = accept_expected(spans, W)
    assert want[0].tolist() == rows and want[1].tolist() == n
    # guard elements on both sides of each output: the two sections lie in
    # one buffer, so an element in front, S odd or even the pad word
    # between n_emit and the end, and an element behind
    words = ops.spec_accept_words(S, W)
    GUARD = 0x5A5A5A5A5A5A5A5A
    big = torch.full((words + 2,), GUARD, dtype=torch.int64, device=DEV)
    emitted, n_emit = ops.spec_accept(
        sampled.to(DEV), drafts.to(DEV), cu.to(DEV), W, out=big[1:-1])
    assert torch.equal(emitted.cpu(), want[0])
    assert torch.equal(n_emit.cpu(), want[1])
    host = big.cpu()
    assert host[0] == GUARD and host[-1] == GUARD
    if S % 2:
        assert host[1:-1][S * W:].view(torch.int32)[S] == 0x5A5A5A5A


def test_spec_accept_kernel_malformed_spans():
    sampled = torch.arange(10, 16, device=DEV)
    drafts = torch.tensor([10, 11, -1, 13, 14, -1], device=DEV)
    cu = torch.tensor([0, 0, 7, 3, 6, 9, -1, 2], dtype=torch.int32)
    want = ops.spec_accept(sampled.cpu(), drafts.cpu(), cu, 3)
    assert want[1].tolist() == [0, 0, 0, 3, 0, 0, 0]
    got = ops.spec_accept(sampled, drafts, cu.to(DEV), 3)
    assert torch.equal(got[0].cpu(), want[0])
    assert torch.equal(got[1].cpu(), want[1])


# ---------------------------------------------------------- verify_drafts

@pytest.mark.parametrize("V", [4099, 32000])
def test_verify_drafts_equals_the_sequential_sampler(V):
    sampler, spans, emitted = check_verify(V, DEV)
    table = sampler.penalty_table
    for (seq, _), toks in zip(spans, emitted):
        slot = table.slot_of(seq)
        if slot >= 0:
            want = torch.bincount(torch.tensor(seq.all_token_ids + toks),
                                  minlength=V).int()
            assert torch.equal(table.counts[slot].cpu(), want)


# ------------------------------------------------------------------ engine

PROMPTS = [[5, 3, 8, 1] * 15, [11, 13, 17] * 20]
# penalties that favour the history, so that sampled tokens return to the
# context and the n-gram proposer finds drafts on random-init weights
BACK = dict(repetition_penalty=0.8, presence_penalty=-1.0,
            frequency_penalty=-0.5)
SAMPLED = dict(max_tokens=24, temperature=0.8, top_k=50, top_p=0.9,
               seed=1234, logprobs=2, **BACK)


def spec_engine():
    return make_engine(speculative=SpeculativeConfig(
        num_speculative_tokens=4, prompt_lookup_min=1))


def generate(eng, sampling, prompts=PROMPTS):
    ids = [eng.add_request(p, SamplingParams(**sampling)) for p in prompts]
    done = {}
    while eng.has_unfinished():
        for o in eng.step():
            if o.finished:
                done[o.request_id] = o
    return [done[i] for i in ids]


def test_engine_drafts_fire_for_sampled_penalised_logprobs_requests():
    runs = []
    for _ in range(2):
        eng = spec_engine()
        outs = generate(eng, SAMPLED)
        print(f"drafted {eng.num_spec_draft_tokens} accepted "
              f"{eng.num_spec_accepted_tokens}")
        assert eng.num_spec_draft_tokens > 0
        assert eng.num_spec_accepted_tokens <= eng.num_spec_draft_tokens
        for o in outs:
            assert len(o.output_token_ids) == 24
            assert len(o.logprobs) == 24
        table = eng.sampler.penalty_table
        assert not table._slot_of and len(table._free) == 64
        runs.append([o.output_token_ids for o in outs])
    # two fresh engines give identical tokens
    assert runs[0] == runs[1]


# top-k keeps ties, so top_k=1 equals greedy only where every row has a
# unique maximum. The bf16 logits of the random-init model tie at the
# maximum now and then: of eight prompt pairs of this form, 24 tokens each,
# two had no tied row (this one and the same with 505.. / 511..) and gave
# equal runs; five of the six with tied rows gave different ones.
UNTIED_PROMPTS = [[105, 103, 108, 101] * 15, [111, 113, 117] * 20]


def test_engine_top_k_1_equals_the_greedy_speculative_run(monkeypatch):
    """Both runs go through verify_drafts on one engine."""
    tied = []
    sample_tokens = ops.sample_tokens

    def spy(logits, *a):
        top = logits.max(dim=-1, keepdim=True).values
        tied.append(((logits == top).sum(dim=-1) > 1).sum())
        return sample_tokens(logits, *a)

    monkeypatch.setattr(ops, "sample_tokens", spy)
    eng = spec_engine()
    greedy = generate(eng, dict(max_tokens=24), UNTIED_PROMPTS)
    drafted = eng.num_spec_draft_tokens
    assert drafted > 0
    # the premise: no row of the greedy run had a tied maximum
    assert int(torch.stack(tied).sum()) == 0
    top1 = generate(eng, dict(max_tokens=24, temperature=1.0, top_k=1),
                    UNTIED_PROMPTS)
    assert eng.num_spec_draft_tokens > drafted
    assert ([o.output_token_ids for o in top1]
            == [o.output_token_ids for o in greedy])
    table = eng.sampler.penalty_table
    assert not table._slot_of and len(table._free) == 64
