"""Speculative decoding for sampled, penalised and logprobs requests on the
CPU reference: ops.spec_accept, ops.apply_penalties_spec against
Sampler._apply_penalties on extended histories, Sampler.verify_drafts
against a row-by-row emulation with Sampler.sample, and the engine wiring
(tiny model). The case builders are shared with the GPU tests."""

import copy

import pytest
import torch

import fusioninfer_amd.ops as ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sampler import Sampler
from fusioninfer_amd.engine.sequence import SamplingParams, Sequence
from fusioninfer_amd.engine.spec_decode import SpeculativeConfig
from fusioninfer_amd.models.registry import get_model_config
from tests.test_device_penalties import penalty_case


# ------------------------------------------------------------ spec_accept

def accept_case(spans, width, device="cpu"):
    """spans: (sampled tokens, drafts) per span; the bonus row's draft slot
    is filled with -1. Returns the op's inputs."""
    sampled, drafts, cu = [], [], [0]
    for toks, d in spans:
        assert len(toks) == len(d) + 1
        sampled += toks
        drafts += list(d) + [-1]
        cu.append(len(sampled))
    return (
        torch.tensor(sampled, dtype=torch.int64, device=device),
        torch.tensor(drafts, dtype=torch.int64, device=device),
        torch.tensor(cu, dtype=torch.int32, device=device),
        width,
    )


def accept_expected(spans, width):
    """Independent of the reference: plain list arithmetic."""
    rows, n = [], []
    for toks, d in spans:
        m = 0
        while m < len(d) and toks[m] == d[m]:
            m += 1
        rows.append(toks[:m + 1] + [-1] * (width - m - 1))
        n.append(m + 1)
    return rows, n


def random_spans(S, seed, max_k=ops.SPEC_MAX_DRAFT):
    g = torch.Generator().manual_seed(seed)
    spans = []
    for i in range(S):
        k = int(torch.randint(0, max_k + 1, (1,), generator=g))
        toks = torch.randint(0, 1 << 40, (k + 1,), generator=g).tolist()
        d = toks[:k]
        cut = int(torch.randint(0, k + 2, (1,), generator=g))
        if cut < k:  # otherwise all accepted
            d[cut] = toks[cut] + 1
        spans.append((toks, d))
    return spans


@pytest.mark.parametrize("name,spans", [
    ("all accepted", [([4, 5, 6, 7], [4, 5, 6])]),
    ("rejected at row 0", [([4, 5, 6, 7], [9, 5, 6])]),
    ("rejected in the middle", [([4, 5, 6, 7], [4, 9, 6])]),
    ("bonus row only", [([8], [])]),
    ("unequal spans", [([1, 2, 3], [1, 2]), ([7], []),
                       ([4, 5, 6, 7, 8], [4, 5, 0, 7]), ([3, 3], [2])]),
])
def test_spec_accept_cases(name, spans):
    W = 5
    emitted, n_emit = ops.spec_accept(*accept_case(spans, W))
    rows, n = accept_expected(spans, W)
    assert emitted.dtype == torch.int64 and n_emit.dtype == torch.int32
    assert emitted.tolist() == rows, name
    assert n_emit.tolist() == n, name


def test_spec_accept_outputs_share_one_buffer():
    spans = random_spans(7, 0)
    buf = torch.full((ops.spec_accept_words(7, 17),), 99, dtype=torch.int64)
    emitted, n_emit = ops.spec_accept(*accept_case(spans, 17), out=buf)
    rows, n = accept_expected(spans, 17)
    assert emitted.tolist() == rows and n_emit.tolist() == n
    again = ops.spec_accept_sections(buf.clone(), 7, 17)
    assert again[0].tolist() == rows and again[1].tolist() == n


def test_spec_accept_malformed_spans_emit_nothing():
    sampled = torch.arange(10, 16)
    drafts = torch.tensor([10, 11, -1, 13, 14, -1])
    for cu in ([0, 0, 6], [0, 7, 6], [-1, 3, 6], [3, 0, 6], [0, 6, 9],
               [1 << 30, -(1 << 31), 6]):
        emitted, n_emit = ops.spec_accept(
            sampled, drafts, torch.tensor(cu, dtype=torch.int32), 4)
        assert n_emit[0] == 0 and emitted[0].tolist() == [-1] * 4, cu
    # a span longer than the width, next to a good one
    emitted, n_emit = ops.spec_accept(
        sampled, drafts, torch.tensor([0, 3, 6], dtype=torch.int32), 2)
    assert n_emit.tolist() == [0, 0]
    emitted, n_emit = ops.spec_accept(
        sampled, drafts, torch.tensor([0, 3, 6], dtype=torch.int32), 3)
    assert emitted.tolist() == [[10, 11, 12], [13, 14, 15]]


def test_spec_accept_rejects_bad_arguments():
    good = accept_case([([1, 2, 3], [1, 2])], 3)
    ops.spec_accept(*good)
    s, d, cu, w = good
    for bad in (
        (s.int(), d, cu, w), (s, d.int(), cu, w), (s, d[:2], cu, w),
        (s, d, cu.long(), w), (s, d, cu[:1], w), (s, d, cu, 0),
        (s, d, cu, ops.SPEC_MAX_DRAFT + 2), (s.view(1, 3), d, cu, w),
    ):
        with pytest.raises(ValueError):
            ops.spec_accept(*bad)
    with pytest.raises(ValueError):
        ops.spec_accept(s, d, cu, w, out=torch.empty(3, dtype=torch.int64))


# --------------------------------------------------- apply_penalties_spec

def spec_penalty_case(T, V, E, first=0, big_count=40):
    """penalty_case plus extra [T, E]: per row a mix of a token the history
    does not hold, one it holds, a token twice (frequency counts it twice),
    ids outside [0, V) and the -1 padding; row 0 keeps all E slots valid.
    Returns the case, extra and the sequences with the in-range extras
    appended to their histories."""
    logits, seqs, counts, slot_ids, params = penalty_case(
        T, V, first, big_count)
    g = torch.Generator().manual_seed(77 * T + V + E)
    extra = torch.full((T, E), -1, dtype=torch.int64)
    ahead = []
    for i, s in enumerate(seqs):
        hist = set(s.all_token_ids)
        zero = next(t for t in range(V - 1, -1, -1) if t not in hist)
        held = s.all_token_ids[0]
        pool = [zero, held, zero, V, 1 << 40, -1, V - 1, 0, -7]
        ids = [pool[j % len(pool)] for j in range(E)]
        if i == 0:
            ids = [zero] + torch.randint(
                0, V, (E - 1,), generator=g).tolist()
        extra[i] = torch.tensor(ids)
        a = copy.copy(s)
        a.output_token_ids = s.output_token_ids + [
            t for t in ids if 0 <= t < V]
        ahead.append(a)
        # the new token's logit is one the penalties change
        logits[i, zero] = 2.5
    return logits, ahead, counts, slot_ids, params, extra


@pytest.mark.parametrize("E", [1, 4, 16])
def test_penalties_spec_equals_the_sampler_on_extended_histories(E):
    logits, ahead, counts, slot_ids, params, extra = spec_penalty_case(
        5, 4099, E)
    want = Sampler()._apply_penalties(logits.clone(), ahead)
    keep = counts.clone()
    got = ops.apply_penalties_spec(
        logits.clone(), counts, slot_ids, params, extra)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(counts, keep)
    # the extras matter: without them the result differs
    plain = ops.apply_penalties(logits.clone(), counts, slot_ids, params)
    assert not torch.equal(plain.view(torch.int32), want.view(torch.int32))
    live = (slot_ids >= 0).nonzero().flatten().tolist()
    for i in live:
        zero = int(extra[i, 0])
        assert counts[slot_ids[i], zero] == 0
        assert got[i, zero] != logits[i, zero]


def test_penalties_spec_repeated_extra_counts_twice():
    V = 64
    logits = torch.full((1, V), 2.0)
    counts = torch.zeros(1, V, dtype=torch.int32)
    counts[0, 3] = 1
    slot = torch.zeros(1, dtype=torch.int32)
    params = torch.tensor([[1.0, 1.0, 0.0, 0.25]])
    extra = torch.tensor([[9, 3, 9, -1, V, 1 << 40]])
    got = ops.apply_penalties_spec(logits.clone(), counts, slot, params,
                                   extra)
    want = logits.clone()
    want[0, 9] = 2.0 - 0.25 * 2
    want[0, 3] = 2.0 - 0.25 * 2
    assert torch.equal(got, want)


def test_penalties_spec_rejects_bad_arguments():
    logits, _, counts, slot_ids, params, extra = spec_penalty_case(5, 64, 4)
    ops.apply_penalties_spec(logits, counts, slot_ids, params, extra)
    big = torch.full((5, ops.SPEC_MAX_DRAFT + 1), -1, dtype=torch.int64)
    for bad in (
        (logits.double(), counts, slot_ids, params, extra),
        (logits.t(), counts, slot_ids, params, extra),
        (logits, counts.long(), slot_ids, params, extra),
        (logits, counts[:, :63], slot_ids, params, extra),
        (logits, counts, slot_ids.long(), params, extra),
        (logits, counts, slot_ids, params[:, :3], extra),
        (logits, counts, slot_ids, params, extra.int()),
        (logits, counts, slot_ids, params, extra[:4]),
        (logits, counts, slot_ids, params, extra[:, :0]),
        (logits, counts, slot_ids, params, big),
        (logits, counts, slot_ids, params, extra[0]),
    ):
        with pytest.raises(ValueError):
            ops.apply_penalties_spec(*bad)


# ---------------------------------------------------------- verify_drafts

PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.5,
                 frequency_penalty=0.2)
# (sampling, rows, where the draft is made to differ; None = all accepted)
MIXED = [
    (dict(), 5, None),                                        # greedy
    (dict(temperature=0.8, top_k=50, top_p=0.9, min_p=0.02, seed=11), 4, 1),
    (dict(temperature=0.9, seed=12, **PENALTIES), 5, None),
    (dict(**PENALTIES), 3, 0),                       # greedy, penalised
    (dict(temperature=0.7, top_k=20, seed=13, logprobs=3), 4, None),
    (dict(logprobs=3, **PENALTIES), 1, None),        # no draft
    (dict(temperature=1.0, seed=14, logprobs=3, **PENALTIES), 5, 3),
]


def sequential(sampler, logits, seq, draft, rows):
    """Row-by-row emulation of one span with the non-speculative sampler:
    row j is sampled for a copy of the sequence whose output holds the
    tokens accepted so far; the first sample that differs from the draft
    ends the span. draft=None accepts everything (builds the chain).
    Returns (tokens, logprobs entries)."""
    cur = copy.copy(seq)
    cur.output_token_ids = list(seq.output_token_ids)
    toks, entries = [], []
    for j in range(rows):
        tok, lp = sampler.sample_with_logprobs(
            logits[j:j + 1].clone(), [cur])
        tok = int(tok)
        toks.append(tok)
        if lp is not None:
            entries.append(lp.entries(lp.buf.cpu())[0])
        cur.output_token_ids.append(tok)
        if draft is not None and (j == len(draft) or tok != draft[j]):
            break
    sampler.release_penalty_slot(cur)
    return toks, entries


def mixed_case(V, device="cpu"):
    """Logits [R, V] on `device` (a few hot columns per span, so that
    tokens repeat and the penalties bite) and the spans of MIXED: drafts
    are the tokens the sequential path emits, changed at one place where
    MIXED says so. Returns (logits, spans, expected tokens, expected
    logprobs entries)."""
    g = torch.Generator().manual_seed(V)
    spans, want_toks, want_lp, blocks = [], [], [], []
    emu = Sampler(backend="fused", device=device, seed=5)
    for i, (sampling, rows, differ) in enumerate(MIXED):
        x = torch.randn(rows, V, generator=g)
        hot = torch.randint(0, V, (6,), generator=g)
        x[:, hot] += 4.0
        x = x.to(device)
        prompt = hot[:3].tolist() * 4 + [int(hot[3])]
        seq = Sequence(f"m{i}", prompt, SamplingParams(**sampling))
        seq.output_token_ids = torch.randint(
            0, V, (i,), generator=g).tolist()
        chain, _ = sequential(emu, x, seq, None, rows)
        draft = chain[:rows - 1]
        if differ is not None:
            draft[differ] = (draft[differ] + 1) % V
        toks, entries = sequential(emu, x, seq, draft, rows)
        assert len(toks) == (rows if differ is None else differ + 1)
        spans.append((seq, draft))
        want_toks.append(toks)
        want_lp.append(entries if "logprobs" in sampling else None)
        blocks.append(x)
    return torch.cat(blocks), spans, want_toks, want_lp


def check_verify(V, device="cpu", **sampler_kw):
    logits, spans, want_toks, want_lp = mixed_case(V, device)
    sampler = Sampler(backend="fused", device=device, seed=5, **sampler_kw)
    hist = [list(s.all_token_ids) for s, _ in spans]
    emitted, accepted, lps = sampler.verify_drafts(logits.clone(), spans)
    assert emitted == want_toks
    assert accepted == [len(t) - 1 for t in want_toks]
    assert lps == want_lp
    assert any(t is not None for t in want_lp)
    # the sequences themselves are left alone
    assert [list(s.all_token_ids) for s, _ in spans] == hist
    return sampler, spans, emitted


def test_verify_drafts_equals_the_sequential_sampler():
    sampler, spans, emitted = check_verify(4099)
    # the table now holds history + emitted tokens of every penalised span
    table = sampler.penalty_table
    for i, ((seq, _), toks) in enumerate(zip(spans, emitted)):
        slot = table.slot_of(seq)
        assert (slot >= 0) == ("presence_penalty" in MIXED[i][0])
        if slot >= 0:
            want = torch.bincount(torch.tensor(seq.all_token_ids + toks),
                                  minlength=4099).int()
            assert torch.equal(table.counts[slot], want)
            assert table._counted_len[slot] == seq.num_tokens + len(toks)


def test_verify_drafts_without_enough_slots_takes_the_host_rows():
    check_verify(4099, penalty_slots=1)
    check_verify(4099, device_penalties=False)


def test_verify_drafts_transfers(monkeypatch):
    """One parameter copy to the device; the ops run once each."""
    calls = []
    for name in ("apply_penalties_spec", "sample_tokens", "spec_accept",
                 "penalty_counts_add", "token_logprobs"):
        orig = getattr(ops, name)

        def spy(*a, _orig=orig, _name=name, **k):
            calls.append(_name)
            return _orig(*a, **k)

        monkeypatch.setattr(ops, name, spy)
    logits, spans, want_toks, _ = mixed_case(257)
    sampler = Sampler(backend="fused", seed=5)
    sampler.penalty_table.sync([s for s, _ in spans], 257)
    del calls[:]
    emitted, _, _ = sampler.verify_drafts(logits, spans)
    assert emitted == want_toks
    assert calls == ["apply_penalties_spec", "sample_tokens", "spec_accept",
                     "penalty_counts_add", "token_logprobs"]


def test_verify_drafts_rejects_what_it_cannot_run():
    seq = Sequence("a", [1, 2, 3], SamplingParams())
    with pytest.raises(RuntimeError):
        Sampler().verify_drafts(torch.zeros(2, 8), [(seq, [1])])
    fused = Sampler(backend="fused")
    with pytest.raises(ValueError):
        fused.verify_drafts(torch.zeros(3, 8), [(seq, [1])])
    with pytest.raises(ValueError):
        fused.verify_drafts(torch.zeros(18, 8), [(seq, [1] * 17)])


# ------------------------------------------------------------------ engine

PROMPTS = [[5, 3, 8, 1] * 10, [11, 13, 17] * 8]
# penalties that favour the history (rp < 1, negative presence and
# frequency): sampled tokens then come back to tokens of the context, which
# is what lets the n-gram proposer find drafts for a sampled request on a
# random-init model
SAMPLED = dict(max_tokens=24, temperature=0.8, top_k=50, top_p=0.9, seed=11,
               repetition_penalty=0.8, presence_penalty=-0.5,
               frequency_penalty=-0.3, logprobs=2)
PENALTIES_BACK = dict(repetition_penalty=0.8, presence_penalty=-0.5,
                      frequency_penalty=-0.3, temperature=0.8, top_k=50,
                      top_p=0.9, seed=21, logprobs=1)


def make_engine(speculative=None, **kw):
    cfg = EngineConfig(
        model=get_model_config("tiny-qwen3"),
        cache=CacheConfig(num_gpu_blocks=256),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=1024, max_model_len=256
        ),
        seed=3,
        sampler_backend=kw.pop("sampler_backend", "fused"),
        speculative=speculative,
        **kw,
    )
    torch.manual_seed(0)
    return LLMEngine(cfg, device="cpu")


def generate(eng, sampling, prompts=PROMPTS):
    ids = [eng.add_request(p, SamplingParams(**sampling)) for p in prompts]
    done = {}
    while eng.has_unfinished():
        for o in eng.step():
            if o.finished:
                done[o.request_id] = o
    return [done[i] for i in ids]


def tokens(outs):
    return [o.output_token_ids for o in outs]


def ngram(**kw):
    return SpeculativeConfig(num_speculative_tokens=4, prompt_lookup_min=1,
                             **kw)


_PLAIN = {}


def plain_run():
    """The non-speculative fused engine on SAMPLED, computed once."""
    if not _PLAIN:
        _PLAIN["outs"] = generate(make_engine(), SAMPLED)
    return _PLAIN["outs"]


def test_engine_drafts_for_sampled_penalised_logprobs_requests():
    eng = make_engine(ngram())
    outs = generate(eng, SAMPLED)
    assert eng.num_spec_draft_tokens > 0
    assert 0 < eng.num_spec_accepted_tokens <= eng.num_spec_draft_tokens
    assert tokens(outs) == tokens(plain_run())
    # one entry per token; the values come from another attention path
    # than the plain engine's (verify rows are prefill rows), so they are
    # not compared bit for bit here: test_verify_drafts_* does that
    for o in outs:
        assert len(o.logprobs) == len(o.output_token_ids) == 24
        assert all(lp <= 0.0 and len(top) == 2 for lp, top in o.logprobs)
    table = eng.sampler.penalty_table
    assert not table._slot_of and len(table._free) == 64


def test_sampled_verify_off_keeps_the_old_eligibility():
    eng = make_engine(ngram(sampled_verify=False))
    outs = generate(eng, SAMPLED)
    assert eng.num_spec_draft_tokens == 0
    assert tokens(outs) == tokens(plain_run())
    # greedy requests still draft there, and through the same verify pass
    greedy = generate(eng, dict(max_tokens=24))
    assert eng.num_spec_draft_tokens > 0
    assert tokens(greedy) == tokens(generate(make_engine(),
                                             dict(max_tokens=24)))
    assert SpeculativeConfig().sampled_verify is True


def test_torch_backend_is_unchanged():
    eng = make_engine(ngram(), sampler_backend="torch")
    assert not eng._device_verify
    generate(eng, dict(SAMPLED, logprobs=None))
    assert eng.num_spec_draft_tokens == 0
    generate(eng, dict(max_tokens=24))
    assert eng.num_spec_draft_tokens > 0


def test_eligibility_predicate():
    eng = make_engine(ngram(), penalty_slots=1)
    ok = eng.proposer.draftable
    assert ok == eng._seq_draftable

    def seq(name="s", **kw):
        return Sequence(name, PROMPTS[0], SamplingParams(**kw))

    assert ok(seq(temperature=0.9))
    assert ok(seq(logprobs=ops.LOGPROBS_MAX_TOP))
    assert not ok(seq(logprobs=ops.LOGPROBS_MAX_TOP + 1))
    assert not ok(seq(logit_bias={1: 2.0}))
    assert not ok(seq(prompt_logprobs=1))
    assert not ok(seq(guided=object()))
    a, b = seq("a", presence_penalty=0.5), seq("b", presence_penalty=0.5)
    assert ok(a) and ok(b)
    eng.sampler.penalty_table.sync([a], 64)
    assert ok(a) and not ok(b)
    assert not make_engine(ngram(), device_logprobs=False).proposer.draftable(
        seq(logprobs=1))
    assert not make_engine(ngram(), device_penalties=False
                           ).proposer.draftable(a)


def test_long_drafts_are_truncated_to_the_kernel_limit():
    prompts = [[7, 9] * 40]
    plain = tokens(generate(make_engine(), dict(max_tokens=60),
                            prompts=prompts))
    eng = make_engine(SpeculativeConfig(num_speculative_tokens=40))
    # a proposer that knows the continuation and drafts 40 tokens of it
    eng.proposer.propose_all = lambda seqs: [
        plain[0][len(s.output_token_ids):][:40] for s in seqs]
    seen = []
    orig = eng.sampler.verify_drafts

    def spy(logits, spans):
        seen.extend(len(d) for _, d in spans)
        return orig(logits, spans)

    eng.sampler.verify_drafts = spy
    outs = generate(eng, dict(max_tokens=60), prompts=prompts)
    assert tokens(outs) == plain
    assert max(seen) == ops.SPEC_MAX_DRAFT
    assert eng.num_spec_draft_tokens == sum(seen)


def draft_engine(**kw):
    return make_engine(SpeculativeConfig(
        method="draft_model", model="tiny-qwen3",
        num_speculative_tokens=4), **kw)


def test_draft_model_of_the_same_architecture_top_k_1():
    """Draft == target weights: with top_k=1 at temperature 1 the only
    token left is the argmax the draft proposed, so everything is
    accepted. (top-k keeps ties, so this presumes a unique maximum at
    every step; the greedy run below shows these prompts have one, since
    a tie would make the two runs differ.)"""
    prompts = [[3, 9, 27, 4] * 4, [8, 8, 1] * 5]
    eng = draft_engine()
    outs = generate(eng, dict(max_tokens=21, temperature=1.0, top_k=1),
                    prompts=prompts)
    assert eng.num_spec_draft_tokens > 0
    assert eng.num_spec_accepted_tokens == eng.num_spec_draft_tokens
    assert eng.proposer._state == {}
    greedy = generate(make_engine(), dict(max_tokens=21), prompts=prompts)
    assert tokens(outs) == tokens(greedy)


def test_stop_token_inside_an_accepted_span():
    """The verify pass counts every emitted token into the table; when the
    engine stops on one of them, the rest is dropped with the slot, and
    the next owner of that slot starts from its own history."""
    sampling = dict(max_tokens=24, **PENALTIES_BACK)
    free_run = generate(make_engine(), sampling)
    spec = make_engine(ngram())
    spans = []
    orig = spec.sampler.verify_drafts

    def spy(logits, sp):
        out = orig(logits, sp)
        spans.extend((s.seq_id, len(s.output_token_ids), len(t))
                     for (s, _), t in zip(sp, out[0]))
        return out

    spec.sampler.verify_drafts = spy
    assert tokens(generate(spec, sampling)) == tokens(free_run)
    # a span of request 0 that emitted at least two tokens: stop on its
    # first one, so that the span goes on behind the stop
    sid, at, _ = next(s for s in spans if s[0] == free_run[0].request_id
                      and s[2] >= 2)
    first = free_run[0].output_token_ids
    stop = first[at]
    cut = first.index(stop) + 1
    assert cut <= at + 1 < len(first)
    stopped = dict(sampling, ignore_eos=False, stop_token_ids=[stop])
    plain = make_engine()
    table = spec.sampler.penalty_table
    for _ in range(2):
        outs = generate(spec, stopped)
        want = generate(plain, stopped)
        assert tokens(outs) == tokens(want)
        assert outs[0].output_token_ids == first[:cut]
        assert outs[0].finish_reason == "stop"
        assert not table._slot_of and len(table._free) == 64
    # the slots are reused by later requests, which are still exact
    assert tokens(generate(spec, sampling)) == tokens(free_run)
    assert not table._slot_of and len(table._free) == 64



def test_cli_switch():
    from fusioninfer_amd.server.__main__ import (
        build_engine_config, parse_args,
    )

    base = ["--model", "Qwen3-0.6B", "--speculative-config"]
    cfg = build_engine_config(parse_args(base + ['{"method": "ngram"}']))
    assert cfg.speculative.sampled_verify is True
    cfg = build_engine_config(parse_args(
        base + ['{"method": "ngram", "sampled_verify": false}']))
    assert cfg.speculative.sampled_verify is False
