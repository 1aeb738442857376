"""Device-side logit_bias and grammar masks on the CPU reference:
ops.apply_logit_mods against the literal host path of
LLMEngine._sample_and_emit, the packed masks and the non-mutating walk of
guided.py, draft trimming, and the engine wiring (tiny model, one token per
byte). The case builders are shared with the GPU tests."""

import re

import pytest
import torch

import fusioninfer_amd.ops as ops
from fusioninfer_amd.config import EngineConfig
from fusioninfer_amd.engine.sampler import Sampler
from fusioninfer_amd.engine.sequence import SamplingParams, Sequence
from fusioninfer_amd.guided import (
    GbnfGrammar, GuidedDecoder, GuidedMaskCache, JsonGrammar, RegexGrammar,
    Vocabulary, build_guided,
)
from tests.test_spec_sampled import PROMPTS, generate, make_engine, ngram, tokens

SHAPES = [(1, 31), (1, 32), (3, 33), (5, 4099), (33, 32000)]
KINDS = ["both", "mask", "bias_oov", "neither", "bias", "mask_id_M",
         "mask_id_big", "ones_bias"]


def as_bits(t):
    return t.contiguous().view(torch.int32)


def pack_bits(allowed, garbage=True):
    """bool [V] -> int32 [ceil(V / 32)], bit v & 31 of word v >> 5, written
    out longhand (independent of guided.py and of the reference). With
    `garbage` the bits of the last word at positions >= V are a mix of set
    and clear ones (a clear one would be a store past the row if the kernel
    looked at it), without it they are all clear."""
    V = allowed.numel()
    W = (V + 31) // 32
    words = [0] * W
    for v in allowed.nonzero().flatten().tolist():
        words[v >> 5] |= 1 << (v & 31)
    if garbage:
        for v in range(V, W * 32):
            if v % 3:
                words[v >> 5] |= 1 << (v & 31)
    return torch.tensor(
        [w - (1 << 32) if w >= 1 << 31 else w for w in words],
        dtype=torch.int32)


class ModsCase:
    """Inputs of ops.apply_logit_mods plus what the host path needs: per
    row the bool mask (or None) and the bias dict."""

    def __init__(self, T, V):
        g = torch.Generator().manual_seed(1000 * T + V)
        self.T, self.V = T, V
        self.logits = torch.randn(T, V, generator=g) * 4
        dense = torch.rand(V, generator=g) < 0.3
        dense[0] = False  # a disallowed column every masked row can bias
        dense[V - 1] = True
        ones = torch.ones(V, dtype=torch.bool)
        ones[V // 2] = False  # all-ones words but one
        sparse = torch.zeros(V, dtype=torch.bool)
        sparse[torch.randperm(V, generator=g)[:max(V // 30, 1)]] = True
        self.bool_masks = [dense, ones, sparse]
        self.masks = torch.stack([pack_bits(m) for m in self.bool_masks])
        M = len(self.bool_masks)
        self.row_mask, self.bias, mask_ids = [], [], []
        for t in range(T):
            kind = KINDS[t % len(KINDS)]
            mid, bias = -1, {}
            some = torch.randperm(V, generator=g)[:min(V, 40)].tolist()
            vals = (torch.randn(len(some), generator=g) * 50).tolist()
            if kind == "both":
                mid = 0
                bias = dict(zip(some, vals))
                bias[0] = 100.0  # disallowed by `dense`: must end at -inf
                bias[V - 1] = -7.5  # allowed
            elif kind == "mask":
                mid = 2 if t % 2 else 0
            elif kind == "bias_oov":
                bias = {-1: 3.0, V: 4.0, 2**31 - 1: 5.0, some[0]: vals[0]}
            elif kind == "bias":
                bias = dict(zip(some, vals))
            elif kind == "mask_id_M":
                mid = M
                bias = {some[1 % len(some)]: 1.25}
            elif kind == "mask_id_big":
                mid = 1 << 30
            elif kind == "ones_bias":
                mid = 1
                bias = {V // 2: 9.0, some[0]: vals[0]}
            mask_ids.append(mid)
            live = self.bool_masks[mid] if 0 <= mid < M else None
            self.row_mask.append(live)
            self.bias.append(bias)
            if live is not None:
                # a NaN under a cleared bit must still become -inf
                off = (~live).nonzero().flatten()
                self.logits[t, off[len(off) // 2]] = float("nan")
        self.mask_ids = torch.tensor(mask_ids, dtype=torch.int32)
        cu, ids, vals = [0], [], []
        for b in self.bias:
            ids += list(b.keys())
            vals += list(b.values())
            cu.append(len(ids))
        self.bias_cu = torch.tensor(cu, dtype=torch.int32)
        self.bias_ids = torch.tensor(ids, dtype=torch.int64).to(torch.int32)
        self.bias_vals = torch.tensor(vals, dtype=torch.float32)

    def args(self, device="cpu"):
        return tuple(x.to(device) for x in (
            self.mask_ids, self.masks, self.bias_cu, self.bias_ids,
            self.bias_vals))

    def touched(self):
        """bool [T, V]: the elements the op may store to (disallowed ones
        and allowed biased ones)."""
        hit = torch.zeros(self.T, self.V, dtype=torch.bool)
        for t in range(self.T):
            for k in self.bias[t]:
                if 0 <= k < self.V:
                    hit[t, k] = True
            if self.row_mask[t] is not None:
                hit[t] &= self.row_mask[t]
                hit[t] |= ~self.row_mask[t]
        return hit


def host_path(logits, case):
    """LLMEngine._sample_and_emit's own lines, row by row: the indexed add
    of the in-vocabulary bias entries, then masked_fill_(~allowed, -inf)."""
    out = logits.clone()
    V = out.shape[1]
    for t in range(case.T):
        bias = case.bias[t]
        ids = [k for k in bias if 0 <= k < V]
        if ids:
            out[t, ids] += torch.tensor(
                [bias[k] for k in ids], dtype=out.dtype, device=out.device)
        if case.row_mask[t] is not None:
            allowed = case.row_mask[t].to(out.device)
            out[t].masked_fill_(~allowed, float("-inf"))
    return out


# ---------------------------------------------------------- reference op

@pytest.mark.parametrize("T,V", SHAPES)
def test_reference_equals_the_host_path(T, V):
    case = ModsCase(T, V)
    want = host_path(case.logits, case)
    got = ops.apply_logit_mods(case.logits.clone(), *case.args())
    assert torch.equal(as_bits(got), as_bits(want))
    assert not torch.equal(as_bits(got), as_bits(case.logits))
    # the halves alone, and rows nothing applies to
    m_ids, masks, cu, ids, vals = case.args()
    only_mask = ops.apply_logit_mods(case.logits.clone(), m_ids, masks)
    only_bias = ops.apply_logit_mods(
        case.logits.clone(), bias_cu=cu, bias_ids=ids, bias_vals=vals)
    for t in range(T):
        live = case.row_mask[t]
        if live is None:
            assert torch.equal(as_bits(only_mask[t]), as_bits(case.logits[t]))
            assert torch.equal(as_bits(only_bias[t]), as_bits(want[t]))
        else:
            assert bool((only_mask[t][~live] == float("-inf")).all())
            assert torch.equal(as_bits(only_mask[t][live]),
                               as_bits(case.logits[t][live]))
            assert bool((want[t][~live] == float("-inf")).all())
        if not case.bias[t] and live is None:
            assert torch.equal(as_bits(got[t]), as_bits(case.logits[t]))
    same = ops.apply_logit_mods(case.logits.clone())
    assert torch.equal(as_bits(same), as_bits(case.logits))


def test_garbage_bits_past_the_vocabulary_are_ignored():
    V = 33
    allowed = torch.zeros(V, dtype=torch.bool)
    allowed[[1, 32]] = True
    logits = torch.arange(2 * V, dtype=torch.float32).view(2, V)
    ids = torch.zeros(2, dtype=torch.int32)
    a = ops.apply_logit_mods(
        logits.clone(), ids, pack_bits(allowed, garbage=True)[None])
    b = ops.apply_logit_mods(
        logits.clone(), ids, pack_bits(allowed, garbage=False)[None])
    assert torch.equal(a, b)
    assert a[0].isfinite().nonzero().flatten().tolist() == [1, 32]


def test_argument_checks():
    case = ModsCase(3, 33)
    m_ids, masks, cu, ids, vals = case.args()
    x = case.logits.clone()
    ops.apply_logit_mods(x, m_ids, masks, cu, ids, vals)
    wide = torch.zeros(3, 66)[:, ::2]
    bad = [
        dict(logits=x[0]),
        dict(logits=x.double()),
        dict(logits=wide),
        dict(mask_ids=m_ids.long()),
        dict(mask_ids=m_ids[:2]),
        dict(mask_ids=None),
        dict(masks=None),
        dict(masks=masks.long()),
        dict(masks=masks[0]),
        dict(masks=torch.zeros(3, 3, dtype=torch.int32)),
        dict(masks=torch.zeros(0, 2, dtype=torch.int32)),
        dict(masks=torch.zeros(3, 4, dtype=torch.int32)[:, ::2]),
        dict(bias_cu=cu.long()),
        dict(bias_cu=cu[:3]),
        dict(bias_cu=None),
        dict(bias_ids=ids.long()),
        dict(bias_ids=ids[:-1]),
        dict(bias_ids=ids.view(1, -1)),
        dict(bias_ids=None),
        dict(bias_vals=vals.double()),
        dict(bias_vals=vals[:-1]),
        dict(bias_vals=None),
        dict(bias_vals=torch.zeros(2 * vals.numel())[::2]),
        dict(masks=masks.to("meta")),
        dict(bias_vals=vals.to("meta")),
    ]
    for change in bad:
        kw = dict(logits=x, mask_ids=m_ids, masks=masks, bias_cu=cu,
                  bias_ids=ids, bias_vals=vals)
        kw.update(change)
        with pytest.raises(ValueError):
            ops.apply_logit_mods(**kw)
    big = torch.empty(ops.PENALTY_MAX_ROWS + 1, 1)
    with pytest.raises(ValueError):
        ops.apply_logit_mods(
            big, torch.zeros(big.shape[0], dtype=torch.int32),
            torch.zeros(1, 1, dtype=torch.int32))
    huge = torch.empty(1, 1 << 30, device="meta")
    with pytest.raises(ValueError):
        ops.apply_logit_mods(
            huge, torch.zeros(1, dtype=torch.int32, device="meta"),
            torch.zeros(1, 1 << 25, dtype=torch.int32, device="meta"))


# ------------------------------------------------------------ guided.py

def byte_vocab(vocab_size):
    """One token per byte: ids 3..258 decode to one latin-1 char, every
    other id to "". A literal regex then forces one token id per step."""
    return Vocabulary(
        vocab_size, lambda t: chr(t - 3) if 3 <= t < 259 else "")


def ids_of(text):
    return [ord(c) + 3 for c in text]


def text_of(toks):
    return "".join(chr(t - 3) for t in toks)


VOCAB = byte_vocab(1024)  # tiny-qwen3's vocabulary size
SMALL = byte_vocab(300)


@pytest.mark.parametrize("grammar,text", [
    (RegexGrammar(r"[ab]{3}-\d{2}"), "abb-42"),
    (JsonGrammar(root_object=True), '{"k": [1, true]}'),
    (GbnfGrammar('root ::= [a-z]+ ("-" [0-9]{2,3})?'), "abc-123"),
])
def test_packed_mask_equals_mask(grammar, text):
    cache = GuidedMaskCache(grammar, SMALL)
    dec = GuidedDecoder(cache)
    states = dec.walk(ids_of(text))
    assert len(states) == len(text) + 1
    empties = 0
    for st in states:
        m = cache.mask(st, "cpu")
        words, nonempty = cache.packed_mask(st)
        assert words.dtype == torch.int32 and words.device.type == "cpu"
        assert tuple(words.shape) == ((300 + 31) // 32,)
        assert torch.equal(words, pack_bits(m, garbage=False))
        assert nonempty is bool(m.any())
        empties += not nonempty
        again = cache.packed_mask(st)
        assert again[0] is words and again[1] is nonempty
    if isinstance(grammar, RegexGrammar):
        assert empties == 1  # the state after the last character


def test_walk_does_not_move_the_cursor():
    dec = build_guided("regex", "(abcd){2}", SMALL)
    dec.advance_token(ids_of("a")[0])
    before = dec.state
    states = dec.walk(ids_of("bcda"))
    assert dec.state is before and not dec.dead
    assert len(states) == 5 and states[0] is before
    fresh = build_guided("regex", "(abcd){2}", SMALL)
    g = fresh.cache.grammar
    fresh.advance_token(ids_of("a")[0])
    for tok, st in zip(ids_of("bcda"), states[1:]):
        fresh.advance_token(tok)
        assert g.signature(fresh.state) == g.signature(st)
    # a killing token ends the walk, an out-of-vocabulary id too
    assert len(dec.walk(ids_of("bcxd"))) == 3
    assert len(dec.walk(ids_of("b") + [300, 5])) == 2
    assert dec.walk([]) == [before]
    assert dec.state is before and not dec.dead
    dec.advance_token(ids_of("z")[0])
    assert dec.dead and dec.walk(ids_of("b")) == []
    assert dec.packed_allowed() is None


def test_walk_ends_at_a_grammar_error():
    dec = build_guided("regex", "ab*c", SMALL)

    class Exploding:
        def __init__(self, inner):
            self.inner, self.calls = inner, 0

        def initial(self):
            return self.inner.initial()

        def step(self, state, ch):
            self.calls += 1
            if self.calls > 2:
                raise ValueError("state explosion")
            return self.inner.step(state, ch)

    cache = GuidedMaskCache(Exploding(dec.cache.grammar), SMALL)
    walker = GuidedDecoder(cache)
    assert len(walker.walk(ids_of("abbbc"))) == 3


def test_draft_trimming():
    dec = build_guided("regex", "(abcd){2}", SMALL)
    n = dec.valid_draft_len
    assert n(ids_of("abcd")) == 4  # fully valid, not yet complete
    assert n(ids_of("abxd")) == 2  # disallowed at position 2
    assert n(ids_of("xbcd")) == 0
    assert n([]) == 0
    assert n(ids_of("ab") + [1]) == 2  # "" tokens are in no mask
    assert n(ids_of("ab") + [5000]) == 2
    assert n(ids_of("abcdabcd")) == 7  # the completing token is cut
    assert n(ids_of("abcdabcda")) == 7
    # complete but extendable states keep their drafts
    more = build_guided("regex", "a+", SMALL)
    assert more.valid_draft_len(ids_of("aaa")) == 3
    for tok in ids_of("abcdabc"):
        dec.advance_token(tok)
    assert n(ids_of("d")) == 0
    dec.advance_token(ids_of("q")[0])
    assert dec.dead and n(ids_of("a")) == 0


# ------------------------------------------------------------- sampler

def test_sampler_switch_needs_the_fused_backend():
    assert not Sampler().device_logit_mods
    assert not Sampler(backend="fused").device_logit_mods
    assert not Sampler(device_logit_mods=True).device_logit_mods
    assert Sampler(backend="fused", device_logit_mods=True).device_logit_mods


def test_sampler_gathers_shared_masks_and_cached_bias(monkeypatch):
    smp = Sampler(backend="fused", device_logit_mods=True)
    V = 300
    a = build_guided("regex", "(ab)+", SMALL)
    b = build_guided("regex", "(ab)+", SMALL)
    c = build_guided("regex", "(ab)+", SMALL)
    c.advance_token(ids_of("a")[0])
    biased = SamplingParams(logit_bias={7: 2.0, V: 1.0, -1: 1.0, 9: -3.0})
    seqs = [
        Sequence("a", [1], SamplingParams(guided=a)),
        Sequence("b", [1], SamplingParams(guided=b, logit_bias={5: 1.0})),
        Sequence("c", [1], SamplingParams(guided=c)),
        Sequence("d", [1], biased),
        Sequence("e", [1], SamplingParams()),
    ]
    mods = smp._gather_logit_mods(
        [(s, None if s.sampling.guided is None else s.sampling.guided.state)
         for s in seqs], V)
    assert mods.mask_ids == [0, 0, 1, -1, -1] and len(mods.masks) == 2
    assert mods.bias_cu == [0, 0, 1, 1, 3, 3]
    assert torch.cat(mods.bias_ids).tolist() == [5, 7, 9]
    first = biased._bias_arrays
    smp._gather_logit_mods([(seqs[3], None)], V)
    assert biased._bias_arrays is first
    # one buffer, one launch
    calls = []
    real = ops.apply_logit_mods
    monkeypatch.setattr(ops, "apply_logit_mods",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    logits = torch.randn(5, V)
    out = smp.sample(logits.clone(), seqs)
    assert len(calls) == 1
    assert text_of(out[:3].tolist()) == "aab"
    # only out-of-vocabulary entries: nothing to do
    oov = Sequence("f", [1], SamplingParams(logit_bias={V: 1.0}))
    assert smp._gather_logit_mods([(oov, None)], V) is None


def test_verify_drafts_rejects_a_draft_outside_the_grammar():
    smp = Sampler(backend="fused", device_logit_mods=True)
    seq = Sequence("a", [1], SamplingParams(
        guided=build_guided("regex", "(ab)+", SMALL)))
    with pytest.raises(ValueError):
        smp.verify_drafts(torch.zeros(3, 300), [(seq, ids_of("ax"))])


# -------------------------------------------------------------- engine

ABCD = ids_of("abcd" * 3)


def guided_params(kind, spec, **kw):
    return SamplingParams(guided=build_guided(kind, spec, VOCAB), **kw)


def run_one(eng, prompt, sp):
    rid = eng.add_request(prompt, sp)
    steps = 0
    while eng.has_unfinished():
        steps += 1
        for o in eng.step():
            if o.finished and o.request_id == rid:
                done = o
    return done, steps


def test_forced_guided_output_drafts_and_accepts_everything():
    want = ids_of("abcd" * 10)
    eng = make_engine(ngram(), device_logit_mods=True)
    out, steps = run_one(
        eng, ABCD, guided_params("regex", "(abcd){10}", max_tokens=64))
    assert out.output_token_ids == want
    assert out.finish_reason == "stop"
    assert eng.num_spec_draft_tokens > 0
    assert eng.num_spec_accepted_tokens == eng.num_spec_draft_tokens
    assert steps < len(want)
    off = make_engine(ngram())
    out_off, steps_off = run_one(
        off, ABCD, guided_params("regex", "(abcd){10}", max_tokens=64))
    assert off.num_spec_draft_tokens == 0
    assert out_off.output_token_ids == want
    assert out_off.finish_reason == "stop"
    assert steps < steps_off


def test_free_guided_output_equals_the_plain_run():
    def sp():
        return guided_params("regex", "[ab]{24}", max_tokens=40,
                             temperature=0.8, seed=5)

    prompt = ids_of("abbabaab" * 3)
    plain, _ = run_one(make_engine(), prompt, sp())
    assert re.fullmatch("[ab]{24}", text_of(plain.output_token_ids))
    assert plain.finish_reason == "stop"
    for spec in (None, ngram()):
        for on in (True, False):
            if spec is None and not on:
                continue
            eng = make_engine(spec, device_logit_mods=on)
            out, _ = run_one(eng, prompt, sp())
            assert out.output_token_ids == plain.output_token_ids, (spec, on)
            assert out.finish_reason == "stop"
            if spec is not None:
                assert (eng.num_spec_draft_tokens > 0) is on


def test_biased_sequences_stay_pipelined():
    sampling = dict(max_tokens=16, logit_bias={7: 100.0})
    eng = make_engine(device_logit_mods=True)
    assert eng._seq_async_ok(
        Sequence("s", PROMPTS[0], SamplingParams(**sampling)))
    outs = generate(eng, sampling)
    assert eng.num_async_steps > 0
    assert all(t == [7] * 16 for t in tokens(outs))
    off = make_engine()
    assert tokens(generate(off, sampling)) == tokens(outs)
    assert off.num_async_steps == 0


def test_negative_bias_changes_the_greedy_token():
    plain = tokens(generate(make_engine(), dict(max_tokens=8)))
    first = plain[0][0]
    sampling = dict(max_tokens=8, logit_bias={first: -100.0})
    on = tokens(generate(make_engine(device_logit_mods=True), sampling))
    assert on[0] != plain[0] and first not in on[0]
    assert on == tokens(generate(make_engine(), sampling))
    sampled = dict(sampling, temperature=0.8, top_k=20, seed=4,
                   presence_penalty=0.5)
    assert tokens(generate(make_engine(device_logit_mods=True), sampled)) == (
        tokens(generate(make_engine(), sampled)))
    # the host-penalty fall-back keeps bias in front of the penalties too
    assert tokens(generate(make_engine(device_logit_mods=True,
                                       device_penalties=False), sampled)) == (
        tokens(generate(make_engine(device_penalties=False), sampled)))


def test_biased_sequences_draft():
    sampling = dict(max_tokens=16, logit_bias={7: 100.0})
    eng = make_engine(ngram(), device_logit_mods=True)
    outs = generate(eng, sampling)
    assert eng.num_spec_draft_tokens > 0
    assert eng.num_spec_accepted_tokens == eng.num_spec_draft_tokens
    assert all(t == [7] * 16 for t in tokens(outs))
    off = make_engine(ngram())
    generate(off, sampling)
    assert off.num_spec_draft_tokens == 0


def test_switch_off_keeps_the_old_eligibility():
    assert EngineConfig().device_logit_mods is False
    biased = Sequence("b", PROMPTS[0], SamplingParams(logit_bias={1: 2.0}))
    guided = Sequence("g", PROMPTS[0], guided_params("regex", "a+"))
    off = make_engine(ngram())
    assert not off.sampler.device_logit_mods
    for s in (biased, guided):
        assert not off._seq_async_ok(s)
        assert not off.proposer.draftable(s)
    on = make_engine(ngram(), device_logit_mods=True)
    assert on._seq_async_ok(biased) and not on._seq_async_ok(guided)
    assert on.proposer.draftable(biased) and on.proposer.draftable(guided)
    torch_eng = make_engine(ngram(), sampler_backend="torch",
                            device_logit_mods=True)
    assert not torch_eng.sampler.device_logit_mods
    assert not torch_eng._seq_async_ok(biased)


def test_cli_flag():
    from fusioninfer_amd.server.__main__ import (
        build_engine_config, parse_args,
    )

    base = ["--model", "Qwen3-0.6B", "--sampler-backend", "fused"]
    assert build_engine_config(parse_args(base)).device_logit_mods is False
    cfg = build_engine_config(parse_args(base + ["--device-logit-mods"]))
    assert cfg.device_logit_mods is True


def test_no_launch_when_no_row_needs_it(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("apply_logit_mods must not run")

    monkeypatch.setattr(ops, "apply_logit_mods", boom)
    for spec in (None, ngram()):
        eng = make_engine(spec, device_logit_mods=True)
        outs = generate(eng, dict(max_tokens=12))
        assert all(len(t) == 12 for t in tokens(outs))


def test_out_of_vocabulary_bias_is_ignored():
    plain = tokens(generate(make_engine(), dict(max_tokens=8)))
    sampling = dict(max_tokens=8, logit_bias={10**6: 50.0, -3: 50.0})
    eng = make_engine(device_logit_mods=True)
    assert tokens(generate(eng, sampling)) == plain


def test_empty_grammar_finishes_without_emitting():
    eng = make_engine(device_logit_mods=True)
    sp = guided_params("regex", "ab", max_tokens=8)
    sp.guided.advance_token(ids_of("z")[0])  # dead before the first token
    out, _ = run_one(eng, ABCD, sp)
    assert out.output_token_ids == [] and out.finish_reason == "stop"
