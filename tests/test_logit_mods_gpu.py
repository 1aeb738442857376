"""Device-side logit_bias and grammar masks on the GPU (logit_mods.hip):
the kernel bit for bit against the torch host path, untouched elements and
guard rows, Sampler.verify_drafts / sample_with_logprobs against the same
calls on logits modified by torch, and the engine (4-layer Qwen3-0.6B as in
test_fused_sampler_gpu, one token per byte)."""

import re

import pytest
import torch

from fusioninfer_amd import ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sampler import Sampler
from fusioninfer_amd.engine.sequence import SamplingParams, Sequence
from fusioninfer_amd.engine.spec_decode import SpeculativeConfig
from fusioninfer_amd.guided import build_guided
from fusioninfer_amd.models.registry import get_model_config
from tests.test_logit_mods import (
    ModsCase, as_bits, byte_vocab, host_path, ids_of, text_of,
)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 4096), (5, 4099), (33, 32000), (2, 33)]


@pytest.mark.parametrize("T,V", SHAPES)
def test_kernel_equals_the_host_path(T, V):
    case = ModsCase(T, V)
    want = host_path(case.logits.to(DEV), case)
    got = ops.apply_logit_mods(case.logits.clone().to(DEV), *case.args(DEV))
    assert torch.equal(as_bits(got), as_bits(want))
    assert not torch.equal(as_bits(got), as_bits(case.logits.to(DEV)))
    m_ids, masks, cu, ids, vals = case.args(DEV)
    none = SimpleCase(case, mask=False, bias=False)
    for half, args in (
        (SimpleCase(case, bias=False), dict(mask_ids=m_ids, masks=masks)),
        (SimpleCase(case, mask=False),
         dict(bias_cu=cu, bias_ids=ids, bias_vals=vals)),
    ):
        got = ops.apply_logit_mods(case.logits.clone().to(DEV), **args)
        want = host_path(case.logits.to(DEV), half)
        assert torch.equal(as_bits(got), as_bits(want))
    assert torch.equal(as_bits(host_path(case.logits, none)),
                       as_bits(case.logits))


class SimpleCase:
    """A ModsCase with one half taken out, for host_path."""

    def __init__(self, case, mask=True, bias=True):
        self.T = case.T
        self.row_mask = case.row_mask if mask else [None] * case.T
        self.bias = case.bias if bias else [{}] * case.T


@pytest.mark.parametrize("T,V", SHAPES)
def test_untouched_elements_and_guard_rows(T, V):
    case = ModsCase(T, V)
    hit = case.touched()
    # a NaN payload pattern wherever the kernel must not write: allowed
    # elements without a bias, rows with neither mask nor bias
    payload = (0x7FC00000 + 1 + torch.arange(T * V, dtype=torch.int32)
               % 0x1FFFFF).view(T, V).view(torch.float32)
    logits = torch.where(hit, case.logits, payload)
    assert (~hit).all(dim=1).any() or T < 4

    # one guard row on each side of logits and of masks
    big_l = torch.full((T + 2, V), float("nan"))
    big_l.view(torch.int32)[0] = 0x7FC01234
    big_l.view(torch.int32)[-1] = 0x7FC04321
    big_l[1:-1] = logits
    M, W = case.masks.shape
    big_m = torch.full((M + 2, W), 0x0F0F0F0F, dtype=torch.int32)
    big_m[1:-1] = case.masks
    dl, dm = big_l.to(DEV), big_m.to(DEV)
    m_ids, _, cu, ids, vals = case.args(DEV)
    ops.apply_logit_mods(dl[1:-1], m_ids, dm[1:-1], cu, ids, vals)
    out = dl.cpu()
    assert torch.equal(dm.cpu(), big_m)
    assert torch.equal(m_ids.cpu(), case.mask_ids)
    assert torch.equal(cu.cpu(), case.bias_cu)
    assert torch.equal(ids.cpu(), case.bias_ids)
    assert torch.equal(as_bits(vals.cpu()), as_bits(case.bias_vals))
    # nothing in front of the first row, nothing past the last one: the
    # last mask word's bits >= V hold set and clear ones
    assert torch.equal(as_bits(out[0]), as_bits(big_l[0]))
    assert torch.equal(as_bits(out[-1]), as_bits(big_l[-1]))
    inner = out[1:-1]
    assert torch.equal(as_bits(inner)[~hit], as_bits(logits)[~hit])
    assert not torch.isnan(inner[hit]).any()
    for t in range(T):
        live = case.row_mask[t]
        if live is not None:
            assert bool((inner[t][~live] == float("-inf")).all())
    want = host_path(logits, case)
    assert torch.equal(as_bits(inner)[hit], as_bits(want)[hit])


def test_last_row_garbage_bits_do_not_reach_the_guard():
    """V = 33: the second mask word has one real bit; the others say
    'disallowed' and would be stores into the guard row."""
    V = 33
    masks = torch.tensor([[-1, 1], [0, 0]], dtype=torch.int32)
    big = torch.arange(4 * V, dtype=torch.float32).view(4, V).to(DEV)
    before = big.clone()
    ops.apply_logit_mods(
        big[1:3], torch.tensor([0, 1], dtype=torch.int32, device=DEV),
        masks.to(DEV))
    assert torch.equal(big[0], before[0]) and torch.equal(big[3], before[3])
    assert torch.equal(big[1], before[1])
    assert bool((big[2] == float("-inf")).all())


# -------------------------------------------------------------- sampler

V_S = 4099
VOCAB_S = byte_vocab(V_S)
SAMPLED = dict(temperature=0.8, top_k=50, top_p=0.95)


def guided_seq(name, spec, consumed, **kw):
    g = build_guided("regex", spec, VOCAB_S)
    for tok in ids_of(consumed):
        g.advance_token(tok)
    return Sequence(name, [5, 6, 7], SamplingParams(guided=g, **kw))


def torch_modified(logits, rows):
    """The host path on the device: rows = (sequence, grammar state or
    None) per logits row."""
    out = logits.clone()
    V = out.shape[1]
    for r, (s, st) in enumerate(rows):
        bias = s.sampling.logit_bias
        ids = [t for t in bias if 0 <= t < V]
        if ids:
            out[r, ids] += torch.tensor(
                [bias[t] for t in ids], dtype=out.dtype, device=out.device)
        if st is not None:
            allowed = s.sampling.guided.cache.mask(st, out.device)
            out[r].masked_fill_(~allowed, float("-inf"))
    return out


def plain_clone(s):
    sp = s.sampling
    return Sequence(s.seq_id, s.prompt_token_ids, SamplingParams(
        max_tokens=sp.max_tokens, temperature=sp.temperature, top_k=sp.top_k,
        top_p=sp.top_p, seed=sp.seed, logprobs=sp.logprobs))


def test_verify_drafts_equals_torch_modified_logits():
    spans = [
        (guided_seq("a", "(ab)+", "", seed=3, logprobs=2, **SAMPLED),
         ids_of("aba")),
        (guided_seq("b", "[ab]{8}c", "ab"), ids_of("ba")),
        (Sequence("c", [9, 8], SamplingParams(
            logit_bias={5: 30.0, 77: -2.0, V_S + 5: 1.0}, seed=9,
            **SAMPLED)), [5, 5, 9]),
        (Sequence("d", [1, 2], SamplingParams(seed=4, **SAMPLED)), [3]),
    ]
    rows = []
    for s, d in spans:
        g = s.sampling.guided
        states = g.walk(d) if g is not None else [None] * (len(d) + 1)
        assert len(states) == len(d) + 1
        rows += [(s, st) for st in states]
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(len(rows), V_S, generator=g) * 3).to(DEV)
    got = Sampler(seed=1, device=DEV, backend="fused",
                  device_logit_mods=True).verify_drafts(logits.clone(), spans)
    want = Sampler(seed=1, device=DEV, backend="fused").verify_drafts(
        torch_modified(logits, rows),
        [(plain_clone(s), d) for s, d in spans])
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2] == want[2] and got[2][0] is not None
    # the masks did their work: guided spans emit grammar text only
    assert set(text_of(got[0][0])) <= set("ab")
    assert set(text_of(got[0][1])) <= set("abc")
    # and the cursors have not moved
    assert spans[0][0].sampling.guided.walk([])[0] is (
        spans[0][0].sampling.guided.state)


def test_sample_with_logprobs_equals_torch_modified_logits():
    seqs = [
        guided_seq("a", "(ab)+", "a", logprobs=5),
        guided_seq("b", "(ab)+", "a", seed=3, logprobs=5, **SAMPLED),
        Sequence("c", [9, 8], SamplingParams(
            logit_bias={5: 30.0, 77: -2.0}, seed=9, logprobs=5, **SAMPLED)),
        Sequence("d", [1, 2], SamplingParams(logprobs=5)),
    ]
    rows = [(s, None if s.sampling.guided is None
             else s.sampling.guided.state) for s in seqs]
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(len(seqs), V_S, generator=g) * 3).to(DEV)
    got = Sampler(seed=1, device=DEV, backend="fused",
                  device_logit_mods=True).sample_with_logprobs(
        logits.clone(), seqs)
    want = Sampler(seed=1, device=DEV, backend="fused").sample_with_logprobs(
        torch_modified(logits, rows), [plain_clone(s) for s in seqs])
    assert torch.equal(got[0], want[0])
    assert got[1].num_top == want[1].num_top == [5] * 4
    assert torch.equal(got[1].buf, want[1].buf)
    assert text_of(got[0][:2].tolist()) == "bb"


# --------------------------------------------------------------- engine

_ENGINES = {}
_VOCAB = {}


def engine(spec, mods):
    key = (spec, mods)
    if key not in _ENGINES:
        mc = get_model_config("Qwen3-0.6B")
        mc.num_layers = 4
        cfg = EngineConfig(
            model=mc,
            cache=CacheConfig(num_gpu_blocks=512),
            scheduler=SchedulerConfig(
                max_num_seqs=16, max_num_batched_tokens=2048,
                max_model_len=512,
            ),
            seed=7,
            sampler_backend="fused",
            device_logit_mods=mods,
            speculative=SpeculativeConfig(
                num_speculative_tokens=4, prompt_lookup_min=1,
            ) if spec else None,
        )
        torch.manual_seed(0)
        _ENGINES[key] = LLMEngine(cfg, device=DEV)
    return _ENGINES[key]


def guided_params(kind, spec, **kw):
    if "v" not in _VOCAB:
        _VOCAB["v"] = byte_vocab(get_model_config("Qwen3-0.6B").vocab_size)
    return SamplingParams(guided=build_guided(kind, spec, _VOCAB["v"]), **kw)


def run_one(eng, prompt, sp):
    rid = eng.add_request(prompt, sp)
    steps = 0
    while eng.has_unfinished():
        steps += 1
        for o in eng.step():
            if o.finished and o.request_id == rid:
                done = o
    return done, steps


def test_engine_forced_guided_output_drafts():
    want = ids_of("abcd" * 10)
    prompt = ids_of("abcd" * 3)
    spec = engine(True, True)
    d0, a0 = spec.num_spec_draft_tokens, spec.num_spec_accepted_tokens
    out, steps = run_one(
        spec, prompt, guided_params("regex", "(abcd){10}", max_tokens=64))
    drafted = spec.num_spec_draft_tokens - d0
    print(f"drafted {drafted} accepted "
          f"{spec.num_spec_accepted_tokens - a0} steps {steps}")
    assert out.output_token_ids == want and out.finish_reason == "stop"
    assert drafted > 0
    assert spec.num_spec_accepted_tokens - a0 == drafted
    assert steps < len(want)
    plain, _ = run_one(
        engine(False, True), prompt,
        guided_params("regex", "(abcd){10}", max_tokens=64))
    assert plain.output_token_ids == want and plain.finish_reason == "stop"


def test_engine_free_guided_output_drafts():
    spec = engine(True, True)
    d0 = spec.num_spec_draft_tokens
    out, _ = run_one(
        spec, ids_of("abbabaab" * 3),
        guided_params("regex", "[ab]{24}", max_tokens=40, temperature=0.8,
                      seed=5))
    assert re.fullmatch("[ab]{24}", text_of(out.output_token_ids))
    assert out.finish_reason == "stop"
    assert spec.num_spec_draft_tokens > d0


def test_engine_biased_sequence_stays_pipelined():
    eng = engine(False, True)
    before = eng.num_async_steps
    out, _ = run_one(eng, list(range(50, 120)),
                     SamplingParams(max_tokens=16, logit_bias={7: 100.0}))
    assert out.output_token_ids == [7] * 16
    assert eng.num_async_steps > before


def test_engine_switch_on_equals_switch_off():
    """Speculation off: both runs share every kernel but apply_logit_mods
    (against the host's indexed add and masked_fill_)."""
    on, off = engine(False, True), engine(False, False)
    prompt = list(range(50, 120))
    choices = ["yes", "no", "maybe", "never"]
    outs = []
    for eng in (on, off):
        choice, _ = run_one(eng, prompt, guided_params(
            "choice", choices, max_tokens=16, temperature=0.9, seed=21))
        biased, _ = run_one(eng, prompt, SamplingParams(
            max_tokens=16, temperature=0.9, top_k=40, seed=22,
            logit_bias={t: 4.0 for t in range(100, 400)}))
        outs.append((choice.output_token_ids, biased.output_token_ids))
    assert outs[0] == outs[1]
    assert text_of(outs[0][0]) in choices
    assert len(outs[0][1]) == 16
    assert off.sampler.device_logit_mods is False
