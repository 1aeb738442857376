"""Device-side sampling penalties on the CPU reference: ops.apply_penalties
against Sampler._apply_penalties, ops.penalty_counts_add, the PenaltyTable
bookkeeping and the engine wiring (tiny model). The case builder is shared
with the GPU tests."""

import pytest
import torch

import fusioninfer_amd.ops as ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sampler import (
    PenaltyTable, Sampler, penalty_params,
)
from fusioninfer_amd.engine.sequence import SamplingParams, Sequence
from fusioninfer_amd.models.registry import get_model_config

# (repetition, presence, frequency); row i of a case takes MIXES[(first + i)
# % 10]. Rows 0-4: each penalty alone, all three (negative presence), none.
# Rows 5-9: a negative presence alone, all three, none, rp < 1, rp + freq.
MIXES = [
    (1.3, 0.0, 0.0), (1.0, 0.5, 0.0), (1.0, 0.0, 0.2), (1.7, -0.4, 0.3),
    (1.0, 0.0, 0.0),
    (1.0, -0.7, 0.0), (1.3, 0.5, 0.2), (1.0, 0.0, 0.0), (0.8, 0.0, 0.0),
    (1.05, 0.0, 1.5),
]


def _penalised(mix):
    return mix != (1.0, 0.0, 0.0)


def penalty_case(T, V, first=0, big_count=40):
    """Inputs for one shape (CPU tensors): logits with both signs, +-0 and
    -inf at penalised tokens, sequences whose histories repeat tokens up to
    `big_count` times, and the device-side view of the same: counts [T + 2,
    V] with the slots in scrambled order, slot_ids (-1 for the rows without
    penalties, whose params are set to values that would change the row)
    and params."""
    g = torch.Generator().manual_seed(1000 * T + V + first)
    logits = torch.randn(T, V, generator=g) * 4
    S = T + 2
    order = torch.randperm(S, generator=g).tolist()
    counts = torch.zeros(S, V, dtype=torch.int32)
    seqs, slots, params = [], [], []
    for i in range(T):
        mix = MIXES[(first + i) % len(MIXES)]
        n = 20 + int(torch.randint(0, 200, (1,), generator=g))
        hist = torch.randint(0, V, (n,), generator=g)
        hot = hist[:3].tolist()
        hist = torch.cat([
            hist,
            torch.full((big_count,), hot[0]),
            torch.full((7,), hot[1]),
            torch.tensor([0, V - 1]),  # the row's first and last column
        ])
        hist = hist[torch.randperm(hist.numel(), generator=g)]
        special = hist.unique()[:8].tolist()
        for tok, val in zip(special, (0.0, -0.0, float("-inf"), 1e-30,
                                      -1e-30, 37.5, -37.5, float("-inf"))):
            logits[i, tok] = val
        seqs.append(Sequence(
            f"s{i}", hist[:5].tolist(),
            SamplingParams(repetition_penalty=mix[0],
                           presence_penalty=mix[1],
                           frequency_penalty=mix[2]),
        ))
        seqs[-1].output_token_ids = hist[5:].tolist()
        if _penalised(mix):
            slot = order[i]
            counts[slot] = torch.bincount(hist, minlength=V).int()
            params.append(penalty_params(seqs[-1].sampling))
        else:
            slot = -1
            params.append([2.0, 0.5, 1.0, 1.0])
        slots.append(slot)
    return (
        logits, seqs, counts,
        torch.tensor(slots, dtype=torch.int32),
        torch.tensor(params, dtype=torch.float32),
    )


# ------------------------------------------------------------------- ops

@pytest.mark.parametrize("first", [0, 5])
def test_cpu_fallback_equals_the_sampler(first):
    logits, seqs, counts, slot_ids, params = penalty_case(5, 4099, first)
    assert (slot_ids == -1).sum() == 1
    want = Sampler()._apply_penalties(logits.clone(), seqs)
    assert not torch.equal(want, logits)
    keep = counts.clone()
    got = ops.apply_penalties(logits.clone(), counts, slot_ids, params)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(counts, keep)


def test_counts_add_on_cpu():
    S, V = 3, 50
    counts = torch.zeros(S, V, dtype=torch.int32)
    slot_ids = torch.tensor([0, 0, 2, -1, 3, 2, 1, 1], dtype=torch.int32)
    token_ids = torch.tensor([7, 7, 49, 5, 5, -1, 50, 1 << 40])
    ops.penalty_counts_add(counts, slot_ids, token_ids)
    want = torch.zeros(S, V, dtype=torch.int32)
    want[0, 7] = 2
    want[2, 49] = 1
    assert torch.equal(counts, want)


def test_dispatch_rejects_bad_arguments():
    logits, _, counts, slot_ids, params = penalty_case(5, 64)
    good = (logits, counts, slot_ids, params)
    ops.apply_penalties(*good)
    for bad in (
        (logits.double(), counts, slot_ids, params),
        (logits.t(), counts, slot_ids, params),
        (logits[0], counts, slot_ids, params),
        (logits, counts.long(), slot_ids, params),
        (logits, counts[:, :63], slot_ids, params),
        (logits, counts, slot_ids.long(), params),
        (logits, counts, slot_ids[:4], params),
        (logits, counts, slot_ids, params[:, :3]),
        (logits, counts, slot_ids, params.double()),
    ):
        with pytest.raises(ValueError):
            ops.apply_penalties(*bad)
    tok = torch.zeros(5, dtype=torch.int64)
    ops.penalty_counts_add(counts, slot_ids, tok)
    for bad in (
        (counts.long(), slot_ids, tok),
        (counts, slot_ids.long(), tok),
        (counts, slot_ids, tok.int()),
        (counts, slot_ids, tok[:4]),
        (counts[0], slot_ids, tok),
    ):
        with pytest.raises(ValueError):
            ops.penalty_counts_add(*bad)


# ----------------------------------------------------------------- table

V_TABLE = 257


def _bincount(seq):
    return torch.bincount(torch.tensor(seq.all_token_ids),
                          minlength=V_TABLE).int()


def _pen_seq(name, prompt, **kw):
    kw = kw or dict(repetition_penalty=1.3, presence_penalty=0.5,
                    frequency_penalty=0.2)
    return Sequence(name, prompt, SamplingParams(**kw))


def test_table_follows_the_sequences():
    sampler = Sampler(backend="fused", penalty_slots=3)
    host = Sampler(backend="fused", device_penalties=False)
    table = sampler.penalty_table
    assert host.penalty_table is None
    assert table.counts is None
    a = _pen_seq("a", [3, 3, 9, 200])
    b = _pen_seq("b", [1, 2, 3] * 5, frequency_penalty=0.4)
    c = _pen_seq("c", [256, 0, 256], presence_penalty=-0.3)
    plain = Sequence("plain", [4, 5, 6], SamplingParams())
    d = None
    seqs = [a, plain, b, c]
    g = torch.Generator().manual_seed(0)
    for step in range(12):
        if step == 5:
            # b finishes; a new sequence takes over its slot
            slot_b = table.slot_of(b)
            sampler.release_penalty_slot(b)
            assert table.slot_of(b) == -1
            d = _pen_seq("d", [7] * 30)
            seqs = [a, plain, d, c]
        if step == 8:
            # tokens the table did not see: the row is rebuilt
            c.output_token_ids.extend([11, 11])
        rebuilds = table.num_rebuilds
        logits = torch.randn(len(seqs), V_TABLE, generator=g) * 3
        out = sampler.sample(logits.clone(), seqs)
        # same tokens as the host path on the same logits
        assert torch.equal(out, host.sample(logits.clone(), seqs))
        first_use = {0: 3, 5: 1, 8: 1}
        assert table.num_rebuilds - rebuilds == first_use.get(step, 0)
        if step == 5:
            assert table.slot_of(d) == slot_b
        for s, tok in zip(seqs, out.tolist()):
            s.append_token(tok)
        assert table.slot_of(plain) == -1
        for s in seqs:
            if s is not plain:
                row = table.counts[table.slot_of(s)]
                assert torch.equal(row, _bincount(s)), (step, s.seq_id)
    assert table.counts.shape == (3, V_TABLE)
    assert table.counts.dtype == torch.int32


def test_table_full_falls_back_to_the_host_row():
    table = PenaltyTable(1)
    a, b = _pen_seq("a", [1, 1, 2]), _pen_seq("b", [2, 2, 3])
    assert table.sync([a, b], V_TABLE) == [0, -1]
    table.release(a)
    assert table.sync([b, a], V_TABLE) == [0, -1]
    assert torch.equal(table.counts[0], _bincount(b))

    # the out-of-slot row takes the host path: same tokens as all-host
    a, b = _pen_seq("a", [1, 1, 2]), _pen_seq("b", [2, 2, 3])
    logits = torch.zeros(2, V_TABLE)
    logits[:, 1], logits[:, 2], logits[:, 3] = 1.0, 1.1, 0.9
    got = Sampler(backend="fused", penalty_slots=1).sample(
        logits.clone(), [a, b])
    want = Sampler(backend="fused", device_penalties=False).sample(
        logits.clone(), [a, b])
    assert got.tolist() == want.tolist() == [3, 1]


# ---------------------------------------------------------------- engine

PROMPTS = [[5, 3, 8, 1] * 10, [11, 13, 17] * 8]
PENALTIES = dict(repetition_penalty=1.3, presence_penalty=0.5,
                 frequency_penalty=0.2)


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


def generate(eng, sampling):
    ids = [eng.add_request(p, SamplingParams(**sampling)) for p in PROMPTS]
    done = {}
    while eng.has_unfinished():
        for o in eng.step():
            if o.finished:
                done[o.request_id] = o.output_token_ids
    return [done[i] for i in ids]


def test_engine_keeps_penalised_sequences_on_the_chain():
    sampling = dict(max_tokens=12, **PENALTIES)
    eng = make_engine()
    assert eng._async_decode
    first = generate(eng, sampling)
    assert eng.num_async_steps > 0
    table = eng.sampler.penalty_table
    assert table.counts.shape[0] == 64
    # every slot came back
    assert not table._slot_of and len(table._free) == 64

    host = make_engine(device_penalties=False)
    assert host.sampler.penalty_table is None
    assert generate(host, sampling) == first
    assert host.num_async_steps == 0

    one = make_engine(penalty_slots=1)
    assert generate(one, sampling) == first


def test_stop_token_inside_the_chain_returns_the_slot():
    """A sequence that ends on a stop token while pipelined is still in
    the batch of the step already launched; sampling that step must not
    give it a slot again."""
    free_run = generate(make_engine(), dict(max_tokens=12, **PENALTIES))
    # the first token at position >= 3 of the first sequence that it has
    # not emitted before: stopping on it ends the sequence mid-chain
    first = free_run[0]
    pos = next(i for i in range(3, 12) if first[i] not in first[:i])
    sampling = dict(max_tokens=12, ignore_eos=False,
                    stop_token_ids=[first[pos]], **PENALTIES)

    eng = make_engine()
    table = eng.sampler.penalty_table
    host = make_engine(device_penalties=False)
    for _ in range(3):
        before = eng.num_async_steps
        rebuilds = table.num_rebuilds
        tokens = generate(eng, sampling)
        assert tokens[0] == first[:pos + 1]
        assert tokens == generate(host, sampling)
        assert eng.num_async_steps > before
        # one build per sequence, none for the one that had finished
        assert table.num_rebuilds - rebuilds == 2
        assert not table._slot_of and len(table._free) == 64


def test_finished_sequence_gets_no_slot():
    from fusioninfer_amd.engine.sequence import SeqStatus

    sampler = Sampler(backend="fused", penalty_slots=2)
    table = sampler.penalty_table
    a, b = _pen_seq("a", [1, 1, 2]), _pen_seq("b", [2, 2, 3])
    b.status = SeqStatus.FINISHED
    assert table.sync([a, b], V_TABLE) == [0, -1]
    assert table.slot_of(b) == -1 and table.num_rebuilds == 1
    sampler.sample(torch.zeros(2, V_TABLE), [a, b])
    assert table.slot_of(b) == -1 and len(table._free) == 1


def test_out_of_slots_is_not_pipeline_eligible():
    eng = make_engine(penalty_slots=1)
    a = Sequence("a", PROMPTS[0], SamplingParams(**PENALTIES))
    b = Sequence("b", PROMPTS[1], SamplingParams(**PENALTIES))
    plain = Sequence("p", PROMPTS[1], SamplingParams())
    table = eng.sampler.penalty_table
    # the checks take nothing: one slot is free for either, not for both
    assert eng._seq_async_ok(a) and eng._seq_async_ok(b)
    assert eng.sampler.penalty_slots_cover([a, plain])
    assert not eng.sampler.penalty_slots_cover([a, b, plain])
    assert not table._slot_of and len(table._free) == 1
    assert table.sync([a, b, plain], 64) == [0, -1, -1]
    assert eng._seq_async_ok(a)
    assert not eng._seq_async_ok(b)
    assert eng._seq_async_ok(plain)
    assert eng.sampler.penalty_slots_cover([a, plain])
    assert not eng.sampler.penalty_slots_cover([a, b])
    # other chain breakers stay
    biased = Sequence("c", PROMPTS[0], SamplingParams(logit_bias={1: 2.0}))
    assert not eng._seq_async_ok(biased)
    # the torch backend and the switch keep penalties off the chain
    assert not make_engine(device_penalties=False)._seq_async_ok(a)


def test_no_penalised_sequence_allocates_and_launches_nothing(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("penalty op launched")

    monkeypatch.setattr(ops, "apply_penalties", boom)
    monkeypatch.setattr(ops, "penalty_counts_add", boom)
    eng = make_engine()
    generate(eng, dict(max_tokens=6))
    generate(eng, dict(max_tokens=6, temperature=0.8, seed=5))
    assert eng.sampler.penalty_table.counts is None
    assert eng.sampler.penalty_table.num_rebuilds == 0


def test_config_defaults_and_cli_flags():
    from fusioninfer_amd.server.__main__ import (
        build_engine_config, parse_args,
    )

    cfg = EngineConfig()
    assert cfg.penalty_slots == 64 and cfg.device_penalties is True
    cfg = build_engine_config(parse_args(["--model", "Qwen3-0.6B"]))
    assert cfg.penalty_slots == 64 and cfg.device_penalties is True
    cfg = build_engine_config(parse_args(
        ["--model", "Qwen3-0.6B", "--penalty-slots", "8",
         "--no-device-penalties"]))
    assert cfg.penalty_slots == 8 and cfg.device_penalties is False
    # torch backend: no table whatever the switch says
    assert Sampler(backend="torch").penalty_table is None
