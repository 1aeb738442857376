"""Batched multi-LoRA slot path on the CPU reference: ops.lora_apply,
the LoRASlots table, slot ownership in LoRARegistry and the enable_lora
engine wiring (tiny model)."""

import math

import pytest
import torch

import fusioninfer_amd.ops as ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sequence import SamplingParams
from fusioninfer_amd.lora import LoRAAdapter, LoRABatch, LoRARegistry, LoRASlots
from fusioninfer_amd.models.registry import get_model_config
from fusioninfer_amd.ops import reference as ref

PROMPT = [5, 3, 8, 1] * 10
ATOL = RTOL = 2e-2  # the project's bf16 tolerance (test_ops_gpu)


def make_engine(enable_lora, max_lora_rank=16, max_loras=8, seed=0):
    cfg = EngineConfig(
        model=get_model_config("tiny-qwen3"),
        cache=CacheConfig(num_gpu_blocks=256),
        scheduler=SchedulerConfig(
            max_num_seqs=8, max_num_batched_tokens=1024, max_model_len=256
        ),
        seed=seed,
        enable_lora=enable_lora,
        max_lora_rank=max_lora_rank,
        max_loras=max_loras,
    )
    return LLMEngine(cfg, device="cpu")


def make_stacks(S, K, N, R, ranks, seed=0):
    """A std 1/sqrt(K), B std 1/sqrt(R), scales in [0.5, 2]; rows/columns
    beyond each slot's rank are zero."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(S, R, K, generator=g) / math.sqrt(K)
    b = torch.randn(S, N, R, generator=g) / math.sqrt(R)
    for s, r in enumerate(ranks):
        a[s, r:] = 0
        b[s, :, r:] = 0
    scales = 0.5 + 1.5 * torch.rand(S, generator=g)
    return a.bfloat16(), b.bfloat16(), scales.float()


def test_ref_lora_apply_matches_per_adapter_loop():
    T, K, N, R, S = 37, 128, 96, 16, 3
    ranks = [4, 8, 16]
    a, b, scales = make_stacks(S, K, N, R, ranks)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(T, K, generator=g).bfloat16()
    out0 = torch.randn(T, N, generator=g).bfloat16()
    ids = torch.randint(-1, S, (T,), generator=g, dtype=torch.int32)
    assert (ids == -1).any() and all((ids == s).any() for s in range(S))

    got = ops.lora_apply(out0.clone(), x, ids, a, b, scales)

    groups = []
    for s in range(S):
        ad = LoRAAdapter.__new__(LoRAAdapter)
        ad.name, ad.rank, ad.scaling = f"a{s}", ranks[s], float(scales[s])
        ad.weights = [{"qkv": (a[s, : ranks[s]], b[s, :, : ranks[s]])}]
        groups.append((ad, (ids == s).nonzero().flatten()))
    exp = out0.clone()
    LoRABatch(groups).apply(0, "qkv", x, exp)

    torch.testing.assert_close(got.float(), exp.float(), atol=ATOL, rtol=RTOL)
    base = ids == -1
    assert torch.equal(got[base], out0[base])
    assert not torch.equal(got[~base], out0[~base])


def test_ref_out_of_range_ids_leave_rows_bit_identical():
    T, K, N, R, S = 9, 64, 32, 16, 2
    a, b, scales = make_stacks(S, K, N, R, [16, 16])
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T, K, generator=g).bfloat16()
    out0 = torch.randn(T, N, generator=g).bfloat16()
    ids = torch.tensor([0, -1, S, 1, -1, S, 0, S + 5, -7], dtype=torch.int32)
    got = ref.lora_apply(out0.clone(), x, ids, a, b, scales)
    untouched = (ids < 0) | (ids >= S)
    assert torch.equal(got[untouched].view(torch.int16),
                       out0[untouched].view(torch.int16))
    assert not torch.equal(got[~untouched], out0[~untouched])


@pytest.mark.parametrize("K,N,R", [(96, 32, 16), (64, 24, 16), (64, 32, 8),
                                   (64, 32, 144)])
def test_lora_apply_rejects_unsupported_shapes(K, N, R):
    S, T = 2, 3
    with pytest.raises(ValueError):
        ops.lora_apply(
            torch.zeros(T, N, dtype=torch.bfloat16),
            torch.zeros(T, K, dtype=torch.bfloat16),
            torch.zeros(T, dtype=torch.int32),
            torch.zeros(S, R, K, dtype=torch.bfloat16),
            torch.zeros(S, N, R, dtype=torch.bfloat16),
            torch.ones(S),
        )


def test_slot_assignment_eviction_reuse_and_zero_padding():
    mc = get_model_config("tiny-qwen3")
    slots = LoRASlots(mc, max_loras=2, max_lora_rank=10)
    assert slots.rank == 16 and slots.usable  # rounded up to 16
    reg = LoRARegistry(max_loras=2, max_cpu_loras=4, slots=slots)
    addrs = [t.data_ptr() for layer in slots.layers
             for ts in layer.values() for t in ts]

    a = LoRAAdapter("a", 4, 8.0, mc, seed=1)
    b = LoRAAdapter("b", 4, 8.0, mc, seed=2)
    c = LoRAAdapter("c", 4, 8.0, mc, seed=3)
    reg.add(a)
    reg.add(b)
    assert sorted((reg.slot_of("a"), reg.slot_of("b"))) == [0, 1]

    # rank-4 adapter in an R=16 table: copied rows, zero padding beyond
    sa = reg.slot_of("a")
    for li in (0, mc.num_layers - 1):
        for tgt, (a_stack, b_stack, scales) in slots.layers[li].items():
            A, B = a.weights[li][tgt]
            assert torch.equal(a_stack[sa, :4], A)
            assert torch.equal(b_stack[sa, :, :4], B)
            assert not a_stack[sa, 4:].any() and not b_stack[sa, :, 4:].any()
            assert float(scales[sa]) == a.scaling

    # LRU eviction ("a" is the oldest) frees its slot; "c" reuses it with
    # different contents
    reg.add(c)
    assert reg.slot_of("a") is None and reg.num_resident() == 2
    assert reg.slot_of("c") == sa and slots.owner(sa) == "c"
    a_stack, b_stack, scales = slots.layers[0]["qkv"]
    assert torch.equal(a_stack[sa, :4], c.weights[0]["qkv"][0])
    assert not torch.equal(a_stack[sa, :4], a.weights[0]["qkv"][0])

    # paging "a" back in evicts the LRU ("b") and takes b's slot
    sb = reg.slot_of("b")
    reg.get("a")
    assert reg.slot_of("b") is None and reg.slot_of("a") == sb

    # remove frees the slot: scales zeroed, next add lands there
    assert reg.remove("c")
    assert slots.owner(sa) is None
    assert all(float(ts[2][sa]) == 0.0
               for layer in slots.layers for ts in layer.values())
    reg.add(LoRAAdapter("d", 8, 8.0, mc, seed=4))
    assert reg.slot_of("d") == sa

    # the stacks were never reallocated
    assert addrs == [t.data_ptr() for layer in slots.layers
                     for ts in layer.values() for t in ts]


def test_oversize_rank_stays_resident_without_slot():
    mc = get_model_config("tiny-qwen3")
    slots = LoRASlots(mc, max_loras=2, max_lora_rank=16)
    reg = LoRARegistry(max_loras=2, max_cpu_loras=4, slots=slots)
    reg.add(LoRAAdapter("big", 32, 8.0, mc, seed=1))
    assert reg.num_resident() == 1 and reg.slot_of("big") is None
    with pytest.raises(ValueError):
        LoRASlots(mc, max_loras=2, max_lora_rank=256)


def _run_mixed(eng):
    """tests/test_lora.py's scenario: a solo base run, then a base and an
    adapter request batched together."""
    eng.add_lora("tuned", rank=8, seed=42)
    base = eng.generate([PROMPT], SamplingParams(max_tokens=6))[0]
    r_base = eng.add_request(PROMPT, SamplingParams(max_tokens=6))
    r_lora = eng.add_request(PROMPT, SamplingParams(max_tokens=6),
                             lora_name="tuned")
    outs = {}
    while eng.has_unfinished():
        for o in eng.step():
            if o.finished:
                outs[o.request_id] = o
    return (base.output_token_ids, outs[r_base].output_token_ids,
            outs[r_lora].output_token_ids)


def test_engine_enable_lora_matches_torch_path():
    torch.manual_seed(0)
    solo0, base0, lora0 = _run_mixed(make_engine(False))
    torch.manual_seed(0)
    eng = make_engine(True)
    solo1, base1, lora1 = _run_mixed(eng)
    r = eng.runner
    assert r.lora_slots is not None and r.num_lora_slot_steps > 0
    assert r.num_lora_loop_steps == 0
    assert base1 == solo1 == solo0 == base0  # base rows untouched
    assert lora1 == lora0
    assert lora1 != base1


def test_engine_oversize_rank_uses_loop_path():
    torch.manual_seed(0)
    eng = make_engine(True, max_lora_rank=16)
    eng.add_lora("big", rank=32, seed=42)
    req = eng.add_request(PROMPT, SamplingParams(max_tokens=4),
                          lora_name="big")
    while eng.has_unfinished():
        eng.step()
    r = eng.runner
    assert req is not None
    assert r.num_lora_loop_steps > 0 and r.num_lora_eager_steps > 0
    assert r.num_lora_slot_steps == 0 and r.num_lora_graph_replays == 0

    # a fitting adapter on the same engine takes the slot path; a step
    # mixing it with the oversize one falls back as a whole
    eng.add_lora("small", rank=8, seed=7)
    eng.add_request(PROMPT, SamplingParams(max_tokens=3), lora_name="small")
    while eng.has_unfinished():
        eng.step()
    assert r.num_lora_slot_steps > 0
    loops = r.num_lora_loop_steps
    slot_steps = r.num_lora_slot_steps
    eng.add_request(PROMPT, SamplingParams(max_tokens=3), lora_name="small")
    eng.add_request(PROMPT, SamplingParams(max_tokens=3), lora_name="big")
    while eng.has_unfinished():
        eng.step()
    assert r.num_lora_loop_steps > loops
    assert r.num_lora_slot_steps == slot_steps
