"""enable_lora on the GPU engine: slot kernels vs the per-adapter torch
path, hipGraph-replayed LoRA decode, and adapter hot swap under captured
graphs (Qwen3-0.6B truncated to 4 layers, as in test_engine_gpu)."""

import pytest
import torch

from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.block_manager import BlockManager
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sequence import SamplingParams, Sequence
from fusioninfer_amd.models.registry import get_model_config

pytestmark = pytest.mark.gpu

PROMPTS = [list(range(50, 120)), [11, 13, 17] * 20]


def make_engine(enable_lora, enforce_eager, max_seqs=16):
    mc = get_model_config("Qwen3-0.6B")
    mc.num_layers = 4
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=512),
        scheduler=SchedulerConfig(
            max_num_seqs=max_seqs, max_num_batched_tokens=2048,
            max_model_len=512,
        ),
        seed=7,
        enforce_eager=enforce_eager,
        enable_lora=enable_lora,
        max_loras=4,
        max_lora_rank=16,
    )
    return LLMEngine(cfg, device="cuda:0")


def run_requests(eng, reqs, max_tokens=8):
    """reqs: [(prompt, lora_name)] batched together -> token lists."""
    ids = [
        eng.add_request(p, SamplingParams(max_tokens=max_tokens), lora_name=n)
        for p, n in reqs
    ]
    done = {}
    while eng.has_unfinished():
        for o in eng.step():
            if o.finished:
                done[o.request_id] = o.output_token_ids
    return [done[i] for i in ids]


def test_slot_path_logits_match_torch_path():
    """Teacher-forced decode logits of an adapter request: slot kernels
    (enable_lora) vs the per-adapter torch loop."""

    def decode_logits(enable_lora):
        torch.manual_seed(0)
        eng = make_engine(enable_lora, True)
        eng.add_lora("tuned", rank=8, seed=42)
        runner = eng.runner
        bm = BlockManager(runner.num_gpu_blocks, eng.cfg.cache.block_size)
        seq = Sequence("s", list(range(10, 150)), SamplingParams())
        seq.lora_name = "tuned"
        bm.allocate(seq)
        runner.execute_prefill([seq], bm)
        seq.output_token_ids = [321]  # forced: same context in both runs
        bm.append_slot(seq)
        logits = runner.execute_decode([seq], bm).float().cpu()
        return logits, runner

    l_slot, r_slot = decode_logits(True)
    l_loop, r_loop = decode_logits(False)
    assert r_slot.num_lora_slot_steps == 2 and r_slot.num_lora_loop_steps == 0
    assert r_loop.num_lora_slot_steps == 0 and r_loop.num_lora_loop_steps == 2
    rel = ((l_slot - l_loop).norm() / l_loop.norm()).item()
    print(f"slot vs torch path decode logits: rel L2 {rel:.4g}")
    assert rel < 0.05, rel


def test_lora_graph_replay_matches_eager():
    torch.manual_seed(0)
    reqs = [(PROMPTS[0], None), (PROMPTS[1], "tuned")]
    eager = make_engine(True, True)
    eager.add_lora("tuned", rank=8, seed=42)
    exp = run_requests(eager, reqs)
    assert eager.runner.num_lora_graph_replays == 0
    assert eager.runner.num_lora_eager_steps > 0

    graphed = make_engine(True, False)
    graphed.add_lora("tuned", rank=8, seed=42)
    got = run_requests(graphed, reqs)
    assert got == exp
    r = graphed.runner
    assert r.num_lora_graph_replays > 0 and r.num_lora_eager_steps == 0

    # base-only batches keep replaying the base graphs
    replays = r.num_lora_graph_replays
    base = run_requests(graphed, [(PROMPTS[0], None), (PROMPTS[1], None)])
    assert r.num_lora_graph_replays == replays
    assert base[0] == got[0]       # base request unchanged by its batch mate
    assert base[1] != got[1]       # the adapter moved its own request


def test_hot_swap_under_captured_graphs():
    """Adapter "a" generates, is removed, "b" lands in the freed slot: the
    captured graphs must serve b's weights. The two requests use different
    prompts: the prefix cache keys blocks on token ids alone, so a shared
    prompt would hand b the KV blocks written under a."""
    torch.manual_seed(0)
    eng = make_engine(True, False)
    eng.add_lora("a", rank=8, seed=1)
    slot = eng.runner.lora_registry.slot_of("a")
    run_requests(eng, [(PROMPTS[0], "a")])
    replays = eng.runner.num_lora_graph_replays
    assert replays > 0
    assert eng.remove_lora("a")
    eng.add_lora("b", rank=8, seed=2)
    assert eng.runner.lora_registry.slot_of("b") == slot
    out_b = run_requests(eng, [(PROMPTS[1], "b")])
    assert eng.runner.num_lora_graph_replays > replays

    fresh = make_engine(True, True)
    fresh.add_lora("b", rank=8, seed=2)
    exp_b = run_requests(fresh, [(PROMPTS[1], "b")])
    assert out_b == exp_b
    # and "a" in that slot would have answered differently
    stale = make_engine(True, True)
    stale.add_lora("b", rank=8, seed=1)
    assert run_requests(stale, [(PROMPTS[1], "b")]) != exp_b
