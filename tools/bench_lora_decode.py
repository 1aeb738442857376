"""Decode step time with live LoRA adapters (run on a GPU box).

Usage: python tools/bench_lora_decode.py MODE [--model Qwen3-8B]
           [--batch 64] [--adapters 4] [--rank 16] [--steps 40]

MODE  slots-graph  enable_lora, hipGraph-replayed LoRA decode
      slots-eager  enable_lora, enforce_eager (slot kernels, no graphs)
      loop-eager   enable_lora off: per-adapter torch loop, eager decode
                   (the only LoRA decode path without enable_lora)
      base-graph   no adapter rows at all (graph-replayed base decode)

Sequence i of the batch uses adapter i % (adapters + 1); the last residue
is a base row, so the batch mixes base and adapter requests. Times
runner.execute_decode (host batch preparation + forward + logits) with a
device synchronise per step and prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.block_manager import BlockManager
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sequence import SamplingParams, Sequence
from fusioninfer_amd.models.registry import get_model_config


def main():
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=["slots-graph", "slots-eager",
                                    "loop-eager", "base-graph"])
    p.add_argument("--model", default="Qwen3-8B")
    p.add_argument("--layers", type=int, default=0, help="truncate (0=all)")
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--adapters", type=int, default=4)
    p.add_argument("--rank", type=int, default=16)
    p.add_argument("--prompt-len", type=int, default=128)
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=8)
    args = p.parse_args()

    mc = get_model_config(args.model)
    if args.layers:
        mc.num_layers = args.layers
    slots = args.mode.startswith("slots")
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=4096),
        scheduler=SchedulerConfig(
            max_num_seqs=args.batch, max_num_batched_tokens=8192,
            max_model_len=512,
        ),
        enforce_eager=args.mode.endswith("eager"),
        enable_lora=slots,
        max_loras=max(args.adapters, 1),
        max_lora_rank=max(args.rank, 16),
    )
    eng = LLMEngine(cfg, device="cuda:0")
    use_lora = args.mode != "base-graph"
    if use_lora:
        for a in range(args.adapters):
            eng.add_lora(f"ad{a}", rank=args.rank, seed=100 + a)
    runner = eng.runner
    bm = BlockManager(runner.num_gpu_blocks, cfg.cache.block_size)
    seqs = []
    for i in range(args.batch):
        s = Sequence(f"s{i}", [(7 * i + j) % 1000 + 5
                               for j in range(args.prompt_len)],
                     SamplingParams())
        a = i % (args.adapters + 1)
        s.lora_name = f"ad{a}" if use_lora and a < args.adapters else None
        bm.allocate(s)
        seqs.append(s)
    for i in range(0, args.batch, 16):
        runner.execute_prefill(seqs[i:i + 16], bm)
    for s in seqs:
        s.output_token_ids = [11]
        bm.append_slot(s)

    times = []
    for step in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.execute_decode(seqs, bm)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if step >= args.warmup:
            times.append(dt)
        for s in seqs:  # teacher-forced: the cost does not depend on tokens
            s.output_token_ids.append(11)
            bm.append_slot(s)
    print(json.dumps({
        "mode": args.mode, "model": args.model, "layers": mc.num_layers,
        "batch": args.batch, "adapters": args.adapters if use_lora else 0,
        "rank": args.rank, "steps": len(times),
        "step_ms_median": round(statistics.median(times) * 1e3, 3),
        "step_ms_min": round(min(times) * 1e3, 3),
        "step_ms_max": round(max(times) * 1e3, 3),
        "lora_graph_replays": runner.num_lora_graph_replays,
        "lora_eager_steps": runner.num_lora_eager_steps,
    }))


if __name__ == "__main__":
    main()
