#!/usr/bin/env python3
"""FusionInfer-AMD flagship serving benchmark.

Measures the BASELINE.json metric — goodput (completed requests/s) and p50
TTFT for Qwen3-8B serving on MI355X — on synthetic requests with
random-init weights (no network in this environment; BASELINE.md documents
that the reference publishes no numbers of its own).

One rank per GPU (DP replicas, weak scaling — the reference's `replicas`
orchestration). Each rank runs a closed-loop load: target
concurrency is kept topped up; a bench "step" is one engine iteration
(one continuous-batching scheduler step + forward). Timed region:
barrier + torch.cuda.synchronize on both sides of EXACTLY --steps steps.

Measurement stability (round-2): before the timed window the closed loop
is ramped until every initially-admitted request has completed and been
replaced (full turnover), so the window sees steady-state serving only.
Goodput is reported as (generated tokens / elapsed) / E[tokens per
request]; E[tokens/req] == --gen-len exactly by construction of the load
(gen lengths uniform with mean gen_len), so this equals completed
requests / elapsed in expectation but with far lower variance in short
windows (completions are a count of ~1/step; token throughput is stable
per step). The raw completion count and completions/s are also reported.
TTFT samples come only from requests admitted after the turnover ramp
(steady-state admissions), never from the synchronized initial burst.

A plain run does only what the headline figure needs: engine set-up, the
turnover ramp, --warmup steps, the --steps timed steps, the optional
output dump and the one JSON result line. Everything else this benchmark
may grow (baselines, other precisions or sizes, per-kernel figures) belongs
behind --full, which is off by default; today nothing else is measured, so
--full runs the same thing.

--dump-outputs DIR writes, after the timed steps, what the timed path
handed its caller in the last timed step that delivered tokens, as
DIR/<name>.npy (ranks > 0 append _rank<R> to the name):
  last_step_request_index    [n]     float64, N of request id "req-N"
  last_step_new_token_ids    [n, k]  float64, tokens emitted that step (-1 pad)
  last_step_output_token_ids [n, L]  float64, all tokens so far (-1 pad)
  last_step_finished         [n]     float64, 1.0 where the request finished
  last_logits_request_index  [m]     float64, request of each logits row
  last_logits_sample         [m, C]  float32, the logits of the last
                                     sampling call in the window at a fixed
                                     seeded sample of C <= 4096 vocab columns
Prompts, generation lengths and weights are seeded, and request "req-N"
always carries the N-th generated prompt. The one wall-clock input of the
engine is the scheduler's admission aging window, so with --dump-outputs
(and no explicit --admission-ms) admission is made count-based only: a
held prompt is released by the token threshold or an idle decode set,
never by its age. The schedule, and with it the dumped step, is then the
same from run to run, and two builds can be compared output for output.

Usage:
  python bench.py --gpus 1 --steps 64 --warmup 16
  python bench.py --gpus 1 --steps 64 --warmup 16 --dump-outputs bench_out
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import time

import torch
import torch.distributed as dist


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=64)
    p.add_argument("--warmup", type=int, default=16)
    p.add_argument("--model", type=str, default="Qwen3-8B")
    p.add_argument("--prompt-len", type=int, default=1024)
    p.add_argument("--gen-len", type=int, default=128)
    p.add_argument("--concurrency", type=int, default=256)
    p.add_argument("--max-batched-tokens", type=int, default=8192)
    p.add_argument("--admission-ms", type=float, default=None,
                   help="admission-hysteresis aging window (scheduler "
                        "default when unset)")
    p.add_argument("--enforce-eager", action="store_true")
    p.add_argument("--kv-cache-dtype", choices=["auto", "fp8"], default="auto",
                   help="fp8 = e4m3 KV cache (halves KV bytes)")
    p.add_argument("--quantization", choices=["fp8"], default=None,
                   help="opt-in fp8 serving mode (headline stays bf16)")
    p.add_argument("--tp", type=int, default=1, help="tensor-parallel degree")
    p.add_argument("--shared-prefix-len", type=int, default=0,
                   help="shared-prefix workload (BASELINE config #4): each "
                        "prompt = one of 8 shared prefixes of this length + "
                        "a unique tail; exercises prefix caching")
    p.add_argument("--spec-tokens", type=int, default=0,
                   help="enable ngram speculative decoding with this draft "
                        "length, and make prompts locally repetitive so the "
                        "prompt-lookup proposer has matches (spec-decode "
                        "workload mode; headline stays spec-off)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last timed "
                        "step's outputs as DIR/<name>.npy (see module "
                        "docstring); makes prompt admission count-based "
                        "so the schedule is reproducible")
    p.add_argument("--full", action="store_true",
                   help="also run every secondary measurement or check "
                        "(none today: the plain run is the whole benchmark)")
    return p.parse_args()


class ClosedLoopLoad:
    """Keeps `concurrency` requests in flight; tracks completions + TTFT."""

    def __init__(self, engine, prompt_len: int, gen_len: int, concurrency: int,
                 vocab: int, seed: int, shared_prefix_len: int = 0,
                 repetitive: bool = False):
        self.repetitive = repetitive
        self.engine = engine
        self.gen_len = gen_len
        self.prompt_len = prompt_len
        self.concurrency = concurrency
        self.vocab = vocab
        self.rng = torch.Generator().manual_seed(seed)
        self.completion_times = []
        self.first_token_times = {}
        self.ttfts = []
        self.prefixes = []
        if shared_prefix_len > 0:
            self.prefixes = [
                torch.randint(0, vocab, (shared_prefix_len,),
                              generator=self.rng).tolist()
                for _ in range(8)
            ]

    def _new_prompt(self):
        if self.repetitive:
            # period-P repeated random chunk: summarization/extraction-like
            # texts where ngram prompt-lookup actually lands drafts
            period = 32
            chunk = torch.randint(0, self.vocab, (period,),
                                  generator=self.rng).tolist()
            reps = (self.prompt_len + period - 1) // period
            return (chunk * reps)[: self.prompt_len]
        if self.prefixes:
            i = int(torch.randint(0, len(self.prefixes), (1,),
                                  generator=self.rng))
            tail_len = max(self.prompt_len - len(self.prefixes[i]), 8)
            tail = torch.randint(0, self.vocab, (tail_len,),
                                 generator=self.rng).tolist()
            return self.prefixes[i] + tail
        return torch.randint(
            0, self.vocab, (self.prompt_len,), generator=self.rng
        ).tolist()

    def _new_params(self):
        from fusioninfer_amd.engine.sequence import SamplingParams

        # gen lengths uniform in [gen_len/2, 3*gen_len/2] (mean = gen_len):
        # staggers completions so goodput is measurable in short windows
        lo, hi = max(self.gen_len // 2, 1), self.gen_len + self.gen_len // 2
        n = int(torch.randint(lo, hi + 1, (1,), generator=self.rng))
        return SamplingParams(max_tokens=n, temperature=0.0)

    def top_up(self):
        in_flight = self.engine.num_waiting() + self.engine.num_running()
        for _ in range(self.concurrency - in_flight):
            self.engine.add_request(self._new_prompt(), self._new_params())

    def step(self):
        outs = self.engine.step()
        now = time.monotonic()
        for o in outs:
            if o.finished:
                self.completion_times.append(now)
                if o.ttft is not None:
                    self.ttfts.append(o.ttft)
        self.top_up()


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # Honest n_gpus: --gpus N is a claim that N ranks are running. Refuse
    # to produce a record that says N GPUs while executing on fewer
    # (e.g. `bench.py --gpus 8` launched without torchrun).
    if args.gpus != world:
        raise SystemExit(
            f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}. "
            f"Launch N>1 via: python -m torch.distributed.run --nnodes=1 "
            f"--nproc-per-node {args.gpus} --master-addr 127.0.0.1 "
            f"bench.py --gpus {args.gpus} ..."
        )
    use_cuda = torch.cuda.is_available()
    device = f"cuda:{local_rank}" if use_cuda else "cpu"
    if use_cuda:
        torch.cuda.set_device(local_rank)

    distributed = world > 1
    if distributed:
        dist.init_process_group(backend="nccl" if use_cuda else "gloo")

    from fusioninfer_amd.config import (
        CacheConfig,
        EngineConfig,
        ParallelConfig,
        SchedulerConfig,
    )
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config(args.model)
    mc.quantization = args.quantization
    max_len = args.prompt_len + args.gen_len + 64
    admission_ms = args.admission_ms
    if args.dump_outputs is not None and admission_ms is None:
        # reproducible schedule: no prompt is ever released by wall-clock
        # age (a negative --admission-ms keeps the adaptive window)
        admission_ms = 1e12
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(
            num_gpu_blocks=None if use_cuda else 4096,
            gpu_memory_utilization=0.85,
            kv_cache_dtype=args.kv_cache_dtype,
        ),
        scheduler=SchedulerConfig(
            max_num_seqs=args.concurrency,
            max_num_batched_tokens=args.max_batched_tokens,
            max_model_len=max_len,
            **({"prefill_admission_ms": (
                None if admission_ms < 0 else admission_ms)}
               if admission_ms is not None else {}),
        ),
        parallel=ParallelConfig(
            tensor_parallel_size=args.tp, rank=rank, world_size=world
        ),
        seed=1234 + rank,
        enforce_eager=args.enforce_eager,
    )
    if args.spec_tokens > 0:
        from fusioninfer_amd.engine.spec_decode import SpeculativeConfig

        cfg.speculative = SpeculativeConfig(
            num_speculative_tokens=args.spec_tokens,
            disable_by_batch_size=0,  # the bench measures spec as asked;
                                      # pick the regime via --concurrency
        )
    # TP: ranks form DP groups of size tp; only group leaders drive load.
    driver_group = None
    if distributed and args.tp > 1:
        driver_ranks = list(range(0, world, args.tp))
        driver_group = dist.new_group(driver_ranks)

    engine = LLMEngine(cfg, device=device)

    if args.tp > 1 and not engine.is_driver:
        engine.worker_loop()   # released by stop_workers() after timing
        _aggregate_and_report(args, rank, world, distributed, device,
                              use_cuda, 0.0, 0, 0, [], is_driver=False)
        if distributed:
            dist.destroy_process_group()
        return

    load = ClosedLoopLoad(
        engine, args.prompt_len, args.gen_len, args.concurrency,
        mc.vocab_size, seed=99 + rank,
        shared_prefix_len=args.shared_prefix_len,
        repetitive=args.spec_tokens > 0,
    )
    load.top_up()
    # a plain run executes the untapped engine; the taps only exist when
    # their result is going to be written
    tap = _tap_engine(engine) if args.dump_outputs else None

    def barrier_sync():
        if distributed:
            dist.barrier(group=driver_group)
        if use_cuda:
            torch.cuda.synchronize()

    # Load initialization: ramp the closed loop to FULL TURNOVER — every
    # request of the synchronized initial burst has completed and been
    # replaced by steady-state admissions — so the timed window measures
    # steady-state serving for ANY --steps/--warmup. Bounded.
    ramp_limit = 10 * (args.prompt_len // 64 + 2 * args.gen_len) + 800
    ramp_target = args.concurrency + max(args.concurrency // 4, 4)
    ramp = 0
    while len(load.completion_times) < ramp_target and ramp < ramp_limit:
        load.step()
        ramp += 1
    # TTFT samples before this mark belong to (or overlap) the initial
    # burst; only steady-state admissions count from here on.
    steady_ttft_mark = len(load.ttfts)

    for _ in range(args.warmup):
        load.step()

    barrier_sync()
    t0 = time.monotonic()
    completed_before = len(load.completion_times)
    tokens_before = engine.num_generated_tokens
    ttft_mark = len(load.ttfts)
    if tap is not None:
        tap["outs"] = []
    for _ in range(args.steps):
        load.step()
    barrier_sync()
    elapsed = time.monotonic() - t0

    completed = len(load.completion_times) - completed_before
    gen_tokens = engine.num_generated_tokens - tokens_before
    # Prefer window-local TTFTs; with too few samples (short windows),
    # widen to all steady-state samples — never to the initial burst.
    ttfts = load.ttfts[ttft_mark:]
    if len(ttfts) < 16:
        ttfts = load.ttfts[steady_ttft_mark:]

    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, rank, tap)

    engine.stop_workers()
    spec_stats = None
    if args.spec_tokens > 0 and engine.num_spec_draft_tokens:
        spec_stats = {
            "draft_tokens": engine.num_spec_draft_tokens,
            "accepted_tokens": engine.num_spec_accepted_tokens,
            "accept_rate": round(
                engine.num_spec_accepted_tokens
                / max(engine.num_spec_draft_tokens, 1), 3
            ),
        }
    _aggregate_and_report(args, rank, world, distributed, device, use_cuda,
                          elapsed, completed, gen_tokens, ttfts,
                          is_driver=True, spec_stats=spec_stats)
    if distributed:
        dist.destroy_process_group()


def _tap_engine(engine):
    """Keep references to what the engine last handed its caller: the
    outputs of the most recent step() that delivered any, and the logits
    (with their row -> request map) of the most recent sampling call. No
    copy, no sync: each tap costs the timed path one Python call per step."""
    tap = {"outs": [], "logits": None, "req": None}
    step = engine.step
    sample = engine.sampler.sample

    def tapped_step():
        outs = step()
        if outs:
            tap["outs"] = outs
        return outs

    def tapped(logits, seqs):
        tap["logits"] = logits
        tap["req"] = [s.seq_id for s in seqs]
        return sample(logits, seqs)

    engine.step = tapped_step
    engine.sampler.sample = tapped
    return tap


def _req_index(request_id) -> float:
    return float(str(request_id).rsplit("-", 1)[-1])


def _dump_outputs(out_dir, rank, tap, max_cols=4096):
    import numpy as np

    outs = tap["outs"]

    os.makedirs(out_dir, exist_ok=True)
    suffix = f"_rank{rank}" if rank else ""

    def save(name, arr):
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), arr)

    def padded(rows):
        width = max((len(r) for r in rows), default=0)
        arr = np.full((len(rows), width), -1.0, dtype=np.float64)
        for i, r in enumerate(rows):
            arr[i, :len(r)] = r
        return arr

    save("last_step_request_index",
         np.array([_req_index(o.request_id) for o in outs], dtype=np.float64))
    save("last_step_new_token_ids", padded([o.new_token_ids for o in outs]))
    save("last_step_output_token_ids",
         padded([o.output_token_ids for o in outs]))
    save("last_step_finished",
         np.array([float(o.finished) for o in outs], dtype=np.float64))
    if tap["logits"] is not None:
        logits = tap["logits"]
        vocab = logits.shape[-1]
        cols = torch.randperm(
            vocab, generator=torch.Generator().manual_seed(4242)
        )[:max_cols].sort().values
        sample = logits.index_select(-1, cols.to(logits.device))
        save("last_logits_request_index",
             np.array([_req_index(r) for r in tap["req"]], dtype=np.float64))
        save("last_logits_sample", sample.float().cpu().numpy())


def _aggregate_and_report(args, rank, world, distributed, device, use_cuda,
                          elapsed, completed, gen_tokens, ttfts, is_driver,
                          spec_stats=None):
    if distributed:
        dev = device if use_cuda else "cpu"
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        c = torch.tensor([completed, gen_tokens], dtype=torch.float64,
                         device=dev)
        dist.all_reduce(c)
        completed, gen_tokens = float(c[0].item()), float(c[1].item())
        all_ttfts = [None] * world
        dist.all_gather_object(all_ttfts, ttfts)
        ttfts = [x for lst in all_ttfts for x in lst]

    if rank != 0:
        return
    # Low-variance goodput estimator: token throughput / E[tokens per
    # request]; E[tokens/req] == gen_len exactly by construction of the
    # load, so this equals completions/elapsed in expectation (see module
    # docstring). Raw completions/s reported alongside.
    goodput = (
        (gen_tokens / elapsed) / args.gen_len if elapsed > 0 else 0.0
    )
    completed_per_s = completed / elapsed if elapsed > 0 else 0.0
    p50_ttft_ms = (
        statistics.median(ttfts) * 1000.0 if ttfts else float("nan")
    )
    dp = (world // args.tp) if distributed else args.gpus
    result = {
        "metric": f"goodput req/s ({args.model} serving, closed-loop)",
        "value": round(goodput, 3),
        "unit": "req/s",
        "n_gpus": world if distributed else args.gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / max(args.steps, 1) * 1000.0, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": (args.quantization or "bf16")
        + ("+kv_fp8" if args.kv_cache_dtype == "fp8" else ""),
        "data": "synthetic",
        "p50_ttft_ms": round(p50_ttft_ms, 1),
        "completed_requests": int(completed),
        "completed_req_per_s": round(completed_per_s, 3),
        **({"spec_decode": spec_stats} if spec_stats else {}),
        "tokens_per_s": round(gen_tokens / elapsed, 1) if elapsed else 0.0,
        "config": {
            "model": args.model,
            "global_batch": args.concurrency * dp,
            "seq_len": args.prompt_len + args.gen_len,
            "prompt_len": args.prompt_len,
            "gen_len": args.gen_len,
            "parallelism": f"dp{dp}"
            + (f"-tp{args.tp}" if args.tp > 1 else ""),
        },
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
