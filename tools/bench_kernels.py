"""Microbenchmarks for the FusionInfer-AMD HIP kernels (run on a GPU box).

Usage: python tools/bench_kernels.py
           [prefill|decode|elementwise|lora|sampling|sampling_e2e|penalties|
            penalties_e2e|logprobs|logprobs_e2e|spec_verify|
            spec_sampled_e2e|logit_mods|guided_spec_e2e|bias_pipelining|all]
Prints per-shape timing + achieved TFLOP/s (attention) or GB/s (memory ops).
"""

import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import fusioninfer_amd.ops as ops


def timeit(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_prefill():
    """Dense and paged prefill at the Qwen3-8B head counts, both schedules
    from one process: `off` is the ascending tile table on the (tile, head)
    grid (what FI_PF_TILE_ORDER=0 selects), `on` the heaviest-first table
    with the heads of a tile adjacent. The module flag is flipped between
    calls; tables are prebuilt, tile_rows as the engine picks them
    (ops.prefill_tile_rows). Device-event time per call, median of 3
    alternating rounds x 20 calls after a warm-up of each. The paged rows
    read a bf16 cache with shuffled block ids and no cached prefix, the
    benchmark's prefill step."""
    print("== prefill attention (varlen causal, GQA 32/8, D=128) ==")
    print("| kind | shape | tile_rows | off us | off TF/s | on us | on TF/s "
          "| off/on |")
    print("|---|---|---|---|---|---|---|---|")
    Hq, Hk, D, bs = 32, 8, 128, 16
    scale = 1.0 / math.sqrt(D)
    shapes = [("dense", 1, 1024), ("dense", 8, 1024), ("dense", 4, 2048),
              ("dense", 1, 8192), ("dense", 16, 512), ("paged", 8, 1024),
              ("paged", 1, 8192)]
    for kind, nseq, L in shapes:
        T = nseq * L
        q = torch.randn(T, Hq, D, dtype=torch.bfloat16, device="cuda")
        cu = torch.arange(0, nseq + 1, dtype=torch.int32, device="cuda") * L
        lens = [L] * nseq
        rows = ops.prefill_tile_rows(lens)
        tables = {
            on: ops.build_prefill_tiles(lens, device="cuda", rows=rows,
                                        heaviest_first=on)
            for on in (False, True)
        }
        if kind == "dense":
            k = torch.randn(T, Hk, D, dtype=torch.bfloat16, device="cuda")
            v = torch.randn_like(k)

            def call(on):
                ts, tr = tables[on]
                return ops.prefill_attention(q, k, v, cu, scale, ts, tr, rows)
        else:
            nblk = L // bs
            kc = torch.randn(nseq * nblk + 1, Hk, bs, D,
                             dtype=torch.bfloat16, device="cuda")
            vc = torch.randn_like(kc)
            bt = (1 + torch.randperm(nseq * nblk, device="cuda")).int()
            bt = bt.view(nseq, nblk).contiguous()
            slk = torch.full((nseq,), L, dtype=torch.int32, device="cuda")
            out = torch.empty_like(q)

            def call(on):
                ts, tr = tables[on]
                return ops.prefill_attention_paged(
                    q, kc, vc, bt, cu, slk, scale, ts, tr, rows, out=out)

        def run(on):
            ops.PF_TILE_ORDER = on  # selects the dispatch map per call
            return call(on)

        default = ops.PF_TILE_ORDER
        try:
            first = run(False).clone()  # the paged calls share `out`
            same = torch.equal(first, run(True))
            times = {False: [], True: []}
            for on in times:
                for _ in range(5):
                    run(on)
            torch.cuda.synchronize()
            for _ in range(3):
                for on in times:
                    times[on] += _event_times_us(lambda: run(on), 20)
        finally:
            ops.PF_TILE_ORDER = default
        assert same, "the two schedules must give the same bits"
        # causal flops: 2 matmuls * L*(L+1)/2 * D * 2 per head
        flops = nseq * Hq * 2 * (L * (L + 1) / 2) * D * 2
        off, on = _median(times[False]), _median(times[True])
        print(f"| {kind} | {nseq}x{L} | {rows} | {off:.1f} | "
              f"{flops / off / 1e6:.0f} | {on:.1f} | {flops / on / 1e6:.0f} "
              f"| {off / on:.2f}x |", flush=True)


def bench_decode(group=4):
    Hq, Hk = 32, 32 // group
    print(f"== paged decode attention (GQA 32/{Hk}, G={group}, D=128, bs=16) ==")
    for batch, ctx in [(1, 1024), (8, 1024), (64, 1024), (256, 1024),
                       (64, 4096), (256, 2048), (8, 8192)]:
        D, bs = 128, 16
        nblk = (ctx + bs - 1) // bs
        total_blocks = batch * nblk + 1
        q = torch.randn(batch, Hq, D, dtype=torch.bfloat16, device="cuda")
        k_cache = torch.randn(total_blocks, Hk, bs, D, dtype=torch.bfloat16,
                              device="cuda")
        v_cache = torch.randn_like(k_cache)
        bt = torch.arange(1, total_blocks, dtype=torch.int32, device="cuda")
        bt = bt.view(batch, nblk)
        lens = torch.full((batch,), ctx, dtype=torch.int32, device="cuda")
        t = timeit(lambda: ops.paged_attention_decode(q, k_cache, v_cache, bt, lens))
        gb = batch * ctx * Hk * D * 2 * 2 / 1e9  # K+V bytes actually needed
        k8 = k_cache.to(torch.float8_e4m3fn)
        v8 = v_cache.to(torch.float8_e4m3fn)
        t8 = timeit(lambda: ops.paged_attention_decode(q, k8, v8, bt, lens))
        print(f"  b{batch} ctx{ctx}: {t*1e6:8.1f} us  {gb/t:7.0f} GB/s (KV) | "
              f"fp8kv {t8*1e6:8.1f} us  {gb/2/t8:7.0f} GB/s")


def bench_elementwise():
    print("== rmsnorm / silu_mul / rope (bf16) ==")
    for T in [64, 256, 2048, 8192]:
        H = 4096
        x = torch.randn(T, H, dtype=torch.bfloat16, device="cuda")
        r = torch.randn_like(x)
        w = torch.randn(H, dtype=torch.bfloat16, device="cuda")
        t = timeit(lambda: ops.fused_add_rms_norm(x, r, w, 1e-6))
        gb = T * H * 2 * 4 / 1e9  # r x read, write x2
        print(f"  fused_add_rms_norm T={T}: {t*1e6:7.1f} us {gb/t:6.0f} GB/s")
        y = torch.randn(T, 24576, dtype=torch.bfloat16, device="cuda")
        t = timeit(lambda: ops.silu_and_mul(y))
        gb = T * 24576 * 2 * 1.5 / 1e9
        print(f"  silu_and_mul T={T}:       {t*1e6:7.1f} us {gb/t:6.0f} GB/s")
        _bench_rope_cache(T)


def _bench_rope_cache(T):
    """qk-norm + RoPE + KV-cache write at the Qwen3-8B shape (Hq 32, Hk 8,
    D 128, qkv row stride 6144, bf16 cache): the two-kernel path
    (rope_qk_norm_ + reshape_and_cache) and the fused rope_qk_norm_cache_
    on the same buffers, alternating, best of three rounds. GB/s is over
    the bytes the result needs, for both: q and k read, q written, v read,
    both cache rows written (the pair moves more: it writes k back and
    reads it again)."""
    Hq, Hk, D, bs = 32, 8, 128, 16
    qkv = torch.randn(T, (Hq + 2 * Hk) * D, dtype=torch.bfloat16,
                      device="cuda")
    q = qkv[:, : Hq * D]
    k = qkv[:, Hq * D : (Hq + Hk) * D]
    v = qkv[:, (Hq + Hk) * D :]
    qw = torch.randn(D, dtype=torch.bfloat16, device="cuda")
    kw = torch.randn(D, dtype=torch.bfloat16, device="cuda")
    pos = torch.arange(T, dtype=torch.int32, device="cuda") % 1152
    cos_sin = ops.compute_cos_sin_cache(D, 1152, 1e6).to("cuda")
    nblocks = (T + bs - 1) // bs
    k_cache = torch.zeros(nblocks, Hk, bs, D, dtype=torch.bfloat16,
                          device="cuda")
    v_cache = torch.zeros_like(k_cache)
    slots = torch.randperm(nblocks * bs, device="cuda")[:T].int()

    def pair():
        ops.rope_qk_norm_(q, k, pos, cos_sin, Hq, Hk, D, qw, kw, 1e-6)
        ops.reshape_and_cache(k, v, k_cache, v_cache, slots)

    def fused():
        ops.rope_qk_norm_cache_(q, k, v, pos, cos_sin, Hq, Hk, D, k_cache,
                                v_cache, slots, qw, kw, 1e-6)

    def rope_only():
        ops.rope_qk_norm_(q, k, pos, cos_sin, Hq, Hk, D, qw, kw, 1e-6)

    tp = tf = tr = float("inf")
    for _ in range(3):
        tp = min(tp, timeit(pair, iters=50))
        tf = min(tf, timeit(fused, iters=50))
        tr = min(tr, timeit(rope_only, iters=50))
        # q is renormalised in place every call; keep it O(1)
        qkv.normal_()
    gb = T * D * 2 * (2 * Hq + 4 * Hk) / 1e9
    print(f"  rope+cache pair T={T}:    {tp*1e6:7.1f} us {gb/tp:6.0f} GB/s"
          f"  (rope_qk_norm_ alone {tr*1e6:.1f} us)")
    print(f"  rope_qk_norm_cache_ T={T}:{tf*1e6:7.1f} us {gb/tf:6.0f} GB/s"
          f"  ({tp/tf:.2f}x)")


def bench_lora():
    """ops.lora_apply (HIP shrink + expand, one call for all adapters) vs
    the per-adapter torch loop (LoRABatch groups: gather, two hipBLASLt
    GEMMs, scale, scatter-add per adapter) on the same inputs, at the
    Qwen3-8B projection shapes, R = 64. Every row carries an adapter,
    rows are dealt round-robin over `nad` adapters; the loop's row-index
    tensors are prebuilt on the device (its per-step host work is not
    charged). The two are timed alternately, three rounds, best of each."""
    from fusioninfer_amd.lora import LoRAAdapter, LoRABatch

    R, S = 64, 8
    print("== lora_apply vs per-adapter torch loop (bf16, R=64, 8 slots) ==")
    print("| K->N | T | adapters | lora_apply us | torch loop us | loop/kernel |")
    print("|---|---|---|---|---|---|")
    for K, N in [(4096, 6144), (4096, 4096), (4096, 24576), (12288, 4096)]:
        a = (torch.randn(S, R, K, device="cuda") / math.sqrt(K)).bfloat16()
        b = (torch.randn(S, N, R, device="cuda") / math.sqrt(R)).bfloat16()
        scales = torch.full((S,), 2.0, device="cuda")
        adapters = []
        for s in range(S):
            ad = LoRAAdapter.__new__(LoRAAdapter)
            ad.name, ad.rank, ad.scaling = f"a{s}", R, 2.0
            ad.weights = [{"t": (a[s], b[s])}]
            adapters.append(ad)
        for T in (64, 256, 2048):
            x = torch.randn(T, K, dtype=torch.bfloat16, device="cuda")
            out = torch.randn(T, N, dtype=torch.bfloat16, device="cuda")
            for nad in (1, 4, 8):
                ids = (torch.arange(T, device="cuda") % nad).int()
                loop = LoRABatch([
                    (adapters[s], (ids == s).nonzero().flatten())
                    for s in range(nad)
                ])
                slot = LoRABatch(slot_ids=ids, slots=_OneTarget(a, b, scales))
                tk = tl = float("inf")
                for _ in range(3):
                    tk = min(tk, timeit(
                        lambda: slot.apply(0, "t", x, out), iters=50))
                    tl = min(tl, timeit(
                        lambda: loop.apply(0, "t", x, out), iters=50))
                print(f"| {K}->{N} | {T} | {nad} | {tk*1e6:.1f} | "
                      f"{tl*1e6:.1f} | {tl/tk:.2f}x |")


def _event_times_us(fn, iters):
    """Per-call device-event times (us), one synchronise at the end."""
    evs = [(torch.cuda.Event(enable_timing=True),
            torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in evs]


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def bench_sampling():
    """Sampler.sample with the torch and the fused backend on the same
    logits (V = 151936, Qwen3), per parameter mix. Device-event time per
    call (host work that delays the queue included), median of 3
    alternating rounds x 20 calls after a warm-up of each; `kernel` is
    ops.sample_tokens alone on prebuilt device parameters."""
    from fusioninfer_amd.engine.sampler import Sampler
    from fusioninfer_amd.engine.sequence import SamplingParams, Sequence

    V = 151936
    mixes = {
        "greedy": lambda i: dict(),
        "top_p 0.9": lambda i: dict(temperature=0.7, top_p=0.9),
        "top_k 50 + top_p 0.9 + min_p 0.05": lambda i: dict(
            temperature=0.7, top_k=50, top_p=0.9, min_p=0.05),
        "top_p 0.9, half seeded": lambda i: dict(
            temperature=0.7, top_p=0.9, seed=(i if i % 2 else None)),
    }
    print("== Sampler.sample, torch vs fused backend (V=151936, fp32) ==")
    print("| mix | T | torch us | fused us | kernel us | torch/fused |")
    print("|---|---|---|---|---|---|")
    for T in (8, 64, 256):
        logits = torch.randn(T, V, device="cuda") * 4
        for name, mk in mixes.items():
            seqs = []
            for i in range(T):
                s = Sequence(f"s{i}", [1, 2, 3], SamplingParams(**mk(i)))
                s.output_token_ids = [0] * (i % 7)
                seqs.append(s)
            samplers = {
                b: Sampler(0, "cuda", backend=b) for b in ("torch", "fused")
            }
            sp = [s.sampling for s in seqs]
            params = (
                torch.tensor([p.temperature for p in sp], device="cuda"),
                torch.tensor([p.top_k for p in sp], dtype=torch.int32,
                             device="cuda"),
                torch.tensor([p.top_p for p in sp], device="cuda"),
                torch.tensor([p.min_p for p in sp], device="cuda"),
                torch.tensor([[p.seed or 0, i] for i, p in enumerate(sp)],
                             dtype=torch.int64, device="cuda"),
            )
            fns = {
                "torch": lambda: samplers["torch"].sample(logits, seqs),
                "fused": lambda: samplers["fused"].sample(logits, seqs),
                "kernel": lambda: ops.sample_tokens(logits, *params),
            }
            times = {k: [] for k in fns}
            for k, fn in fns.items():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            for _ in range(3):
                for k, fn in fns.items():
                    times[k] += _event_times_us(fn, 20)
            med = {k: _median(v) for k, v in times.items()}
            print(f"| {name} | {T} | {med['torch']:.1f} | {med['fused']:.1f} "
                  f"| {med['kernel']:.1f} | "
                  f"{med['torch'] / med['fused']:.2f}x |", flush=True)


def bench_sampling_e2e():
    """End-to-end: the 4-layer Qwen3-0.6B test engine, 64 seeded sampled
    sequences (temperature 0.8, top_p 0.9), 64 tokens each, both sampler
    backends. One untimed generation first (graph replays, allocator),
    then one timed: wall ms per engine step and pipelined steps taken."""
    from fusioninfer_amd.config import (CacheConfig, EngineConfig,
                                        SchedulerConfig)
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.engine.sequence import SamplingParams
    from fusioninfer_amd.models.registry import get_model_config

    print("== engine decode, 64 seeded sampled sequences (4-layer "
          "Qwen3-0.6B) ==")
    print("| backend | steps | ms/step | num_async_steps |")
    print("|---|---|---|---|")
    for backend in ("torch", "fused"):
        mc = get_model_config("Qwen3-0.6B")
        mc.num_layers = 4
        cfg = EngineConfig(
            model=mc,
            cache=CacheConfig(num_gpu_blocks=2048),
            scheduler=SchedulerConfig(
                max_num_seqs=64, max_num_batched_tokens=4096,
                max_model_len=512,
            ),
            seed=7,
            sampler_backend=backend,
        )
        torch.manual_seed(0)
        eng = LLMEngine(cfg, device="cuda:0")

        def run():
            for i in range(64):
                eng.add_request(
                    [(7 * i + j) % 1000 + 10 for j in range(32)],
                    SamplingParams(max_tokens=64, temperature=0.8,
                                   top_p=0.9, seed=100 + i),
                )
            steps0, async0 = eng.num_steps, eng.num_async_steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while eng.has_unfinished():
                eng.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return (dt, eng.num_steps - steps0,
                    eng.num_async_steps - async0)

        run()
        dt, steps, n_async = run()
        print(f"| {backend} | {steps} | {dt / steps * 1e3:.2f} | {n_async} |",
              flush=True)
        del eng
        torch.cuda.empty_cache()


def bench_penalties():
    """ops.apply_penalties (+ the per-step ops.penalty_counts_add) against
    Sampler._apply_penalties on the same inputs: V = 151936, every row
    penalised (repetition 1.3, presence 0.5, frequency 0.2) with a history
    of about 1k tokens. Device-event time per call, median of 3 alternating
    rounds x 20 calls after a warm-up of each. GB/s counts the bytes the
    kernel has to move: the histogram rows once, plus a 16 B read and a 4 B
    write per touched column. fused_add_rms_norm at [2048, 4096] runs in
    the same process as the bandwidth yardstick."""
    from fusioninfer_amd.engine.sampler import Sampler
    from fusioninfer_amd.engine.sequence import SamplingParams, Sequence

    V = 151936
    H = 4096
    x = torch.randn(2048, H, dtype=torch.bfloat16, device="cuda")
    r = torch.randn_like(x)
    w = torch.randn(H, dtype=torch.bfloat16, device="cuda")
    norm = lambda: ops.fused_add_rms_norm(x, r, w, 1e-6)  # noqa: E731
    for _ in range(5):
        norm()
    t_norm = _median(_event_times_us(norm, 60))
    print("== penalties: apply_penalties vs Sampler._apply_penalties "
          "(V=151936, ~1k-token histories) ==")
    print(f"fused_add_rms_norm [2048, 4096]: {t_norm:.1f} us, "
          f"{2048 * H * 2 * 4 / t_norm / 1e3:.0f} GB/s")
    print("| T | host path us | kernel us | kernel GB/s | counts_add us "
          "| host/kernel |")
    print("|---|---|---|---|---|---|")
    sampler = Sampler(0, "cuda")
    g = torch.Generator().manual_seed(0)
    for T in (8, 64, 256):
        logits = torch.randn(T, V, device="cuda") * 4
        seqs, touched = [], 0
        counts = torch.zeros(T, V, dtype=torch.int32)
        for i in range(T):
            hist = torch.randint(0, V, (960 + i % 128,), generator=g)
            hist[::9] = hist[0]  # one hot token
            s = Sequence(f"s{i}", hist[:32].tolist(), SamplingParams(
                repetition_penalty=1.3, presence_penalty=0.5,
                frequency_penalty=0.2))
            s.output_token_ids = hist[32:].tolist()
            seqs.append(s)
            counts[i] = torch.bincount(hist, minlength=V).int()
            touched += int((counts[i] > 0).sum())
        counts = counts.cuda()
        slot_ids = torch.arange(T, dtype=torch.int32, device="cuda")
        params = torch.tensor([[1.3, 1 / 1.3, 0.5, 0.2]] * T,
                              dtype=torch.float32, device="cuda")
        sampled = torch.randint(0, V, (T,), device="cuda")
        fns = {
            "host": lambda: sampler._apply_penalties(logits, seqs),
            "kernel": lambda: ops.apply_penalties(logits, counts, slot_ids,
                                                  params),
            "add": lambda: ops.penalty_counts_add(counts, slot_ids, sampled),
        }
        times = {k: [] for k in fns}
        for k, fn in fns.items():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(3):
            for k, fn in fns.items():
                times[k] += _event_times_us(fn, 20)
            logits.normal_()  # penalised in place every call; keep it O(1)
        med = {k: _median(v) for k, v in times.items()}
        gb = (T * V * 4 + touched * 20) / 1e9
        print(f"| {T} | {med['host']:.1f} | {med['kernel']:.1f} | "
              f"{gb / (med['kernel'] * 1e-6):.0f} | {med['add']:.1f} | "
              f"{med['host'] / med['kernel']:.0f}x |", flush=True)


def bench_penalties_e2e(runs=3):
    """End-to-end: the 4-layer Qwen3-0.6B test engine, fused backend, 64
    penalised seeded sequences, 64 tokens each, device_penalties on and
    off. One untimed generation per engine first, then `runs` timed ones:
    wall ms per engine step and pipelined steps taken."""
    from fusioninfer_amd.config import (CacheConfig, EngineConfig,
                                        SchedulerConfig)
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.engine.sequence import SamplingParams
    from fusioninfer_amd.models.registry import get_model_config

    print("== engine decode, 64 penalised seeded sequences (4-layer "
          "Qwen3-0.6B, fused backend) ==")
    print("| device_penalties | run | steps | ms/step | num_async_steps |")
    print("|---|---|---|---|---|")
    for on in (True, False):
        mc = get_model_config("Qwen3-0.6B")
        mc.num_layers = 4
        cfg = EngineConfig(
            model=mc,
            cache=CacheConfig(num_gpu_blocks=2048),
            scheduler=SchedulerConfig(
                max_num_seqs=64, max_num_batched_tokens=4096,
                max_model_len=512,
            ),
            seed=7,
            sampler_backend="fused",
            device_penalties=on,
        )
        torch.manual_seed(0)
        eng = LLMEngine(cfg, device="cuda:0")

        def run():
            for i in range(64):
                eng.add_request(
                    [(7 * i + j) % 1000 + 10 for j in range(32)],
                    SamplingParams(max_tokens=64, temperature=0.8,
                                   top_p=0.9, seed=100 + i,
                                   repetition_penalty=1.3,
                                   presence_penalty=0.5,
                                   frequency_penalty=0.2),
                )
            steps0, async0 = eng.num_steps, eng.num_async_steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while eng.has_unfinished():
                eng.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return (dt, eng.num_steps - steps0,
                    eng.num_async_steps - async0)

        run()
        for i in range(runs):
            dt, steps, n_async = run()
            print(f"| {on} | {i} | {steps} | {dt / steps * 1e3:.2f} | "
                  f"{n_async} |", flush=True)
        del eng
        torch.cuda.empty_cache()


def _host_logprobs(logits, tokens, k):
    """The torch path of LLMEngine._sample_and_emit for rows that ask for
    logprobs: one log_softmax over the slice, then per row a topk and the
    blocking float() / int() reads."""
    lp = torch.log_softmax(logits, dim=-1)
    out = []
    for j, tok in enumerate(tokens):
        top = {}
        if k > 0:
            vals, idx = lp[j].topk(k)
            top = {int(t): float(v) for t, v in zip(idx, vals)}
        out.append((float(lp[j, tok]), top))
    return out


def bench_logprobs():
    """ops.token_logprobs against the torch path of _sample_and_emit on the
    same logits: V = 151936, every row asking. The kernel is timed with
    device events (median of 3 alternating rounds x 20 calls after a
    warm-up); the torch path ends in host reads, so it is timed on the host
    clock around a synchronise (median of 3 rounds x 5 calls). "kernel +
    readback" adds the one device-to-host copy and the decoding into the
    engine's entry format. GB/s counts one read of the logits; the kernel
    reads a row two to seven times (max, sum, three descent levels, the
    list pass, part of the tie scan), from the L2 after the first.
    fused_add_rms_norm at [2048, 4096] runs in the same process as the
    bandwidth yardstick."""
    from fusioninfer_amd.engine.sampler import DeviceLogprobs

    V = 151936
    H = 4096
    x = torch.randn(2048, H, dtype=torch.bfloat16, device="cuda")
    r = torch.randn_like(x)
    w = torch.randn(H, dtype=torch.bfloat16, device="cuda")
    norm = lambda: ops.fused_add_rms_norm(x, r, w, 1e-6)  # noqa: E731
    for _ in range(5):
        norm()
    t_norm = _median(_event_times_us(norm, 60))
    print("== logprobs: token_logprobs vs log_softmax + per-row topk "
          "(V=151936) ==")
    print(f"fused_add_rms_norm [2048, 4096]: {t_norm:.1f} us, "
          f"{2048 * H * 2 * 4 / t_norm / 1e3:.0f} GB/s")
    print("| T | k | torch path us | kernel us | kernel GB/s (one read) | "
          "kernel + readback us | torch/kernel |")
    print("|---|---|---|---|---|---|---|")
    for T in (8, 64, 256):
        logits = torch.randn(T, V, device="cuda") * 4
        sampled = torch.randint(0, V, (T,), device="cuda")
        tokens = sampled.tolist()
        for k in (0, 5, 20):
            W = max(k, 1)
            num_top = torch.full((T,), k, dtype=torch.int32, device="cuda")
            buf = torch.empty(T * (1 + 2 * W), dtype=torch.int32,
                              device="cuda")
            out = DeviceLogprobs.sections(buf, T, W)
            lp = DeviceLogprobs(buf, [k] * T, W)
            kernel = lambda: ops.token_logprobs(  # noqa: E731
                logits, sampled, num_top, out=out)

            def full():
                kernel()
                return lp.entries(buf.cpu())

            host = lambda: _host_logprobs(logits, tokens, k)  # noqa: E731
            for fn in (kernel, full, host):
                fn()
            torch.cuda.synchronize()
            t_k, t_full, t_host = [], [], []
            for _ in range(3):
                t_k += _event_times_us(kernel, 20)
                t_full.append(timeit(full, iters=5, warmup=1) * 1e6)
                t_host.append(timeit(host, iters=5, warmup=1) * 1e6)
            mk, mf, mh = _median(t_k), _median(t_full), _median(t_host)
            print(f"| {T} | {k} | {mh:.0f} | {mk:.1f} | "
                  f"{T * V * 4 / mk / 1e3:.0f} | {mf:.0f} | "
                  f"{mh / mk:.0f}x |", flush=True)


def bench_logprobs_e2e(runs=3):
    """End-to-end: the 4-layer Qwen3-0.6B test engine, fused backend, 64
    greedy sequences with logprobs=5, 64 tokens each, device_logprobs on
    and off, and the same batch without logprobs as the floor. One untimed
    generation per engine first, then `runs` timed ones: wall ms per engine
    step and pipelined steps taken."""
    from fusioninfer_amd.config import (CacheConfig, EngineConfig,
                                        SchedulerConfig)
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.engine.sequence import SamplingParams
    from fusioninfer_amd.models.registry import get_model_config

    print("== engine decode, 64 sequences with logprobs=5 (4-layer "
          "Qwen3-0.6B, fused backend) ==")
    print("| device_logprobs | logprobs | run | steps | ms/step | "
          "num_async_steps |")
    print("|---|---|---|---|---|---|")
    for on, want in ((True, 5), (False, 5), (True, None)):
        mc = get_model_config("Qwen3-0.6B")
        mc.num_layers = 4
        cfg = EngineConfig(
            model=mc,
            cache=CacheConfig(num_gpu_blocks=2048),
            scheduler=SchedulerConfig(
                max_num_seqs=64, max_num_batched_tokens=4096,
                max_model_len=512,
            ),
            seed=7,
            sampler_backend="fused",
            device_logprobs=on,
        )
        torch.manual_seed(0)
        eng = LLMEngine(cfg, device="cuda:0")

        def run():
            for i in range(64):
                eng.add_request(
                    [(7 * i + j) % 1000 + 10 for j in range(32)],
                    SamplingParams(max_tokens=64, logprobs=want),
                )
            steps0, async0 = eng.num_steps, eng.num_async_steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while eng.has_unfinished():
                eng.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return (dt, eng.num_steps - steps0,
                    eng.num_async_steps - async0)

        run()
        for i in range(runs):
            dt, steps, n_async = run()
            print(f"| {on} | {want} | {i} | {steps} | "
                  f"{dt / steps * 1e3:.2f} | {n_async} |", flush=True)
        del eng
        torch.cuda.empty_cache()


def bench_spec_verify():
    """Speculative verification at V = 151936: Sampler.verify_drafts
    (penalties + draw + acceptance + histogram update + logprobs on the
    device, seeded sampled penalised spans of 1 + 4 rows with logprobs=2)
    against the host argmax loop the greedy-only path runs on the same
    number of rows (argmax(...).tolist() and the Python comparison). Both
    end in the device-to-host copy the engine waits for, so the figure is
    host wall time per call, synchronised; medians of 30 calls after 5."""
    from fusioninfer_amd.engine.sampler import Sampler
    from fusioninfer_amd.engine.sequence import SamplingParams, Sequence

    V, k = 151936, 4
    print("== speculative verification, V = 151936, spans of 1 + 4 rows ==")
    print("| rows | spans | verify_drafts us | host argmax loop us |")
    print("|---|---|---|---|")
    g = torch.Generator().manual_seed(0)
    for R in (5, 40, 160):
        S = R // (k + 1)
        logits = (torch.randn(R, V, generator=g) * 3).to("cuda:0")
        sampler = Sampler(seed=1, device="cuda:0", backend="fused")
        spans = []
        for i in range(S):
            seq = Sequence(
                f"b{i}", torch.randint(0, V, (200,), generator=g).tolist(),
                SamplingParams(temperature=0.8, top_k=50, top_p=0.9,
                               seed=i, repetition_penalty=1.3,
                               presence_penalty=0.5, frequency_penalty=0.2,
                               logprobs=2))
            spans.append(
                (seq, torch.randint(0, V, (k,), generator=g).tolist()))

        def device():
            # in place on the logits: give every call the same input
            sampler.verify_drafts(logits.clone(), spans)
            for seq, _ in spans:
                # the sequences do not grow here: tell the table so, or
                # every call would rebuild the rows from the history
                slot = sampler.penalty_table.slot_of(seq)
                sampler.penalty_table._counted_len[slot] = seq.num_tokens

        def host():
            x = logits.clone()
            greedy = x.argmax(dim=-1).tolist()
            for i, (_, d) in enumerate(spans):
                gs = greedy[i * (k + 1):(i + 1) * (k + 1)]
                m = 0
                while m < k and d[m] == gs[m]:
                    m += 1

        def wall(fn):
            out = []
            for i in range(35):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= 5:
                    out.append((time.perf_counter() - t0) * 1e6)
            return _median(out)

        print(f"| {R} | {S} | {wall(device):.0f} | {wall(host):.0f} |",
              flush=True)


def bench_spec_sampled_e2e(runs=3):
    """End-to-end: the 4-layer Qwen3-0.6B test engine, fused backend, n-gram
    proposer (4 draft tokens, 1-gram lookup), 1 / 4 / 16 concurrent seeded
    sampled requests on repetitive prompts with penalties that favour the
    history, 64 tokens each, SpeculativeConfig.sampled_verify on and off
    from one build, runs alternating. Wall ms per emitted token and the
    acceptance rate. The weights are random: the acceptance rate says
    nothing about real checkpoints."""
    from fusioninfer_amd.config import (CacheConfig, EngineConfig,
                                        SchedulerConfig)
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.engine.sequence import SamplingParams
    from fusioninfer_amd.engine.spec_decode import SpeculativeConfig
    from fusioninfer_amd.models.registry import get_model_config

    def engine(on):
        mc = get_model_config("Qwen3-0.6B")
        mc.num_layers = 4
        cfg = EngineConfig(
            model=mc,
            cache=CacheConfig(num_gpu_blocks=2048),
            scheduler=SchedulerConfig(
                max_num_seqs=16, max_num_batched_tokens=4096,
                max_model_len=512,
            ),
            seed=7,
            sampler_backend="fused",
            speculative=SpeculativeConfig(
                num_speculative_tokens=4, prompt_lookup_min=1,
                sampled_verify=on),
        )
        torch.manual_seed(0)
        return LLMEngine(cfg, device="cuda:0")

    engines = {True: engine(True), False: engine(False)}

    def run(eng, n):
        for i in range(n):
            eng.add_request(
                [11 + i, 13 + i, 17 + i] * 20,
                SamplingParams(max_tokens=64, temperature=0.8, top_k=50,
                               top_p=0.9, seed=100 + i,
                               repetition_penalty=0.8,
                               presence_penalty=-1.0,
                               frequency_penalty=-0.5),
            )
        d0, a0 = eng.num_spec_draft_tokens, eng.num_spec_accepted_tokens
        t0g = eng.num_generated_tokens
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.has_unfinished():
            eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return (dt, eng.num_generated_tokens - t0g,
                eng.num_spec_draft_tokens - d0,
                eng.num_spec_accepted_tokens - a0)

    print("== engine decode, seeded sampled requests under n-gram "
          "speculation (4-layer Qwen3-0.6B, fused backend) ==")
    print("| requests | sampled_verify | run | tokens | ms/token | drafted "
          "| accepted | acceptance |")
    print("|---|---|---|---|---|---|---|---|")
    for n in (1, 4, 16):
        for on in (True, False):
            run(engines[on], n)  # untimed
        for i in range(runs):
            for on in (True, False):
                dt, toks, drafted, acc = run(engines[on], n)
                rate = f"{acc / drafted:.2f}" if drafted else "-"
                print(f"| {n} | {on} | {i} | {toks} | "
                      f"{dt / toks * 1e3:.3f} | {drafted} | {acc} | "
                      f"{rate} |", flush=True)


def _wall_us(fn, n=30, warm=5):
    out = []
    for i in range(n + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e6)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def bench_logit_mods():
    """ops.apply_logit_mods plus the copy of its input to the device against
    the engine's host path, V = 151936. Masks: every row masked, 4 distinct
    masks of about 3 % allowed tokens; host path = per row the device-cached
    bool[V] mask, bool(m.any()) and masked_fill_. Bias: every row with 300
    entries; host path = per row a fresh torch.tensor(...) and an indexed
    add. Wall time per call with a synchronize on both sides (the host path
    synchronises by itself), median (min-max) of 30 after 5 warm-up calls;
    'kernel us' is the device-event time of the launch alone."""
    import numpy as np

    V = 151936
    W = (V + 31) // 32
    g = torch.Generator().manual_seed(0)
    bool_masks = [torch.rand(V, generator=g) < 0.03 for _ in range(4)]
    packed = []
    for m in bool_masks:
        bits = torch.zeros(W * 32, dtype=torch.uint8)
        bits[:V] = m
        packed.append(torch.from_numpy(
            np.packbits(bits.numpy(), bitorder="little").view("<i4")))
    dev_masks = [m.cuda() for m in bool_masks]
    bias_ids = torch.randperm(V, generator=g)[:300].tolist()
    bias_vals = torch.randn(300, generator=g).tolist()
    print("== logit_mods: apply_logit_mods + its input copy vs the host "
          "path (V=151936) ==")
    print("| config | T | bytes to device | device path us (min-max) | "
          "kernel us | host path us (min-max) | host/device |")
    print("|---|---|---|---|---|---|---|")
    for T in (1, 8, 64, 256):
        logits = torch.randn(T, V, device="cuda") * 4
        # masks
        host = torch.empty(T + 4 * W, dtype=torch.int32).pin_memory()
        host[:T] = torch.arange(T, dtype=torch.int32) % 4
        host[T:] = torch.cat(packed)
        dev = host.cuda()

        def dev_mask():
            d = host.to("cuda", non_blocking=True)
            ops.apply_logit_mods(logits, d[:T], d[T:].view(4, W))

        def host_mask():
            for t in range(T):
                m = dev_masks[t % 4]
                if bool(m.any()):
                    logits[t].masked_fill_(~m, float("-inf"))

        k_us = _median(_event_times_us(
            lambda: ops.apply_logit_mods(logits, dev[:T],
                                         dev[T:].view(4, W)), 40))
        d_us, h_us = _wall_us(dev_mask), _wall_us(host_mask)
        print(f"| masks | {T} | {host.numel() * 4} | {d_us[0]:.0f} "
              f"({d_us[1]:.0f}-{d_us[2]:.0f}) | {k_us:.1f} | {h_us[0]:.0f} "
              f"({h_us[1]:.0f}-{h_us[2]:.0f}) | {h_us[0] / d_us[0]:.1f}x |",
              flush=True)
        # bias
        B = 300 * T
        hostb = torch.empty(T + 1 + 2 * B, dtype=torch.int32).pin_memory()
        hostb[:T + 1] = torch.arange(T + 1, dtype=torch.int32) * 300
        hostb[T + 1:T + 1 + B] = torch.tensor(bias_ids * T,
                                              dtype=torch.int32)
        hostb[T + 1 + B:].view(torch.float32).copy_(
            torch.tensor(bias_vals * T))
        devb = hostb.cuda()

        def split(d):
            return dict(bias_cu=d[:T + 1], bias_ids=d[T + 1:T + 1 + B],
                        bias_vals=d[T + 1 + B:].view(torch.float32))

        def dev_bias():
            ops.apply_logit_mods(
                logits, **split(hostb.to("cuda", non_blocking=True)))

        def host_bias():
            for t in range(T):
                logits[t, bias_ids] += torch.tensor(
                    bias_vals, dtype=logits.dtype, device=logits.device)

        logits.normal_()
        k_us = _median(_event_times_us(
            lambda: ops.apply_logit_mods(logits, **split(devb)), 40))
        d_us, h_us = _wall_us(dev_bias), _wall_us(host_bias)
        print(f"| bias | {T} | {hostb.numel() * 4} | {d_us[0]:.0f} "
              f"({d_us[1]:.0f}-{d_us[2]:.0f}) | {k_us:.1f} | {h_us[0]:.0f} "
              f"({h_us[1]:.0f}-{h_us[2]:.0f}) | {h_us[0] / d_us[0]:.1f}x |",
              flush=True)


def _mods_engine(mods, spec, max_seqs=16):
    from fusioninfer_amd.config import (CacheConfig, EngineConfig,
                                        SchedulerConfig)
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.engine.spec_decode import SpeculativeConfig
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config("Qwen3-0.6B")
    mc.num_layers = 4
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=2048),
        scheduler=SchedulerConfig(
            max_num_seqs=max_seqs, max_num_batched_tokens=4096,
            max_model_len=512,
        ),
        seed=7,
        sampler_backend="fused",
        device_logit_mods=mods,
        speculative=SpeculativeConfig(
            num_speculative_tokens=4, prompt_lookup_min=1) if spec else None,
    )
    torch.manual_seed(0)
    return LLMEngine(cfg, device="cuda:0")


def bench_guided_spec_e2e(runs=3):
    """End-to-end: the 4-layer Qwen3-0.6B test engine, fused backend, one
    token per byte, guided requests on a JSON-like regex with fixed keys
    (three records), greedy, the prompt holding one record of that shape;
    n-gram proposer with k = 4. 1 and 8 concurrent requests. Three engines
    from one build, runs alternating: switch on + drafting, switch on
    without drafting, switch off (the host mask path; with the switch off a
    guided request never drafts, so that is the parent's behaviour with or
    without a proposer). Tokens/s and the acceptance rate. The weights are
    random: the free parts of the output (names, digits) are whatever the
    model prefers, so the acceptance rate says nothing about real
    checkpoints."""
    from fusioninfer_amd.engine.sequence import SamplingParams
    from fusioninfer_amd.guided import Vocabulary, build_guided

    rec = r'\{"name": "[a-z]{4}", "id": [0-9]{3}, "active": (true|false)\}'
    regex = rec + ", " + rec + ", " + rec
    prompt = [ord(c) + 3 for c in
              '{"name": "abcd", "id": 123, "active": true}, ']
    engines = {
        "on, drafting": _mods_engine(True, True),
        "on, no drafting": _mods_engine(True, False),
        "off (host masks)": _mods_engine(False, True),
    }
    vocab = Vocabulary(engines["on, drafting"].cfg.model.vocab_size,
                       lambda t: chr(t - 3) if 3 <= t < 259 else "")

    def run(eng, n):
        for i in range(n):
            eng.add_request(prompt, SamplingParams(
                max_tokens=200, guided=build_guided("regex", regex, vocab)))
        d0, a0 = eng.num_spec_draft_tokens, eng.num_spec_accepted_tokens
        t0g, s0 = eng.num_generated_tokens, eng.num_steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.has_unfinished():
            eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return (dt, eng.num_generated_tokens - t0g, eng.num_steps - s0,
                eng.num_spec_draft_tokens - d0,
                eng.num_spec_accepted_tokens - a0)

    print("== guided requests under n-gram speculation (4-layer "
          "Qwen3-0.6B, fused backend, JSON-like regex) ==")
    print("| requests | device_logit_mods | run | tokens | steps | tokens/s "
          "| drafted | accepted | acceptance |")
    print("|---|---|---|---|---|---|---|---|---|")
    for n in (1, 8):
        for eng in engines.values():
            run(eng, n)  # untimed
        for i in range(runs):
            for name, eng in engines.items():
                dt, toks, steps, drafted, acc = run(eng, n)
                rate = f"{acc / drafted:.2f}" if drafted else "-"
                print(f"| {n} | {name} | {i} | {toks} | {steps} | "
                      f"{toks / dt:.0f} | {drafted} | {acc} | {rate} |",
                      flush=True)


def bench_bias_pipelining(runs=3):
    """64 plain greedy sequences plus one with a logit_bias, 64 tokens each,
    4-layer Qwen3-0.6B test engine, fused backend, device_logit_mods off and
    on: wall ms per engine step and the share of pipelined steps."""
    from fusioninfer_amd.engine.sequence import SamplingParams

    print("== 64 greedy sequences + 1 biased one (4-layer Qwen3-0.6B, "
          "fused backend) ==")
    print("| device_logit_mods | run | steps | ms/step | pipelined steps | "
          "share |")
    print("|---|---|---|---|---|---|")
    # max_num_seqs is a decode-graph bucket: the static decode buffers are
    # sized by the largest bucket below it
    engines = {on: _mods_engine(on, False, max_seqs=128)
               for on in (False, True)}

    def run(eng):
        for i in range(65):
            eng.add_request(
                [(7 * i + j) % 1000 + 10 for j in range(32)],
                SamplingParams(
                    max_tokens=64,
                    logit_bias={t: 2.0 for t in range(500, 800)}
                    if i == 64 else None),
            )
        steps0, async0 = eng.num_steps, eng.num_async_steps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while eng.has_unfinished():
            eng.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, eng.num_steps - steps0, eng.num_async_steps - async0

    for eng in engines.values():
        run(eng)
    for i in range(runs):
        for on, eng in engines.items():
            dt, steps, n_async = run(eng)
            print(f"| {on} | {i} | {steps} | {dt / steps * 1e3:.2f} | "
                  f"{n_async} | {n_async / steps:.2f} |", flush=True)


class _OneTarget:
    """Minimal stand-in for LoRASlots: one layer, one target."""

    def __init__(self, a, b, scales):
        self.layers = [{"t": (a, b, scales)}]


def bench_mxfp4():
    """The four Qwen3-8B projections at decode-to-prefill batch sizes:
    mxfp4_linear, mxfp4_dequant + F.linear, bf16 F.linear and the fp8
    _scaled_mm path. Median device-event time per call; GB/s is the
    weight bytes each path has to stream (4.25 / 16 / 8 bits per weight;
    dequant + F.linear also writes and re-reads the bf16 copy) over that
    time."""
    import torch.nn.functional as F

    from fusioninfer_amd import ops
    from fusioninfer_amd.quantization import (
        fp8_linear, quantize_weight_fp8, quantize_weight_mxfp4)

    shapes = [("qkv", 6144, 4096), ("o", 4096, 4096),
              ("gate_up", 24576, 4096), ("down", 4096, 12288)]
    print("\n## MXFP4 W4A16 projections (Qwen3-8B shapes, median us, "
          "weight GB/s)")
    print("| layer NxK | M | mxfp4_linear | dequant+linear | bf16 linear | "
          "fp8 scaled_mm | bf16/mxfp4 |")
    print("|---|---|---|---|---|---|---|")
    for name, N, K in shapes:
        w = torch.randn(N, K, device="cuda", dtype=torch.bfloat16) * 0.02
        packed, scale = quantize_weight_mxfp4(w)
        w8, s8 = quantize_weight_fp8(w)
        scratch = torch.empty(N, K, device="cuda", dtype=torch.bfloat16)
        b4 = N * K // 2 + N * K // 32
        b16 = 2 * N * K
        for M in (1, 8, 32, 64, 128, 256, 512):
            x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
            out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)

            def dq_linear():
                ops.mxfp4_dequant(packed, scale, out=scratch)
                return F.linear(x, scratch)

            cols = []
            for fn, nbytes in (
                (lambda: ops.mxfp4_linear(x, packed, scale, out=out), b4),
                (dq_linear, b4 + 2 * b16),
                (lambda: F.linear(x, w), b16),
                (lambda: fp8_linear(x, w8, s8), N * K),
            ):
                for _ in range(10):
                    fn()
                us = _median(_event_times_us(fn, 100))
                cols.append((us, nbytes / us / 1e3))
            print(f"| {name} {N}x{K} | {M} | "
                  + " | ".join(f"{u:.1f} ({g:.0f})" for u, g in cols)
                  + f" | {cols[2][0] / cols[0][0]:.2f}x |", flush=True)


def bench_mxfp4_moe(rounds=3):
    """The expert GEMM pair (gate_up with fused SwiGLU, then down) of
    Qwen3-30B-A3B (E = 128, top-8, H = 2048, I = 768) for bf16 moe_gemm,
    moe_gemm_fp8 and moe_gemm_mxfp4 in one process, on the same seeded
    random routing; alignment is excluded (the fp8 pair is also given its
    activations already quantised). Each figure is the median of 100
    device-event times after 10 warm-up calls; `rounds` alternating rounds
    are taken and the fastest and slowest round median printed. block_m
    follows the bf16 / fp8 rule of MoEMLP; from T = 256 on both block_m are
    timed to show each kernel's crossover."""
    from fusioninfer_amd import ops
    from fusioninfer_amd.quantization import (
        quantize_weight_fp8, quantize_weight_mxfp4)

    E, topk, H, inter = 128, 8, 2048, 768
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    def draw(*shape):
        return (torch.randn(*shape, generator=g, device=dev) * 0.02).to(
            torch.bfloat16)

    w = {}
    for name, N, K in (("gate_up", 2 * inter, H), ("down", H, inter)):
        oi = torch.stack([draw(N, K) for _ in range(E)])  # [E, O, I]
        q = [quantize_weight_mxfp4(oi[e]) for e in range(E)]
        q8 = [quantize_weight_fp8(oi[e]) for e in range(E)]
        kn = oi.transpose(1, 2).contiguous()
        w8 = torch.stack([a for a, _ in q8]).transpose(1, 2).contiguous()
        w[name] = dict(
            bf16=ops.pack_moe_weights(kn),
            fp8=ops.pack_moe_weights(w8.view(torch.int8)).view(
                torch.float8_e4m3fn),
            fp8_s=torch.stack([s for _, s in q8]).float().contiguous(),
            mx_p=torch.stack([p for p, _ in q]),
            mx_s=torch.stack([s for _, s in q]),
        )
        del oi, kn, w8, q, q8
    nbytes = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 4.25 / 8}
    print("\n## MXFP4 MoE experts: gate_up + down pair, Qwen3-30B-A3B shapes "
          f"(median us, fastest..slowest of {rounds} rounds)")
    print("| T | block_m | bf16 moe_gemm | moe_gemm_fp8 | moe_gemm_mxfp4 | "
          "bf16 fastest / mxfp4 slowest | fp8 fastest / mxfp4 slowest |")
    print("|---|---|---|---|---|---|---|")
    for T in (1, 8, 64, 256, 1024, 2048, 4096, 8192):
        x = draw(T, H)
        logits = torch.randn(T, E, generator=g, device=dev)
        _, topi = ops.moe_router_topk(logits, topk, True)
        rule = 128 if T * topk >= 64 * E else 16
        for block_m in ((16, 128) if T >= 256 else (rule,)):
            s, e, n, _, PM = ops.moe_align(topi, 0, E, block_m)
            act = torch.empty(PM, inter, device=dev, dtype=torch.bfloat16)
            y = torch.empty(PM, H, device=dev, dtype=torch.bfloat16)
            x8, xs = ops.quant_fp8_rows(x)
            xs = xs.float()
            ops.moe_gemm(act, x, w["gate_up"]["bf16"], s, e, n, block_m, True)
            a8, a_s = ops.quant_fp8_rows(act)
            a_s = a_s.float()
            gu, dn = w["gate_up"], w["down"]

            def bf16():
                ops.moe_gemm(act, x, gu["bf16"], s, e, n, block_m, True)
                ops.moe_gemm(y, act, dn["bf16"], s, e, n, block_m, False)

            def fp8():
                ops.moe_gemm_fp8(act, x8, xs, gu["fp8"], gu["fp8_s"], s, e, n,
                                 block_m, True)
                ops.moe_gemm_fp8(y, a8, a_s, dn["fp8"], dn["fp8_s"], s, e, n,
                                 block_m, False)

            def mxfp4():
                ops.moe_gemm_mxfp4(act, x, gu["mx_p"], gu["mx_s"], s, e, n,
                                   block_m, True)
                ops.moe_gemm_mxfp4(y, act, dn["mx_p"], dn["mx_s"], s, e, n,
                                   block_m, False)

            meds = {"bf16": [], "fp8": [], "mxfp4": []}
            for _ in range(rounds):
                for name, fn in (("bf16", bf16), ("fp8", fp8),
                                 ("mxfp4", mxfp4)):
                    for _ in range(10):
                        fn()
                    meds[name].append(_median(_event_times_us(fn, 100)))
            mark = "" if block_m == rule else " (off-rule)"
            print(f"| {T} | {block_m}{mark} | "
                  + " | ".join(f"{min(m):.1f}..{max(m):.1f}"
                               for m in meds.values())
                  + f" | {min(meds['bf16']) / max(meds['mxfp4']):.2f}x"
                  + f" | {min(meds['fp8']) / max(meds['mxfp4']):.2f}x |",
                  flush=True)
    active = 3 * H * inter  # weights of one expert
    print("weight bytes per active expert: "
          + ", ".join(f"{k} {active * v / 1e6:.2f} MB"
                      for k, v in nbytes.items()))


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    torch.manual_seed(0)
    if which in ("prefill", "all"):
        bench_prefill()
    if which in ("decode", "all"):
        bench_decode(group=4)
        bench_decode(group=8)
    if which in ("elementwise", "all"):
        bench_elementwise()
    if which in ("lora", "all"):
        bench_lora()
    if which in ("sampling", "all"):
        bench_sampling()
    if which in ("sampling_e2e", "all"):
        bench_sampling_e2e()
    if which in ("penalties", "all"):
        bench_penalties()
    if which in ("penalties_e2e", "all"):
        bench_penalties_e2e()
    if which in ("logprobs", "all"):
        bench_logprobs()
    if which in ("logprobs_e2e", "all"):
        bench_logprobs_e2e()
    if which in ("spec_verify", "all"):
        bench_spec_verify()
    if which in ("spec_sampled_e2e", "all"):
        bench_spec_sampled_e2e()
    if which in ("logit_mods", "all"):
        bench_logit_mods()
    if which in ("guided_spec_e2e", "all"):
        bench_guided_spec_e2e()
    if which in ("bias_pipelining", "all"):
        bench_bias_pipelining()
    if which in ("mxfp4", "all"):
        bench_mxfp4()
    if which in ("mxfp4_moe", "all"):
        bench_mxfp4_moe()
