"""Helpers shared by tests/test_int4.py and tests/test_int4_gpu.py."""


def pack(q):
    return (q[:, 0::2] | (q[:, 1::2] << 4)).contiguous()


def engine(quant, model="tiny-qwen3", G=64, device="cpu", eager=False,
           model_path=None):
    from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.models.registry import get_model_config

    mc = get_model_config(model)
    mc.quantization, mc.int4_group_size, mc.model_path = quant, G, model_path
    cfg = EngineConfig(
        model=mc, cache=CacheConfig(num_gpu_blocks=64),
        scheduler=SchedulerConfig(
            max_num_seqs=4, max_num_batched_tokens=256, max_model_len=128),
        seed=11, enforce_eager=eager)
    return LLMEngine(cfg, device=device)


def prefill_logits(eng, prompt):
    from fusioninfer_amd.engine.block_manager import BlockManager
    from fusioninfer_amd.engine.sequence import SamplingParams, Sequence

    bm = BlockManager(eng.runner.num_gpu_blocks, eng.cfg.cache.block_size)
    seq = Sequence("s", list(prompt), SamplingParams())
    bm.allocate(seq)
    return eng.runner.execute_prefill([seq], bm).double().cpu()
