"""paged_attention_shortq off the GPU: argument checks, the CPU path, and
the engine's verify_attention switch."""

import pytest
import torch

import attention_cases as ac
import fusioninfer_amd.ops as ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.engine.sequence import SamplingParams
from fusioninfer_amd.engine.spec_decode import SpeculativeConfig
from fusioninfer_amd.models.registry import get_model_config
from fusioninfer_amd.ops import reference as ref

PROMPTS = [[3, 1, 4, 1, 5, 9] * 6, [2, 7, 2, 7, 2, 7, 2, 7] * 4,
           [11, 12, 13] * 10]


def make_engine(speculative):
    cfg = EngineConfig(
        model=get_model_config("tiny-qwen3"),
        cache=CacheConfig(num_gpu_blocks=256),
        scheduler=SchedulerConfig(max_num_seqs=8, max_num_batched_tokens=1024,
                                  max_model_len=256),
        speculative=speculative, seed=0)
    return LLMEngine(cfg, device="cpu")


def small_case():
    return ac.build_prefill_paged_case([33, 5], [17, 5], 64, hq=8, hk=2)


def test_cpu_path_is_the_paged_prefill_reference():
    c = small_case()
    want = ref.prefill_attention_paged(*c, 0.125)
    assert torch.equal(ops.paged_attention_shortq(*c, 0.125, max_q=17), want)
    out = torch.empty_like(c[0])
    assert ops.paged_attention_shortq(*c, 0.125, out=out) is out
    assert torch.equal(out, want)


def _bad(name):
    q, k, v, bt, cu, lens = small_case()
    kw = {}
    if name == "q dtype":
        q = q.float()
    elif name == "cache dtype":
        k, v = k.half(), v.half()
    elif name == "cache dtypes differ":
        v = v.to(torch.float8_e4m3fn)
    elif name == "head_dim":
        q, k, v = q[..., :32], k[..., :32], v[..., :32]
    elif name == "block size":
        k, v = k[:, :, :8], v[:, :, :8]
    elif name == "Hq % Hk":
        q = q[:, :7]
    elif name == "G > 8":
        q, k, v = torch.cat([q, q, q], 1), k[:, :1], v[:, :1]
    elif name == "index dtype":
        cu = cu.long()
    elif name == "index device":
        lens = lens.to("meta")
    elif name == "max_q low":
        kw["max_q"] = 0
    elif name == "max_q high":
        kw["max_q"] = ops.SHORTQ_MAX_ROWS + 1
    elif name == "T > S * max_q":
        kw["max_q"] = 10
    elif name == "out":
        kw["out"] = torch.empty_like(q)[:, :, ::2]
    return (q, k, v, bt, cu, lens), kw


@pytest.mark.parametrize("name", [
    "q dtype", "cache dtype", "cache dtypes differ", "head_dim", "block size",
    "Hq % Hk", "G > 8", "index dtype", "index device", "max_q low",
    "max_q high", "T > S * max_q", "out"])
def test_rejects(name):
    args, kw = _bad(name)
    with pytest.raises(ValueError):
        ops.paged_attention_shortq(*args, **kw)


def test_cpu_engine_shortq_equals_prefill():
    sp = SamplingParams(max_tokens=24)
    outs = {}
    for mode in ("prefill", "shortq"):
        torch.manual_seed(0)
        eng = make_engine(SpeculativeConfig(num_speculative_tokens=4,
                                            verify_attention=mode))
        outs[mode] = [o.output_token_ids
                      for o in eng.generate(PROMPTS, sp)]
        assert eng.num_spec_draft_tokens > 0
    assert outs["shortq"] == outs["prefill"]


def test_unknown_verify_attention_is_rejected():
    with pytest.raises(ValueError, match="verify_attention"):
        make_engine(SpeculativeConfig(verify_attention="decode"))
