"""paged_attention_shortq on the GPU against the float64 paged-prefill
reference, on one adversarial batch (needles, anti-needles, poisoned pads,
permuted tables; see attention_cases.py), plus the engine's verify steps."""

import functools

import pytest
import torch

import attention_cases as ac
import fusioninfer_amd.ops as ops

pytestmark = pytest.mark.gpu

# (total ctx, new rows): one block; no prefix; rows either side of a block
# edge; the widest speculative span; rows either side of a partition edge;
# SHORTQ_MAX_ROWS across 1024; the decode shape over four partitions
CTX = [1, 5, 17, 33, 514, 1030, 1537]
NEW = [1, 5, 2, 17, 5, 32, 1]
SPAN17 = 3  # index of the (33, 17) sequence


@functools.lru_cache(maxsize=None)
def case(head_dim, group, fp8, nan_pads=False):
    c = ac.build_prefill_paged_case(CTX, NEW, head_dim, hq=2 * group, hk=2,
                                    fp8=fp8, nan_pads=nan_pads)
    assert c[3].shape[1] == 97
    scale = head_dim ** -0.5
    want = ac.ref64_prefill_paged(*c, scale, q_rounding="bf16_prescaled")
    return tuple(t.cuda() for t in c), scale, want


def sub_batch(c, seqs):
    """(q, k_cache, v_cache, tables, cu, lens) of some sequences of a case;
    an index of None adds a sequence with no q rows."""
    q, k, v, tables, cu, lens = c
    rows, new_cu, idx = [], [0], []
    for s in seqs:
        if s is not None:
            rows.append(q[int(cu[s]):int(cu[s + 1])])
        new_cu.append(new_cu[-1] + (0 if s is None else rows[-1].shape[0]))
        idx.append(0 if s is None else s)
    return (torch.cat(rows), k, v, tables[idx].contiguous(),
            torch.tensor(new_cu, dtype=torch.int32, device=q.device),
            lens[idx].contiguous())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
@pytest.mark.parametrize("group", [1, 4, 7, 8])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_adversarial_batch(head_dim, group, fp8):
    c, scale, want = case(head_dim, group, fp8)
    got = ops.paged_attention_shortq(*c, scale)
    err = ac.row_rel_err(got, want).max().item()
    print(f"shortq D={head_dim} G={group} fp8={fp8}: max row_rel_err {err:.5f}")
    assert err < ac.KERNEL_TOL


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_nan_pads(fp8):
    c, scale, want = case(128, 4, fp8, nan_pads=True)
    got = ops.paged_attention_shortq(*c, scale)
    assert not torch.isnan(got.float()).any()
    assert ac.row_rel_err(got, want).max().item() < ac.KERNEL_TOL


def test_grid_and_batch_invariance():
    c, scale, _ = case(128, 4, False)
    cu = c[4]
    alone = ops.paged_attention_shortq(*sub_batch(c, [SPAN17]), scale)
    full = ops.paged_attention_shortq(*c, scale, max_q=32)
    keep = [s for s in range(len(CTX)) if NEW[s] <= 17]
    part = sub_batch(c, keep)
    small = ops.paged_attention_shortq(*part, scale, max_q=17)
    k0 = int(part[4][keep.index(SPAN17)])
    assert torch.equal(full[int(cu[SPAN17]):int(cu[SPAN17 + 1])], alone)
    assert torch.equal(small[k0:k0 + 17], alone)


def test_out_into_guarded_rows():
    c, scale, _ = case(64, 7, True)
    batch = sub_batch(c, [1, None, SPAN17])
    want = ops.paged_attention_shortq(*batch, scale)
    T = want.shape[0]
    buf = torch.full((T + 4,) + tuple(want.shape[1:]), 7.0,
                     dtype=torch.bfloat16, device="cuda")
    got = ops.paged_attention_shortq(*batch, scale, out=buf[2:2 + T])
    assert got.data_ptr() == buf[2:].data_ptr()
    assert torch.equal(buf[2:2 + T], want)
    assert (buf[:2] == 7.0).all() and (buf[2 + T:] == 7.0).all()
    # the empty sequence left no trace: the other two are what they are alone
    assert torch.equal(
        want[:5], ops.paged_attention_shortq(*sub_batch(c, [1]), scale))
    assert torch.equal(
        want[5:], ops.paged_attention_shortq(*sub_batch(c, [SPAN17]), scale))


def test_engine_verify_steps_run_shortq(monkeypatch):
    from fusioninfer_amd.config import (CacheConfig, EngineConfig,
                                        SchedulerConfig)
    from fusioninfer_amd.engine.llm_engine import LLMEngine
    from fusioninfer_amd.engine.sequence import SamplingParams
    from fusioninfer_amd.engine.spec_decode import SpeculativeConfig
    from fusioninfer_amd.models.registry import get_model_config

    def engine(speculative):
        cfg = EngineConfig(
            model=get_model_config("tiny-qwen3"),
            cache=CacheConfig(num_gpu_blocks=512),
            scheduler=SchedulerConfig(max_num_seqs=16,
                                      max_num_batched_tokens=2048,
                                      max_model_len=512),
            speculative=speculative, seed=7, enforce_eager=False)
        return LLMEngine(cfg, device="cuda:0")

    prompts = [[3, 1, 4, 1, 5, 9] * 8, [2, 7, 2, 7, 2, 7] * 8]
    sp = SamplingParams(max_tokens=24)
    ref = [o.output_token_ids for o in engine(None).generate(prompts, sp)]
    rows = {"shortq": [], "prefill": []}
    for name, key in (("paged_attention_shortq", "shortq"),
                      ("prefill_attention_paged", "prefill")):
        real = getattr(ops, name)

        def counted(q, *a, _real=real, _key=key, **kw):
            rows[_key].append(q.shape[0])
            return _real(q, *a, **kw)

        monkeypatch.setattr(ops, name, counted)
    eng = engine(SpeculativeConfig(num_speculative_tokens=4,
                                   verify_attention="shortq"))
    outs = eng.generate(prompts, sp)
    assert [o.output_token_ids for o in outs] == ref
    assert eng.num_spec_draft_tokens > 0
    # verify steps (at most 2 x 5 rows) ran shortq; only the prompts' own
    # prefill (48 rows each) went through the prefill kernel
    assert rows["shortq"] and max(rows["shortq"]) <= 10
    assert min(rows["prefill"]) >= 48
