"""token_logprobs kernel (sampling.hip) on the GPU: against the float64
reference on every non-skipped row, ties, determinism, row independence,
and the engine with sampler_backend="fused" (4-layer Qwen3-0.6B, the
configuration of test_fused_sampler_gpu).

Tolerance of the values: 1e-4 absolute. lp = x - (m + logf(S)) with |lp|
<= 64 carries about three fp32 roundings at magnitude <= 64 (3 * 2^-18 =
1.1e-5), the error of logf and of the 2^17-term sum of exponentials
relative to S (a few 1e-6), in all about 2e-5. On these inputs CPU fp32
log_softmax is off by 1.6e-5 at V = 151936 and a 1024-strided fixed-order
sum by 2.8e-6. The ids carry no rounding: they are compared exactly."""

import pytest
import torch

from fusioninfer_amd import ops
from fusioninfer_amd.config import CacheConfig, EngineConfig, SchedulerConfig
from fusioninfer_amd.engine.llm_engine import LLMEngine
from fusioninfer_amd.models.registry import get_model_config
from tests.test_device_logprobs import (
    NINF, assert_entries_agree, check_against, generate, logprobs_case,
    sentinel_out, tokens,
)
from tests.test_fused_sampler_gpu import PROMPTS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 5), (3, 50), (33, 1000), (257, 4099), (4, 151936)]


def run_case(T, V, rows=None):
    (logits, token_ids, num_top), want = logprobs_case(T, V)
    sel = slice(None) if rows is None else rows
    n = logits[sel].shape[0]
    return ops.token_logprobs(
        logits[sel].contiguous().to(DEV), token_ids[sel].to(DEV),
        num_top[sel].to(DEV), out=sentinel_out(n, 32, DEV),
    )


@pytest.mark.parametrize("T,V", SHAPES)
def test_kernel_matches_reference(T, V):
    (_, _, num_top), want = logprobs_case(T, V)
    assert (num_top >= 0).any()
    check_against(run_case(T, V), want, num_top)


def test_narrow_output_and_default_allocation():
    (logits, token_ids, num_top), want = logprobs_case(33, 1000)
    args = (logits.to(DEV), token_ids.to(DEV), num_top.to(DEV))
    chosen, ids, lp = ops.token_logprobs(*args, out=sentinel_out(33, 7, DEV))
    rows = num_top >= 0
    # k = min(num_top, 7): the first columns of the wide result
    capped = want[1][:, :7].clone()
    assert torch.equal(ids.cpu()[rows], capped[rows])
    assert (ids.cpu()[~rows] == -77).all()
    assert torch.equal(chosen.cpu()[rows], run_case(33, 1000)[0].cpu()[rows])
    chosen, ids, lp = ops.token_logprobs(*args)
    assert ids.shape == (33, 32)
    assert torch.equal(ids.cpu()[rows], want[1][rows])


def test_out_of_range_token_is_rejected_before_indexing():
    logits = torch.randn(6, 50, generator=torch.Generator().manual_seed(1))
    tok = torch.tensor([-1, 50, 1 << 40, -(1 << 40), (1 << 31) + 3, 49])
    num_top = torch.full((6,), 2, dtype=torch.int32)
    chosen, ids, lp = ops.token_logprobs(
        logits.to(DEV), tok.to(DEV), num_top.to(DEV), width=2)
    assert torch.isnan(chosen[:5]).all() and torch.isfinite(chosen[5])
    w_chosen, w_ids, _ = ops.token_logprobs(logits, tok, num_top, width=2)
    assert torch.equal(ids.cpu(), w_ids)
    assert abs(float(chosen[5]) - float(w_chosen[5])) <= 1e-4


# ------------------------------------------------------------------ ties

def top_ids(x, k, W=32):
    x = torch.as_tensor(x, dtype=torch.float32).view(1, -1)
    chosen, ids, lp = ops.token_logprobs(
        x.to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
        torch.tensor([k], dtype=torch.int32, device=DEV), width=W)
    want = ops.token_logprobs(
        x, torch.zeros(1, dtype=torch.int64),
        torch.tensor([k], dtype=torch.int32), width=W)
    assert torch.equal(ids.cpu(), want[1])
    fin = torch.isfinite(want[2])
    assert torch.equal(lp.cpu()[~fin], want[2][~fin])
    assert ((lp.cpu()[fin] - want[2][fin]).abs() <= 1e-4).all()
    return ids[0, :k].tolist()


def test_all_equal_row():
    assert top_ids(torch.full((50,), 0.75), 5) == [0, 1, 2, 3, 4]


def test_tie_at_the_boundary_takes_the_lowest_indices():
    x = torch.linspace(-6.0, -1.0, 1000)
    x[900], x[17] = 2.0, 1.5
    x[401], x[400], x[950] = 1.0, 1.0, 1.0  # 3rd == 4th == 5th
    assert top_ids(x, 3) == [900, 17, 400]
    assert top_ids(x, 4) == [900, 17, 400, 401]


def test_ties_straddling_a_scan_tile():
    x = torch.linspace(-6.0, -1.0, 3 * 4096 + 5)
    x[9000] = 3.0
    x[4095], x[4096], x[8192] = 1.0, 1.0, 1.0
    assert top_ids(x, 2) == [9000, 4095]
    assert top_ids(x, 3) == [9000, 4095, 4096]
    assert top_ids(x, 4) == [9000, 4095, 4096, 8192]


def test_tie_at_the_last_index_of_an_odd_row():
    x = torch.linspace(-6.0, -1.0, 4099)
    x[7], x[4098] = 1.0, 1.0
    assert top_ids(x, 2) == [7, 4098]
    x[7] = -7.0
    assert top_ids(x, 1) == [4098]


def test_zero_signs_tie_at_the_boundary():
    x = -torch.ones(200) - torch.rand(
        200, generator=torch.Generator().manual_seed(2))
    x[150] = 4.0
    x[20], x[120] = -0.0, 0.0
    assert top_ids(x, 2) == [150, 20]
    x[20], x[120] = 0.0, -0.0
    assert top_ids(x, 2) == [150, 20]
    assert top_ids(x, 3) == [150, 20, 120]


def test_minus_inf_entries_fill_in_index_order():
    x = torch.full((300,), NINF)
    x[250], x[3] = 1.0, 2.0
    assert top_ids(x, 5) == [3, 250, 0, 1, 2]
    assert top_ids(torch.full((300,), NINF), 4) == [0, 1, 2, 3]


# ----------------------------------------------------------- determinism

def test_same_call_twice_is_bit_identical():
    a, b = run_case(257, 4099), run_case(257, 4099)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_row_is_independent_of_its_batch():
    full = run_case(33, 1000)
    alone = run_case(33, 1000, rows=slice(5, 6))
    for x, y in zip(full, alone):
        assert torch.equal(x[5:6].view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------- engine

def make_engine(**kw):
    mc = get_model_config("Qwen3-0.6B")
    mc.num_layers = 4
    cfg = EngineConfig(
        model=mc,
        cache=CacheConfig(num_gpu_blocks=512),
        scheduler=SchedulerConfig(
            max_num_seqs=16, max_num_batched_tokens=2048, max_model_len=512,
        ),
        seed=7,
        sampler_backend="fused",
        **kw,
    )
    torch.manual_seed(0)
    return LLMEngine(cfg, device=DEV)


def test_engine_device_logprobs():
    greedy = dict(max_tokens=16)
    seeded = dict(max_tokens=16, temperature=0.8, top_k=50, top_p=0.9,
                  seed=1234)
    eng = make_engine()
    host = make_engine(device_logprobs=False)
    for sampling in (greedy, seeded):
        before = eng.num_async_steps
        got = generate(eng, dict(logprobs=5, **sampling), PROMPTS)
        assert eng.num_async_steps > before
        want = generate(host, dict(logprobs=5, **sampling), PROMPTS)
        assert host.num_async_steps == 0
        plain = generate(eng, sampling, PROMPTS)
        assert tokens(got) == tokens(want) == tokens(plain)
        assert all(o.logprobs == [] for o in plain)
        for a, b in zip(got, want):
            assert len(a.output_token_ids) == 16
            assert_entries_agree(a, b, 5)
            if sampling is greedy:
                for tok, (c, top) in zip(a.output_token_ids, a.logprobs):
                    assert top[tok] == c == max(top.values())
