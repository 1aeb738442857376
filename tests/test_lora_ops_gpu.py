"""HIP lora_apply kernels (shrink + expand) vs ref.lora_apply on CPU copies.

Inputs: x, out ~ N(0,1); A std 1/sqrt(K), B std 1/sqrt(R), scales in
[0.5, 2], so the delta is O(1) like out. Tolerance: the project's bf16
atol = rtol = 2e-2 (test_ops_gpu.assert_close_bf16)."""

import functools
import math

import pytest
import torch

import fusioninfer_amd.ops as ops
from fusioninfer_amd.ops import reference as ref
from tests.test_ops_gpu import assert_close_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (T, K, N, R, S): one row / one tile; tail tile + R=16 half k-step; odd T,
# N not a multiple of the 256-column workgroup, 8 slots; K = 12288
SHAPES = [
    (1, 64, 16, 16, 1),
    (17, 1024, 4096, 16, 4),
    (33, 3072, 1040, 64, 8),
    (40, 12288, 1024, 64, 8),
]


def setup_module():
    assert ops.has_native(), "HIP extension must be present on a GPU box"


@functools.lru_cache(maxsize=None)
def case(T, K, N, R, S):
    """CPU inputs for one shape. Slot 0 has rank 4 (zero-padded to R); the
    last slot (when S > 1) has B == 0."""
    g = torch.Generator().manual_seed(1000 + T + K + N + R + S)
    x = torch.randn(T, K, generator=g).bfloat16()
    out = torch.randn(T, N, generator=g).bfloat16()
    a = torch.randn(S, R, K, generator=g) / math.sqrt(K)
    b = torch.randn(S, N, R, generator=g) / math.sqrt(R)
    a[0, 4:] = 0
    b[0, :, 4:] = 0
    if S > 1:
        b[S - 1] = 0
    scales = (0.5 + 1.5 * torch.rand(S, generator=g)).float()
    return x, out, a.bfloat16(), b.bfloat16(), scales


def patterns(T, S):
    """name -> [T] int32 slot ids."""
    pats = {
        "none": torch.full((T,), -1, dtype=torch.int32),
        "one_slot": torch.full((T,), S - 1 if S == 1 else S - 2,
                               dtype=torch.int32),
        "rank4_slot": torch.zeros(T, dtype=torch.int32),
    }
    if S > 1:
        # every adapter row of a 16-token tile on a different slot, -1
        # interleaved (8 slots: [0,-1,1,-1,...,7,-1] per tile)
        t = torch.arange(T)
        mixed = torch.where(t % 2 == 0, (t // 2) % S, torch.tensor(-1))
        pats["mixed"] = mixed.to(torch.int32)
        pats["zero_b_slot"] = torch.full((T,), S - 1, dtype=torch.int32)
    return pats


@functools.lru_cache(maxsize=None)
def expected(shape, pat):
    x, out, a, b, scales = case(*shape)
    ids = patterns(shape[0], shape[4])[pat]
    return ref.lora_apply(out.clone(), x, ids, a, b, scales)


def run_gpu(shape, ids):
    x, out, a, b, scales = case(*shape)
    got = out.to(DEV, copy=True)
    ops.lora_apply(got, x.to(DEV), ids.to(DEV), a.to(DEV), b.to(DEV),
                   scales.to(DEV))
    return got.cpu()


CASES = [(s, p) for s in SHAPES for p in patterns(s[0], s[4])]


@pytest.mark.parametrize("shape,pat", CASES,
                         ids=[f"{'x'.join(map(str, s))}-{p}" for s, p in CASES])
def test_lora_apply_matches_reference(shape, pat):
    ids = patterns(shape[0], shape[4])[pat]
    out0 = case(*shape)[1]
    got = run_gpu(shape, ids)
    exp = expected(shape, pat)
    err = (got.float() - exp.float()).abs().max().item()
    print(f"lora_apply {shape} {pat}: max abs err {err:.4g}")
    assert_close_bf16(got, exp)
    base = ids < 0
    assert torch.equal(got[base].view(torch.int16),
                       out0[base].view(torch.int16))
    if pat in ("none", "zero_b_slot"):
        # no adapter / zero B: bitwise identical to the input
        assert torch.equal(got.view(torch.int16), out0.view(torch.int16))
    else:
        assert not torch.equal(got[~base], out0[~base])
    # deterministic: a second call gives the same bits
    again = run_gpu(shape, ids)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))


def test_row_result_independent_of_batch():
    """Row 5 of the T=33 mixed case, computed alone with T=1, bit for bit."""
    shape = SHAPES[2]
    x, out, a, b, scales = case(*shape)
    ids = patterns(shape[0], shape[4])["mixed"]
    ids = ids.clone()
    ids[5] = 3  # an adapter row at an odd position of the tile
    full = run_gpu(shape, ids)
    solo = out[5:6].to(DEV, copy=True)
    ops.lora_apply(solo, x[5:6].to(DEV), ids[5:6].to(DEV), a.to(DEV),
                   b.to(DEV), scales.to(DEV))
    assert not torch.equal(full[5], out[5])
    assert torch.equal(full[5].view(torch.int16),
                       solo.cpu()[0].view(torch.int16))


def test_lora_apply_under_graph_capture():
    """Captured once, replayed with changed slot ids and changed slot
    contents (copy_ into the same stacks): must match eager."""
    shape = SHAPES[1]
    T, K, N, R, S = shape
    x, out, a, b, scales = case(*shape)
    pats = patterns(T, S)
    xs, a_d, b_d, sc_d = x.to(DEV), a.to(DEV), b.to(DEV), scales.to(DEV)
    ids_d = pats["none"].to(DEV)
    out_d = out.to(DEV, copy=True)

    ops.lora_apply(out_d, xs, ids_d, a_d, b_d, sc_d)  # warm-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.lora_apply(out_d, xs, ids_d, a_d, b_d, sc_d)

    # replay 1: new slot ids
    out_d.copy_(out)
    ids_d.copy_(pats["mixed"])
    g.replay()
    got1 = out_d.cpu()
    eager1 = run_gpu(shape, pats["mixed"])
    assert torch.equal(got1.view(torch.int16), eager1.view(torch.int16))
    assert_close_bf16(got1, expected(shape, "mixed"))

    # replay 2: slot 1 takes slot 2's contents, slot ids all 1
    a_d[1].copy_(a_d[2])
    b_d[1].copy_(b_d[2])
    sc_d[1:2].copy_(sc_d[2:3])
    out_d.copy_(out)
    ids_d.fill_(1)
    g.replay()
    got2 = out_d.cpu()
    exp2 = ref.lora_apply(out.clone(), x,
                          torch.full((T,), 2, dtype=torch.int32), a, b, scales)
    assert_close_bf16(got2, exp2)
    assert not torch.equal(got2, got1)
