"""Attention kernels on adversarial inputs vs matched-rounding float64.

Inputs come from tests/attention_cases.py (needles at partition and block
edges, finite poison in every slot a kernel must not attend, permuted block
tables); tests/test_attention_cases.py proves on the CPU that each of the
usual kernel mistakes moves them by at least 10x the bound used here.

Every numeric assertion is row_rel_err (L2 over D per row and head) against
the float64 reference with the q_rounding of the score path that runs:
<= KERNEL_TOL = 2^-6, four times the 2^-8 that rounding the exact result
to bf16 costs. The bound is not derived from any kernel output.
"""

import functools
import math
import os
import subprocess
import sys

import pytest
import torch

import attention_cases as ac
import fusioninfer_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -65536.0  # exact in bf16, far from any attention output here


def setup_module():
    assert ops.has_native(), "HIP extension must be present on a GPU box"


def _to_dev(*tensors):
    return [t.to(DEV) for t in tensors]


def _assert_rows(name, got, want64):
    err = ac.row_rel_err(got, want64)
    worst = float(err.max())
    print(f"{name}: max row_rel_err {worst:.5f} (bound {ac.KERNEL_TOL:.5f})")
    assert bool(torch.isfinite(got.float()).all()), name
    assert worst <= ac.KERNEL_TOL, (name, worst, err.argmax().item())


# ------------------------------------------------------------------ decode

@functools.lru_cache(maxsize=2)
def _decode_case(grid, head_dim, group, fp8):
    lens, table_blocks = ac.DECODE_GRIDS[grid]
    seed = 1000 * head_dim + 10 * group + int(fp8) + len(lens)
    return ac.build_decode_case(lens, head_dim, group, fp8, table_blocks, seed)


def _check_decode(grid, head_dim, group, fp8, mfma=True):
    case = _decode_case(grid, head_dim, group, fp8)
    scale = 1.0 / math.sqrt(head_dim)
    want = ac.ref64_decode(*case, scale,
                           q_rounding=ac.decode_q_rounding(fp8, group, mfma))
    got = ops.paged_attention_decode(*_to_dev(*case), scale)
    name = (f"decode {grid} D={head_dim} G={group} "
            f"{'fp8' if fp8 else 'bf16'} {'mfma' if mfma else 'scalar'}")
    _assert_rows(name, got, want)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("group", [1, 2, 4, 8])
@pytest.mark.parametrize("head_dim", [64, 128])
@pytest.mark.parametrize("grid", ["wide", "full"])
def test_decode_adversarial(grid, head_dim, group, fp8):
    """wide: 5 partitions, 8-wave kernels, the longest row fills 4 and most
    rows leave 3-4 empty. full: 4 partitions, 4-wave kernels with the G=4
    and G=8 head split."""
    _check_decode(grid, head_dim, group, fp8)


_SCALAR_SCORES_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import test_attention_adversarial_gpu as t
t.setup_module()
for grid in ("wide", "full"):
    for fp8 in (False, True):
        for head_dim, group in ((128, 1), (128, 4), (128, 8), (64, 4)):
            t._check_decode(grid, head_dim, group, fp8, mfma=False)
"""


def test_decode_adversarial_scalar_scores():
    """FI_DECODE_MFMA=0 (read once per process, hence one fresh child):
    every case takes the scalar scores, which keep Q in fp32, so the
    reference rounds nothing. A miss raises in the child."""
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    child = subprocess.run(
        [sys.executable, "-c", _SCALAR_SCORES_CHILD, tests_dir],
        env={**os.environ, "FI_DECODE_MFMA": "0"},
        cwd=os.path.dirname(tests_dir), capture_output=True, text=True,
        timeout=300,
    )
    print(child.stdout)
    assert child.returncode == 0, child.stderr[-2000:]
    assert child.stdout.count("scalar: max row_rel_err") == 16


@pytest.mark.parametrize("grid", ["wide", "full"])
def test_decode_adversarial_out(grid):
    """out= rows of a larger buffer: every row overwritten, the guard rows
    on either side untouched, same bits as the allocating call."""
    head_dim, group, fp8 = 128, 4, False
    case = _decode_case(grid, head_dim, group, fp8)
    scale = 1.0 / math.sqrt(head_dim)
    dev = _to_dev(*case)
    S = case[0].shape[0]
    buf = torch.full((S + 2, *case[0].shape[1:]), SENTINEL,
                     dtype=torch.bfloat16, device=DEV)
    ret = ops.paged_attention_decode(*dev, scale, out=buf[1:S + 1])
    assert ret.data_ptr() == buf[1].data_ptr()
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
    assert not bool((buf[1:S + 1] == SENTINEL).any())
    assert torch.equal(buf[1:S + 1], ops.paged_attention_decode(*dev, scale))
    want = ac.ref64_decode(*case, scale,
                           q_rounding=ac.decode_q_rounding(fp8, group))
    _assert_rows(f"decode out= {grid}", buf[1:S + 1], want)


# ----------------------------------------------------------------- prefill

@functools.lru_cache(maxsize=2)
def _prefill_case(head_dim, fp8, nan_pads=False):
    ctx_lens, new_lens = ac.PREFILL_PAGED
    case = ac.build_prefill_paged_case(ctx_lens, new_lens, head_dim, 8, 2,
                                       fp8, seed=500 + head_dim + int(fp8),
                                       nan_pads=nan_pads)
    want = ac.ref64_prefill_paged(*case, 1.0 / math.sqrt(head_dim),
                                  q_rounding="bf16_prescaled")
    return case, want


@pytest.mark.parametrize("tile_rows", [None, 128], ids=["default", "rows128"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_prefill_paged_adversarial(head_dim, fp8, tile_rows):
    """ctx_start 64, 17, 17, 403, 487; new lengths across the 32-row wave
    block and the workgroup tile; diagonal probes with an anti-needle one
    past the diagonal; default tiling and the 128-row (4-wave) variant."""
    case, want = _prefill_case(head_dim, fp8)
    q, kc, vc, bt, cu, slk = _to_dev(*case)
    got = ops.prefill_attention_paged(q, kc, vc, bt, cu, slk,
                                      1.0 / math.sqrt(head_dim),
                                      tile_rows=tile_rows)
    _assert_rows(f"prefill paged D={head_dim} {'fp8' if fp8 else 'bf16'} "
                 f"tile_rows={tile_rows}", got, want)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_prefill_paged_nan_pads(fp8):
    """The paged prefill kernel clamps source rows to k_len-1 and never
    reads a pad slot or an unowned block: NaN there must not reach the
    output. (Prefill only; decode's contract is in docs/kernels.md.)"""
    head_dim = 128
    case, want = _prefill_case(head_dim, fp8, nan_pads=True)
    assert bool(torch.isnan(case[1].float()).any())
    assert bool(torch.isnan(case[2].float()).any())
    assert bool(torch.isfinite(want).all())
    q, kc, vc, bt, cu, slk = _to_dev(*case)
    got = ops.prefill_attention_paged(q, kc, vc, bt, cu, slk,
                                      1.0 / math.sqrt(head_dim))
    _assert_rows(f"prefill paged NaN pads {'fp8' if fp8 else 'bf16'}",
                 got, want)


@pytest.mark.parametrize("head_dim", [64, 128])
def test_prefill_dense_adversarial_rows128(head_dim):
    """Dense prefill_attention with diagonal probes at tile_rows=128."""
    lens = ac.PREFILL_DENSE_LENS
    case = ac.build_prefill_paged_case(lens, lens, head_dim, 8, 2, False,
                                       seed=900 + head_dim)
    q, kc, vc, bt, cu, slk = case
    scale = 1.0 / math.sqrt(head_dim)
    want = ac.ref64_prefill_paged(*case, scale, q_rounding="bf16_prescaled")
    k, v = ac.dense_kv_from_paged(kc, vc, bt, slk)
    got = ops.prefill_attention(*_to_dev(q, k, v, cu), scale, tile_rows=128)
    _assert_rows(f"prefill dense D={head_dim} tile_rows=128", got, want)
