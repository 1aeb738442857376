"""The prefill kernels give the same bits for any tile-table order and for
both dispatch maps (FI_PF_TILE_ORDER).

A tile's arithmetic, its KV order and its online-softmax order do not
depend on where the tile sits in the table or on which workgroup id runs
it, so every comparison here is torch.equal, not a tolerance. Accuracy
against float64 is the business of test_attention_adversarial_gpu.py.
"""

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_cases as ac
import fusioninfer_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
HQ, HK = 8, 2                      # G = 4
# (ctx, new) per sequence of the paged batch
PAGED = [(0, 1), (17, 64), (403, 300), (487, 513), (0, 257)]
DENSE_LENS = [1, 63, 257, 513]
SENTINEL = -65536.0


def setup_module():
    assert ops.has_native(), "HIP extension must be present on a GPU box"


@functools.lru_cache(maxsize=None)
def _paged_case(head_dim, fp8):
    """Scattered (permuted) block ids come with the builder."""
    total = [c + n for c, n in PAGED]
    new = [n for _, n in PAGED]
    case = ac.build_prefill_paged_case(total, new, head_dim, HQ, HK, fp8,
                                       seed=7100 + head_dim + int(fp8))
    return tuple(t.to(DEV) for t in case)


@functools.lru_cache(maxsize=None)
def _dense_case(head_dim):
    case = ac.build_prefill_paged_case(DENSE_LENS, DENSE_LENS, head_dim, HQ,
                                       HK, False, seed=7300 + head_dim)
    q, kc, vc, bt, cu, slk = case
    k, v = ac.dense_kv_from_paged(kc, vc, bt, slk)
    return tuple(t.to(DEV) for t in (q, k, v, cu))


def _tables(new_lens, ctx_starts, rows, seed):
    """name -> (tile_seq, tile_row0): ascending, heaviest first, shuffled."""
    asc = ops.build_prefill_tiles(new_lens, device=DEV, rows=rows,
                                  ctx_starts=ctx_starts, heaviest_first=False)
    heavy = ops.build_prefill_tiles(new_lens, device=DEV, rows=rows,
                                    ctx_starts=ctx_starts,
                                    heaviest_first=True)
    assert not torch.equal(asc[1], heavy[1])
    perm = torch.randperm(asc[0].numel(),
                          generator=torch.Generator().manual_seed(seed))
    perm = perm.to(DEV)
    return {"ascending": asc, "heaviest": heavy,
            "shuffled": (asc[0][perm].contiguous(),
                         asc[1][perm].contiguous())}


def _into_guarded(run, like):
    """run(out) into rows [1, 1+n) of a sentinel buffer; the guard rows
    must survive."""
    n = like.shape[0]
    buf = torch.full((n + 2, *like.shape[1:]), SENTINEL, dtype=like.dtype,
                     device=DEV)
    ret = run(buf[1:n + 1])
    assert ret.data_ptr() == buf[1].data_ptr()
    assert bool((buf[0] == SENTINEL).all())
    assert bool((buf[-1] == SENTINEL).all())
    return buf[1:n + 1]


@pytest.mark.parametrize("rows", [128, 256])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_paged_any_table_order(head_dim, fp8, rows):
    q, kc, vc, bt, cu, slk = _paged_case(head_dim, fp8)
    scale = 1.0 / math.sqrt(head_dim)
    tables = _tables([n for _, n in PAGED], [c for c, _ in PAGED], rows,
                     seed=rows + head_dim)
    outs = {}
    for name, (ts, tr) in tables.items():
        def run(out):
            return ops.prefill_attention_paged(
                q, kc, vc, bt, cu, slk, scale, tile_seq=ts, tile_row0=tr,
                tile_rows=rows, out=out)
        outs[name] = run(None)
        assert torch.equal(_into_guarded(run, q), outs[name]), name
    assert bool(torch.isfinite(outs["ascending"].float()).all())
    assert torch.equal(outs["heaviest"], outs["ascending"])
    assert torch.equal(outs["shuffled"], outs["ascending"])
    # the table the op builds for itself (from seq_lens_k and cu_seqlens_q)
    own = ops.prefill_attention_paged(q, kc, vc, bt, cu, slk, scale,
                                      tile_rows=rows)
    assert torch.equal(own, outs["ascending"])


@pytest.mark.parametrize("rows", [128, 256])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_dense_any_table_order(head_dim, rows):
    q, k, v, cu = _dense_case(head_dim)
    scale = 1.0 / math.sqrt(head_dim)
    tables = _tables(DENSE_LENS, None, rows, seed=3 * rows + head_dim)
    outs = {
        name: ops.prefill_attention(q, k, v, cu, scale, tile_seq=ts,
                                    tile_row0=tr, tile_rows=rows)
        for name, (ts, tr) in tables.items()
    }
    assert bool(torch.isfinite(outs["ascending"].float()).all())
    assert torch.equal(outs["heaviest"], outs["ascending"])
    assert torch.equal(outs["shuffled"], outs["ascending"])
    own = ops.prefill_attention(q, k, v, cu, scale, tile_rows=rows)
    assert torch.equal(own, outs["ascending"])


def _switch_outputs():
    """The seeded cases through the ops' own tables: what the process-wide
    switch decides (table order and dispatch map). name -> uint16 array."""
    res = {}
    for head_dim in (64, 128):
        scale = 1.0 / math.sqrt(head_dim)
        for fp8 in (False, True):
            for rows in (128, 256):
                o = ops.prefill_attention_paged(
                    *_paged_case(head_dim, fp8), scale, tile_rows=rows)
                res[f"paged_d{head_dim}_fp8{int(fp8)}_r{rows}"] = o
        for rows in (128, 256):
            o = ops.prefill_attention(*_dense_case(head_dim), scale,
                                      tile_rows=rows)
            res[f"dense_d{head_dim}_r{rows}"] = o
    return {k: v.view(torch.int16).cpu().numpy() for k, v in res.items()}


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import test_prefill_tile_order_gpu as t
t.setup_module()
assert not t.ops.PF_TILE_ORDER
for name, arr in t._switch_outputs().items():
    np.save(sys.argv[2] + "/" + name + ".npy", arr)
"""


def test_switch_off_same_bits(tmp_path):
    """FI_PF_TILE_ORDER is read once at import, hence one fresh child with
    it off: ascending table, (tile, head) grid with the tile fastest. Its
    outputs must equal this process's, bit for bit."""
    assert ops.PF_TILE_ORDER, "the suite runs with the switch at its default"
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    child = subprocess.run(
        [sys.executable, "-c", _CHILD, tests_dir, str(tmp_path)],
        env={**os.environ, "FI_PF_TILE_ORDER": "0"},
        cwd=os.path.dirname(tests_dir), capture_output=True, text=True,
        timeout=300,
    )
    assert child.returncode == 0, child.stderr[-2000:]
    here = _switch_outputs()
    assert len(here) == 12
    for name, arr in here.items():
        other = np.load(tmp_path / f"{name}.npy")
        assert np.array_equal(arr, other), name
