"""`out=` of ops.paged_attention_decode and ops.prefill_attention_paged.

The model hands each op its rows of one [T, Hq*D] buffer. Writing there
must give exactly what the allocating call returns and touch nothing
outside the slice.
"""

import pytest
import torch

import fusioninfer_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
Hq, Hk, D, BS = 8, 2, 128, 16
SENTINEL = -7.0


def setup_module():
    assert ops.has_native(), "HIP extension must be present on a GPU box"


def _cache_and_tables(ctx_lens, seed):
    torch.manual_seed(seed)
    nblk = [(c + BS - 1) // BS for c in ctx_lens]
    k_cache = torch.randn(sum(nblk) + 1, Hk, BS, D, dtype=torch.bfloat16,
                          device=DEV)
    v_cache = torch.randn_like(k_cache)
    bt = torch.zeros(len(ctx_lens), max(nblk), dtype=torch.int32, device=DEV)
    nxt = 1
    for s, n in enumerate(nblk):
        bt[s, :n] = torch.arange(nxt, nxt + n, dtype=torch.int32)
        nxt += n
    lens = torch.tensor(ctx_lens, dtype=torch.int32, device=DEV)
    return k_cache, v_cache, bt, lens


def _check_into_slice(n, run):
    """run(out) with out=None allocates; with out = rows [2, 2+n) of a
    larger sentinel buffer it must write the same bits there and only
    there."""
    expected = run(None)
    assert expected.shape == (n, Hq, D)
    buf = torch.full((n + 5, Hq * D), SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    out = buf[2 : 2 + n].view(n, Hq, D)
    got = run(out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(buf[2 : 2 + n].view(n, Hq, D), expected)
    assert (buf[:2] == SENTINEL).all() and (buf[2 + n :] == SENTINEL).all()
    return buf


def test_decode_out():
    ctx_lens = [1, 40, 600]  # 600 tokens: two 512-token partitions
    k_cache, v_cache, bt, lens = _cache_and_tables(ctx_lens, seed=21)
    S = len(ctx_lens)
    assert bt.shape[1] * BS > ops.DECODE_PARTITION_TOKENS
    q = torch.randn(S, Hq, D, dtype=torch.bfloat16, device=DEV)

    def run(out):
        return ops.paged_attention_decode(q, k_cache, v_cache, bt, lens,
                                          out=out)

    buf = _check_into_slice(S, run)
    # a column slice of the buffer has the right shape but is not dense
    wide = torch.empty(S, 2 * Hq * D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        run(wide[:, : Hq * D].view(S, Hq, D))
    with pytest.raises((ValueError, RuntimeError)):
        run(buf[:S])  # wrong shape


def test_prefill_paged_out():
    new_lens, ctx_lens = [5, 33], [5, 50]
    k_cache, v_cache, bt, lens_k = _cache_and_tables(ctx_lens, seed=22)
    Tn = sum(new_lens)
    q = torch.randn(Tn, Hq, D, dtype=torch.bfloat16, device=DEV)
    cu_q = torch.tensor([0, 5, 38], dtype=torch.int32, device=DEV)

    def run(out):
        return ops.prefill_attention_paged(q, k_cache, v_cache, bt, cu_q,
                                           lens_k, out=out)

    _check_into_slice(Tn, run)
    wide = torch.empty(Tn, 2 * Hq * D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        run(wide[:, : Hq * D].view(Tn, Hq, D))
