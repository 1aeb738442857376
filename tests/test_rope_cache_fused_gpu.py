"""ops.rope_qk_norm_cache_ against the two kernels it replaces.

The fused op must give, bit for bit, what ops.rope_qk_norm_ followed by
ops.reshape_and_cache give: the same q, the same k_cache and v_cache
(fp8 caches compared as raw bytes). Both paths run on copies of one set
of inputs built like the model's: q, k and v are column slices of one
[T, (Hq + 2 Hk) * D] buffer.

Padding rows: three slots are -1 at T = 33. At T = 3 only one is, since
three would leave that case (the 48-head Qwen3-8B layout) without a single
cache write to compare.
"""

import pytest
import torch

import fusioninfer_amd.ops as ops
from fusioninfer_amd.ops import reference as ref
from tests.test_ops_gpu import assert_close_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda"
NBLOCKS, BS = 12, 16
BF16_SENTINEL = -7.0   # exactly representable, far from N(0, 1) data
FP8_SENTINEL = 0x5A    # raw byte


def setup_module():
    assert ops.has_native(), "HIP extension must be present on a GPU box"


def _caches(Hk, D, fp8):
    shape = (NBLOCKS, Hk, BS, D)
    if fp8:
        mk = lambda: torch.full(shape, FP8_SENTINEL, dtype=torch.uint8,
                                device=DEV).view(torch.float8_e4m3fn)
    else:
        mk = lambda: torch.full(shape, BF16_SENTINEL, dtype=torch.bfloat16,
                                device=DEV)
    return mk(), mk()


def _raw(cache):
    """Bit view of a cache: bytes for fp8, int16 for bf16."""
    if cache.dtype == torch.float8_e4m3fn:
        return cache.view(torch.uint8)
    return cache.view(torch.int16)


def _inputs(T, Hq, Hk, D, qk_norm, fp8, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(T, (Hq + 2 * Hk) * D, generator=g).to(torch.bfloat16)
    if fp8:  # out-of-range V rows: the +-448 clamp must run
        vcols = slice((Hq + Hk) * D, None)
        qkv[0, vcols] *= 2000
        qkv[T - 1, vcols] *= 2000
    positions = torch.randint(0, 500, (T,), generator=g, dtype=torch.int32)
    slots = torch.randperm(NBLOCKS * BS, generator=g)[:T].to(torch.int32)
    pad_rows = [1, T // 2, T - 2] if T > 3 else [1]
    slots[pad_rows] = -1
    qw = kw = None
    if qk_norm:
        qw = torch.randn(D, generator=g).to(torch.bfloat16).to(DEV)
        kw = torch.randn(D, generator=g).to(torch.bfloat16).to(DEV)
    cos_sin = ops.compute_cos_sin_cache(D, 512, 10000.0).to(DEV)
    return (qkv.to(DEV), positions.to(DEV), slots.to(DEV), pad_rows, qw, kw,
            cos_sin)


def _split(qkv, Hq, Hk, D):
    return (qkv[:, : Hq * D], qkv[:, Hq * D : (Hq + Hk) * D],
            qkv[:, (Hq + Hk) * D :])


@pytest.mark.parametrize("shape", [(33, 8, 2), (3, 32, 8)])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("qk_norm", [True, False], ids=["norm", "nonorm"])
@pytest.mark.parametrize("D", [64, 128])
def test_fused_equals_pair(D, qk_norm, fp8, shape):
    T, Hq, Hk = shape
    qkv, positions, slots, pad_rows, qw, kw, cos_sin = _inputs(
        T, Hq, Hk, D, qk_norm, fp8, seed=11)
    k_inv, v_inv = (1.0 / 3.0, 1.0 / 4.0) if fp8 else (1.0, 1.0)

    # the existing pair
    qkv_a = qkv.clone()
    qa, ka, va = _split(qkv_a, Hq, Hk, D)
    kc_a, vc_a = _caches(Hk, D, fp8)
    ops.rope_qk_norm_(qa, ka, positions, cos_sin, Hq, Hk, D, qw, kw, 1e-6)
    ops.reshape_and_cache(ka, va, kc_a, vc_a, slots, k_inv, v_inv)

    # the fused op
    qkv_b = qkv.clone()
    qb, kb, vb = _split(qkv_b, Hq, Hk, D)
    kc_b, vc_b = _caches(Hk, D, fp8)
    ret = ops.rope_qk_norm_cache_(
        qb, kb, vb, positions, cos_sin, Hq, Hk, D, kc_b, vc_b, slots,
        qw, kw, 1e-6, k_inv, v_inv)
    assert ret is qb

    assert torch.equal(qb, qa)
    assert torch.equal(_raw(kc_b), _raw(kc_a))
    assert torch.equal(_raw(vc_b), _raw(vc_a))
    # v is read only
    assert torch.equal(vb, _split(qkv, Hq, Hk, D)[2])

    # q rows of padding tokens are processed like any other
    assert not torch.equal(qb[pad_rows], _split(qkv, Hq, Hk, D)[0][pad_rows])

    # only the slots of non-padding tokens were written
    written = torch.zeros(NBLOCKS * BS, dtype=torch.bool, device=DEV)
    written[slots[slots >= 0].long()] = True
    assert int(written.sum()) == T - len(pad_rows)
    sentinel = (FP8_SENTINEL if fp8 else
                torch.tensor(BF16_SENTINEL, dtype=torch.bfloat16)
                .view(torch.int16).item())
    for cache in (kc_b, vc_b):
        # [B, Hk, 16, D] -> [B*16 slots, Hk, D]
        by_slot = _raw(cache).permute(0, 2, 1, 3).reshape(NBLOCKS * BS, Hk, D)
        assert (by_slot[~written] == sentinel).all()
        # a written row holding nothing but the sentinel would be a miss
        assert (by_slot[written] != sentinel).any(dim=-1).all()

    if fp8:  # e4m3fn NaN is S.1111.111
        for cache in (kc_b, vc_b):
            assert ((_raw(cache) & 0x7F) != 0x7F).all()
        # and the clamp did run: some V bytes sit at +-448 (0x7E / 0xFE)
        assert ((_raw(vc_b) & 0x7F) == 0x7E).any()


def test_fused_vs_reference():
    """Ties the fused op to ops/reference.py, not only to the old kernels."""
    T, Hq, Hk, D = 33, 8, 2, 128
    qkv, positions, slots, pad_rows, qw, kw, cos_sin = _inputs(
        T, Hq, Hk, D, True, False, seed=12)
    q, k, v = _split(qkv.clone(), Hq, Hk, D)
    q_ref, k_ref = ref.rope_qk_norm(
        q.cpu().view(T, Hq, D), k.cpu().view(T, Hk, D), positions.cpu().long(),
        cos_sin.cpu(), qw.cpu(), kw.cpu(), 1e-6)
    keep = (slots >= 0).cpu()
    kc_ref = torch.full((NBLOCKS, Hk, BS, D), BF16_SENTINEL,
                        dtype=torch.bfloat16)
    vc_ref = kc_ref.clone()
    ref.reshape_and_cache(
        k_ref[keep], v.cpu().view(T, Hk, D)[keep], kc_ref, vc_ref,
        slots.cpu()[keep].long())

    kc, vc = _caches(Hk, D, False)
    ops.rope_qk_norm_cache_(q, k, v, positions, cos_sin, Hq, Hk, D, kc, vc,
                            slots, qw, kw, 1e-6)
    assert_close_bf16(q.cpu().view(T, Hq, D), q_ref)
    assert_close_bf16(kc.cpu(), kc_ref)
    assert torch.equal(vc.cpu(), vc_ref)


def test_unsupported_inputs_raise():
    T, Hq, Hk = 4, 2, 1
    positions = torch.zeros(T, dtype=torch.int32, device=DEV)
    slots = torch.arange(T, dtype=torch.int32, device=DEV)

    def call(D, bs):
        qkv = torch.zeros(T, (Hq + 2 * Hk) * D, dtype=torch.bfloat16,
                          device=DEV)
        q, k, v = _split(qkv, Hq, Hk, D)
        kc = torch.zeros(2, Hk, bs, D, dtype=torch.bfloat16, device=DEV)
        cos_sin = torch.zeros(8, D, dtype=torch.float32, device=DEV)
        ops.rope_qk_norm_cache_(q, k, v, positions, cos_sin, Hq, Hk, D, kc,
                                torch.zeros_like(kc), slots)

    call(128, 16)  # the supported neighbour of both cases passes
    with pytest.raises((ValueError, RuntimeError)):
        call(96, 16)
    with pytest.raises((ValueError, RuntimeError)):
        call(128, 32)
