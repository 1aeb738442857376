"""Row kernels vs float64 on the cases of tests/rowwise_cases.py.

Every call goes to the binding (`ops._C.<op>`) with row slices of
sentinel-filled buffers, so each test also checks that the rows before and
after the ones it was given, and every read-only input, keep their bits.
tests/test_rowwise_cases.py shows on the CPU that the bounds used here are
satisfiable and that the cases catch the defects they were built for.

Each test prints its worst error / bound ratio (pytest -s shows them).
"""

import pytest
import torch

import fusioninfer_amd.ops as ops
import rowwise_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda"
REJECT = (ValueError, RuntimeError)


def setup_module():
    assert ops.has_native(), "HIP extension must be present on a GPU box"


# ------------------------------------------------------------ guarded calls

def _guarded_bf16(rows_cpu):
    """[T, W] bf16 -> ([T+2, W] sentinel-framed GPU buffer, its rows 1..T)."""
    t, w = rows_cpu.shape
    buf = torch.full((t + 2, w), rc.BF16_SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    buf[1:t + 1] = rows_cpu.to(DEV)
    return buf, buf[1:t + 1]


def _guarded_out(t, w, fp8):
    if fp8:
        buf = torch.full((t + 2, w), rc.FP8_SENTINEL, dtype=torch.uint8,
                         device=DEV)
        return buf, buf[1:t + 1].view(torch.float8_e4m3fn)
    buf = torch.full((t + 2, w), rc.BF16_SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    return buf, buf[1:t + 1]


def _bits(t):
    t = t.contiguous()
    if t.dtype == torch.uint8:
        return t
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _assert_guards(buf, what):
    fill = rc.FP8_SENTINEL if buf.dtype == torch.uint8 else rc.BF16_SENTINEL
    want = torch.full_like(buf[0], fill)
    assert torch.equal(_bits(buf[0]), _bits(want)), f"{what}: row before"
    assert torch.equal(_bits(buf[-1]), _bits(want)), f"{what}: row after"


def run_op(case):
    """One guarded launch of case['op']; outputs on the CPU in the layout
    rc.check_case takes (fp8 outputs as uint8 codes)."""
    op = case["op"]
    fp8 = op in rc.FP8_OPS
    x_cpu = case["x"]
    t = x_cpu.shape[0]
    width = x_cpu.shape[1] // 2 if op in rc.SILU_OPS else x_cpu.shape[1]
    what = f"{op}/{case['name']}"

    x_buf, x = _guarded_bf16(x_cpu)
    frames = [("x", x_buf)]
    read_only = []
    if op not in ("fused_add_rms_norm",):
        read_only.append(("x", x_buf, x_buf.clone()))
    w = res = res_buf = None
    if op in rc.NORM_OPS:
        w_buf, w_rows = _guarded_bf16(case["weight"][None, :])
        w = w_rows[0]
        frames.append(("weight", w_buf))
        read_only.append(("weight", w_buf, w_buf.clone()))
    if op in rc.FUSED_OPS:
        res_buf, res = _guarded_bf16(case["residual"])
        frames.append(("residual", res_buf))
    out_buf = out = sc_buf = sc = None
    if op != "fused_add_rms_norm":
        out_buf, out = _guarded_out(t, width, fp8)
        frames.append(("out", out_buf))
    if fp8:
        sc_buf = torch.full((t + 2,), rc.BF16_SENTINEL, dtype=torch.float32,
                            device=DEV)
        sc = sc_buf[1:t + 1]

    C = ops._C
    if op == "rms_norm":
        C.rms_norm(out, x, w, rc.EPS)
    elif op == "fused_add_rms_norm":
        C.fused_add_rms_norm(x, res, w, rc.EPS)
        out_buf, out = x_buf, x
    elif op == "rms_norm_fp8":
        C.rms_norm_fp8(out, sc, x, w, rc.EPS)
    elif op == "fused_add_rms_norm_fp8":
        C.fused_add_rms_norm_fp8(out, sc, x, res, w, rc.EPS)
    elif op == "silu_and_mul":
        C.silu_and_mul(out, x)
    elif op == "silu_and_mul_fp8":
        C.silu_and_mul_fp8(out, sc, x)
    elif op == "quant_fp8_rows":
        C.quant_fp8_rows(out, sc, x)
    else:
        raise AssertionError(op)
    torch.cuda.synchronize()

    for name, buf in frames:
        _assert_guards(buf, f"{what} {name}")
    for name, buf, before in read_only:
        assert torch.equal(_bits(buf), _bits(before)), \
            f"{what}: read-only {name} changed"
    outs = {"out": out_buf[1:t + 1].cpu()}
    if fp8:
        guard = torch.full((), rc.BF16_SENTINEL, dtype=torch.float32)
        assert sc_buf[0].cpu() == guard and sc_buf[-1].cpu() == guard, \
            f"{what}: scale guards"
        outs["scales"] = sc.cpu()
    if res is not None:
        outs["residual"] = res.cpu()
    return outs


def _run_cases(op, width):
    worst = {}
    for case in rc.cases_for(op, width):
        ratios = rc.check_case(case, run_op(case))
        for key, r in ratios.items():
            worst[key] = max(worst.get(key, 0.0), r)
    print(f"\nratio {op} W={width}: " +
          " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------- tests

@pytest.mark.parametrize("width", rc.WIDTHS)
@pytest.mark.parametrize("op", rc.NORM_OPS)
def test_norm(op, width):
    _run_cases(op, width)


@pytest.mark.parametrize("width", rc.WIDTHS)
def test_silu_and_mul(width):
    _run_cases("silu_and_mul", width)


@pytest.mark.parametrize("width", rc.WIDTHS + rc.WIDE_WIDTHS)
@pytest.mark.parametrize("op", rc.QUANT_OPS)
def test_row_quant_fp8(op, width):
    _run_cases(op, width)


@pytest.mark.parametrize("op", rc.QUANT_OPS)
def test_row_quant_fp8_tiny_rows(op):
    case = rc.tiny_row_case(op)
    outs = run_op(case)
    rc.check_case(case, outs)
    assert (outs["scales"] == rc.MIN_SCALE).all()


def test_silu_and_mul_second_grid_stride():
    case = rc.silu_stride_case()
    ratios = rc.check_case(case, run_op(case))
    print(f"\nratio silu_and_mul {case['name']}: bf16={ratios['bf16']:.3f}")


def test_wrappers_agree_with_bindings():
    """The ops.* wrappers allocate the outputs the bindings are given here;
    one case each shows they hand over the same tensors."""
    for op in rc.OPS:
        case = rc.random_case(op, 2056)
        x = case["x"].to(DEV)
        w = case.get("weight")
        w = w.to(DEV) if w is not None else None
        r = case.get("residual")
        r = r.to(DEV) if r is not None else None
        if op == "rms_norm":
            got = {"out": ops.rms_norm(x, w, rc.EPS)}
        elif op == "fused_add_rms_norm":
            o, nr = ops.fused_add_rms_norm(x, r, w, rc.EPS)
            got = {"out": o, "residual": nr}
        elif op == "rms_norm_fp8":
            o, s = ops.rms_norm_fp8(x, w, rc.EPS)
            got = {"out": o, "scales": s}
        elif op == "fused_add_rms_norm_fp8":
            o, s, nr = ops.fused_add_rms_norm_fp8(x, r, w, rc.EPS)
            got = {"out": o, "scales": s, "residual": nr}
        elif op == "silu_and_mul":
            got = {"out": ops.silu_and_mul(x)}
        elif op == "silu_and_mul_fp8":
            o, s = ops.silu_and_mul_fp8(x)
            got = {"out": o, "scales": s}
        else:
            o, s = ops.quant_fp8_rows(x)
            got = {"out": o, "scales": s}
        want = run_op(case)
        for key, val in want.items():
            g = got[key].cpu()
            if g.dtype == torch.float8_e4m3fn:
                g = g.view(torch.uint8)
            assert torch.equal(_bits(g), _bits(val)), (op, key)


# ------------------------------------------------------------- rejections

def _norm_args(width, t=2):
    x = torch.ones(t, width, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(width, dtype=torch.bfloat16, device=DEV)
    return x, w


def _call_norm(op, x, w, out=None, scales=None, residual=None):
    t, width = x.shape
    if residual is None:
        residual = torch.ones_like(x)
    if out is None:
        out = (torch.empty(t, width, dtype=torch.float8_e4m3fn, device=DEV)
               if op in rc.FP8_OPS else torch.empty_like(x))
    if scales is None:
        scales = torch.empty(t, dtype=torch.float32, device=DEV)
    C = ops._C
    if op == "rms_norm":
        C.rms_norm(out, x, w, rc.EPS)
    elif op == "fused_add_rms_norm":
        C.fused_add_rms_norm(x, residual, w, rc.EPS)
    elif op == "rms_norm_fp8":
        C.rms_norm_fp8(out, scales, x, w, rc.EPS)
    else:
        C.fused_add_rms_norm_fp8(out, scales, x, residual, w, rc.EPS)


@pytest.mark.parametrize("op", rc.NORM_OPS)
def test_norm_rejects_bad_arguments(op):
    # widths the kernels cannot serve: not a multiple of 8, above 16384
    for width in (2884, 4, 16392, 18944):
        x, w = _norm_args(width)
        with pytest.raises(REJECT):
            _call_norm(op, x, w)
    x, w = _norm_args(2056)
    bad_weights = [
        w.float(),                                            # dtype
        w[:-8],                                               # too short
        torch.ones(2064, dtype=torch.bfloat16, device=DEV),   # too long
        torch.ones(2 * 2056, dtype=torch.bfloat16, device=DEV)[::2],
        w.cpu(),                                              # device
    ]
    for bad in bad_weights:
        with pytest.raises(REJECT):
            _call_norm(op, x, bad)
    if op in rc.FUSED_OPS:
        with pytest.raises(REJECT):
            _call_norm(op, x, w, residual=torch.ones_like(x)[:1])
    if op == "rms_norm":
        with pytest.raises(REJECT):
            _call_norm(op, x, w, out=torch.empty_like(x)[:1])
        with pytest.raises(REJECT):
            _call_norm(op, x, w, out=torch.empty(2, 2048, dtype=torch.bfloat16,
                                                 device=DEV))
    if op in rc.FP8_OPS:
        f8 = dict(dtype=torch.float8_e4m3fn, device=DEV)
        with pytest.raises(REJECT):
            _call_norm(op, x, w, out=torch.empty(1, 2056, **f8))
        with pytest.raises(REJECT):
            _call_norm(op, x, w, out=torch.empty(2, 2048, **f8))
        with pytest.raises(REJECT):
            _call_norm(op, x, w, out=torch.empty_like(x))
        with pytest.raises(REJECT):
            _call_norm(op, x, w, scales=torch.empty(1, dtype=torch.float32,
                                                    device=DEV))
    # and the same arguments, unbroken, are accepted
    _call_norm(op, x, w)
    torch.cuda.synchronize()


def test_silu_and_quant_reject_bad_arguments():
    C = ops._C
    f8 = dict(dtype=torch.float8_e4m3fn, device=DEV)
    bf = dict(dtype=torch.bfloat16, device=DEV)
    sc = torch.empty(2, dtype=torch.float32, device=DEV)
    x = torch.ones(2, 2 * 264, **bf)
    with pytest.raises(REJECT):       # 2 * 260 columns: I % 8 != 0
        C.silu_and_mul(torch.empty(2, 260, **bf), torch.ones(2, 520, **bf))
    with pytest.raises(REJECT):       # rows do not match
        C.silu_and_mul(torch.empty(1, 264, **bf), x)
    with pytest.raises(REJECT):       # columns do not match
        C.silu_and_mul(torch.empty(2, 256, **bf), x)
    with pytest.raises(REJECT):
        C.silu_and_mul_fp8(torch.empty(2, 260, **f8), sc,
                           torch.ones(2, 520, **bf))
    with pytest.raises(REJECT):
        C.silu_and_mul_fp8(torch.empty(1, 264, **f8), sc, x)
    with pytest.raises(REJECT):
        C.silu_and_mul_fp8(torch.empty(2, 264, **f8), sc[:1], x)
    with pytest.raises(REJECT):       # cols % 8 != 0
        C.quant_fp8_rows(torch.empty(2, 260, **f8), sc,
                         torch.ones(2, 260, **bf))
    with pytest.raises(REJECT):
        C.quant_fp8_rows(torch.empty(2, 256, **f8), sc,
                         torch.ones(2, 264, **bf))
    with pytest.raises(REJECT):
        C.quant_fp8_rows(torch.empty(2, 264, **f8), sc[:1],
                         torch.ones(2, 264, **bf))
    C.silu_and_mul(torch.empty(2, 264, **bf), x)
    C.silu_and_mul_fp8(torch.empty(2, 264, **f8), sc, x)
    C.quant_fp8_rows(torch.empty(2, 264, **f8), sc, torch.ones(2, 264, **bf))
    torch.cuda.synchronize()


@pytest.mark.parametrize("head_dim", [32, 96, 256])
def test_rope_qk_norm_rejects_head_dim(head_dim):
    T, Hq, Hk = 2, 2, 1
    q = torch.ones(T, Hq * head_dim, dtype=torch.bfloat16, device=DEV)
    k = torch.ones(T, Hk * head_dim, dtype=torch.bfloat16, device=DEV)
    cos_sin = torch.ones(4, head_dim, dtype=torch.float32, device=DEV)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    with pytest.raises(REJECT):
        ops.rope_qk_norm_(q, k, pos, cos_sin, Hq, Hk, head_dim)
    with pytest.raises(REJECT):
        ops._C.rope_qk_norm(q, k, None, None, cos_sin, pos, Hq, Hk, head_dim,
                            1e-6)


def test_rope_qk_norm_rejects_bad_shapes():
    T, Hq, Hk, D = 2, 2, 1, 64
    bf = dict(dtype=torch.bfloat16, device=DEV)
    q = torch.ones(T, Hq * D, **bf)
    k = torch.ones(T, Hk * D, **bf)
    cos_sin = torch.ones(4, D, dtype=torch.float32, device=DEV)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    C = ops._C
    with pytest.raises(REJECT):       # q holds one head, two are announced
        C.rope_qk_norm(q[:, :D], k, None, None, cos_sin, pos, Hq, Hk, D, 1e-6)
    with pytest.raises(REJECT):       # weight of the wrong length
        C.rope_qk_norm(q, k, torch.ones(128, **bf), None, cos_sin, pos, Hq,
                       Hk, D, 1e-6)
    with pytest.raises(REJECT):       # weight of the wrong dtype
        C.rope_qk_norm(q, k, torch.ones(D, device=DEV), None, cos_sin, pos,
                       Hq, Hk, D, 1e-6)
    with pytest.raises(REJECT):       # too few positions
        C.rope_qk_norm(q, k, None, None, cos_sin, pos[:1], Hq, Hk, D, 1e-6)
    with pytest.raises(REJECT):       # cos_sin of another head size
        C.rope_qk_norm(q, k, None, None, cos_sin[:, :32].contiguous(), pos,
                       Hq, Hk, D, 1e-6)
    C.rope_qk_norm(q, k, None, None, cos_sin, pos, Hq, Hk, D, 1e-6)
    torch.cuda.synchronize()


def _attn_args(hq, hk, d, t=3):
    bf = dict(dtype=torch.bfloat16, device=DEV)
    q = torch.ones(t, hq, d, **bf)
    k_cache = torch.ones(4, hk, 16, d, **bf)
    tables = torch.tensor([[1], [2], [3]], dtype=torch.int32, device=DEV)[:t]
    lens = torch.ones(t, dtype=torch.int32, device=DEV)
    return q, k_cache, tables, lens


@pytest.mark.parametrize("hq,hk,d", [(28, 4, 128), (6, 2, 128), (3, 4, 128),
                                     (4, 2, 96), (4, 2, 256), (4, 2, 32)])
def test_paged_attention_decode_rejects_group_and_head_dim(hq, hk, d):
    """Hq / Hk outside {1, 2, 4, 8} (7 is Qwen2.5-7B at TP=1) and head sizes
    other than 64 and 128 have no kernel; the launcher used to abort."""
    q, k_cache, tables, lens = _attn_args(hq, hk, d)
    with pytest.raises(REJECT):
        ops.paged_attention_decode(q, k_cache, k_cache.clone(), tables, lens)


@pytest.mark.parametrize("d", [32, 96, 256])
def test_prefill_attention_rejects_head_dim(d):
    q, k_cache, tables, lens = _attn_args(4, 2, d)
    kv = torch.ones(3, 2, d, dtype=torch.bfloat16, device=DEV)
    cu = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=DEV)
    with pytest.raises(REJECT):
        ops.prefill_attention(q, kv, kv.clone(), cu)
    with pytest.raises(REJECT):
        ops.prefill_attention_paged(q, k_cache, k_cache.clone(), tables, cu,
                                    lens)


@pytest.mark.parametrize("op", rc.FP8_OPS)
def test_fp8_wrappers_take_leading_dimensions(op):
    """[2, 3, W] input: one scale per row, shaped [2, 3], and the bits of
    the same rows given as [6, W] (which test_norm / test_row_quant_fp8
    hold to float64)."""
    case = rc.random_case(op, 264)
    case["x"] = torch.cat([case["x"], case["x"].flip(0)])
    if "residual" in case:
        case["residual"] = torch.cat([case["residual"]] * 2)

    def call(shape):
        x = case["x"].to(DEV).view(*shape, -1)
        if op in rc.NORM_OPS:
            w = case["weight"].to(DEV)
            if op in rc.FUSED_OPS:
                r = case["residual"].to(DEV).view(*shape, -1)
                return ops.fused_add_rms_norm_fp8(x, r, w, rc.EPS)[:2]
            return ops.rms_norm_fp8(x, w, rc.EPS)
        if op == "silu_and_mul_fp8":
            return ops.silu_and_mul_fp8(x)
        return ops.quant_fp8_rows(x)

    q2, s2 = call((6,))
    q3, s3 = call((2, 3))
    assert tuple(s3.shape) == (2, 3) and tuple(q3.shape[:2]) == (2, 3)
    assert torch.equal(_bits(s3.cpu().view(6)), _bits(s2.cpu()))
    assert torch.equal(q3.cpu().view(torch.uint8).view(6, -1),
                       q2.cpu().view(torch.uint8))


def test_rope_qk_norm_rejects_other_device_inputs():
    T, Hq, Hk, D = 2, 2, 1, 64
    bf = dict(dtype=torch.bfloat16, device=DEV)
    q, k = torch.ones(T, Hq * D, **bf), torch.ones(T, Hk * D, **bf)
    cos_sin = torch.ones(4, D, dtype=torch.float32, device=DEV)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    C = ops._C
    for bad in ((q, k.cpu(), cos_sin, pos), (q, k, cos_sin.cpu(), pos),
                (q, k, cos_sin, pos.cpu())):
        with pytest.raises(REJECT):
            C.rope_qk_norm(bad[0], bad[1], None, None, bad[2], bad[3], Hq, Hk,
                           D, 1e-6)
    if torch.cuda.device_count() > 1:
        with pytest.raises(REJECT):
            C.rope_qk_norm(q, k, None, None, cos_sin.to("cuda:1"), pos, Hq,
                           Hk, D, 1e-6)


# -------------------------------------------------------------------- rope

def _qkv_frame(q3, k3):
    """[T+2, (Hq + 2 Hk) D] sentinel buffer holding q | k | V = sentinel in
    rows 1..T; returns (buffer, q rows, k rows)."""
    t, hq, d = q3.shape
    hk = k3.shape[1]
    buf = torch.full((t + 2, (hq + 2 * hk) * d), rc.BF16_SENTINEL,
                     dtype=torch.bfloat16, device=DEV)
    buf[1:t + 1, : hq * d] = q3.reshape(t, -1).to(DEV)
    buf[1:t + 1, hq * d: (hq + hk) * d] = k3.reshape(t, -1).to(DEV)
    return buf, buf[1:t + 1, : hq * d], buf[1:t + 1, hq * d: (hq + hk) * d]


def _assert_qkv_frame(buf, hq, hk, d):
    sentinel = torch.full((), rc.BF16_SENTINEL, dtype=torch.bfloat16,
                          device=DEV)
    assert (buf[0] == sentinel).all() and (buf[-1] == sentinel).all()
    assert (buf[:, (hq + hk) * d:] == sentinel).all(), "V columns written"


@pytest.mark.parametrize("head_dim", [64, 128])
def test_rope_position_zero_is_identity(head_dim):
    T, Hq, Hk, P = 5, 6, 2, 64
    g = torch.Generator().manual_seed(head_dim)
    q3 = torch.randn(T, Hq, head_dim, generator=g).to(torch.bfloat16)
    k3 = torch.randn(T, Hk, head_dim, generator=g).to(torch.bfloat16)
    cos_sin = ops.compute_cos_sin_cache(head_dim, P, 10000.0)
    assert (cos_sin[0, : head_dim // 2] == 1).all()
    assert (cos_sin[0, head_dim // 2:] == 0).all()
    buf, q, k = _qkv_frame(q3, k3)
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    ops.rope_qk_norm_(q, k, pos, cos_sin.to(DEV), Hq, Hk, head_dim)
    torch.cuda.synchronize()
    assert torch.equal(_bits(q.cpu()), _bits(q3.reshape(T, -1)))
    assert torch.equal(_bits(k.cpu()), _bits(k3.reshape(T, -1)))
    _assert_qkv_frame(buf, Hq, Hk, head_dim)


@pytest.mark.parametrize("qk_norm", [False, True])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_rope_qk_norm_against_float64(head_dim, qk_norm):
    T, Hq, Hk, P = 7, 6, 2, 512
    pos_cpu = torch.tensor([P - 1, 0, 1, 17, 255, P - 2, 300],
                           dtype=torch.int32)
    cos_sin = ops.compute_cos_sin_cache(head_dim, P, 10000.0).cpu()
    g = torch.Generator().manual_seed(3)
    qw = kw = None
    if qk_norm:
        qw = (1.0 + 0.5 * torch.randn(head_dim, generator=g)).to(torch.bfloat16)
        kw = (1.0 + 0.5 * torch.randn(head_dim, generator=g)).to(torch.bfloat16)
    q3 = rc.rope_inputs(T, Hq, head_dim, pos_cpu, cos_sin, qw, seed=11)
    k3 = rc.rope_inputs(T, Hk, head_dim, pos_cpu, cos_sin, kw, seed=12)
    buf, q, k = _qkv_frame(q3, k3)
    ops.rope_qk_norm_(
        q, k, pos_cpu.to(DEV), cos_sin.to(DEV), Hq, Hk, head_dim,
        qw.to(DEV) if qk_norm else None, kw.to(DEV) if qk_norm else None,
        rc.EPS)
    torch.cuda.synchronize()
    rq = rc.check_bf16(q.cpu().view(T, Hq, head_dim),
                       rc.rope64(q3, pos_cpu, cos_sin, qw), "rope q")
    rk = rc.check_bf16(k.cpu().view(T, Hk, head_dim),
                       rc.rope64(k3, pos_cpu, cos_sin, kw), "rope k")
    print(f"\nratio rope_qk_norm D={head_dim} norm={qk_norm}: "
          f"q={rq:.3f} k={rk:.3f}")
    _assert_qkv_frame(buf, Hq, Hk, head_dim)


# ------------------------------------------------------------------- cache

def test_reshape_and_cache_second_grid_stride():
    case = rc.cache_case()
    shape = (case["nblocks"], case["kv_heads"], case["block"],
             case["head_dim"])
    k_ref = torch.full(shape, rc.BF16_SENTINEL, dtype=torch.bfloat16)
    v_ref = k_ref.clone()
    rc.cache_reference(case, k_ref, v_ref)
    k_cache = torch.full(shape, rc.BF16_SENTINEL, dtype=torch.bfloat16,
                         device=DEV)
    v_cache = k_cache.clone()
    k, v = case["k"].to(DEV), case["v"].to(DEV)
    ops.reshape_and_cache(k, v, k_cache, v_cache, case["slots"].to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(_bits(k_cache.cpu()), _bits(k_ref))
    assert torch.equal(_bits(v_cache.cpu()), _bits(v_ref))
    # most of the cache was written, the unowned slots were not
    sentinel = torch.full((), rc.BF16_SENTINEL, dtype=torch.bfloat16)
    untouched = (k_ref == sentinel).all(dim=-1).all(dim=1)   # [B, block]
    assert untouched.sum() == shape[0] * shape[2] - (case["tokens"] - 4)
    assert torch.equal(_bits(k.cpu()), _bits(case["k"]))
    assert torch.equal(_bits(v.cpu()), _bits(case["v"]))
