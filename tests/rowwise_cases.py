"""Inputs, float64 oracles and checkers for the row kernels (helper, no tests).

The row kernels (rms_norm, fused_add_rms_norm, their fp8 variants,
silu_and_mul, silu_and_mul_fp8, quant_fp8_rows) are compared with float64
arithmetic on the bf16 inputs. `ops.reference` is not the oracle: it rounds
through bf16 before quantising and the kernels do not.

Three kinds of case:

* random: heavy-tailed rows (randn times per-column powers of two over 12
  binades, row magnitudes 1e-3 / 1 / 1e2, gates across [-100, 100]) checked
  with the bounds below;
* exact: inputs on which every fp32 step of a correct kernel is exact, so
  the expected bits are known and compared bitwise;
* needle: rows whose sum of squares or absmax lives in one or two columns
  at wave and iteration edges, so a reduction that loses a contribution is
  off by a large factor.

Bounds (derivations in docs/kernels.md, "Row-kernel test bounds"):

* bf16 outputs: |got - want| <= 2^-8 |want| + 1e-30 per element;
* fp8 outputs, per row with scale s and float64 result y:
    1. |s - max|y|/448| <= 2^-16 max|y|/448 (rows with amax < 1e-8:
       s == fp32(1e-8)/448);
    2. |q s - y| <= (0.5 ulp8(z) + 2^-15 |z|) s with z = y/s;
    3. the byte at the row's argmax is 0x7E or 0xFE, no byte is 0x7F / 0xFF.

`emulate` is a float32 model of what the kernels compute (unrounded before
quantisation) with switchable defects; tests/test_rowwise_cases.py holds it
to the checkers and checks that every defect is caught. Nothing here
imports or inspects a kernel.
"""

from __future__ import annotations

import torch

EPS = 1e-6
FP8_MAX = 448.0
ITER_COLS = 2048          # 256 lanes x 8 columns per kernel iteration
WAVE_COLS = 512           # 64 lanes x 8 columns

WIDTHS = [8, 264, 2048, 2056, 3584, 5120, 6152, 8192, 10232, 12288, 14336,
          16384]
WIDE_WIDTHS = [16392, 18944, 28672]   # quant.hip's two-pass kernel

NORM_OPS = ("rms_norm", "fused_add_rms_norm", "rms_norm_fp8",
            "fused_add_rms_norm_fp8")
QUANT_OPS = ("silu_and_mul_fp8", "quant_fp8_rows")
OPS = NORM_OPS + ("silu_and_mul",) + QUANT_OPS
FP8_OPS = ("rms_norm_fp8", "fused_add_rms_norm_fp8") + QUANT_OPS
FUSED_OPS = ("fused_add_rms_norm", "fused_add_rms_norm_fp8")
SILU_OPS = ("silu_and_mul", "silu_and_mul_fp8")

BF16_REL = 2.0 ** -8
BF16_ABS = 1e-30
SCALE_REL = 2.0 ** -16
FP8_REL = 2.0 ** -15
MIN_SCALE = float(torch.tensor(1e-8, dtype=torch.float32)
                  / torch.tensor(448.0, dtype=torch.float32))

BF16_SENTINEL = -7.0
FP8_SENTINEL = 0x5A

MUTANTS = ("swap_bytes", "swap_words", "drop_wave", "skip_partial",
           "scale_from_bf16", "swap_gate_up", "prev_row_scale")


def widths_for(op):
    return WIDTHS + (WIDE_WIDTHS if op in QUANT_OPS else [])


# ------------------------------------------------------------------ e4m3

def _e4m3_table():
    b = torch.arange(256, dtype=torch.uint8)
    v = b.view(torch.float8_e4m3fn).to(torch.float64)
    return b, v


_ALL_BYTES, _ALL_VALUES = _e4m3_table()
# every finite code but -0 (0x80); 0x7F and 0xFF are the NaNs
E4M3_BYTES = torch.tensor(
    [b for b in range(256) if b not in (0x7F, 0x80, 0xFF)], dtype=torch.uint8)
E4M3_NONZERO_BYTES = E4M3_BYTES[E4M3_BYTES != 0]


def e4m3_decode(bytes_u8: torch.Tensor) -> torch.Tensor:
    """uint8 codes -> float64 values."""
    return _ALL_VALUES[bytes_u8.long()]


def ulp8(z: torch.Tensor) -> torch.Tensor:
    """Spacing of e4m3 around |z| (float64), evaluated at |z|(1 + 2^-15) so
    that a binade edge takes the larger spacing."""
    a = z.abs() * (1.0 + FP8_REL)
    e = torch.floor(torch.log2(a.clamp(min=2.0 ** -20))).clamp(min=-6.0)
    return torch.exp2(e - 3.0)


# ----------------------------------------------------------------- oracles

def rms_norm64(x64, w64, eps=EPS):
    inv = torch.rsqrt((x64 * x64).mean(dim=-1, keepdim=True) + eps)
    return x64 * inv * w64


def silu_mul64(gu64):
    inter = gu64.shape[-1] // 2
    g, u = gu64[..., :inter], gu64[..., inter:]
    return g / (1.0 + torch.exp(-g)) * u


def oracle(case):
    """float64 result of the op on the case's bf16 inputs: (y, new_residual
    or None)."""
    if "_oracle" in case:
        return case["_oracle"]
    op = case["op"]
    x = case["x"].to(torch.float64)
    res = None
    if op in NORM_OPS:
        if op in FUSED_OPS:
            res = x + case["residual"].to(torch.float64)
            x = res
        y = rms_norm64(x, case["weight"].to(torch.float64))
    elif op in SILU_OPS:
        y = silu_mul64(x)
    else:
        y = x
    case["_oracle"] = (y, res)
    return y, res


def rope64(x, positions, cos_sin, weight=None, eps=EPS):
    """NeoX rotary embedding after an optional per-head RMSNorm, float64.
    x [T, H, D] bf16, positions [T], cos_sin [P, D] fp32 (cos | sin)."""
    x = x.to(torch.float64)
    d = x.shape[-1]
    if weight is not None:
        x = rms_norm64(x, weight.to(torch.float64), eps)
    cs = cos_sin.to(torch.float64)[positions.long()]
    c, s = cs[:, None, : d // 2], cs[:, None, d // 2:]
    x1, x2 = x[..., : d // 2], x[..., d // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rope_cancellation(x, positions, cos_sin, weight=None, eps=EPS):
    """|result| / (|term 1| + |term 2|) per element of rope64."""
    x = x.to(torch.float64)
    d = x.shape[-1]
    if weight is not None:
        x = rms_norm64(x, weight.to(torch.float64), eps)
    cs = cos_sin.to(torch.float64)[positions.long()]
    c, s = cs[:, None, : d // 2], cs[:, None, d // 2:]
    x1, x2 = x[..., : d // 2], x[..., d // 2:]
    num = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).abs()
    den = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                     (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return num / den.clamp(min=1e-300)


def rope_inputs(tokens, heads, head_dim, positions, cos_sin, weight, seed):
    """[T, heads, D] bf16 randn whose rotary terms never cancel beyond 2^6.

    The 2^-8 relative bound leaves 2^-9 for the fp32 arithmetic, whose error
    is about 2^-22 of the larger TERM; a result 2^13 times smaller than its
    terms would eat that, and among thousands of random elements a few are.
    Elements that cancel beyond 2^6 are drawn again (with their rotary
    partner); this looks only at the inputs and the float64 result."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(tokens, heads, head_dim, generator=g).to(torch.bfloat16)
    for _ in range(50):
        bad = rope_cancellation(x, positions, cos_sin, weight) < 2.0 ** -6
        if not bad.any():
            return x
        half = head_dim // 2
        bad = bad[..., :half] | bad[..., half:]
        bad = torch.cat([bad, bad], dim=-1)
        fresh = torch.randn(x.shape, generator=g).to(torch.bfloat16)
        x = torch.where(bad, fresh, x)
    raise AssertionError("rope_inputs did not converge")


# ---------------------------------------------------------------- checkers

def bits16(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def check_bf16(got: torch.Tensor, want64: torch.Tensor, what="") -> float:
    """|got - want| <= 2^-8 |want| + 1e-30 per element; returns the worst
    error / bound ratio."""
    got64 = got.to(torch.float64)
    assert torch.isfinite(got64).all(), f"{what}: non-finite output"
    bound = BF16_REL * want64.abs() + BF16_ABS
    ratio = ((got64 - want64).abs() / bound).max().item()
    assert ratio <= 1.0, f"{what}: bf16 error / bound = {ratio:.3f}"
    return ratio


def check_fp8(q_bytes: torch.Tensor, scales: torch.Tensor, y64: torch.Tensor,
              what="") -> dict:
    """The three per-row fp8 checks; returns the worst error / bound ratios."""
    assert q_bytes.dtype == torch.uint8 and scales.dtype == torch.float32
    assert q_bytes.shape == y64.shape and scales.shape == y64.shape[:1]
    # 3a. no NaN byte anywhere
    nan = (q_bytes == 0x7F) | (q_bytes == 0xFF)
    assert not nan.any(), f"{what}: {int(nan.sum())} NaN bytes"
    amax = y64.abs().amax(dim=-1)
    s = scales.to(torch.float64)
    # 1. the scale
    tiny = amax < 1e-8
    want_s = torch.where(tiny, torch.full_like(amax, MIN_SCALE), amax / FP8_MAX)
    s_err = (s - want_s).abs()
    assert (s_err[tiny] == 0).all(), f"{what}: tiny rows need s = 1e-8/448"
    s_ratio = (s_err / (SCALE_REL * want_s)).max().item()
    assert s_ratio <= 1.0, f"{what}: scale error / bound = {s_ratio:.3f}"
    # 2. the elements
    sc = s[:, None]
    z = y64 / sc
    bound = (0.5 * ulp8(z) + FP8_REL * z.abs()) * sc
    e_ratio = ((e4m3_decode(q_bytes) * sc - y64).abs() / bound).max().item()
    assert e_ratio <= 1.0, f"{what}: fp8 error / bound = {e_ratio:.3f}"
    # 3b. the row maximum maps to +-448
    live = ~tiny
    arg = y64.abs().argmax(dim=-1)
    top = q_bytes.gather(1, arg[:, None])[:, 0] & 0x7F
    assert (top[live] == 0x7E).all(), f"{what}: argmax byte is not +-448"
    return {"scale": s_ratio, "elem": e_ratio}


def check_case(case, outs) -> dict:
    """Hold the outputs of one op to every check its case defines. `outs`:
    'out' (bf16, or uint8 e4m3 codes), 'scales' (fp32) and 'residual' (bf16)
    where the op has them. Returns the worst error / bound ratios."""
    op, what = case["op"], f"{case['op']}/{case['name']}"
    y, res = oracle(case)
    ratios = {}
    if op in FP8_OPS:
        ratios.update(check_fp8(outs["out"], outs["scales"], y, what))
    else:
        ratios["bf16"] = check_bf16(outs["out"], y, what)
    if op in FUSED_OPS:
        ratios["residual"] = check_bf16(outs["residual"], res,
                                        what + " residual")
    exact = case.get("exact", {})
    if "out_bits" in exact:
        assert torch.equal(bits16(outs["out"]), exact["out_bits"]), \
            f"{what}: output bits differ"
    if "out_bytes" in exact:
        assert torch.equal(outs["out"], exact["out_bytes"]), \
            f"{what}: fp8 bytes differ"
    if "scales" in exact:
        assert torch.equal(outs["scales"], exact["scales"]), \
            f"{what}: scales differ"
    if "residual_bits" in exact:
        assert torch.equal(bits16(outs["residual"]), exact["residual_bits"]), \
            f"{what}: residual bits differ"
    for r, cols in enumerate(case.get("needles", [])):
        mask = torch.zeros(y.shape[1], dtype=torch.bool)
        mask[cols] = True
        if op in FP8_OPS:
            assert (outs["out"][r][mask] == 0x7E).all(), \
                f"{what}: row {r} needle byte is not 0x7E"
        if case["kind"] == "needle_sumsq":
            rest = outs["out"][r][~mask]
            zero = (rest & 0x7F) == 0 if op in FP8_OPS else rest.float() == 0
            assert zero.all(), f"{what}: row {r} has a nonzero off the needle"
    return ratios


# ------------------------------------------------------------------- cases

def _seed(op, kind, width):
    return OPS.index(op) * 1000003 + width * 31 + sum(map(ord, kind))


def _heavy(rows, cols, g):
    """randn times per-column powers of two over 12 binades, float32."""
    k = torch.randint(-6, 6, (cols,), generator=g).to(torch.float32)
    return torch.randn(rows, cols, generator=g) * torch.exp2(k)


ROW_MAGS = (1e-3, 1.0, 1e2)


def random_case(op, width):
    g = torch.Generator().manual_seed(_seed(op, "random", width))
    mags = torch.tensor(ROW_MAGS)[:, None]
    t = len(ROW_MAGS)
    case = {"op": op, "kind": "random", "name": f"random-{width}"}
    if op in SILU_OPS:
        gate = (torch.rand(t, width, generator=g) * 200.0 - 100.0)
        # a third of the gates near zero, where silu is not ~ identity or 0
        near = torch.rand(t, width, generator=g) < 1 / 3
        gate = torch.where(near, gate / 25.0, gate)
        gate[:, 0] = torch.tensor([-100.0, 100.0, -88.0])
        up = _heavy(t, width, g) * mags
        case["x"] = torch.cat([gate, up], dim=1).to(torch.bfloat16)
        return case
    case["x"] = (_heavy(t, width, g) * mags).to(torch.bfloat16)
    if op in NORM_OPS:
        case["weight"] = _heavy(1, width, g)[0].to(torch.bfloat16)
    if op in FUSED_OPS:
        case["residual"] = (_heavy(t, width, g) * mags).to(torch.bfloat16)
    return case


def _sign_pattern(rows, width):
    c = torch.arange(width)
    r = torch.arange(rows)[:, None]
    return torch.where(((c * 5 + c // 8 + c // ITER_COLS + r) % 3) == 0,
                       -1.0, 1.0)


def _int_code(rows, width):
    """bf16-exact integers in [-127, 127] that differ between a column and
    its neighbours 4, 8, 256 and 2048 columns away and between rows."""
    c = torch.arange(width)
    r = torch.arange(rows)[:, None]
    return ((r * 89 + c + (c // 256) * 37 + (c // ITER_COLS) * 11) % 255
            - 127).to(torch.float32)


def _e4m3_draw(rows, width, g, table=E4M3_BYTES):
    """Random e4m3 codes with one +-448 planted per row at a column that
    varies with the row."""
    b = table[torch.randint(0, len(table), (rows, width), generator=g)]
    for r in range(rows):
        b[r, (37 + r * 2051) % width] = 0x7E if r % 2 == 0 else 0xFE
    return b


EXACT_K = (-20, -7, 0, 9, 20)   # quant_fp8_rows: row r is z * 2^k[r]
EXACT_A = (0, 3, 7)             # norm rows: |x| = 2^a[r]


def exact_case(op, width):
    g = torch.Generator().manual_seed(_seed(op, "exact", width))
    case = {"op": op, "kind": "exact", "name": f"exact-{width}"}
    if op == "quant_fp8_rows":
        t = len(EXACT_K)
        zb = _e4m3_draw(t, width, g)
        k = torch.tensor(EXACT_K, dtype=torch.float64)[:, None]
        x = (e4m3_decode(zb) * torch.exp2(k)).to(torch.bfloat16)
        assert torch.equal(x.to(torch.float64), e4m3_decode(zb) * torch.exp2(k))
        case["x"] = x
        case["exact"] = {"out_bytes": zb,
                         "scales": torch.exp2(k[:, 0]).to(torch.float32)}
    elif op in SILU_OPS:
        t = 3
        gate = torch.full((t, width), 64.0)
        if op == "silu_and_mul":
            up = _int_code(t, width)
            case["exact"] = {
                "out_bits": bits16((64.0 * up).to(torch.bfloat16))}
        else:
            zb = _e4m3_draw(t, width, g)
            up = e4m3_decode(zb).to(torch.float32)
            case["exact"] = {"out_bytes": zb,
                             "scales": torch.full((t,), 64.0)}
        case["x"] = torch.cat([gate, up], dim=1).to(torch.bfloat16)
        assert torch.equal(case["x"][:, width:].float(), up)
    else:
        t = len(EXACT_A)
        sign = _sign_pattern(t, width)
        mag = torch.exp2(torch.tensor(EXACT_A, dtype=torch.float32))[:, None]
        x = sign * mag
        exact = {}
        if op in FP8_OPS:
            # nonzero codes: sign * 0 would ask for a -0 byte
            wb = _e4m3_draw(1, width, g, E4M3_NONZERO_BYTES)[0]
            w = e4m3_decode(wb).to(torch.float32)
            want = (sign * w).to(torch.float8_e4m3fn).view(torch.uint8)
            assert torch.equal(e4m3_decode(want),
                               (sign * w).to(torch.float64))
            exact["out_bytes"] = want
        else:
            w = _int_code(1, width)[0]
            exact["out_bits"] = bits16((sign * w).to(torch.bfloat16))
        case["weight"] = w.to(torch.bfloat16)
        assert torch.equal(case["weight"].float(), w)
        if op in FUSED_OPS:
            case["x"] = (0.75 * x).to(torch.bfloat16)
            case["residual"] = (0.25 * x).to(torch.bfloat16)
            exact["residual_bits"] = bits16(x.to(torch.bfloat16))
        else:
            case["x"] = x.to(torch.bfloat16)
        case["exact"] = exact
    return case


def needle_columns(width):
    """Single-needle columns, then pairs in two waves / two iterations."""
    cols = [0, 7, 8, 511, 512, 2047, 2048, width - 8, width - 1]
    if width % ITER_COLS:
        cols += [(width // ITER_COLS) * ITER_COLS, width - 1]
    singles = sorted({c for c in cols if 0 <= c < width})
    pairs = []
    if width > WAVE_COLS + 5:
        pairs.append((3, WAVE_COLS + 5))             # waves 0 and 1
    if width > ITER_COLS:
        pairs.append((3, ITER_COLS + 3))             # same lane, iterations 0, 1
        pairs.append((WAVE_COLS + 1, width - 2))     # wave 1, last iteration
    return [(c,) for c in singles] + pairs


def _needle_weight(width):
    return 1.0 + (torch.arange(width) % 7).to(torch.float32) * 0.25


def needle_sumsq_case(op, width):
    assert op in NORM_OPS
    rows = needle_columns(width)
    x = torch.zeros(len(rows), width)
    for r, cols in enumerate(rows):
        x[r, list(cols)] = 3.0
    case = {"op": op, "kind": "needle_sumsq", "name": f"needle-sumsq-{width}",
            "weight": torch.ones(width).to(torch.bfloat16)
            if op in FP8_OPS else _needle_weight(width).to(torch.bfloat16),
            "needles": [list(c) for c in rows]}
    if op in FUSED_OPS:
        case["x"] = (x * (2.0 / 3.0)).to(torch.bfloat16)
        case["residual"] = (x / 3.0).to(torch.bfloat16)
    else:
        case["x"] = x.to(torch.bfloat16)
    return case


def needle_amax_case(op, width):
    assert op in FP8_OPS
    g = torch.Generator().manual_seed(_seed(op, "amax", width))
    rows = needle_columns(width)
    t = len(rows)
    case = {"op": op, "kind": "needle_amax", "name": f"needle-amax-{width}",
            "needles": [list(c) for c in rows]}
    if op == "silu_and_mul_fp8":
        gate = torch.randn(t, width, generator=g)
        up = 0.01 * torch.randn(t, width, generator=g)
        for r, cols in enumerate(rows):
            gate[r, list(cols)] = 10.0
            up[r, list(cols)] = 10.0
        case["x"] = torch.cat([gate, up], dim=1).to(torch.bfloat16)
        return case
    x = 0.01 * torch.randn(t, width, generator=g)
    for r, cols in enumerate(rows):
        x[r, list(cols)] = 100.0
    if op in NORM_OPS:
        case["weight"] = torch.ones(width).to(torch.bfloat16)
    if op in FUSED_OPS:
        case["x"] = (0.75 * x).to(torch.bfloat16)
        case["residual"] = (0.25 * x).to(torch.bfloat16)
    else:
        case["x"] = x.to(torch.bfloat16)
    return case


def tiny_row_case(op):
    """Rows whose absmax is below 1e-8, zero rows among them: s = 1e-8/448."""
    assert op in QUANT_OPS
    width = 264
    x = torch.zeros(3, width)
    x[1, 5] = 3e-9
    x[2] = 1e-12
    if op == "silu_and_mul_fp8":   # silu(64) = 64
        x = torch.cat([torch.full((3, width), 64.0), x / 64.0], dim=1)
    return {"op": op, "kind": "tiny", "name": "tiny-rows",
            "x": x.to(torch.bfloat16)}


SILU_STRIDE_SHAPE = (520, 8192)   # > 2048 * 256 vectors: a second grid stride


def silu_stride_case():
    t, width = SILU_STRIDE_SHAPE
    up = _int_code(t, width)
    x = torch.cat([torch.full((t, width), 64.0), up], dim=1).to(torch.bfloat16)
    return {"op": "silu_and_mul", "kind": "exact", "name": f"stride-{t}x{width}",
            "x": x,
            "exact": {"out_bits": bits16((64.0 * up).to(torch.bfloat16))}}


def cases_for(op, width):
    """Every case of one op at one width."""
    out = [random_case(op, width), exact_case(op, width)]
    if op in NORM_OPS:
        out.append(needle_sumsq_case(op, width))
    if op in FP8_OPS:
        out.append(needle_amax_case(op, width))
    return out


def all_cases():
    for op in OPS:
        for width in widths_for(op):
            yield from cases_for(op, width)
    for op in QUANT_OPS:
        yield tiny_row_case(op)


# --------------------------------------------------------------- emulation

def _f32_to_e4m3_bytes(v32):
    return v32.to(torch.float8_e4m3fn).view(torch.uint8)


def emulate(case, mutant=None):
    """float32 model of the kernels: fp32 reductions, the value quantised
    unrounded, scale = max(amax, 1e-8) / 448, q = e4m3(v * (1 / scale)).
    `mutant` switches in one of the defects of MUTANTS; a defect that does
    not apply to the op leaves the model unchanged."""
    assert mutant is None or mutant in MUTANTS
    op = case["op"]
    x = case["x"].to(torch.float32)
    outs = {}
    if op in SILU_OPS:
        width = x.shape[1] // 2
        g, u = x[:, :width], x[:, width:]
        if mutant == "swap_gate_up":
            g, u = u, g
    else:
        width = x.shape[1]
    col = torch.arange(width)
    # columns whose contribution the reductions see / that get written
    seen = torch.ones(width, dtype=torch.bool)
    written = torch.ones(width, dtype=torch.bool)
    if mutant == "drop_wave":
        seen &= (col % ITER_COLS) // WAVE_COLS != 3
    if mutant == "skip_partial" and width % ITER_COLS:
        part = col >= (width // ITER_COLS) * ITER_COLS
        seen &= ~part
        written &= ~part

    def prev_row(v):
        return torch.cat([v[:1], v[:-1]], dim=0)

    if op in NORM_OPS:
        if op in FUSED_OPS:
            x = x + case["residual"].to(torch.float32)
            outs["residual"] = x.to(torch.bfloat16)
        sumsq = (x * x)[:, seen].sum(dim=1, keepdim=True)
        inv_rms = torch.rsqrt(sumsq / width + torch.tensor(EPS))
        if mutant == "prev_row_scale" and op not in FP8_OPS:
            inv_rms = prev_row(inv_rms)
        y = x * inv_rms * case["weight"].to(torch.float32)
    elif op in SILU_OPS:
        y = g / (1.0 + torch.exp(-g)) * u
    else:
        y = x

    if op not in FP8_OPS:
        out = y.to(torch.bfloat16)
        out[:, ~written] = 0
        outs["out"] = out
        return outs

    src = y.to(torch.bfloat16).to(torch.float32) \
        if mutant == "scale_from_bf16" else y
    amax = src.abs()[:, seen].amax(dim=1, keepdim=True) if seen.any() \
        else torch.zeros(y.shape[0], 1)
    scale = torch.clamp(amax, min=1e-8) / torch.tensor(FP8_MAX)
    if mutant == "prev_row_scale":
        scale = prev_row(scale)
    inv_scale = 1.0 / scale
    q = _f32_to_e4m3_bytes(y * inv_scale)   # no clamp, as the kernels
    q[:, ~written] = 0
    if mutant == "swap_bytes":
        q = q.view(-1, width // 2, 2).flip(-1).reshape(-1, width)
    if mutant == "swap_words":
        q = q.view(-1, width // 8, 2, 4).flip(-2).reshape(-1, width)
    outs["out"] = q.contiguous()
    outs["scales"] = scale[:, 0].contiguous()
    return outs


# which ops each defect can touch (test_rowwise_cases wants it caught in all)
MUTANT_OPS = {
    "swap_bytes": FP8_OPS,
    "swap_words": FP8_OPS,
    "drop_wave": NORM_OPS + QUANT_OPS,
    "skip_partial": OPS,
    "scale_from_bf16": ("rms_norm_fp8", "fused_add_rms_norm_fp8",
                        "silu_and_mul_fp8"),
    "swap_gate_up": SILU_OPS,
    "prev_row_scale": NORM_OPS + QUANT_OPS,
}


# ------------------------------------------------- fp8 overflow confirmation

def scaled_amax_f32(amax32: torch.Tensor) -> torch.Tensor:
    """fl(amax * fl(1 / fl(max(amax, 1e-8) / 448))) in float32: what the
    row maximum becomes right before the (unclamped) e4m3 conversion."""
    assert amax32.dtype == torch.float32
    scale = torch.clamp(amax32, min=1e-8) / torch.tensor(FP8_MAX)
    return amax32 * (1.0 / scale)


def positive_finite_bf16() -> torch.Tensor:
    """Every positive finite bf16 value, subnormals included, as float32."""
    bits = torch.arange(1, 0x7F80, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------ reshape cache

CACHE_GRID_CAP_VECS = 2048 * 256   # cache.hip: 2048 blocks of 256 lanes


def cache_case(kv_heads=8, head_dim=128, block=16):
    """Smallest T whose vectors of 8 exceed the launcher's grid cap, so the
    grid-stride loop takes a second stride. Scattered slots, some negative."""
    vec_per_tok = kv_heads * head_dim // 8
    tokens = CACHE_GRID_CAP_VECS // vec_per_tok + 1
    nblocks = (tokens + block - 1) // block + 3
    g = torch.Generator().manual_seed(77)
    k = torch.randn(tokens, kv_heads * head_dim, generator=g).to(torch.bfloat16)
    v = torch.randn(tokens, kv_heads * head_dim, generator=g).to(torch.bfloat16)
    slots = torch.randperm(nblocks * block, generator=g)[:tokens].to(torch.int32)
    # padding rows, the last token (second stride) among them
    pad = torch.tensor([0, 5, tokens // 2, tokens - 1])
    slots[pad] = torch.tensor([-1, -7, -1, -1], dtype=torch.int32)
    return {"k": k, "v": v, "slots": slots, "nblocks": nblocks,
            "kv_heads": kv_heads, "head_dim": head_dim, "block": block,
            "tokens": tokens}


def cache_reference(case, k_cache, v_cache):
    """Reference scatter into CPU caches [B, Hk, block, D], in place."""
    hk, d, bs = case["kv_heads"], case["head_dim"], case["block"]
    slots = case["slots"].long()
    live = slots >= 0
    blk, off = slots[live] // bs, slots[live] % bs
    k_cache[blk, :, off] = case["k"][live].view(-1, hk, d)
    v_cache[blk, :, off] = case["v"][live].view(-1, hk, d)
