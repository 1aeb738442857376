"""Int4 group-quantised W4A16 HIP kernels and engine mode on the GPU.

The oracle is a GEMM on dq(W) (reference.int4_dequant). Shapes are those of
tests/test_mxfp4_gpu.py (K: 1, 3, 9 chunks; N: one tile, no multiple of 64;
M: tile tails, all three instances, a second row block), for every G."""

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q
from int4_cases import engine, pack, prefill_logits

pytestmark = pytest.mark.gpu

KS = (128, 384, 1152)
NS = (16, 48, 272)
MS = (1, 3, 16, 17, 33, 64, 65, 130)
GS = (32, 64, 128)
DEV = "cuda:0"
# exact result rounded to bf16 is within 2^-9 per element; 4x margin for
# the accumulation order (docs/kernels.md convention)
ROW_REL_BOUND = 2.0 ** -7

_cache = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def weight(kind, N, K, G):
    """GPU (packed, scale, zero, dq(W)); kind is "random" (codes, zeros, fp16
    scales), "pow2" (scales in {0.5, 1, 2}) or "gauss" (quantised gaussian)."""
    key = (kind, N, K, G)
    if key not in _cache:
        g = _gen(N * 7919 + K + G)
        if kind == "gauss":
            p, s, z = Q.quantize_weight_int4(
                torch.randn(N, K, generator=g) * 0.02, G)
        else:
            p = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8)
            z = torch.randint(0, 16, (N, K // G), generator=g).to(torch.uint8)
            if kind == "pow2":
                s = 2.0 ** torch.randint(-1, 2, (N, K // G), generator=g)
            else:
                s = torch.rand(N, K // G, generator=g) * 0.03 + 1e-3
            s = s.to(torch.float16)
        dq = ref.int4_dequant(p, s, z, G)
        _cache[key] = (p.to(DEV), s.to(DEV), z.to(DEV), dq.to(DEV))
    return _cache[key]


def row_rel_err(got, want64):
    num = (got.double() - want64).norm(dim=-1)
    return (num / want64.norm(dim=-1)).max().item()


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_column_readout_exact(K, N, G):
    """One-hot x rows read columns of dq(W) back, bit for bit: nibble order,
    lane -> k map, group index. The rows visit every k of a 128-k step."""
    p, s, z, dq = weight("random", N, K, G)
    row = 0
    for M in MS:
        km = [(r % 128) + 128 * (r % (K // 128)) for r in range(row, row + M)]
        row += M
        x = torch.zeros(M, K, dtype=torch.bfloat16)
        x[torch.arange(M), torch.tensor(km)] = 1.0
        out = ops.int4_linear(x.to(DEV), p, s, z, G)
        assert out.shape == (M, N) and out.dtype == torch.bfloat16
        assert torch.equal(out, dq[:, km].t().contiguous()), (K, N, M, G)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_integer_gemm_exact(K, N, G, with_bias):
    """x in [-4, 4], |q - z| <= 15, scales in {0.5, 1, 2}: every product is a
    multiple of 0.5 and |sum| <= 4 * 15 * 2 * 1152 = 138240 < 2^24 * 0.5, so
    fp32 accumulation is exact in any order and the result must equal the
    float64 reference rounded to bf16."""
    p, s, z, dq = weight("pow2", N, K, G)
    g = _gen(K + N + G)
    bias = None
    if with_bias:
        bias = torch.randint(-8, 9, (N,), generator=g).to(torch.bfloat16).to(DEV)
    for M in MS:
        x = torch.randint(-4, 5, (M, K), generator=g).to(torch.bfloat16).to(DEV)
        want = x.double() @ dq.double().t()
        if with_bias:
            want = want + bias.double()
        out = ops.int4_linear(x, p, s, z, G, bias)
        assert torch.equal(out, want.to(torch.bfloat16)), (K, N, M, G)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_random_data_row_error(K, N, G):
    p, s, z, dq = weight("gauss", N, K, G)
    g = _gen(3 * K + N + G)
    worst = 0.0
    for M in MS:
        x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
        want = x.double() @ dq.double().t()  # no final rounding
        worst = max(worst, row_rel_err(ops.int4_linear(x, p, s, z, G), want))
    print(f"int4_linear K={K} N={N} G={G} max row_rel_err {worst:.3e}")
    assert worst < ROW_REL_BOUND


@pytest.mark.parametrize("G", GS)
def test_batch_invariance_bitwise(G):
    K, N = 1152, 272
    p, s, z, _ = weight("gauss", N, K, G)
    g = _gen(99)
    row = torch.randn(1, K, generator=g).to(torch.bfloat16)
    x33 = torch.randn(33, K, generator=g).to(torch.bfloat16)
    x130 = torch.randn(130, K, generator=g).to(torch.bfloat16)
    x33[5] = row[0]
    x130[77] = row[0]  # second row block, another position in its tile
    alone = ops.int4_linear(row.to(DEV), p, s, z, G)
    assert torch.equal(ops.int4_linear(x33.to(DEV), p, s, z, G)[5], alone[0])
    assert torch.equal(ops.int4_linear(x130.to(DEV), p, s, z, G)[77], alone[0])


@pytest.mark.parametrize("G", GS)
def test_dequant_all_codes_zeros_scales(G):
    """16 codes x 16 zeros x fp16 scales (smallest and largest normal, 1.0,
    full 11-bit significands), changing from group to group, bit for bit."""
    bits = [0x0400, 0x7BFF, 0x3C00, 0x3BFF, 0x3555, 0x2AAB, 0x57FF, 0x0401]
    scales = torch.tensor(bits, dtype=torch.int16).view(torch.float16)
    N, K = 16 * len(bits), 128
    n = torch.arange(N).unsqueeze(1)
    grp = torch.arange(K // G).unsqueeze(0)
    z = ((n + grp) % 16).to(torch.uint8)
    s = scales[(n // 16 + grp) % len(bits)].contiguous()
    q = ((torch.arange(K).unsqueeze(0) * 7 + n) % 16).to(torch.uint8)
    p = pack(q)
    ops.validate_int4_scales(s, z)
    want = ((q.double() - z.double().repeat_interleave(G, dim=1))
            * s.double().repeat_interleave(G, dim=1)).to(torch.bfloat16)
    got = ops.int4_dequant(p.to(DEV), s.to(DEV), z.to(DEV), G)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))
    # the GEMM's expansion is the same one: identity x reads dq back
    eye = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    out = ops.int4_linear(eye, p.to(DEV), s.to(DEV), z.to(DEV), G)
    assert torch.equal(out.t().cpu().view(torch.int16), want.view(torch.int16))


def test_out_into_sentinel_buffer():
    K, N, M, G = 384, 48, 17, 64
    p, s, z, _ = weight("gauss", N, K, G)
    x = torch.randn(M, K, generator=_gen(7)).to(torch.bfloat16).to(DEV)
    inputs = [t.clone() for t in (x, p, s, z)]
    buf = torch.full((M + 4, N), -777.0, dtype=torch.bfloat16, device=DEV)
    out = buf[2:2 + M]
    assert ops.int4_linear(x, p, s, z, G, out=out) is out
    assert torch.equal(out, ops.int4_linear(x, p, s, z, G))
    assert bool((buf[:2] == -777.0).all()) and bool((buf[2 + M:] == -777.0).all())
    for a, b in zip(inputs, (x, p, s, z)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert ops.int4_linear(x[:0], p, s, z, G).shape == (0, N)


def test_layer_dispatch_and_shared_scratch(monkeypatch):
    """M = 8: the HIP GEMM; M = 40: dequant + F.linear via the shared scratch."""
    from fusioninfer_amd.distributed.layers import (
        MergedColumnParallelLinear, RowParallelLinear)

    monkeypatch.setattr(Q, "INT4_MAX_M", 16)
    torch.manual_seed(5)
    holder = torch.nn.Module()
    with torch.device(DEV):
        holder.up = MergedColumnParallelLinear(256, [384, 128], bias=True)
        holder.down = RowParallelLinear(512, 256)
    holder.up.bias.data.normal_()
    assert Q.convert_linear_to_int4(holder, 64) == 2
    dq = {name: Q.dequantize_int4(m.weight_packed, m.weight_scale,
                                  m.weight_zero, 64).double()
          for name, m in (("up", holder.up), ("down", holder.down))}
    calls = []
    real = ops.int4_dequant
    monkeypatch.setattr(ops, "int4_dequant",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    for M, n_dequant in ((8, 0), (40, 2)):
        calls.clear()
        x = torch.randn(M, 256, device=DEV).to(torch.bfloat16)
        y_up = holder.up(x)  # back to back: both go through one scratch
        y_down = holder.down(y_up)
        assert len(calls) == n_dequant
        want_up = x.double() @ dq["up"].t() + holder.up.bias.double()
        assert row_rel_err(y_up, want_up) < ROW_REL_BOUND
        assert row_rel_err(y_down, y_up.double() @ dq["down"].t()) < ROW_REL_BOUND


PROMPTS = [[3, 1, 4] * 6, [2, 7, 1, 8, 2, 8] * 4, list(range(5, 45))]


def test_engine_graph_decode_matches_eager():
    from fusioninfer_amd.engine.sequence import SamplingParams

    sp = SamplingParams(max_tokens=16, temperature=0.0, ignore_eos=True)
    eager = engine("int4", G=128, device=DEV, eager=True).generate(PROMPTS, sp)
    graphed = engine("int4", G=128, device=DEV).generate(PROMPTS, sp)
    for a, b in zip(eager, graphed):
        assert len(a.output_token_ids) == 16
        assert a.output_token_ids == b.output_token_ids


def test_engine_prefill_logits_hip_ops_against_reference_ops(monkeypatch):
    """One int4 engine, first on ops.int4_linear, then on
    reference.int4_linear: metric and bound of the mxfp4 engine test, 4x its
    measured bf16-against-fp32 floor of 7.85e-3 (tests/test_mxfp4_gpu.py)."""
    monkeypatch.setattr(Q, "INT4_MAX_M", 64)  # M = 40 takes the HIP GEMM
    eng = engine("int4", G=128, device=DEV, eager=True)
    got = prefill_logits(eng, PROMPTS[2])
    monkeypatch.setattr(
        ops, "int4_linear",
        lambda x, p, s, z, G, bias=None: ref.int4_linear(x, p, s, z, G, bias))
    err = row_rel_err(got, prefill_logits(eng, PROMPTS[2]))
    print(f"int4 prefill logits row_rel_err {err:.3e}")
    assert err < 4 * 7.85e-3
