"""`mxfp4_moe_activations="mxfp8-wide"` on the CPU: the flag, and the
reference op at block_m 32 against itself at block_m 128."""

from types import SimpleNamespace

import pytest
import torch

import fusioninfer_amd.ops as ops
import fusioninfer_amd.ops.reference as ref
from fusioninfer_amd import quantization as Q
from fusioninfer_amd.models.model import MoEMLP
from tests.test_mxfp4_moe import _engine, _moe_mlps


def test_flag_and_validation():
    from fusioninfer_amd.server.__main__ import build_engine_config, parse_args

    args = parse_args(["--model", "tiny-qwen3-moe", "--quantization", "mxfp4",
                       "--mxfp4-moe-experts", "--mxfp4-moe-activations",
                       "mxfp8-wide"])
    assert build_engine_config(args).model.mxfp4_moe_activations == "mxfp8-wide"
    with pytest.raises(SystemExit):
        parse_args(["--mxfp4-moe-activations", "mxfp8-narrow"])
    with pytest.raises(ValueError, match="mxfp4_moe_activations"):
        _engine("mxfp4", True, mxfp4_moe_activations="mxfp8-narrow")
    mlps = _moe_mlps(
        _engine("mxfp4", True, mxfp4_moe_activations="mxfp8-wide").runner.model)
    assert mlps and all(m.mxfp4_activations == "mxfp8-wide" for m in mlps)


def test_reference_op_block_m_32_equals_128():
    """Through the public op on CPU tensors: every routed gate_up row has the
    same bits under both alignments."""
    g = torch.Generator().manual_seed(5)
    E, K, N, T = 3, 128, 32, 41
    w = torch.randn(E, 2 * N, K, generator=g) * 0.05
    packed, scale = (torch.stack(t) for t in zip(
        *(Q.quantize_weight_mxfp4(w[e]) for e in range(E))))
    x_q, x_s = ref.mxfp8_quant_rows(
        (4 * torch.randn(T, K, generator=g)).to(torch.bfloat16))
    topi = torch.randint(0, E, (T, 1), generator=g)
    mlp = SimpleNamespace(e_start=0, e_end=E)  # all _moe_align reads of self
    got = []
    for bm in (32, 128):
        s, e, n, pos, PM = MoEMLP._moe_align(mlp, topi, bm)
        out = torch.zeros(PM, N, dtype=torch.uint8)
        osc = torch.zeros(PM, 1, dtype=torch.uint8)
        ops.moe_gemm_mxfp4_mxfp8(out.view(torch.float8_e4m3fn), x_q, x_s,
                                 packed, scale, s, e, n, True, osc, block_m=bm)
        got.append(torch.cat([out, osc], 1)[pos.long()])
    assert torch.equal(*got) and bool(got[0][:, :N].any())
