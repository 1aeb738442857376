"""Re-measure LOGITS_FLOOR of tests/test_mxfp4_moe_gpu.py.

The floor is the max-abs difference of the prefill logits between the bf16
`tiny-qwen3-moe` engine on dequantised weights on the GPU and the same
weights on the CPU reference ops, for the test's own prompts. Neither engine
runs the MXFP4 code. Prints the figures; asserts nothing.

Usage (from the repository root, on a GPU):
    python tools/mxfp4_moe_logits_floor.py
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_mxfp4_moe_gpu as t  # noqa: E402


def cpu_copy_of(eng):
    """The same bf16 model on the CPU (reference ops), weights copied over."""
    from fusioninfer_amd.models.model import MoEMLP

    cpu = t._engine(None, True, "cpu")
    for m in eng.runner.model.modules():
        if isinstance(m, MoEMLP):
            m.ensure_unpacked()
    src = dict(eng.runner.model.named_parameters())
    for name, p in cpu.runner.model.named_parameters():
        p.data.copy_(src[name].data.cpu())
    return cpu


def main():
    gpu = t.dequantised_engine()
    cpu = cpu_copy_of(gpu)
    worst = 0.0
    for prompt in (t.PROMPTS[2], t.LONG_PROMPT):
        a = t.prefill_logits(gpu, prompt)
        b = t.prefill_logits(cpu, prompt)
        d = (a - b).abs().max().item()
        print(f"{len(prompt)} tokens: max abs diff {d:.4e}, largest |logit| "
              f"{b.abs().max().item():.4f}, row_rel_err "
              f"{t.row_rel_err(a, b):.4e}")
        worst = max(worst, d)
    print(f"LOGITS_FLOOR (worst) = {worst:.4e}")


if __name__ == "__main__":
    main()
