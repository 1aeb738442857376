"""Multi-adapter LoRA serving.

Capability parity with the reference's `--enable-lora --max-loras
--max-cpu-loras` engine flags and lora-affinity routing (SURVEY.md §2.3;
reference docs/.../runtime-profile.md:370-377, pkg/router/strategy.go:100-113).

Adapters target the four projection GEMMs (qkv, o, gate_up, down). Batched
application groups the step's tokens by adapter and adds
x[rows] @ A^T @ B^T (two skinny GEMMs per adapter per target) to the base
projection output — cheap for the usual 0-2 live adapters per batch.
TP sharding follows the base weights: B is sliced on column-parallel
outputs, A on row-parallel inputs.

With EngineConfig.enable_lora the resident adapters also live in a
LoRASlots table (stacked, zero-padded slots at stable addresses) and a
step applies all of them with one ops.lora_apply call per projection,
indexed by a per-token slot id — the form the LoRA decode graphs replay
(docs/serving_features.md). Each rank builds its table from its own
shards; nothing new goes over the wire.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from fusioninfer_amd.distributed import parallel_state as ps

TARGETS = ("qkv", "o", "gate_up", "down")


class LoRAAdapter:
    def __init__(self, name: str, rank: int, alpha: float, model_cfg,
                 dtype=torch.bfloat16, device="cpu", seed: Optional[int] = None):
        self.name = name
        self.rank = rank
        self.scaling = alpha / rank
        tp = ps.tp_world_size()
        tpr = ps.tp_rank()
        H = model_cfg.hidden_size
        qkv_out = (model_cfg.num_heads + 2 * model_cfg.num_kv_heads) * model_cfg.head_dim
        inter = model_cfg.intermediate_size
        gen = torch.Generator(device="cpu")
        if seed is not None:
            gen.manual_seed(seed)
        # weights[layer][target] = (A [r, in_shard], B [out_shard, r])
        self.weights: List[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = []
        for _ in range(model_cfg.num_layers):
            layer = {}
            for tgt, inf, outf, col in (
                ("qkv", H, qkv_out, True),
                ("o", model_cfg.num_heads * model_cfg.head_dim, H, False),
                ("gate_up", H, 2 * inter, True),
                ("down", inter, H, False),
            ):
                A = torch.randn(rank, inf, generator=gen, dtype=torch.float32) * 0.02
                # seeded B std 0.1: synthetic adapters must move logits
                # enough to flip greedy argmax on random-init base weights
                # (0.02 was within sampler tie-break noise on some seeds)
                B = torch.zeros(outf, rank) if seed is None else (
                    torch.randn(outf, rank, generator=gen, dtype=torch.float32) * 0.1
                )
                if col:  # column-parallel: shard B rows (per-segment is an
                    # approximation: qkv/gate_up segments are contiguous per
                    # rank in the base layout, so shard each segment)
                    B = self._shard_col_segments(B, tgt, model_cfg, tp, tpr)
                else:   # row-parallel: shard A input dim
                    per = inf // tp
                    A = A[:, tpr * per : (tpr + 1) * per]
                layer[tgt] = (
                    A.to(dtype=dtype, device=device),
                    B.to(dtype=dtype, device=device),
                )
            self.weights.append(layer)

    @staticmethod
    def _shard_col_segments(B, tgt, cfg, tp, tpr):
        if tp == 1:
            return B
        if tgt == "qkv":
            sizes = [
                cfg.num_heads * cfg.head_dim,
                cfg.num_kv_heads * cfg.head_dim,
                cfg.num_kv_heads * cfg.head_dim,
            ]
        else:  # gate_up
            sizes = [cfg.intermediate_size, cfg.intermediate_size]
        parts = []
        off = 0
        for sz in sizes:
            per = sz // tp
            parts.append(B[off + tpr * per : off + (tpr + 1) * per])
            off += sz
        return torch.cat(parts, dim=0)

    def to(self, device):
        for layer in self.weights:
            for tgt in list(layer):
                A, B = layer[tgt]
                layer[tgt] = (A.to(device), B.to(device))
        return self

    @classmethod
    def from_safetensors(cls, name: str, path: str, model_cfg,
                         dtype=torch.bfloat16, device="cpu"):
        """Load a PEFT adapter directory (adapter_model.safetensors +
        adapter_config.json). PEFT keeps one (A, B) pair per projection;
        the merged targets (qkv, gate_up) are reconstructed as a
        block-diagonal adapter of rank = sum of the member ranks:
        A = [A_q; A_k; A_v], B with each B_proj in its segment's rows and
        its own rank columns — mathematically identical to applying the
        projections separately. Per-projection alpha/r scaling is folded
        into B, so mixed configs compose; TP sharding then follows the
        base-weight layout (B by column segments, A on row-parallel
        inputs)."""
        import json as _json
        import os

        from safetensors.torch import safe_open

        cfg_path = os.path.join(path, "adapter_config.json")
        alpha_over_r = 1.0
        if os.path.isfile(cfg_path):
            with open(cfg_path) as f:
                pc = _json.load(f)
            if pc.get("r"):
                alpha_over_r = float(
                    pc.get("lora_alpha", pc["r"])
                ) / float(pc["r"])
        st_path = os.path.join(path, "adapter_model.safetensors")
        tensors: Dict[str, torch.Tensor] = {}
        with safe_open(st_path, framework="pt") as sf:
            for k in sf.keys():
                tensors[k] = sf.get_tensor(k)

        def pair(li: int, proj: str):
            for prefix in (
                f"base_model.model.model.layers.{li}.{proj}",
                f"model.layers.{li}.{proj}",
            ):
                a = tensors.get(prefix + ".lora_A.weight")
                b = tensors.get(prefix + ".lora_B.weight")
                if a is not None and b is not None:
                    return a.float(), b.float() * alpha_over_r
            return None

        tp = ps.tp_world_size()
        tpr = ps.tp_rank()
        H = model_cfg.hidden_size
        inter = model_cfg.intermediate_size
        self = cls.__new__(cls)
        self.name = name
        self.scaling = 1.0  # folded into B above
        self.rank = 0
        self.weights = []
        merged = {
            "qkv": (["self_attn.q_proj", "self_attn.k_proj",
                     "self_attn.v_proj"],
                    [model_cfg.num_heads * model_cfg.head_dim,
                     model_cfg.num_kv_heads * model_cfg.head_dim,
                     model_cfg.num_kv_heads * model_cfg.head_dim], H),
            "gate_up": (["mlp.gate_proj", "mlp.up_proj"],
                        [inter, inter], H),
            "o": (["self_attn.o_proj"],
                  [H], model_cfg.num_heads * model_cfg.head_dim),
            "down": (["mlp.down_proj"], [H], inter),
        }
        for li in range(model_cfg.num_layers):
            layer = {}
            for tgt, (projs, seg_sizes, inf) in merged.items():
                pairs = [pair(li, p) for p in projs]
                if not any(p is not None for p in pairs):
                    # adapter does not target this module: rank-1 zeros
                    layer[tgt] = (
                        torch.zeros(1, inf // (tp if tgt in ("o", "down")
                                               else 1), dtype=dtype,
                                    device=device),
                        torch.zeros(
                            sum(s // (tp if tgt in ("qkv", "gate_up")
                                      else 1) for s in seg_sizes), 1,
                            dtype=dtype, device=device),
                    )
                    continue
                ranks = [0 if p is None else p[0].shape[0] for p in pairs]
                R = sum(r for r in ranks) or 1
                A = torch.zeros(R, inf)
                out_total = sum(seg_sizes)
                B = torch.zeros(out_total, R)
                r_off = 0
                seg_off = 0
                for p, r, sz in zip(pairs, ranks, seg_sizes):
                    if p is not None:
                        a, b = p
                        A[r_off: r_off + r] = a
                        B[seg_off: seg_off + sz, r_off: r_off + r] = b
                        r_off += r
                    seg_off += sz
                self.rank = max(self.rank, R)
                if tgt in ("qkv", "gate_up"):
                    B = LoRAAdapter._shard_col_segments(
                        B, tgt, model_cfg, tp, tpr
                    )
                else:
                    per = inf // tp
                    A = A[:, tpr * per: (tpr + 1) * per]
                layer[tgt] = (A.to(dtype=dtype, device=device),
                              B.to(dtype=dtype, device=device))
            self.weights.append(layer)
        return self


def target_dims(model_cfg) -> Dict[str, Tuple[int, int]]:
    """Per-rank (in, out) features of the four LoRA targets — the TP-sharded
    shapes LoRAAdapter produces (B sliced on column-parallel outputs, A on
    row-parallel inputs)."""
    tp = ps.tp_world_size()
    H = model_cfg.hidden_size
    qkv_out = ((model_cfg.num_heads + 2 * model_cfg.num_kv_heads)
               * model_cfg.head_dim)
    inter = model_cfg.intermediate_size
    return {
        "qkv": (H, qkv_out // tp),
        "o": (model_cfg.num_heads * model_cfg.head_dim // tp, H),
        "gate_up": (H, 2 * inter // tp),
        "down": (inter // tp, H),
    }


class LoRASlots:
    """Stacked adapter slots at stable device addresses (Punica/S-LoRA).

    For every layer and target: a_stack [max_loras, R, in],
    b_stack [max_loras, out, R] and scales [max_loras], allocated once and
    never reallocated — captured decode graphs read them by address. R is
    max_lora_rank rounded up to 16; an adapter of lower rank is zero-padded,
    so the kernels need no per-slot rank. A freed slot only has its scales
    zeroed (no token points at it; the next page-in overwrites it).

    `usable` is False when any target's per-rank shape is outside what
    ops.lora_apply supports; then no adapter ever gets a slot and every
    LoRA step stays on the per-adapter torch loop."""

    def __init__(self, model_cfg, max_loras: int, max_lora_rank: int,
                 device="cpu", dtype=torch.bfloat16):
        import fusioninfer_amd.ops as ops

        self.max_loras = max_loras
        self.rank = max(16, (max_lora_rank + 15) // 16 * 16)
        if self.rank > ops.LORA_MAX_RANK:
            raise ValueError(
                f"max_lora_rank={max_lora_rank} exceeds the kernels' "
                f"limit of {ops.LORA_MAX_RANK}"
            )
        self.device = device
        self.dims = target_dims(model_cfg)
        self.usable = all(
            ops.lora_shapes_supported(inf, outf, self.rank)
            for inf, outf in self.dims.values()
        )
        # layers[layer][target] = (a_stack, b_stack, scales)
        self.layers: List[Dict[str, Tuple[torch.Tensor, ...]]] = []
        if self.usable:
            R = self.rank
            for _ in range(model_cfg.num_layers):
                self.layers.append({
                    tgt: (
                        torch.zeros(max_loras, R, inf, dtype=dtype,
                                    device=device),
                        torch.zeros(max_loras, outf, R, dtype=dtype,
                                    device=device),
                        torch.zeros(max_loras, dtype=torch.float32,
                                    device=device),
                    )
                    for tgt, (inf, outf) in self.dims.items()
                })
        self._owner: List[Optional[str]] = [None] * max_loras

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size()
                   for layer in self.layers for ts in layer.values()
                   for t in ts)

    def fits(self, adapter: LoRAAdapter) -> bool:
        """Stored rank (PEFT merged targets: qkv 3r, gate_up 2r) must fit R
        and the shards must have this table's per-rank shapes."""
        if not self.usable or len(adapter.weights) != len(self.layers):
            return False
        for layer in adapter.weights:
            for tgt, (inf, outf) in self.dims.items():
                A, B = layer[tgt]
                if (A.shape[0] > self.rank or A.shape[1] != inf
                        or B.shape[0] != outf):
                    return False
        return True

    def owner(self, slot: int) -> Optional[str]:
        return self._owner[slot]

    def free_slot_index(self) -> Optional[int]:
        for i, o in enumerate(self._owner):
            if o is None:
                return i
        return None

    def load(self, slot: int, adapter: LoRAAdapter) -> None:
        """copy_ the adapter into `slot`, zero-padding to R."""
        for stacks, layer in zip(self.layers, adapter.weights):
            for tgt, (a_stack, b_stack, scales) in stacks.items():
                A, B = layer[tgt]
                r = A.shape[0]
                a_stack[slot].zero_()
                b_stack[slot].zero_()
                a_stack[slot, :r].copy_(A)
                b_stack[slot, :, :r].copy_(B)
                scales[slot] = float(adapter.scaling)
        self._owner[slot] = adapter.name

    def free(self, slot: int) -> None:
        for stacks in self.layers:
            for _, _, scales in stacks.values():
                scales[slot] = 0.0
        self._owner[slot] = None


class LoRABatch:
    """Per-step adapter routing, in one of two forms:

    * groups: [(adapter, row_index_tensor)] — the per-adapter torch loop;
    * slot form: one [T] int32 slot-id tensor (-1 = base row) over a
      LoRASlots table; apply is a single ops.lora_apply call (HIP kernels
      on GPU tensors, static shapes, hipGraph-capturable)."""

    def __init__(self,
                 groups: Optional[List[Tuple[LoRAAdapter, torch.Tensor]]] = None,
                 slot_ids: Optional[torch.Tensor] = None,
                 slots: Optional[LoRASlots] = None):
        assert (groups is None) != (slot_ids is None)
        assert slot_ids is None or slots is not None
        self.groups = groups
        self.slot_ids = slot_ids
        self.slots = slots

    def apply(self, layer_idx: int, target: str, x: torch.Tensor,
              out: torch.Tensor) -> None:
        """out[rows] += scaling * x[rows] @ A^T @ B^T (in place)."""
        if self.slot_ids is not None:
            import fusioninfer_amd.ops as ops

            a_stack, b_stack, scales = self.slots.layers[layer_idx][target]
            ops.lora_apply(out, x, self.slot_ids, a_stack, b_stack, scales)
            return
        for adapter, rows in self.groups:
            A, B = adapter.weights[layer_idx][target]
            xr = x[rows]
            delta = (xr @ A.T) @ B.T
            out[rows] += adapter.scaling * delta


class LoRARegistry:
    """Adapter store with vLLM's --max-loras / --max-cpu-loras tiering:
    at most `max_loras` adapters stay device-resident; the LRU ones park
    in host memory (up to `max_cpu_loras` total) and page back on use.

    With a LoRASlots table, a resident adapter that fits the table also
    owns one of its `max_loras` slots: page-in copies it into a free slot,
    LRU eviction or remove frees the slot. Adapters that do not fit (stored
    rank above the table's R, or an unusable table) stay resident without
    a slot and are served by the per-adapter torch loop."""

    def __init__(self, max_loras: int = 8, max_cpu_loras: int = 16,
                 device: str = "cpu", slots: Optional[LoRASlots] = None):
        self.max_loras = max_loras
        self.max_cpu_loras = max(max_cpu_loras, max_loras)
        self.device = device
        self.slots = slots
        assert slots is None or slots.max_loras >= max_loras
        self._adapters: Dict[str, LoRAAdapter] = {}
        self._resident: Dict[str, int] = {}  # name -> last-use tick
        self._slot_of: Dict[str, int] = {}   # name -> slot (subset of resident)
        self._tick = 0

    def _release_slot(self, name: str) -> None:
        slot = self._slot_of.pop(name, None)
        if slot is not None:
            self.slots.free(slot)

    def _assign_slot(self, adapter: LoRAAdapter) -> None:
        if self.slots is None or not self.slots.fits(adapter):
            return
        slot = self.slots.free_slot_index()
        assert slot is not None, "resident adapters exceed the slot table"
        self.slots.load(slot, adapter)
        self._slot_of[adapter.name] = slot

    def _evict_lru_if_needed(self) -> None:
        while len(self._resident) > self.max_loras:
            lru = min(self._resident, key=self._resident.get)
            del self._resident[lru]
            self._release_slot(lru)
            if self.device != "cpu":
                self._adapters[lru].to("cpu")

    def add(self, adapter: LoRAAdapter) -> None:
        if (len(self._adapters) >= self.max_cpu_loras
                and adapter.name not in self._adapters):
            raise RuntimeError(f"max_cpu_loras={self.max_cpu_loras} reached")
        self._release_slot(adapter.name)  # re-registration replaces contents
        self._adapters[adapter.name] = adapter
        self._tick += 1
        self._resident[adapter.name] = self._tick
        self._evict_lru_if_needed()
        self._assign_slot(adapter)

    def get(self, name: str) -> LoRAAdapter:
        adapter = self._adapters[name]
        self._tick += 1
        if name not in self._resident:
            # page back in from host memory
            if self.device != "cpu":
                adapter.to(self.device)
            self._resident[name] = self._tick
            self._evict_lru_if_needed()
            self._assign_slot(adapter)
        else:
            self._resident[name] = self._tick
        return adapter

    def maybe_get(self, name: Optional[str]) -> Optional[LoRAAdapter]:
        return self.get(name) if name and name in self._adapters else None

    def slot_of(self, name: str) -> Optional[int]:
        """Slot owned by a resident adapter, or None (torch-loop path)."""
        return self._slot_of.get(name)

    def names(self) -> List[str]:
        return sorted(self._adapters)

    def num_resident(self) -> int:
        return len(self._resident)

    def remove(self, name: str) -> bool:
        self._resident.pop(name, None)
        self._release_slot(name)
        return self._adapters.pop(name, None) is not None
