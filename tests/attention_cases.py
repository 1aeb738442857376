"""Adversarial attention inputs and float64 references (helper, no tests).

The attention kernels are compared with float64 references on inputs built
so that the mistakes these kernels can make are O(1) errors, not O(1/ctx):

* needles: a few tokens at partition edges, block edges and the last valid
  slot carry a key aligned with one q head, so that head's softmax mass sits
  on exactly those tokens with equal weights;
* poison: every slot a kernel must not attend (pad slots of a last partial
  block, blocks no sequence owns, block 0) holds a key strongly aligned with
  q and V = +100, finite and at a valid index;
* block tables are a seeded random permutation, never ascending.

The references take `q_rounding`, which reproduces the ONE input rounding a
kernel's score path documents (see `attend64`); everything after it is
float64. This is reference-side arithmetic written from the kernels'
comments; nothing here imports or inspects a kernel.

Known gap these cases keep out of: length 0 (the decode kernel's header
documents it; the engine never sends it). No case uses an out-of-range
block id.
"""

from __future__ import annotations

import math

import torch

BLOCK = 16          # cache block size (tokens)
PARTITION = 512     # decode flash-decoding partition (tokens)
DECODE_KV_HEADS = 2
LOG2E = 1.4426950408889634

NEEDLE_GAIN = 3.0   # K = 3 * sign(q): score 3 * sum|q| * scale
POISON_GAIN = 6.0   # K = 6 * sign(q)
POISON_V = 100.0

# kernel tolerance on row_rel_err: the float64 result rounded to bf16 is
# within 2^-8 by construction (2^-9 per element); the kernels get 4x that
# for fp32 accumulation order, v_exp_f32 and (prefill) P packed to bf16
KERNEL_TOL = 2.0 ** -6
# inputs must make every mutant at least this wrong (test_attention_cases)
MUTANT_MIN_ERR = 10 * KERNEL_TOL

DECODE_LENS = [1, 15, 16, 17, 33, 255, 512, 513, 1023, 1025, 1537]
# name -> (seq_lens, table_blocks): 5 partitions and 11*2*5 = 110 workgroup
# slots (< 256: the 8-wave kernels), 4 partitions and 33*2*4 = 264 slots
# (the 4-wave kernels, G=4 and G=8 head-split)
DECODE_GRIDS = {
    "wide": (DECODE_LENS, 160),
    "full": (DECODE_LENS * 3, 97),
}

PREFILL_PAGED = ([65, 81, 300, 703, 1000], [1, 64, 283, 300, 513])
PREFILL_DENSE_LENS = [1, 33, 257, 300]
PROBE_OFFSETS = (0, 31, 32, 63, 64, 127, 128, 255, 256)


# ---------------------------------------------------------------- references

def row_rel_err(got: torch.Tensor, want64: torch.Tensor) -> torch.Tensor:
    """||got - want||_2 / ||want||_2 over D, per (row, head)."""
    got = got.detach().to("cpu", torch.float64)
    want = want64.detach().to("cpu", torch.float64)
    return (got - want).norm(dim=-1) / want.norm(dim=-1)


def gather_kv64(cache: torch.Tensor, table_row: torch.Tensor, n: int):
    """First n tokens of one sequence: [Hk, n, D] float64."""
    nblk = (n + BLOCK - 1) // BLOCK
    blocks = table_row[:nblk].long()
    hk, d = cache.shape[1], cache.shape[3]
    rows = cache[blocks].to(torch.float64).permute(1, 0, 2, 3)
    return rows.reshape(hk, nblk * BLOCK, d)[:, :n]


def _f32(x) -> torch.Tensor:
    return torch.tensor(x, dtype=torch.float32)


def attend64(q, keys, vals, q_pos, scale, q_rounding=None, prescale="split"):
    """softmax(q k^T * scale) v in float64, row r attending kv <= q_pos[r].

    q [R, Hq, D] (any float dtype), keys/vals [Hk, n, D] float64, q_pos [R].
    q_rounding reproduces one documented input rounding of a score path:

    None              Q as given.
    "bf16_prescaled"  q' = bf16(q * scale * log2e), scores in base 2 (decode
                      MFMA bf16 scores; the prefill kernel). `prescale` is
                      the fp32 association of that product: "split" =
                      (q * scale) * log2e (decode), "folded" =
                      q * (scale * log2e) (prefill).
    "e4m3_per_head"   qs = max(amax_head, 1e-8) / 448, q8 = e4m3(q / qs)
                      saturating, score = (q8 . k) * qs * scale (decode MFMA
                      fp8 scores). The fp32 steps are the kernel's: q times
                      the reciprocal of qs, and qs * scale * log2e.
    """
    R, hq, d = q.shape
    hk = keys.shape[0]
    group = hq // hk
    q32 = q.detach().to(torch.float32)
    if q_rounding is None:
        qe = q32.to(torch.float64)
        post = torch.full((R, hq), float(scale), dtype=torch.float64)
    elif q_rounding == "bf16_prescaled":
        if prescale == "split":
            qp = q32 * _f32(scale) * _f32(LOG2E)
        else:
            qp = q32 * (_f32(scale) * _f32(LOG2E))
        qe = qp.to(torch.bfloat16).to(torch.float64)
        post = torch.full((R, hq), math.log(2.0), dtype=torch.float64)
    elif q_rounding == "e4m3_per_head":
        qs = q32.abs().amax(dim=-1).clamp(min=1e-8) / _f32(448.0)  # [R, Hq]
        q8 = (q32 * (_f32(1.0) / qs).unsqueeze(-1)).clamp(-448.0, 448.0)
        qe = q8.to(torch.float8_e4m3fn).to(torch.float64)
        sc2 = qs * _f32(scale) * _f32(LOG2E)  # base-2 score factor, fp32
        post = sc2.to(torch.float64) * math.log(2.0)
    else:
        raise ValueError(f"unknown q_rounding {q_rounding!r}")
    n = keys.shape[1]
    qg = qe.view(R, hk, group, d)
    scores = torch.einsum("rkgd,knd->rkgn", qg, keys)
    scores = scores * post.view(R, hk, group, 1)
    hidden = torch.arange(n).view(1, 1, 1, n) > q_pos.view(R, 1, 1, 1)
    p = torch.softmax(scores.masked_fill(hidden, float("-inf")), dim=-1)
    return torch.einsum("rkgn,knd->rkgd", p, vals).reshape(R, hq, -1)


def ref64_decode(q, k_cache, v_cache, block_tables, seq_lens, scale,
                 q_rounding=None) -> torch.Tensor:
    """reference.paged_attention_decode in float64, no final rounding."""
    out = torch.empty(q.shape, dtype=torch.float64)
    for s in range(q.shape[0]):
        n = int(seq_lens[s])
        out[s] = attend64(
            q[s:s + 1], gather_kv64(k_cache, block_tables[s], n),
            gather_kv64(v_cache, block_tables[s], n), torch.tensor([n - 1]),
            scale, q_rounding, "split")[0]
    return out


def ref64_prefill_paged(q, k_cache, v_cache, block_tables, cu_seqlens_q,
                        seq_lens_k, scale, q_rounding=None) -> torch.Tensor:
    """reference.prefill_attention_paged in float64, no final rounding."""
    out = torch.empty(q.shape, dtype=torch.float64)
    for s in range(cu_seqlens_q.numel() - 1):
        qs, qe = int(cu_seqlens_q[s]), int(cu_seqlens_q[s + 1])
        n = int(seq_lens_k[s])
        q_pos = (n - (qe - qs)) + torch.arange(qe - qs)
        out[qs:qe] = attend64(
            q[qs:qe], gather_kv64(k_cache, block_tables[s], n),
            gather_kv64(v_cache, block_tables[s], n), q_pos, scale,
            q_rounding, "folded")
    return out


def decode_q_rounding(fp8: bool, group: int, mfma: bool = True):
    """The q_rounding of the score policy the decode dispatch documents for
    a case: bf16 caches take the MFMA bf16 scores, fp8 caches the MFMA fp8
    scores at G=8 only; everything else (and all of FI_DECODE_MFMA=0) is
    the scalar path, which keeps Q in fp32."""
    if not mfma:
        return None
    if not fp8:
        return "bf16_prescaled"
    return "e4m3_per_head" if group == 8 else None


# -------------------------------------------------------------------- inputs

def _sign(x: torch.Tensor) -> torch.Tensor:
    x = x.to(torch.float32)
    return torch.where(x >= 0, torch.ones_like(x), -torch.ones_like(x))


class _PagedBuilder:
    """Background cache, permuted tables and poison shared by both cases.

    aim[s]: [Hq, D], the q row of sequence s that poison is aimed at."""

    def __init__(self, kv_lens, aim, hk, head_dim, table_blocks, gen,
                 nan_pads=False):
        S = len(kv_lens)
        self.hk, self.group = hk, aim[0].shape[0] // hk
        self.kv_lens, self.aim = kv_lens, aim
        nblk = [(n + BLOCK - 1) // BLOCK for n in kv_lens]
        width = table_blocks or max(nblk)
        assert width >= max(nblk)
        # block 0, every sequence's own blocks, one unowned block per
        # sequence (its unused table entries point there)
        B = 1 + sum(nblk) + S
        self.k = 0.1 * torch.randn(B, hk, BLOCK, head_dim, generator=gen)
        self.v = torch.randn(B, hk, BLOCK, head_dim, generator=gen)
        ids = (1 + torch.randperm(B - 1, generator=gen)).to(torch.int32)
        self.tables = torch.empty(S, width, dtype=torch.int32)
        self.k_bad = float("nan") if nan_pads else None
        self.v_bad = float("nan") if nan_pads else POISON_V
        nxt = 0
        for s in range(S):
            self.tables[s, :nblk[s]] = ids[nxt:nxt + nblk[s]]
            nxt += nblk[s]
        for s in range(S):
            unowned = int(ids[nxt + s])
            self.tables[s, nblk[s]:] = unowned
            self._poison(s, unowned, slice(None))
            pad0 = kv_lens[s] % BLOCK
            if pad0:
                self._poison(s, int(self.tables[s, nblk[s] - 1]),
                             slice(pad0, None))
        self._poison(0, 0, slice(None))

    def _poison(self, s, block, slots):
        for kv in range(self.hk):
            if self.k_bad is None:
                self.k[block, kv, slots] = POISON_GAIN * _sign(
                    self.aim[s][kv * self.group])
            else:
                self.k[block, kv, slots] = self.k_bad
        self.v[block, :, slots] = self.v_bad

    def slot(self, s, pos):
        return int(self.tables[s, pos // BLOCK]), pos % BLOCK

    def caches(self, fp8):
        dtype = torch.float8_e4m3fn if fp8 else torch.bfloat16
        return self.k.to(dtype), self.v.to(dtype)


def decode_needle_positions(L: int):
    cand = (0, L - 2, L - 1, PARTITION - 1, PARTITION, 2 * PARTITION - 1,
            2 * PARTITION, ((L - 1) // BLOCK) * BLOCK)
    return sorted({p for p in cand if 0 <= p < L})


def build_decode_case(seq_lens, head_dim, group, fp8=False, table_blocks=None,
                      seed=0):
    """q [S, 2G, D] bf16, k_cache, v_cache [B, 2, 16, D] (bf16 or e4m3),
    block_tables [S, table_blocks] int32, seq_lens [S] int32; all on CPU."""
    gen = torch.Generator().manual_seed(seed)
    hk = DECODE_KV_HEADS
    S = len(seq_lens)
    q = torch.randn(S, hk * group, head_dim, generator=gen).to(torch.bfloat16)
    b = _PagedBuilder(list(seq_lens), [q[s] for s in range(S)], hk, head_dim,
                      table_blocks, gen)
    for s, L in enumerate(seq_lens):
        assert L >= 1
        for i, pos in enumerate(decode_needle_positions(L)):
            blk, off = b.slot(s, pos)
            for kv in range(hk):
                b.k[blk, kv, off] = NEEDLE_GAIN * _sign(
                    q[s, kv * group + i % group])
    k_cache, v_cache = b.caches(fp8)
    return (q, k_cache, v_cache, b.tables,
            torch.tensor(seq_lens, dtype=torch.int32))


def prefill_probe_offsets(new_len: int):
    return sorted({o for o in PROBE_OFFSETS + (new_len - 1,) if o < new_len})


def build_prefill_paged_case(ctx_lens, new_lens, head_dim, hq=8, hk=2,
                             fp8=False, seed=0, nan_pads=False):
    """q [sum(new), Hq, D] bf16 (new tokens only), k_cache, v_cache,
    block_tables int32, cu_seqlens_q [S+1] int32, seq_lens_k [S] int32; CPU.

    ctx_lens are TOTAL context lengths (new tokens included). Probe row i of
    a sequence (absolute position P) aims at kv head i % hk, q head
    (i // hk) % G of it: adjacent probes (31/32, 63/64, ...) land on
    different kv heads, so an anti-needle at P+1 never collides with the
    next probe's needle. (With hk == 1 the needle wins.) Poison is aimed at
    each sequence's last q row. nan_pads=True puts NaN in place of the
    finite poison (pad slots, unowned blocks, block 0)."""
    gen = torch.Generator().manual_seed(seed)
    group = hq // hk
    S = len(ctx_lens)
    cu = [0]
    for n in new_lens:
        cu.append(cu[-1] + n)
    q = torch.randn(cu[-1], hq, head_dim, generator=gen).to(torch.bfloat16)
    b = _PagedBuilder(list(ctx_lens), [q[cu[s + 1] - 1] for s in range(S)],
                      hk, head_dim, None, gen, nan_pads=nan_pads)
    for s in range(S):
        k_len, new = ctx_lens[s], new_lens[s]
        assert 1 <= new <= k_len
        probes = []
        for i, off in enumerate(prefill_probe_offsets(new)):
            kv = i % hk
            aim = _sign(q[cu[s] + off, kv * group + (i // hk) % group])
            probes.append((k_len - new + off, kv, aim))
        for P, kv, aim in probes:      # anti-needles first: needles win
            if P + 1 < k_len:
                blk, o = b.slot(s, P + 1)
                b.k[blk, kv, o] = POISON_GAIN * aim
                b.v[blk, kv, o] = POISON_V
        for P, kv, aim in probes:
            blk, o = b.slot(s, P)
            b.k[blk, kv, o] = NEEDLE_GAIN * aim
    k_cache, v_cache = b.caches(fp8)
    return (q, k_cache, v_cache, b.tables,
            torch.tensor(cu, dtype=torch.int32),
            torch.tensor(ctx_lens, dtype=torch.int32))


def dense_kv_from_paged(k_cache, v_cache, block_tables, seq_lens_k):
    """The same K/V as dense [T, Hk, D] rows (a case with ctx == new)."""
    ks, vs = [], []
    for s in range(seq_lens_k.numel()):
        n = int(seq_lens_k[s])
        for cache, dst in ((k_cache, ks), (v_cache, vs)):
            blocks = block_tables[s, :(n + BLOCK - 1) // BLOCK].long()
            rows = cache[blocks].permute(0, 2, 1, 3)  # [nblk, 16, Hk, D]
            dst.append(rows.reshape(-1, *rows.shape[2:])[:n])
    return torch.cat(ks).contiguous(), torch.cat(vs).contiguous()
