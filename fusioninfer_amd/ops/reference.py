"""Pure-PyTorch fp32 reference implementations of every HIP op.

These are (a) the numerics oracle the GPU kernels are tested against and
(b) the CPU execution path for tests in GPU-less environments. They are
intentionally simple and allocate freely — never used on the GPU hot path
(ops/__init__.py raises if the HIP extension is missing on a GPU box).
"""

from __future__ import annotations

import torch


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """RMSNorm over the last dim. Computes in fp32, returns x.dtype."""
    xf = x.float()
    var = xf.pow(2).mean(dim=-1, keepdim=True)
    out = xf * torch.rsqrt(var + eps) * weight.float()
    return out.to(x.dtype)


def fused_add_rms_norm(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
):
    """residual = residual + x; out = rms_norm(residual). Returns (out, residual)."""
    new_residual = (residual.float() + x.float()).to(x.dtype)
    return rms_norm(new_residual, weight, eps), new_residual


def silu_and_mul(x: torch.Tensor) -> torch.Tensor:
    """x: [..., 2*I] (gate | up) -> silu(gate) * up, in fp32."""
    gate, up = x.float().chunk(2, dim=-1)
    return (torch.nn.functional.silu(gate) * up).to(x.dtype)


def quant_fp8_rows(x: torch.Tensor):
    """Per-row dynamic OCP-e4m3 quantization: (x_fp8 [T, C], scale [T] fp32)."""
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True).clamp(min=1e-8)
    scale = amax / 448.0
    x_fp8 = (xf / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return x_fp8, scale.squeeze(-1)


def rms_norm_fp8(x: torch.Tensor, weight: torch.Tensor, eps: float):
    return quant_fp8_rows(rms_norm(x, weight, eps))


def fused_add_rms_norm_fp8(
    x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float
):
    out, new_residual = fused_add_rms_norm(x, residual, weight, eps)
    x_fp8, scale = quant_fp8_rows(out)
    return x_fp8, scale, new_residual


def silu_and_mul_fp8(x: torch.Tensor):
    return quant_fp8_rows(silu_and_mul(x))


def _llama3_scale_inv_freq(inv_freq: torch.Tensor, sc: dict) -> torch.Tensor:
    """Llama-3.1 rope scaling (HF rope_scaling rope_type="llama3"):
    low-frequency bands are divided by `factor`, high-frequency bands
    kept, with a smooth ramp between (per-wavelength interpolation)."""
    import math

    factor = float(sc.get("factor", 8.0))
    low = float(sc.get("low_freq_factor", 1.0))
    high = float(sc.get("high_freq_factor", 4.0))
    orig = float(sc.get("original_max_position_embeddings", 8192))
    wavelen = 2 * math.pi / inv_freq
    low_wl = orig / low
    high_wl = orig / high
    scaled = torch.where(wavelen > low_wl, inv_freq / factor, inv_freq)
    smooth = (orig / wavelen - low) / (high - low)
    mid = (1 - smooth) * inv_freq / factor + smooth * inv_freq
    is_mid = (wavelen <= low_wl) & (wavelen >= high_wl)
    return torch.where(is_mid, mid, scaled)


def compute_cos_sin_cache(
    head_dim: int, max_positions: int, theta: float, device=None,
    rope_scaling=None,
) -> torch.Tensor:
    """[max_positions, head_dim] fp32; first half cos, second half sin (NeoX).
    rope_scaling: None, or an HF-style dict ({"rope_type": "llama3", ...}
    — the Llama-3.1 long-context frequency remap)."""
    inv_freq = 1.0 / (
        theta ** (torch.arange(0, head_dim, 2, dtype=torch.float32, device=device) / head_dim)
    )
    if rope_scaling:
        kind = rope_scaling.get("rope_type") or rope_scaling.get("type")
        if kind == "llama3":
            inv_freq = _llama3_scale_inv_freq(inv_freq, rope_scaling)
        elif kind == "linear":
            inv_freq = inv_freq / float(rope_scaling.get("factor", 1.0))
        else:
            raise ValueError(f"unsupported rope_scaling {kind!r}")
    t = torch.arange(max_positions, dtype=torch.float32, device=device)
    freqs = torch.outer(t, inv_freq)  # [P, D/2]
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1)


def _apply_rope_neox(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x: [T, H, D]; cos/sin: [T, D/2]. Rotate-half (NeoX) style, fp32."""
    d2 = x.shape[-1] // 2
    x1, x2 = x[..., :d2], x[..., d2:]
    cos = cos.unsqueeze(1)
    sin = sin.unsqueeze(1)
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


def rope_qk_norm(
    q: torch.Tensor,
    k: torch.Tensor,
    positions: torch.Tensor,
    cos_sin: torch.Tensor,
    q_weight=None,
    k_weight=None,
    eps: float = 1e-6,
):
    """Optional per-head RMSNorm (Qwen3 qk-norm) then NeoX RoPE.

    q: [T, Hq, D], k: [T, Hk, D], positions: [T] int. Returns new (q, k).
    """
    dtype = q.dtype
    qf, kf = q.float(), k.float()
    if q_weight is not None:
        qf = rms_norm(qf, q_weight, eps)
    if k_weight is not None:
        kf = rms_norm(kf, k_weight, eps)
    d2 = q.shape[-1] // 2
    cs = cos_sin[positions]  # [T, D]
    cos, sin = cs[:, :d2], cs[:, d2:]
    qf = _apply_rope_neox(qf.float(), cos, sin)
    kf = _apply_rope_neox(kf.float(), cos, sin)
    return qf.to(dtype), kf.to(dtype)


def reshape_and_cache(
    k: torch.Tensor,
    v: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    slot_mapping: torch.Tensor,
    k_inv_scale: float = 1.0,
    v_inv_scale: float = 1.0,
):
    """k/v: [T, Hk, D]; caches: [num_blocks, Hk, block_size, D]; slots: [T].
    fp8 caches quantize at the inverse per-layer static scale (matching
    the HIP kernel); bf16 caches store unscaled."""
    block_size = k_cache.shape[2]
    blk = torch.div(slot_mapping, block_size, rounding_mode="floor")
    off = slot_mapping % block_size
    if k_cache.dtype == torch.float8_e4m3fn:
        # clamp to +-448: v_cvt_pk_fp8_f32 SATURATES out-of-range values
        # where torch's .to(e4m3) would produce NaN
        k_cache[blk, :, off] = (k.float() * k_inv_scale).clamp(
            -448.0, 448.0).to(k_cache.dtype)
        v_cache[blk, :, off] = (v.float() * v_inv_scale).clamp(
            -448.0, 448.0).to(v_cache.dtype)
    else:
        k_cache[blk, :, off] = k.to(k_cache.dtype)
        v_cache[blk, :, off] = v.to(v_cache.dtype)


def paged_attention_decode(
    q: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,
    seq_lens: torch.Tensor,
    scale: float,
) -> torch.Tensor:
    """One-token attention per sequence against the paged cache.

    q: [S, Hq, D]; caches: [B, Hk, bs, D]; block_tables: [S, max_blocks];
    seq_lens: [S] (context length INCLUDING the current token). fp32 math.
    """
    num_seqs, num_heads, head_dim = q.shape
    num_kv_heads = k_cache.shape[1]
    bs = k_cache.shape[2]
    group = num_heads // num_kv_heads
    out = torch.empty_like(q, dtype=torch.float32)
    for s in range(num_seqs):
        ctx = int(seq_lens[s])
        nblk = (ctx + bs - 1) // bs
        blocks = block_tables[s, :nblk].long()
        # [Hk, nblk*bs, D]
        keys = k_cache[blocks].permute(1, 0, 2, 3).reshape(num_kv_heads, -1, head_dim)
        vals = v_cache[blocks].permute(1, 0, 2, 3).reshape(num_kv_heads, -1, head_dim)
        keys = keys[:, :ctx].float()
        vals = vals[:, :ctx].float()
        qh = q[s].float()  # [Hq, D]
        for h in range(num_heads):
            kv_h = h // group
            scores = keys[kv_h] @ qh[h] * scale  # [ctx]
            p = torch.softmax(scores, dim=-1)
            out[s, h] = p @ vals[kv_h]
    return out.to(q.dtype)


def prefill_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens: torch.Tensor,
    scale: float,
    causal: bool = True,
) -> torch.Tensor:
    """Varlen causal attention, dense (non-paged) K/V.

    q: [T, Hq, D]; k/v: [T, Hk, D]; cu_seqlens: [num_seqs+1] int32.
    """
    T, num_heads, head_dim = q.shape
    num_kv_heads = k.shape[1]
    group = num_heads // num_kv_heads
    out = torch.empty_like(q, dtype=torch.float32)
    for i in range(cu_seqlens.numel() - 1):
        s, e = int(cu_seqlens[i]), int(cu_seqlens[i + 1])
        L = e - s
        qf = q[s:e].float()  # [L, Hq, D]
        kf = k[s:e].float()
        vf = v[s:e].float()
        for h in range(num_heads):
            kv_h = h // group
            scores = qf[:, h] @ kf[:, kv_h].T * scale  # [L, L]
            if causal:
                mask = torch.triu(
                    torch.ones(L, L, dtype=torch.bool, device=q.device), diagonal=1
                )
                scores = scores.masked_fill(mask, float("-inf"))
            p = torch.softmax(scores, dim=-1)
            out[s:e, h] = p @ vf[:, kv_h]
    return out.to(q.dtype)


def prefill_attention_paged(
    q: torch.Tensor,            # [Tnew, Hq, D] (new tokens only)
    k_cache: torch.Tensor,      # [B, Hk, bs, D]
    v_cache: torch.Tensor,
    block_tables: torch.Tensor,  # [S, max_blocks]
    cu_seqlens_q: torch.Tensor,  # [S+1] over NEW tokens
    seq_lens_k: torch.Tensor,    # [S] total context length
    scale: float,
) -> torch.Tensor:
    """Context attention: new tokens attend over the paged cache (which
    already contains their own K/V plus any cached prefix)."""
    Tn, num_heads, head_dim = q.shape
    num_kv_heads = k_cache.shape[1]
    bs = k_cache.shape[2]
    group = num_heads // num_kv_heads
    out = torch.empty_like(q, dtype=torch.float32)
    for s in range(cu_seqlens_q.numel() - 1):
        qs, qe = int(cu_seqlens_q[s]), int(cu_seqlens_q[s + 1])
        q_len = qe - qs
        k_len = int(seq_lens_k[s])
        ctx_start = k_len - q_len
        nblk = (k_len + bs - 1) // bs
        blocks = block_tables[s, :nblk].long()
        keys = k_cache[blocks].permute(1, 0, 2, 3).reshape(num_kv_heads, -1, head_dim)
        vals = v_cache[blocks].permute(1, 0, 2, 3).reshape(num_kv_heads, -1, head_dim)
        keys = keys[:, :k_len].float()
        vals = vals[:, :k_len].float()
        qf = q[qs:qe].float()  # [q_len, Hq, D]
        # causal mask with context offset
        kv_pos = torch.arange(k_len, device=q.device)
        q_pos = ctx_start + torch.arange(q_len, device=q.device)
        mask = kv_pos.unsqueeze(0) > q_pos.unsqueeze(1)  # [q_len, k_len]
        for h in range(num_heads):
            kv_h = h // group
            scores = qf[:, h] @ keys[kv_h].T * scale
            scores = scores.masked_fill(mask, float("-inf"))
            p = torch.softmax(scores, dim=-1)
            out[qs:qe, h] = p @ vals[kv_h]
    return out.to(q.dtype)


def gather_kv_blocks(
    k_cache: torch.Tensor, v_cache: torch.Tensor, block_ids: torch.Tensor
) -> torch.Tensor:
    """Pack the given cache blocks into one contiguous staging buffer.

    Returns [2, nblocks, Hk, bs, D] (K plane then V plane) — a single large
    contiguous tensor so the PD handoff is one RCCL send per batch of blocks.
    """
    idx = block_ids.long()
    return torch.stack([k_cache[idx], v_cache[idx]], dim=0).contiguous()


def scatter_kv_blocks(
    staging: torch.Tensor,
    k_cache: torch.Tensor,
    v_cache: torch.Tensor,
    block_ids: torch.Tensor,
):
    idx = block_ids.long()
    k_cache[idx] = staging[0].to(k_cache.dtype)
    v_cache[idx] = staging[1].to(v_cache.dtype)


# ---------------------------------------------------------------- MoE

def unpack_moe_weights(b_packed: torch.Tensor) -> torch.Tensor:
    """Inverse of ops.pack_moe_weights: [E, K/32, N/16, 64, 8] -> [E, K, N]."""
    E, K32, N16, _, _ = b_packed.shape
    return (
        b_packed.view(E, K32, N16, 4, 16, 8)
        .permute(0, 1, 3, 5, 2, 4)
        .reshape(E, K32 * 32, N16 * 16)
        .contiguous()
    )


def moe_gemm(out, a, b_packed, sorted_ids, expert_ids, n_valid,
             block_m: int, gate_up: bool):
    """fp32 reference of the grouped GEMM (CPU; same semantics as the HIP
    kernel incl. padding rows computed from the dummy token row)."""
    w = unpack_moe_weights(b_packed).float()
    n_tiles = int(n_valid.item())
    N = out.shape[1]
    for mt in range(n_tiles):
        e = int(expert_ids[mt])
        r0 = mt * block_m
        rows = slice(r0, r0 + block_m)
        if gate_up:
            src = a[sorted_ids[rows].long()].float()
        else:
            src = a[rows].float()
        acc = src @ w[e]
        if gate_up:
            g, u = acc[:, :N], acc[:, N:]
            acc = torch.nn.functional.silu(g) * u
        out[rows] = acc.to(out.dtype)
    return out


def moe_combine(out, y, pos, w):
    T, H = out.shape
    topk = pos.numel() // T
    acc = torch.zeros(T, H, dtype=torch.float32)
    yv = y.float()
    for t in range(T):
        for k in range(topk):
            p = int(pos[t * topk + k])
            if p < 0:
                continue
            acc[t] += float(w[t * topk + k]) * yv[p]
    out.copy_(acc.to(out.dtype))
    return out


def moe_gemm_fp8(out, a, a_scales, b_packed, b_scales, sorted_ids,
                 expert_ids, n_valid, block_m: int, gate_up: bool):
    """fp32 reference of the grouped fp8 GEMM (dequant then matmul)."""
    E = b_packed.shape[0]
    w = unpack_moe_weights(b_packed.view(torch.int8)).view(
        torch.float8_e4m3fn).float()          # [E, K, NB]
    NB = w.shape[2]
    ws = b_scales.view(E, NB).float()
    n_tiles = int(n_valid.item())
    N = out.shape[1]
    af = a.float() * a_scales.unsqueeze(1).float()
    for mt in range(n_tiles):
        e = int(expert_ids[mt])
        r0 = mt * block_m
        rows = slice(r0, r0 + block_m)
        if gate_up:
            src = af[sorted_ids[rows].long()]
        else:
            src = af[rows]
        acc = src @ (w[e] * ws[e].unsqueeze(0))
        if gate_up:
            g, u = acc[:, :N], acc[:, N:]
            acc = torch.nn.functional.silu(g) * u
        out[rows] = acc.to(out.dtype)
    return out


def lora_apply(out, x, slot_ids, a_stack, b_stack, scales):
    """fp32 reference of the batched multi-LoRA apply (in place on out):
    out[t] += scales[s] * bf16(x[t] @ a_stack[s].T) @ b_stack[s].T with
    s = slot_ids[t]. The shrink result is rounded to bf16 once (as the
    HIP kernels and the per-adapter torch loop do); scale and add run in
    fp32. Rows whose id is outside [0, S) are left untouched."""
    S = a_stack.shape[0]
    ids = slot_ids.long()
    for s in torch.unique(ids).tolist():
        if s < 0 or s >= S:
            continue
        rows = (ids == s).nonzero().flatten()
        y = (x[rows].float() @ a_stack[s].float().T).to(torch.bfloat16)
        delta = y.float() @ b_stack[s].float().T
        out[rows] = (
            out[rows].float() + float(scales[s]) * delta
        ).to(out.dtype)
    return out


# ---------------------------------------------------------------- sampling

_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in pure Python integers.
    counter: 4 u32 words, key: 2 u32 words; returns the 4 output words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (
            (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32,
        )
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return (c0, c1, c2, c3)


def sample_row(x, temperature, top_k, top_p, min_p, seed, offset,
               slack: float = 0.0):
    """One row of sample_tokens. Returns (token, margin, kept): kept is the
    bool mask of tokens that survive the filters (None for a greedy or
    non-finite row, whose margin is inf). `slack` widens the top-p test by
    slack * Z_k and the min-p test by slack * min_p in the keep direction
    (for set-membership checks of tokens drawn with another expf).

    Semantics (shared with sampling.hip): z = x / max(temperature, 1e-5),
    m = max z, w = floor(exp(z - m) * 2^32) as integers; top-k keeps
    z >= k-th largest (ties kept); top-p keeps i iff the mass of top-k
    survivors strictly above z_i is <= floor(floor(p * 2^32) * Z_k / 2^32);
    min-p keeps exp(z - m) >= min(min_p, 1); the draw takes
    r = (philox(seed, offset)[0] * Z) >> 32 and returns the first kept
    index whose inclusive prefix mass exceeds r. Tokens more than ~22.18
    below the max have w = 0 and are unreachable."""
    x = x.detach().to("cpu", torch.float32)
    V = x.numel()
    best = x.max()
    bi = int((x == best).nonzero()[0]) if not torch.isnan(best) else 0
    inf = float("inf")
    temp = torch.as_tensor(temperature, dtype=torch.float32)
    if float(temp) == 0.0 or not (-inf < float(best) < inf):
        return (bi if float(best) > -inf else 0), inf, None
    t = temp.clamp(min=1e-5)
    z = x / t + 0.0
    m = z.max()
    e = torch.exp(z - m)
    w = torch.floor(e.double() * 4294967296.0).to(torch.int64)
    keep = torch.ones(V, dtype=torch.bool)
    margin = inf
    k = int(top_k)
    if 0 < k < V:
        keep &= z >= torch.topk(z, k).values[-1]
    p = float(torch.as_tensor(top_p, dtype=torch.float32))
    if p < 1.0:
        p_fix = int(p * 4294967296.0) if p > 0.0 else 0
        s_idx = keep.nonzero().flatten()
        zs, order = z[s_idx].sort(descending=True, stable=True)
        ws = w[s_idx][order]
        zk = int(ws.sum())
        P = (p_fix * zk) >> 32
        _, inverse, counts = torch.unique_consecutive(
            zs, return_inverse=True, return_counts=True
        )
        group_mass = torch.zeros(counts.numel(), dtype=torch.int64)
        group_mass.index_add_(0, inverse, ws)
        above = (group_mass.cumsum(0) - group_mass)[inverse]
        dist = (above - P).abs().min()
        margin = min(margin, float(dist) / zk)
        keep_s = above <= P + int(slack * zk)
        keep = torch.zeros(V, dtype=torch.bool)
        keep[s_idx[order[keep_s]]] = True
    mp = min(float(torch.as_tensor(min_p, dtype=torch.float32)), 1.0)
    if mp > 0.0:
        # expf errors are relative to the weight itself (<= min_p * 2^32
        # near the flip point), so this test's margin and slack are taken
        # relative to the threshold, which is tighter than relative to Z
        keep_mp = e >= torch.tensor(mp, dtype=torch.float32)
        mp_w = mp * 4294967296.0
        dist = (w[keep].double() - mp_w).abs().min()
        margin = min(margin, float(dist) / mp_w)
        if slack > 0.0:
            keep_mp = w.double() >= mp_w * (1.0 - slack)
        keep &= keep_mp
    wk = torch.where(keep, w, torch.zeros_like(w))
    cum = wk.cumsum(0)
    Z = int(cum[-1])
    u = philox4x32_10(
        (int(offset) & _M32, (int(offset) >> 32) & _M32, 0, 0),
        (int(seed) & _M32, (int(seed) >> 32) & _M32),
    )[0]
    r = (u * Z) >> 32
    tok = int(torch.searchsorted(cum, torch.tensor(r), right=True))
    incl = int(cum[tok])
    excl = incl - int(wk[tok])
    if excl > 0:
        margin = min(margin, (r - excl) / Z)
    if incl < Z:
        margin = min(margin, (incl - r) / Z)
    return tok, margin, keep


def sample_tokens(logits, temperature, top_k, top_p, min_p, rng,
                  return_margin: bool = False):
    """Reference of the fused sampling kernel: logits [T, V] fp32,
    temperature / top_p / min_p [T] fp32, top_k [T] int32, rng [T, 2]
    int64 (seed, offset). Returns [T] int64 tokens; with return_margin
    also a [T] float64 tensor with, per row, the smallest relative
    distance (in units of the mass it is compared against) between any
    comparison made (top-p mass test, min-p test, r against the two
    neighbouring prefix sums) and its flip point — inf for greedy rows."""
    T = logits.shape[0]
    toks, margins = [], []
    rng_l = rng.tolist()
    for i in range(T):
        tok, mg, _ = sample_row(
            logits[i], temperature[i], top_k[i], top_p[i], min_p[i],
            rng_l[i][0], rng_l[i][1],
        )
        toks.append(tok)
        margins.append(mg)
    out = torch.tensor(toks, dtype=torch.int64, device=logits.device)
    if return_margin:
        return out, torch.tensor(margins, dtype=torch.float64)
    return out


# ---------------------------------------------------------------- penalties

def apply_penalties(logits, counts, slot_ids, params):
    """Reference of the penalty kernel, in place on logits [T, V] fp32: the
    torch ops of Sampler._apply_penalties, with the row's (token, count)
    pairs read from counts[slot_ids[t]] ([S, V] int32) instead of a
    unique() over the history, and params[t] = (rp, inv_rp, presence,
    frequency) as fp32. Rows whose slot is outside [0, S) and elements
    whose count is 0 are left untouched. The division is torch's own (the
    GPU kernel multiplies by inv_rp, which matched torch's GPU division by
    a scalar on the build it was tested with)."""
    S = counts.shape[0]
    for t, slot in enumerate(slot_ids.tolist()):
        if slot < 0 or slot >= S:
            continue
        _penalise_row(logits[t], counts[slot], params[t].tolist())
    return logits


def _penalise_row(row, hist, param):
    """The sampler's penalty ops on one logits row, for the tokens whose
    count in hist [V] is nonzero."""
    rp, _, presence, frequency = param
    uniq = hist.nonzero().flatten()
    c = hist[uniq]
    if rp != 1.0:
        vals = row[uniq]
        row[uniq] = torch.where(vals > 0, vals / rp, vals * rp)
    if presence != 0.0:
        row[uniq] -= presence
    if frequency != 0.0:
        row[uniq] -= frequency * c.to(row.dtype)


def apply_penalties_spec(logits, counts, slot_ids, params, extra):
    """Reference of the speculative penalty kernel, in place on logits
    [R, V] fp32: apply_penalties with, per row, the histogram
    counts[slot_ids[r]] plus one count for every id of extra[r] ([E] int64)
    that lies in [0, V); other ids (the -1 padding included) are ignored.
    counts itself is not changed."""
    S, V = counts.shape
    ids = extra.tolist()
    for t, slot in enumerate(slot_ids.tolist()):
        if slot < 0 or slot >= S:
            continue
        hist = counts[slot].clone()
        for tok in ids[t]:
            if 0 <= tok < V:
                hist[tok] += 1
        _penalise_row(logits[t], hist, params[t].tolist())
    return logits


def penalty_counts_add(counts, slot_ids, token_ids):
    """counts[slot_ids[i], token_ids[i]] += 1; entries whose slot is outside
    [0, S) or whose token is outside [0, V) are skipped."""
    S, V = counts.shape
    slots = slot_ids.long()
    ok = (slots >= 0) & (slots < S) & (token_ids >= 0) & (token_ids < V)
    flat = slots[ok] * V + token_ids[ok]
    counts.view(-1).index_add_(
        0, flat, torch.ones_like(flat, dtype=counts.dtype)
    )
    return counts


# ------------------------------------------------ logit_bias / grammar masks

def unpack_mask(words, V):
    """bool[V] of a packed mask [ceil(V / 32)] int32: bit (v & 31) of word
    (v >> 5)."""
    shifts = torch.arange(32, dtype=torch.int32, device=words.device)
    bits = (words.unsqueeze(1) >> shifts) & 1
    return bits.flatten()[:V].bool()


def apply_logit_mods(logits, mask_ids, masks, bias_cu, bias_ids, bias_vals):
    """Reference of the logit_mods kernel, in place on logits [T, V] fp32:
    per row the ops of LLMEngine._sample_and_emit's host path, an indexed
    add of the row's bias entries (ids outside [0, V) dropped) and then
    masked_fill_(~allowed, -inf) with the row's unpacked mask. Either half
    may be None. Rows whose mask id is outside [0, M) have no mask; bias_cu
    is clamped to [0, B)."""
    T, V = logits.shape
    if bias_cu is not None:
        B = bias_ids.numel()
        cu = bias_cu.tolist()
        for t in range(T):
            lo, hi = max(cu[t], 0), min(cu[t + 1], B)
            if lo >= hi:
                continue
            ids = bias_ids[lo:hi].long()
            ok = (ids >= 0) & (ids < V)
            if bool(ok.any()):
                logits[t, ids[ok]] += bias_vals[lo:hi][ok]
    if mask_ids is not None:
        M = masks.shape[0]
        for t, mid in enumerate(mask_ids.tolist()):
            if 0 <= mid < M:
                logits[t].masked_fill_(~unpack_mask(masks[mid], V),
                                       float("-inf"))
    return logits


# ---------------------------------------------------------------- logprobs

def token_logprobs(logits, token_ids, num_top, out):
    """Reference of the token_logprobs kernel and its CPU implementation.

    logits [T, V] fp32, token_ids [T] int64, num_top [T] int32, out =
    (chosen [T] fp32, top_ids [T, W] int32, top_lp [T, W] fp32), written in
    place and returned. Per row t with num_top[t] >= 0 (a negative value
    skips the row: nothing of `out` is touched):

        lp = fp32(x - (m + log(sum(exp(x - m)))))   in float64, m = max x
        chosen[t] = lp[token_ids[t]]                NaN outside [0, V)
        k = min(num_top[t], W, V)
        top_ids[t, :k] = the k largest logits' indices, ordered by (logit
            descending, index ascending), -0.0 equal to +0.0
        top_lp[t, :k] = their lp;  columns >= k: id -1, value -inf

    -inf logits are ordinary values with lp = -inf; a row without a finite
    entry has lp = -inf everywhere (no NaN)."""
    chosen, top_ids, top_lp = out
    T, V = logits.shape
    W = top_ids.shape[1]
    toks = token_ids.tolist()
    for t, want in enumerate(num_top.tolist()):
        if want < 0:
            continue
        x = logits[t].double()
        m = x.max()
        if m == float("-inf"):
            lp = torch.full((V,), float("-inf"))
        else:
            lp = (x - (m + torch.log(torch.exp(x - m).sum()))).float()
        tok = toks[t]
        chosen[t] = lp[tok] if 0 <= tok < V else float("nan")
        k = min(want, W, V)
        top_ids[t] = -1
        top_lp[t] = float("-inf")
        if k > 0:
            # a stable descending sort keeps equal values in index order
            idx = torch.sort(logits[t] + 0.0, descending=True,
                             stable=True).indices[:k]
            top_ids[t, :k] = idx.to(top_ids.dtype)
            top_lp[t, :k] = lp[idx]
    return chosen, top_ids, top_lp


# ------------------------------------------------- speculative verification

def spec_accept(sampled, drafts, span_cu, emitted, n_emit):
    """Reference of the spec_accept kernel and its CPU implementation.

    sampled / drafts [R] int64, span_cu [S + 1] int32, emitted [S, W] int64
    and n_emit [S] int32 written in place and returned. Span s owns rows
    [cu[s], cu[s + 1]); it emits its samples up to and including the first
    row whose sample differs from the draft checked there, the last row of
    the span ending it in any case. Unused columns hold -1. An empty span,
    one longer than W or one that leaves [0, R) emits nothing."""
    R = sampled.numel()
    S, W = emitted.shape
    tok, dr, cu = sampled.tolist(), drafts.tolist(), span_cu.tolist()
    emitted.fill_(-1)
    for s in range(S):
        lo, hi = cu[s], cu[s + 1]
        n = 0
        if 0 <= lo < hi <= R and hi - lo <= W:
            for r in range(lo, hi):
                emitted[s, n] = tok[r]
                n += 1
                if r == hi - 1 or tok[r] != dr[r]:
                    break
        n_emit[s] = n
    return emitted, n_emit


# ------------------------------------------------------------------ MXFP4

# e2m1 code -> value; bit 3 is the sign, code 8 (negative zero) reads +0.0
MXFP4_TABLE = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
               0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


def mxfp4_dequant(w_packed: torch.Tensor, w_scale: torch.Tensor) -> torch.Tensor:
    """OCP MXFP4 -> bf16 [N, K], exact. w_packed [N, K/2] uint8 holds k = 2j
    in the low nibble of byte j and k = 2j + 1 in the high nibble; w_scale
    [N, K/32] uint8 is the e8m0 scale 2^(s - 127) of each 32-k block, with
    s in [8, 247] so every product is zero or a normal bf16."""
    N, half = w_packed.shape
    lut = torch.tensor(MXFP4_TABLE, dtype=torch.float32, device=w_packed.device)
    codes = torch.stack((w_packed & 0xF, w_packed >> 4), dim=-1).reshape(N, -1)
    vals = lut[codes.long()]
    # 2^(s - 127) from its bit pattern: exact for every s in [1, 254]
    scale = (w_scale.to(torch.int32) << 23).view(torch.float32)
    out = vals.view(N, -1, 32) * scale.unsqueeze(-1)
    return out.view(N, 2 * half).to(torch.bfloat16)


def mxfp4_linear(x, w_packed, w_scale, bias=None) -> torch.Tensor:
    """x [M, K] bf16 @ dq(W)^T (+ bias) in fp32, rounded to bf16 once."""
    out = x.float() @ mxfp4_dequant(w_packed, w_scale).float().t()
    if bias is not None:
        out = out + bias.float()
    return out.to(torch.bfloat16)


def moe_gemm_mxfp4(out, a, w_packed, w_scale, sorted_ids, expert_ids, n_valid,
                   block_m: int, gate_up: bool):
    """Grouped W4A16 GEMM on MXFP4 expert weights: the CPU path and the
    semantic reference of the HIP kernel. w_packed [E, NB, K/2] and w_scale
    [E, NB, K/32] hold each expert in the row format of mxfp4_linear (NB =
    2N when gate_up: gate rows, then up rows). Only tiles below n_valid are
    touched; sums and the SwiGLU run in fp32 and the result is rounded to
    bf16 once."""
    n_tiles = int(n_valid.item())
    N = out.shape[1]
    dq = {}
    for mt in range(n_tiles):
        e = int(expert_ids[mt])
        if e not in dq:
            dq[e] = mxfp4_dequant(w_packed[e], w_scale[e]).float()  # [NB, K]
        rows = slice(mt * block_m, (mt + 1) * block_m)
        if gate_up:
            src = a[sorted_ids[rows].long()].float()
        else:
            src = a[rows].float()
        acc = src @ dq[e].t()
        if gate_up:
            g, u = acc[:, :N], acc[:, N:]
            acc = torch.nn.functional.silu(g) * u
        out[rows] = acc.to(out.dtype)
    return out
