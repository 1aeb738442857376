"""Token sampling: penalties, temperature, top-k/top-p/min-p, per-request
seeds — the vLLM SamplingParams surface the reference's delegated engine
exposes."""

from __future__ import annotations

import copy
from typing import List

import torch

from fusioninfer_amd.engine.sequence import Sequence


BACKENDS = ("torch", "fused")

# unseeded draws of the fused backend take Philox offsets from here up;
# seeded requests use len(output_token_ids), far below
_UNSEEDED_OFFSET_BASE = 1 << 62


def _as_i64(v: int) -> int:
    """Wrap an arbitrary Python int into the int64 range (bit pattern kept)."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def _has_penalties(sp) -> bool:
    return (
        sp.repetition_penalty != 1.0
        or sp.presence_penalty != 0.0
        or sp.frequency_penalty != 0.0
    )


def penalty_params(sp):
    """One row of ops.apply_penalties' params: (rp, inv_rp, presence,
    frequency), to be stored as fp32. inv_rp is the reciprocal taken in
    double and then rounded to fp32 (1.7 gives 0x3f169697, the fp32
    quotient 1 / fp32(1.7) would be 0x3f169696). That rule is empirical:
    it is what reproduces the GPU `x / rp` of the torch build this was
    developed against, bit for bit, at rp = 1.3, 1.7, 0.8 and 1.05; it is
    not a documented torch contract. If a torch upgrade makes
    tests/test_device_penalties_gpu.py fail on repetition-penalised
    entries only, this is the line to revisit."""
    rp = float(sp.repetition_penalty)
    return (rp, 1.0 / rp if rp != 0.0 else float("inf"),
            sp.presence_penalty, sp.frequency_penalty)


def device_logprobs_top(sp) -> int:
    """num_top of ops.token_logprobs for one request: the number of top
    entries when the kernel can serve it (at most ops.LOGPROBS_MAX_TOP),
    -1 when the request has no logprobs or asks for more."""
    from fusioninfer_amd import ops

    if sp.logprobs is None:
        return -1
    k = max(int(sp.logprobs), 0)
    return k if k <= ops.LOGPROBS_MAX_TOP else -1


def bias_arrays(sp, vocab_size: int):
    """A request's logit_bias as (ids int32 [n], values fp32 [n]) tensors,
    ids outside [0, vocab_size) dropped (a bad request is ignored, not an
    error). Built once per SamplingParams and kept on it: the bias is a
    constant of the request."""
    hit = getattr(sp, "_bias_arrays", None)
    if hit is not None and hit[0] == vocab_size:
        return hit[1], hit[2]
    items = [(t, v) for t, v in sp.logit_bias.items()
             if 0 <= t < vocab_size]
    ids = torch.tensor([t for t, _ in items], dtype=torch.int32)
    vals = torch.tensor([v for _, v in items], dtype=torch.float32)
    sp._bias_arrays = (vocab_size, ids, vals)
    return ids, vals


class LogitMods:
    """The logit_bias entries and grammar masks of one sampling pass, as
    ops.apply_logit_mods takes them, laid out for the pass's parameter
    buffer (Sampler._pack_rows):

        mask_ids [T] | masks [M, W]                      (with a mask)
        bias_cu [T + 1] | bias_ids [B] | bias_vals [B]   (with a bias)

    Rows in the same grammar state share one mask. `offset` is the first
    word of this section in the buffer, set by _pack_rows."""

    def __init__(self, T, V, mask_ids, masks, bias_cu, bias_ids, bias_vals):
        self.T, self.V, self.W = T, V, (V + 31) // 32
        self.mask_ids = mask_ids  # list of int, or None
        self.masks = masks  # list of int32 [W] CPU tensors
        self.bias_cu = bias_cu  # list of int, or None
        self.bias_ids = bias_ids  # list of int32 tensors, one per biased row
        self.bias_vals = bias_vals
        self.B = bias_cu[-1] if bias_cu is not None else 0
        self.words = 0
        if mask_ids is not None:
            self.words += T + len(masks) * self.W
        if bias_cu is not None:
            self.words += T + 1 + 2 * self.B
        self.offset = None

    def fill(self, host: torch.Tensor) -> None:
        p, T = self.offset, self.T
        if self.mask_ids is not None:
            host[p:p + T].copy_(torch.tensor(self.mask_ids, dtype=torch.int32))
            p += T
            for m in self.masks:
                host[p:p + self.W].copy_(m)
                p += self.W
        if self.bias_cu is not None:
            host[p:p + T + 1].copy_(
                torch.tensor(self.bias_cu, dtype=torch.int32))
            p += T + 1
            if self.B:
                host[p:p + self.B].copy_(torch.cat(self.bias_ids))
                host[p + self.B:p + 2 * self.B].view(torch.float32).copy_(
                    torch.cat(self.bias_vals))

    def apply(self, logits: torch.Tensor, dev: torch.Tensor) -> None:
        """One ops.apply_logit_mods launch on views of the device copy."""
        from fusioninfer_amd import ops

        p, T = self.offset, self.T
        args = [None] * 5
        if self.mask_ids is not None:
            M = len(self.masks)
            args[0] = dev[p:p + T]
            args[1] = dev[p + T:p + T + M * self.W].view(M, self.W)
            p += T + M * self.W
        if self.bias_cu is not None:
            B = self.B
            args[2] = dev[p:p + T + 1]
            args[3] = dev[p + T + 1:p + T + 1 + B]
            args[4] = dev[p + T + 1 + B:p + T + 1 + 2 * B].view(torch.float32)
        ops.apply_logit_mods(logits, *args)


class DeviceLogprobs:
    """ops.token_logprobs outputs of one step in ONE int32 buffer, so that
    a single copy brings them to the host: chosen [T] fp32 | top_ids [T, W]
    int32 | top_lp [T, W] fp32. num_top is the host list the kernel ran
    with; rows with -1 were skipped and hold nothing."""

    def __init__(self, buf: torch.Tensor, num_top: List[int], width: int):
        self.buf = buf
        self.num_top = num_top
        self.width = width

    @staticmethod
    def sections(buf: torch.Tensor, T: int, W: int):
        return (
            buf[:T].view(torch.float32),
            buf[T:T + T * W].view(T, W),
            buf[T + T * W:].view(torch.float32).view(T, W),
        )

    def entries(self, host_buf: torch.Tensor):
        """host_buf: self.buf (or a host copy of it) once its contents are
        there. One (chosen, {id: logprob}) per row, None for skipped
        rows; the format of Sequence.logprobs."""
        T, W = len(self.num_top), self.width
        chosen, ids, vals = (
            x.tolist() for x in self.sections(host_buf, T, W)
        )
        out = []
        for i, k in enumerate(self.num_top):
            if k < 0:
                out.append(None)
                continue
            out.append((chosen[i], {
                t: v for t, v in zip(ids[i][:k], vals[i][:k]) if t >= 0
            }))
        return out


class PenaltyTable:
    """Device-resident token histograms for penalised sequences (the slot
    idea of lora.LoRASlots): counts [num_slots, V] int32, row = slot. The
    host keeps seq_id -> slot and, per slot, `counted_len`: the number of
    tokens of the owner's history the row holds. ops.apply_penalties reads
    the rows, one ops.penalty_counts_add per step adds the sampled ids
    device to device, so a penalised sequence needs no host round trip
    between steps.

    The table is allocated on the first sync() that has a slot to fill. A
    row is (re)built from seq.all_token_ids whenever counted_len differs
    from the history length: first use, preemption-recompute, a discarded
    late token, tokens appended by another path. Reuse of a released slot
    is safe by stream order: the next owner's zero and build are enqueued
    after any add still in flight."""

    def __init__(self, num_slots: int, device: str = "cpu"):
        self.num_slots = max(int(num_slots), 0)
        self.device = device
        self.counts = None  # [num_slots, V] int32, allocated lazily
        self._slot_of = {}  # seq_id -> slot
        self._counted_len = {}  # slot -> tokens held, -1 = never built
        self._free = list(range(self.num_slots - 1, -1, -1))
        self.num_rebuilds = 0

    def slot_of(self, seq: Sequence) -> int:
        return self._slot_of.get(seq.seq_id, -1)

    def acquire(self, seq: Sequence) -> int:
        """The sequence's slot, taking a free one if it has none; -1 when
        the table is full."""
        slot = self._slot_of.get(seq.seq_id)
        if slot is not None:
            return slot
        if not self._free:
            return -1
        slot = self._free.pop()
        self._slot_of[seq.seq_id] = slot
        self._counted_len[slot] = -1
        return slot

    def release(self, seq: Sequence) -> None:
        slot = self._slot_of.pop(seq.seq_id, None)
        if slot is not None:
            del self._counted_len[slot]
            self._free.append(slot)

    def sync(self, seqs: List[Sequence], vocab_size: int) -> List[int]:
        """Slot per row (-1: no penalties, table full, or sequence already
        finished), with every live row holding exactly the histogram of its
        sequence's history. This is the only place that takes slots. A
        finished sequence can still be sampled for (the pipelined chain
        launches its next step before the stop check of the last one); its
        slot is gone, its token will be discarded, and it must not get a
        slot that nothing would release."""
        from fusioninfer_amd import ops

        slots = []
        for s in seqs:
            slot = -1
            if _has_penalties(s.sampling) and not s.is_finished():
                slot = self.acquire(s)
            slots.append(slot)
            if slot < 0:
                continue
            n = len(s.all_token_ids)
            if self._counted_len[slot] == n:
                continue
            if self.counts is None:
                self.counts = torch.zeros(
                    self.num_slots, vocab_size, dtype=torch.int32,
                    device=self.device,
                )
            self.counts[slot].zero_()
            if n:
                # one H2D copy (the history); the slot ids are a device
                # fill
                ops.penalty_counts_add(
                    self.counts,
                    torch.full((n,), slot, dtype=torch.int32,
                               device=self.device),
                    torch.tensor(s.all_token_ids, dtype=torch.int64).to(
                        self.device),
                )
            self._counted_len[slot] = n
            self.num_rebuilds += 1
        return slots

    def add_sampled(self, slots: List[int], slot_ids: torch.Tensor,
                    sampled: torch.Tensor) -> None:
        """Count this step's sampled ids ([T] int64, on the device) into
        the live rows; slot_ids is `slots` as a device int32 tensor."""
        from fusioninfer_amd import ops

        ops.penalty_counts_add(self.counts, slot_ids, sampled)
        for slot in slots:
            if slot >= 0:
                self._counted_len[slot] += 1


class Sampler:
    def __init__(self, seed: int = 0, device: str = "cpu",
                 backend: str = "torch", penalty_slots: int = 64,
                 device_penalties: bool = True,
                 device_logprobs: bool = True,
                 device_logit_mods: bool = False):
        if backend not in BACKENDS:
            raise ValueError(
                f"sampler backend must be one of {BACKENDS}, got {backend!r}"
            )
        self.device = device
        self.base_seed = seed
        self.backend = backend
        self.num_unseeded_draws = 0  # fused backend: running Philox offset
        # fused backend: penalties from device-resident histograms
        self.penalty_table = None
        if backend == "fused" and device_penalties and penalty_slots > 0:
            self.penalty_table = PenaltyTable(penalty_slots, device)
        # fused backend: logprobs from ops.token_logprobs, no host loop
        self.device_logprobs = backend == "fused" and device_logprobs
        # fused backend, opt-in: logit_bias and grammar masks from one
        # ops.apply_logit_mods launch inside the sampling pass; the engine
        # then applies neither on the host
        self.device_logit_mods = backend == "fused" and device_logit_mods
        self.generator = None
        if device != "cpu":
            self.generator = torch.Generator(device=device)
            self.generator.manual_seed(seed)

    def penalty_slot_available(self, seq: Sequence) -> bool:
        """True when the sequence's penalties can run from the device
        table: it owns a slot, or one is free. Takes nothing."""
        t = self.penalty_table
        return t is not None and (t.slot_of(seq) >= 0 or bool(t._free))

    def penalty_slots_cover(self, seqs: List[Sequence]) -> bool:
        """True when every penalised sequence of the batch that has no slot
        yet can get one at the next sample(). Takes nothing."""
        t = self.penalty_table
        need = sum(
            1 for s in seqs
            if _has_penalties(s.sampling)
            and (t is None or t.slot_of(s) < 0)
        )
        return need == 0 or (t is not None and need <= len(t._free))

    def release_penalty_slot(self, seq: Sequence) -> None:
        if self.penalty_table is not None:
            self.penalty_table.release(seq)

    def _gather_logit_mods(self, rows, V: int):
        """The one place that turns requests into ops.apply_logit_mods
        input, for the plain step and for speculative verification. rows:
        (sequence, grammar state or None) per logits row; the state is the
        cursor's for a plain step and the walked-ahead one for row j of a
        span. Returns a LogitMods, or None when the switch is off or no row
        has a mask or an in-vocabulary bias entry (then nothing is
        allocated, copied or launched for it). An empty mask is the
        engine's business (it finishes such a request before sampling)."""
        if not self.device_logit_mods or not any(
            st is not None or s.sampling.logit_bias for s, st in rows
        ):
            return None
        mask_ids, masks, index = [], [], {}
        cu, ids, vals = [0], [], []
        for s, st in rows:
            mid = -1
            if st is not None:
                words, _ = s.sampling.guided.cache.packed_mask(st)
                mid = index.get(id(words))
                if mid is None:
                    mid = index[id(words)] = len(masks)
                    masks.append(words)
            mask_ids.append(mid)
            n = 0
            if s.sampling.logit_bias:
                b_ids, b_vals = bias_arrays(s.sampling, V)
                n = b_ids.numel()
                if n:
                    ids.append(b_ids)
                    vals.append(b_vals)
            cu.append(cu[-1] + n)
        if not masks:
            mask_ids = None
        if cu[-1] == 0:
            cu = None
        if mask_ids is None and cu is None:
            return None
        return LogitMods(len(rows), V, mask_ids, masks, cu, ids, vals)

    def _apply_penalties(self, logits: torch.Tensor, seqs: List[Sequence]):
        """repetition / presence / frequency penalties on already-emitted
        (prompt + output) tokens, OpenAI/vLLM semantics."""
        for i, s in enumerate(seqs):
            sp = s.sampling
            if (
                sp.repetition_penalty == 1.0
                and sp.presence_penalty == 0.0
                and sp.frequency_penalty == 0.0
            ):
                continue
            token_ids = torch.tensor(
                s.all_token_ids, dtype=torch.long, device=logits.device
            )
            uniq, counts = token_ids.unique(return_counts=True)
            row = logits[i]
            if sp.repetition_penalty != 1.0:
                vals = row[uniq]
                row[uniq] = torch.where(
                    vals > 0,
                    vals / sp.repetition_penalty,
                    vals * sp.repetition_penalty,
                )
            if sp.presence_penalty != 0.0:
                row[uniq] -= sp.presence_penalty
            if sp.frequency_penalty != 0.0:
                row[uniq] -= sp.frequency_penalty * counts.to(row.dtype)
        return logits

    def sample_with_logprobs(self, logits: torch.Tensor,
                             seqs: List[Sequence]):
        """sample() plus, with device_logprobs, one ops.token_logprobs launch
        on the logits the draw saw (after logit_bias, guided masks and
        penalties, before temperature) for the rows device_logprobs_top()
        serves. Returns (token ids, DeviceLogprobs or None); None when no
        row is served, and then nothing is launched or allocated. The
        tokens are those of sample()."""
        num_top = None
        if self.device_logprobs:
            tops = [device_logprobs_top(s.sampling) for s in seqs]
            if any(k >= 0 for k in tops):
                num_top = tops
        if num_top is None:
            return self.sample(logits, seqs), None
        return self._sample(logits, seqs, num_top)

    def _sample(self, logits, seqs, num_top=None):
        """The fused backend's step: (token ids, DeviceLogprobs or None)."""
        slots = None
        if self.penalty_table is not None and any(
            _has_penalties(s.sampling) for s in seqs
        ):
            slots = self.penalty_table.sync(seqs, logits.shape[-1])
        mods = None
        if self.device_logit_mods:
            mods = self._gather_logit_mods(
                [(s, None if s.sampling.guided is None
                  else s.sampling.guided.state) for s in seqs],
                logits.shape[-1],
            )
        if slots is None and mods is None:
            logits = self._apply_penalties(logits, seqs)
        # with mods the host penalties wait until bias and mask are in
        return self._sample_fused(logits, seqs, slots, num_top, mods)

    def sample(self, logits: torch.Tensor, seqs: List[Sequence]) -> torch.Tensor:
        """logits: [S, V] fp32; returns [S] int64 token ids."""
        if self.backend == "fused":
            return self._sample(logits, seqs)[0]
        logits = self._apply_penalties(logits, seqs)
        greedy = logits.argmax(dim=-1)
        # host-side check: avoids a device sync on the (common) all-greedy
        # decode step
        if all(s.sampling.temperature == 0 for s in seqs):
            return greedy
        temps = torch.tensor(
            [s.sampling.temperature for s in seqs],
            dtype=torch.float32,
            device=logits.device,
        )
        scaled = logits / temps.clamp(min=1e-5).unsqueeze(1)

        # top-k then top-p filtering, batched over the rows that need it
        # (the per-row Python loop cost milliseconds/step at batch 256)
        V = logits.shape[-1]
        k_rows = [
            i for i, s in enumerate(seqs)
            if s.sampling.temperature != 0 and 0 < s.sampling.top_k < V
        ]
        if k_rows:
            ks = torch.tensor(
                [seqs[i].sampling.top_k for i in k_rows],
                device=logits.device,
            )
            sub = scaled[k_rows]
            top_vals = torch.topk(sub, int(ks.max()), dim=-1).values
            kth = top_vals.gather(1, (ks - 1).unsqueeze(1))
            scaled[k_rows] = sub.masked_fill(sub < kth, float("-inf"))
        p_rows = [
            i for i, s in enumerate(seqs)
            if s.sampling.temperature != 0 and s.sampling.top_p < 1.0
        ]
        if p_rows:
            ps = torch.tensor(
                [seqs[i].sampling.top_p for i in p_rows],
                device=logits.device,
            ).unsqueeze(1)
            sub = scaled[p_rows]
            sorted_logits, idx = sub.sort(dim=-1, descending=True)
            probs = torch.softmax(sorted_logits, dim=-1)
            cut = probs.cumsum(dim=-1) - probs > ps
            sorted_logits = sorted_logits.masked_fill(cut, float("-inf"))
            scaled[p_rows] = torch.empty_like(sub).scatter_(
                1, idx, sorted_logits
            )

        # min-p (vLLM surface): drop tokens whose probability is below
        # min_p * max-probability of the row
        m_rows = [
            i for i, s in enumerate(seqs)
            if s.sampling.temperature != 0 and s.sampling.min_p > 0.0
        ]
        if m_rows:
            mps = torch.tensor(
                [seqs[i].sampling.min_p for i in m_rows],
                device=logits.device,
            ).unsqueeze(1)
            sub = scaled[m_rows]
            pr = torch.softmax(sub, dim=-1)
            cut = pr < mps * pr.max(dim=-1, keepdim=True).values
            scaled[m_rows] = sub.masked_fill(cut, float("-inf"))

        probs = torch.softmax(scaled, dim=-1)
        sampled = torch.empty_like(greedy)
        # group rows by generator: per-request seeds get their own draw
        default_rows = []
        for i, s in enumerate(seqs):
            sp = s.sampling
            if sp.temperature == 0:
                sampled[i] = greedy[i]
            elif sp.seed is not None:
                g = torch.Generator(device=logits.device)
                g.manual_seed(sp.seed + len(s.output_token_ids))
                sampled[i] = torch.multinomial(probs[i], 1, generator=g)[0]
            else:
                default_rows.append(i)
        if default_rows:
            rows = torch.tensor(default_rows, device=logits.device)
            draw = torch.multinomial(
                probs[rows], 1, generator=self.generator
            ).squeeze(1)
            sampled[rows] = draw
        return sampled

    def _pack_rows(self, rows, slots=None, num_top=None, tail_words=0,
                   mods=None):
        """The host side of one fused sampling pass: per-row parameters in
        ONE int32 buffer, so that a single copy takes them to the device.
        rows: (sequence, j) per logits row, j = tokens the row is ahead of
        the sequence's output (0 for a plain step, the row's index inside
        its span under speculative verification). Layout, T = len(rows):

            [0, 8T)    temperature | top_k | top_p | min_p | rng (T x 2
                       int64: (seed, len(output) + j) for seeded rows,
                       (engine seed, 2^62 + running counter) for unseeded
                       ones, (0, 0) at temperature 0)
            [8T, 13T)  only when a slot of `slots` is live: (rp, 1/rp,
                       presence, frequency) as [T, 4] fp32, then the slots
            + T        only with num_top: one int per row
            + mods     only with `mods` (a LogitMods): its mask_ids, masks
                       and bias CSR, mods.words words; mods.offset is set
                       to the first of them
            + tail    tail_words more words for the caller, starting at an
                       even word (int64 views are possible there)

        Returns (buffer, live, pen_words, tail); pen_words is 13 or 8, tail
        the first word of the caller's part."""
        T = len(rows)
        live = slots is not None and any(slot >= 0 for slot in slots)
        pen_words = 13 if live else 8
        row_words = (pen_words + (1 if num_top is not None else 0)) * T
        words = row_words
        if mods is not None:
            mods.offset = row_words
            words += mods.words
        tail = words + (words & 1)
        temps, ks, ps, mps, rng = [], [], [], [], []
        for s, j in rows:
            sp = s.sampling
            temps.append(sp.temperature)
            ks.append(min(max(int(sp.top_k), 0), 2**31 - 1))
            ps.append(sp.top_p)
            mps.append(sp.min_p)
            if sp.temperature == 0:
                rng.append((0, 0))
            elif sp.seed is not None:
                rng.append((_as_i64(sp.seed), len(s.output_token_ids) + j))
            else:
                rng.append((
                    _as_i64(self.base_seed),
                    _as_i64(_UNSEEDED_OFFSET_BASE + self.num_unseeded_draws),
                ))
                self.num_unseeded_draws += 1
        host = torch.empty(tail + tail_words if tail_words else words,
                           dtype=torch.int32)
        host[:T].view(torch.float32).copy_(torch.tensor(temps))
        host[T:2 * T].copy_(torch.tensor(ks, dtype=torch.int32))
        host[2 * T:3 * T].view(torch.float32).copy_(torch.tensor(ps))
        host[3 * T:4 * T].view(torch.float32).copy_(torch.tensor(mps))
        host[4 * T:8 * T].view(torch.int64).copy_(
            torch.tensor(rng, dtype=torch.int64).flatten()
        )
        if live:
            host[8 * T:12 * T].view(torch.float32).copy_(torch.tensor(
                [penalty_params(s.sampling) for s, _ in rows],
                dtype=torch.float32,
            ).flatten())
            host[12 * T:13 * T].copy_(torch.tensor(slots, dtype=torch.int32))
        if num_top is not None:
            host[pen_words * T:row_words].copy_(
                torch.tensor(num_top, dtype=torch.int32))
        if mods is not None:
            mods.fill(host)
        return host, live, pen_words, tail

    def _sample_fused(self, logits: torch.Tensor, seqs: List[Sequence],
                      slots=None, num_top=None, mods=None):
        """One ops.sample_tokens call for the whole mixed batch. The per-row
        parameters are laid out in one host buffer of 8 int32 words per row
        (temperature | top_k | top_p | min_p | rng as 2 x int64) and reach
        the device in a single copy. Seeded rows draw at (seed,
        len(output_token_ids)), unseeded rows at (engine seed, 2^62 +
        running counter): a token depends only on its row and that pair.

        `slots` (PenaltyTable.sync) switches the penalties to the device:
        the same buffer then carries 5 more words per row (rp | 1/rp |
        presence | frequency as [T, 4] fp32, then the slot ids), one
        ops.apply_penalties runs before the draw and one
        ops.penalty_counts_add after it. Penalised rows that got no slot
        take the host _apply_penalties, row by row.

        `num_top` (one int per row, see device_logprobs_top) adds one more
        word per row at the end of the buffer and one ops.token_logprobs
        launch after the draw, on the same logits and the sampled ids.

        `mods` (_gather_logit_mods) appends the step's packed grammar masks
        and logit_bias entries to the same buffer; one ops.apply_logit_mods
        runs first, so penalties, the draw and the logprobs all see bias
        and mask, in the order of the host path.
        Returns (sampled ids, DeviceLogprobs or None)."""
        from fusioninfer_amd import ops

        T = len(seqs)
        host, live, pen_words, _ = self._pack_rows(
            [(s, 0) for s in seqs], slots, num_top, mods=mods)
        dev = host.to(logits.device)
        if logits.dtype != torch.float32:
            logits = logits.float()
        logits = logits.contiguous()
        if mods is not None:
            mods.apply(logits, dev)
            if slots is None:
                self._apply_penalties(logits, seqs)
        if slots is not None:
            for i, s in enumerate(seqs):
                # a finished sequence's token is discarded: no host sync
                # for it either
                if (slots[i] < 0 and _has_penalties(s.sampling)
                        and not s.is_finished()):
                    self._apply_penalties(logits[i:i + 1], [s])
        if live:
            slot_ids = dev[12 * T:13 * T]
            ops.apply_penalties(
                logits, self.penalty_table.counts, slot_ids,
                dev[8 * T:12 * T].view(torch.float32).view(T, 4),
            )
        sampled = ops.sample_tokens(
            logits,
            dev[:T].view(torch.float32),
            dev[T:2 * T],
            dev[2 * T:3 * T].view(torch.float32),
            dev[3 * T:4 * T].view(torch.float32),
            dev[4 * T:8 * T].view(torch.int64).view(T, 2),
        )
        if live:
            self.penalty_table.add_sampled(slots, slot_ids, sampled)
        if num_top is None:
            return sampled, None
        # as wide as the widest request of the step: less to copy back
        W = max(max(num_top), 1)
        buf = torch.empty(T * (1 + 2 * W), dtype=torch.int32,
                          device=logits.device)
        ops.token_logprobs(
            logits, sampled, dev[pen_words * T:(pen_words + 1) * T],
            out=DeviceLogprobs.sections(buf, T, W),
        )
        return sampled, DeviceLogprobs(buf, num_top, W)

    def verify_drafts(self, logits: torch.Tensor, spans):
        """Speculative verification for every drafted span of a step, in
        one pass (fused backend only).

        spans: (sequence, draft tokens) in row order; a span with k drafts
        owns 1 + k rows of logits [R, V]: row j holds the target's logits
        after the history plus drafts[:j]. Both proposers draft
        deterministically, so the draft distribution is one-hot and
        rejection sampling is exact in this form: every row is sampled from
        the target distribution with the span's parameters (row j of a
        seeded request at (seed, len(output) + j), the pair the plain fused
        step would use there), draft j is accepted iff row j's sample equals
        it (probability p(draft)), and the first mismatching sample is the
        corrected token (p restricted to != draft, the residual
        distribution). Greedy spans are the temperature-0 case of the same
        kernel.

        Row j's penalties count the history plus drafts[:j]
        (ops.apply_penalties_spec on the span's PenaltyTable row); after
        ops.spec_accept the emitted tokens are added to the table device
        to device and counted_len advances by the number emitted. If the
        engine then stops inside the span (stop token), counted_len and the
        history disagree, and the slot is released or rebuilt at its next
        sync. Penalised spans without a slot take the host
        _apply_penalties row by row. Logprobs come from one
        ops.token_logprobs launch over all rows, after penalties and before
        temperature.

        With device_logit_mods, one ops.apply_logit_mods runs in front of
        all that: every row of a biased span gets the bias, and row j of a
        guided span the mask of the grammar state after drafts[:j]
        (GuidedDecoder.walk; the draft must stay inside the grammar, which
        the engine's trimming guarantees). Its input rides in the same
        host-to-device copy.

        One host-to-device copy (parameters, drafts, span bounds), at most
        two back (emitted tokens + counts; the logprobs buffer). Returns
        (emitted: list of token lists, accepted: list of int, logprobs:
        list with, per span, the entries of its emitted rows or None — or
        None when no span asked)."""
        from fusioninfer_amd import ops

        if self.backend != "fused":
            raise RuntimeError("verify_drafts needs the fused sampler backend")
        S = len(spans)
        V = logits.shape[-1]
        rows, cu = [], [0]
        for seq, draft in spans:
            if len(draft) > ops.SPEC_MAX_DRAFT:
                raise ValueError(
                    f"verify_drafts: a draft of {len(draft)} tokens exceeds "
                    f"SPEC_MAX_DRAFT = {ops.SPEC_MAX_DRAFT}")
            rows.extend((seq, j) for j in range(len(draft) + 1))
            cu.append(len(rows))
        R = len(rows)
        if S < 1 or tuple(logits.shape) != (R, V):
            raise ValueError(
                f"verify_drafts: {S} spans with {R} rows, logits "
                f"{tuple(logits.shape)}")
        W = max(len(d) for _, d in spans) + 1
        E = max(W - 1, 1)
        span_seqs = [seq for seq, _ in spans]
        penalised = [_has_penalties(s.sampling) for s in span_seqs]
        span_slots = [-1] * S
        if self.penalty_table is not None and any(penalised):
            span_slots = self.penalty_table.sync(span_seqs, V)
        slots = [span_slots[i] for i in range(S) for _ in range(cu[i], cu[i + 1])]
        num_top = None
        if self.device_logprobs:
            span_top = [device_logprobs_top(s.sampling) for s in span_seqs]
            if any(k >= 0 for k in span_top):
                num_top = [span_top[i] for i in range(S)
                           for _ in range(cu[i], cu[i + 1])]

        mods = None
        if self.device_logit_mods:
            row_states = []
            for seq, draft in spans:
                g = seq.sampling.guided
                if g is None:
                    row_states.extend((seq, None) for _ in range(len(draft) + 1))
                    continue
                # row j: the state after drafts[:j], the cursor stays put
                states = g.walk(draft)
                if len(states) != len(draft) + 1:
                    raise ValueError(
                        f"verify_drafts: the draft of {seq.seq_id} leaves "
                        f"its grammar at token {max(len(states) - 1, 0)}; "
                        "trim it first (GuidedDecoder.valid_draft_len)")
                row_states.extend((seq, st) for st in states)
            mods = self._gather_logit_mods(row_states, V)

        live = any(slot >= 0 for slot in span_slots)
        # the caller's part of the buffer: drafts [R] int64 | extra [R, E]
        # int64 (live only) | span_cu [S + 1] | span slots [S] (live only)
        n_extra = 2 * R * E if live else 0
        tail_words = 2 * R + n_extra + (S + 1) + (S if live else 0)
        host, _, pen_words, tail = self._pack_rows(
            rows, slots, num_top, tail_words, mods)
        drafts_h = host[tail:tail + 2 * R].view(torch.int64)
        drafts_h.fill_(-1)
        for i, (_, d) in enumerate(spans):
            if d:
                drafts_h[cu[i]:cu[i] + len(d)] = torch.tensor(
                    d, dtype=torch.int64)
        p = tail + 2 * R
        if live:
            extra_h = host[p:p + n_extra].view(torch.int64).view(R, E)
            extra_h.fill_(-1)
            for i, (_, d) in enumerate(spans):
                for j in range(1, len(d) + 1):
                    extra_h[cu[i] + j, :j] = drafts_h[cu[i]:cu[i] + j]
            p += n_extra
        host[p:p + S + 1].copy_(torch.tensor(cu, dtype=torch.int32))
        if live:
            host[p + S + 1:].copy_(torch.tensor(span_slots, dtype=torch.int32))
        dev = host.to(logits.device)

        if logits.dtype != torch.float32:
            logits = logits.float()
        logits = logits.contiguous()
        if mods is not None:
            # bias and masks first, as on the host path
            mods.apply(logits, dev)
        for i, (seq, d) in enumerate(spans):
            if penalised[i] and span_slots[i] < 0:
                # no slot: the host ops, on the history as row j sees it
                for j in range(len(d) + 1):
                    ahead = copy.copy(seq)
                    ahead.output_token_ids = seq.output_token_ids + d[:j]
                    r = cu[i] + j
                    self._apply_penalties(logits[r:r + 1], [ahead])
        drafts_d = dev[tail:tail + 2 * R].view(torch.int64)
        q = tail + 2 * R
        if live:
            counts = self.penalty_table.counts
            ops.apply_penalties_spec(
                logits, counts, dev[12 * R:13 * R],
                dev[8 * R:12 * R].view(torch.float32).view(R, 4),
                dev[q:q + n_extra].view(torch.int64).view(R, E),
            )
            q += n_extra
        sampled = ops.sample_tokens(
            logits,
            dev[:R].view(torch.float32),
            dev[R:2 * R],
            dev[2 * R:3 * R].view(torch.float32),
            dev[3 * R:4 * R].view(torch.float32),
            dev[4 * R:8 * R].view(torch.int64).view(R, 2),
        )
        acc = torch.empty(ops.spec_accept_words(S, W), dtype=torch.int64,
                          device=logits.device)
        emitted_d, _ = ops.spec_accept(
            sampled, drafts_d, dev[q:q + S + 1], W, out=acc)
        if live:
            # -1 columns (rejected tail) and -1 slots are skipped there
            ops.penalty_counts_add(
                counts,
                dev[q + S + 1:].view(S, 1).expand(S, W).reshape(-1),
                emitted_d.reshape(-1),
            )
        lp = None
        if num_top is not None:
            LW = max(max(num_top), 1)
            buf = torch.empty(R * (1 + 2 * LW), dtype=torch.int32,
                              device=logits.device)
            ops.token_logprobs(
                logits, sampled, dev[pen_words * R:(pen_words + 1) * R],
                out=DeviceLogprobs.sections(buf, R, LW),
            )
            lp = DeviceLogprobs(buf, num_top, LW)

        em_h, n_h = ops.spec_accept_sections(acc.cpu(), S, W)
        em_h, n_h = em_h.tolist(), n_h.tolist()
        emitted = [em_h[i][:n_h[i]] for i in range(S)]
        accepted = [max(n - 1, 0) for n in n_h]
        for slot, n in zip(span_slots, n_h):
            if slot >= 0:
                self.penalty_table._counted_len[slot] += n
        if lp is None:
            return emitted, accepted, None
        entries = lp.entries(lp.buf.cpu())
        logprobs = [
            entries[cu[i]:cu[i] + n_h[i]] if span_top[i] >= 0 else None
            for i in range(S)
        ]
        return emitted, accepted, logprobs
