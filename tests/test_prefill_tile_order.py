"""Heaviest-first prefill tile table (ops.build_prefill_tiles), CPU only.

A causal tile of `rows` q rows starting at row0 of a sequence with ctx
cached tokens and L new ones walks ceil((ctx + min(row0 + rows, L)) / 64)
KV steps of the kernel. The table lists tiles by that cost, descending,
ties by ascending (seq, row0). The kernel hands workgroups out in table
order with all heads of a tile before the next tile, so the second half of
this file replays that order through a list scheduler.
"""

import heapq

import pytest

import fusioninfer_amd.ops as ops

NEW_LENS = [1, 63, 257, 300, 513, 1024]
CTX_STARTS = [0, 17, 403, 0, 487, 64]


def _cost(ctx, L, row0, rows):
    return -(-(ctx + min(row0 + rows, L)) // 64)


def _pairs(table):
    tile_seq, tile_row0 = table
    return list(zip(tile_seq.tolist(), tile_row0.tolist()))


@pytest.mark.parametrize("rows", [128, 256])
@pytest.mark.parametrize("ctx", [CTX_STARTS, None], ids=["ctx", "noctx"])
def test_table_is_sorted_permutation(rows, ctx):
    asc = ops.build_prefill_tiles(NEW_LENS, rows=rows, ctx_starts=ctx,
                                  heaviest_first=False)
    new = ops.build_prefill_tiles(NEW_LENS, rows=rows, ctx_starts=ctx,
                                  heaviest_first=True)
    for t in (*asc, *new):
        assert str(t.dtype) == "torch.int32" and t.dim() == 1
    want_asc = [(s, r0) for s, L in enumerate(NEW_LENS)
                for r0 in range(0, L, rows)]
    assert _pairs(asc) == want_asc
    got = _pairs(new)
    assert sorted(got) == want_asc                     # a permutation
    starts = ctx or [0] * len(NEW_LENS)
    keyed = [(-_cost(starts[s], NEW_LENS[s], r0, rows), s, r0)
             for s, r0 in got]
    costs = [-k[0] for k in keyed]
    assert all(a >= b for a, b in zip(costs, costs[1:]))  # non-increasing
    assert keyed == sorted(keyed)                      # ties by (seq, row0)
    assert len(set(costs)) > 1 and len(costs) > len(set(costs))
    # a pure function of its inputs
    again = ops.build_prefill_tiles(NEW_LENS, rows=rows, ctx_starts=ctx,
                                    heaviest_first=True)
    assert _pairs(again) == got


def test_ctx_starts_change_the_order():
    """Two equal chunks; the one with the longer cached prefix is heavier."""
    got = _pairs(ops.build_prefill_tiles([256, 256], rows=256,
                                         ctx_starts=[0, 1024],
                                         heaviest_first=True))
    assert got == [(1, 0), (0, 0)]
    assert _pairs(ops.build_prefill_tiles([256, 256], rows=256,
                                          heaviest_first=True)) \
        == [(0, 0), (1, 0)]


def test_default_follows_the_switch():
    assert _pairs(ops.build_prefill_tiles(NEW_LENS, rows=256)) == _pairs(
        ops.build_prefill_tiles(NEW_LENS, rows=256,
                                heaviest_first=ops.PF_TILE_ORDER))


def _makespan(costs, slots):
    """List scheduling: each job, in the given order, goes to the slot that
    frees up first."""
    free = [0] * slots
    heapq.heapify(free)
    end = 0
    for c in costs:
        t = heapq.heappop(free) + c
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def test_list_scheduling_8x1024():
    """8 x 1024 new tokens, 256-row tiles, 32 q heads, 512 workgroup slots,
    cost = KV steps. 32 tiles x 32 heads = 1024 workgroups, 256 each of
    cost 4, 8, 12, 16: 10240 units, ideal 10240 / 512 = 20. Descending
    order reaches it (each slot gets 16 + 4 or 12 + 8). The ascending
    table with the tile fastest cycles 4, 8, 12, 16: the first 512 jobs
    occupy every slot, the next 512 land behind them in an order that ends
    at 32."""
    lens, rows, heads, slots = [1024] * 8, 256, 32, 512

    def cost_list(table, heads_adjacent):
        costs = [_cost(0, lens[s], r0, rows) for s, r0 in _pairs(table)]
        if heads_adjacent:      # id = tile * heads + head
            return [c for c in costs for _ in range(heads)]
        return costs * heads    # id = head * ntiles + tile

    new = cost_list(ops.build_prefill_tiles(lens, rows=rows,
                                            heaviest_first=True), True)
    old = cost_list(ops.build_prefill_tiles(lens, rows=rows,
                                            heaviest_first=False), False)
    assert sorted(new) == sorted(old) and sum(new) == 10240
    ideal = -(-sum(new) // slots)
    m_new, m_old = _makespan(new, slots), _makespan(old, slots)
    print(f"ideal {ideal}, heaviest-first {m_new}, ascending {m_old}")
    assert ideal == 20
    assert m_new == ideal
    assert m_old >= 1.5 * ideal
