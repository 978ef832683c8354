"""Numpy models of the order and the distinct (tree id, leaf id) pairs that the library makes on the device (csrc/pairs.hip;
p252_pairs_order_device_into, p252_pairs_unique_device_into).  The key of pair i is the 96-bit number (tree id, leaf id), both parts
unsigned (uint32, uint64); ties keep their index order.

  order(t, j)             the plain model: the indices sorted by (tree id, leaf id, index)
  unique(t, j)            the plain model: (t_out, j_out, first) — the distinct pairs ascending, the lowest index that holds each
  device_order(t, j)      the device's method: records, 12 stable byte passes (a pass whose digit is the same in all keys is
                          skipped), per pass tile counts, a scan per digit value and a ranked scatter -> (order, passes that ran)
  device_unique(t, j)     that sort, then heads, their scan and the compaction -> (t_out, j_out, first)
t may be None: every pair is of tree 0."""
import numpy as np

PASSES = 12  # bytes 0 .. 7 of the leaf id, then bytes 0 .. 3 of the tree id


def _keys(t, j):
    j = np.ascontiguousarray(np.asarray(j)).astype(np.uint64).reshape(-1)
    t = np.zeros(j.size, dtype=np.uint32) if t is None else np.ascontiguousarray(np.asarray(t)).astype(np.uint32).reshape(-1)
    assert t.size == j.size
    return t, j


def order(t, j):
    t, j = _keys(t, j)
    return np.lexsort((np.arange(j.size), j, t.astype(np.uint64))).astype(np.uint32)


def unique(t, j):
    t, j = _keys(t, j)
    o = order(t, j)
    ts, js = t[o], j[o]
    head = np.ones(o.size, dtype=bool)
    head[1:] = (ts[1:] != ts[:-1]) | (js[1:] != js[:-1])
    return ts[head], js[head], o[head]


def digit(t, j, p):
    """byte p of the keys, least significant first"""
    return ((j >> np.uint64(8 * p)) & np.uint64(0xFF)).astype(np.int64) if p < 8 else ((t >> np.uint32(8 * (p - 8))) & np.uint32(0xFF)).astype(np.int64)


def varying_passes(t, j):
    """the passes that run: the digits that differ somewhere from pair 0's (the OR of key ^ key[0]); pass 0 when all keys are equal"""
    t, j = _keys(t, j)
    dj, dt = np.bitwise_or.reduce(j ^ j[0]), np.bitwise_or.reduce(t ^ t[0])
    on = [p for p in range(PASSES) if ((int(dj) >> (8 * p)) & 0xFF if p < 8 else (int(dt) >> (8 * (p - 8))) & 0xFF)]
    return on or [0]


def _sorted_records(t, j, tile):
    """the records {tree, index, leaf} after the passes that run, each pass as the device does it: the place of a record = the start of
    its digit value + the value's count in the tiles before + its rank among the tile's records of that value"""
    t, j = _keys(t, j)
    idx = np.arange(j.size, dtype=np.uint32)
    ran = varying_passes(t, j)
    for p in ran:
        d = digit(t, j, p)
        n_tiles = -(-d.size // tile)
        counts = np.zeros((256, n_tiles), dtype=np.int64)  # digit-major
        tile_of = np.arange(d.size) // tile
        np.add.at(counts, (d, tile_of), 1)
        totals = counts.sum(axis=1)
        start = np.cumsum(totals) - totals
        before = np.cumsum(counts, axis=1) - counts
        # the rank: records of the same value in the same tile that stand before this one
        by = np.lexsort((np.arange(d.size), d, tile_of))
        group = tile_of[by] * 256 + d[by]
        first_of_group = np.r_[True, group[1:] != group[:-1]]
        run_start = np.maximum.accumulate(np.where(first_of_group, np.arange(d.size), 0))
        rank = np.empty(d.size, dtype=np.int64)
        rank[by] = np.arange(d.size) - run_start
        place = start[d] + before[d, tile_of] + rank
        assert np.array_equal(np.sort(place), np.arange(d.size))
        out = np.empty_like(place)
        out[place] = np.arange(d.size)
        t, j, idx = t[out], j[out], idx[out]
    return t, j, idx, ran


def device_order(t, j, tile=2048):
    _, _, idx, ran = _sorted_records(t, j, tile)
    return idx, ran


def device_unique(t, j, tile=2048):
    ts, js, idx, _ = _sorted_records(t, j, tile)
    head = np.ones(idx.size, dtype=bool)
    head[1:] = (ts[1:] != ts[:-1]) | (js[1:] != js[:-1])
    n_tiles = -(-idx.size // tile)
    per_tile = np.add.reduceat(head.astype(np.int64), np.arange(n_tiles) * tile)
    offsets = np.cumsum(per_tile) - per_tile
    at = offsets[np.arange(idx.size) // tile] + (np.cumsum(head) - head) - (np.cumsum(head) - head)[(np.arange(idx.size) // tile) * tile]
    n = int(per_tile.sum())
    t_out, j_out, first = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    t_out[at[head]], j_out[at[head]], first[at[head]] = ts[head], js[head], idx[head]
    return t_out, j_out, first
