"""testsupport/treeshape.py, the one geometry of the numpy models, tied to the ABI in one place: its depth and levels_len are
p252_merkle{4,2}_depth and p252_merkle{4,2}_levels_len, its array forms are its scalar forms element by element, and the levels bound
holds the tree-major levels of any forest it is asked about.  No GPU: the two ABI calls are host arithmetic."""
import numpy as np
import pytest

from testsupport import treeshape as TS


def _sizes(arity):
    """0 .. 300, and arity^j - 1, arity^j, arity^j + 1 for every j with arity^j <= 2^32"""
    out, p = list(range(301)), arity
    while p <= 1 << 32:
        out += [p - 1, p, p + 1]
        p *= arity
    return out


@pytest.mark.parametrize("arity", [4, 2])
def test_depth_and_levels_len_are_the_abis(arity):
    from poseidon252_amd import _lib
    L = _lib.lib()
    depth, levels_len = (L.p252_merkle4_depth, L.p252_merkle4_levels_len) if arity == 4 else (L.p252_merkle2_depth, L.p252_merkle2_levels_len)
    sizes = _sizes(arity)
    assert 1 << 32 in sizes and (1 << 32) + 1 in sizes
    assert [TS.depth(n, arity) for n in sizes] == [depth(n) for n in sizes]
    assert [TS.levels_len(n, arity) for n in sizes] == [levels_len(n) for n in sizes]


@pytest.mark.parametrize("arity", [4, 2])
def test_the_array_forms_are_the_scalar_forms(arity):
    sizes = _sizes(arity)
    arr = np.array(sizes, dtype=np.int64)
    for fn in (TS.depth, TS.levels_len):
        got = fn(arr, arity)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [fn(n, arity) for n in sizes], fn.__name__
        assert isinstance(fn(sizes[5], arity), int) and fn(arr[:0], arity).tolist() == [] and fn(sizes, arity).tolist() == got.tolist()
    widths = TS.level_widths(arr, arity)
    assert len(widths) == TS.depth(max(sizes), arity)
    for i, n in enumerate(sizes):
        own = TS.level_widths(n, arity)
        assert [int(w[i]) for w in widths] == own + [0] * (len(widths) - len(own)), n
        assert own == [-(-n // arity ** l) for l in range(1, len(own) + 1)] and (own[-1] == 1 if own else n <= 1), n
        starts = TS.level_starts(n, arity)
        assert starts == [sum(own[:l]) for l in range(len(own) + 1)] and starts[-1] == TS.levels_len(n, arity), n


def test_offsets_and_block_starts():
    sizes = [5, 0, 1, 17]
    assert TS.offsets(sizes).tolist() == [0, 5, 5, 6, 23] and TS.offsets(sizes).dtype == np.uint64
    off = TS.offsets(np.array(sizes, dtype=np.uint64), start=3, dtype=np.int64)
    assert off.tolist() == [3, 8, 8, 9, 26] and off.dtype == np.int64
    assert TS.offsets([]).tolist() == [0] and TS.offsets([], start=7).tolist() == [7]
    for arity in (4, 2):
        assert TS.block_starts(sizes, arity).tolist() == np.concatenate([[0], np.cumsum([TS.levels_len(n, arity) for n in sizes])]).tolist()


@pytest.mark.parametrize("arity", [4, 2])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_levels_bound_holds_every_forest(arity, seed):
    """seeded forests, some with empty trees: the sum of levels_len over the trees that max_leaves admits (a larger tree is a bad tree: it
    has no block) is at most the bound, for max_leaves at, above and below the largest tree"""
    rng = np.random.default_rng(100 * arity + seed)
    top = arity ** 5 + 1
    sizes = np.floor(np.exp(rng.uniform(0, np.log(top + 1), 200))).astype(np.int64).clip(1, top)
    sizes[rng.random(200) < 0.15] = 0
    sizes[:4] = [top, 1, arity, arity + 1]
    n_leaves = int(sizes.sum())
    for max_leaves in (top, 3 * top, int(np.median(sizes[sizes > 0])), arity, 1):
        admitted = np.where(sizes <= max_leaves, sizes, 0)
        assert (admitted != sizes).any() == (max_leaves < top)
        used = int(TS.levels_len(admitted, arity).sum())
        assert used <= TS.levels_bound(n_leaves, len(sizes), max_leaves, arity), (max_leaves, used)
        assert used <= TS.levels_bound(int(admitted.sum()), len(sizes), max_leaves, arity), (max_leaves, used)  # (the good leaves alone)
    ones = np.ones(50, dtype=np.int64)  # one-leaf trees have no levels: the bound may be 0 (an allocation floor is the caller's)
    assert TS.levels_bound(50, 50, 1, arity) == 50 // (arity - 1) and int(TS.levels_len(ones, arity).sum()) == 0
