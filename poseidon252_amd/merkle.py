"""Arity-4 Merkle trees over Hash::digest(Domain::Merkle4, [c0,c1,c2,c3]) nodes.

The reference removed its tree builder in 0.29.0 (CHANGELOG.md:164-168); only the node hash
remains (src/hash.rs:22-26: total input exactly 4 scalars, empty slots = zero scalar).  The tree is
the obvious composition: levels are hashed while more than one node remains (a single
leaf is its own root), a level whose length is not a multiple of 4 is zero-padded.

Openings (the `poseidon-merkle` use named in AGENTS.md:62-66): an opening of leaf
i is, per level, the 3 siblings of the node on the path and the node's position 0..3 among its
parent's children; `merkle4_path_roots` re-hashes n such branches in one kernel launch.
"""
import numpy as np

from .hash import Context, levels_len, _ARITIES, _arity, _as_scalars, _is_torch, _n_scalars, _ragged_items  # noqa: F401 (levels_len: public here)


def merkle4_tag():
    return _ARITIES[4].tag()


def merkle2_tag():
    return _ARITIES[2].tag()


def permutations(n_leaves):
    """number of Hades permutations a tree over n_leaves costs (= number of internal nodes)"""
    return levels_len(n_leaves)


def merkle4_tree(leaves, tag=None, ctx=None, want_levels=False):
    """leaves: (n,4) uint64 numpy, or a torch CUDA tensor holding n BlsScalars.  Returns the root
    (numpy (4,) / torch (4,) int64 on the same device) and optionally all upper levels bottom-up."""
    ctx = ctx or Context.default()
    tag = merkle4_tag() if tag is None else _as_scalars(tag).reshape(4)
    if _is_torch(leaves):
        import torch
        n = _n_scalars(leaves)
        root = torch.empty(4, dtype=torch.int64, device=leaves.device)
        levels = torch.empty((max(levels_len(n), 1), 4), dtype=torch.int64, device=leaves.device) if want_levels else None
        ctx.merkle4_tree_device(tag, leaves, n, root, levels)
        return (root, levels) if want_levels else root
    return ctx.merkle4_tree(tag, np.asarray(leaves), want_levels=want_levels)


def merkle4_forest(leaves, leaves_per_tree, tag=None, ctx=None, want_levels=False):
    """roots of the n_trees = n / leaves_per_tree independent complete trees stored tree-major in `leaves` (a torch CUDA tensor
    or an (n,4) uint64 numpy array): one kernel launch per level across all trees.  Returns roots (n_trees,4) — torch int64 on
    the device for device input, numpy uint64 otherwise — and optionally the level-major array of all levels."""
    ctx = ctx or Context.default()
    tag = merkle4_tag() if tag is None else _as_scalars(tag).reshape(4)
    dev_in = _is_torch(leaves)
    if not dev_in and not want_levels:  # host leaves, roots only: the library's staged pipeline (no torch needed)
        return ctx.merkle4_forest(tag, leaves, leaves_per_tree)
    import torch
    d = leaves if dev_in else torch.from_numpy(_as_scalars(leaves).reshape(-1, 4).view(np.int64)).to("cuda:%d" % ctx.device)
    n = _n_scalars(d)
    if leaves_per_tree < 1 or n % leaves_per_tree:
        raise ValueError("forest: %d leaves are not a whole number of %d-leaf trees" % (n, leaves_per_tree))
    n_trees = n // leaves_per_tree
    roots = torch.empty((n_trees, 4), dtype=torch.int64, device=d.device)
    levels = torch.empty((max(n_trees * levels_len(leaves_per_tree), 1), 4), dtype=torch.int64, device=d.device) if want_levels else None
    ctx.merkle4_forest_device(tag, d, n_trees, leaves_per_tree, roots, levels)
    if not dev_in:
        torch.cuda.synchronize(d.device)
        roots = roots.cpu().numpy().view(np.uint64)
        levels = levels.cpu().numpy().view(np.uint64) if want_levels else None
    return (roots, levels) if want_levels else roots


def _forest_trees(trees):
    """(flat (S, 4) uint64, offsets (n_trees + 1,) uint64, leaf counts) of a list of (n_t, 4) leaf arrays or of a (flat, offsets) pair, as
    RaggedHashBatch takes messages; every tree is checked here (dtype, empty, decreasing offsets, extent) before any device work"""
    return _ragged_items(trees, "merkle_forest_ragged: ", "tree", "leaves", (ValueError, "merkle_forest_ragged: "), strict=True)


def merkle_forest_ragged(trees, arity=4, tag=None, ctx=None, want_levels=False):
    """roots of trees of DIFFERENT sizes in one call (p252_merkle{4,2}_forest_ragged): each root is what merkle4_tree (arity 2:
    Context.merkle2_tree) returns for that tree alone, and every level is one kernel launch across all trees.  trees: a list of
    (n_t, 4) uint64 leaf arrays, or (flat, offsets) with tree t = flat[offsets[t]:offsets[t+1]].  Returns roots (n_trees, 4)
    uint64; with want_levels also (levels, level_offsets): levels tree-major — tree t's block, at level_offsets[t], is byte for
    byte what the single-tree call writes (unlike merkle4_forest's level-major layout) — and level_offsets the n_trees + 1
    prefix sums of levels_len(n_t, arity)."""
    a = _arity("merkle_forest_ragged", arity)
    flat, off, lens = _forest_trees(trees)
    level_offsets = np.zeros(lens.shape[0] + 1, dtype=np.uint64)
    np.cumsum([levels_len(int(n), arity) for n in lens], out=level_offsets[1:])
    tag = _as_scalars(a.tag() if tag is None else tag).reshape(4)
    if lens.shape[0] == 0:
        roots = np.zeros((0, 4), dtype=np.uint64)
        return (roots, np.zeros((0, 4), dtype=np.uint64), level_offsets) if want_levels else roots
    ctx = ctx or Context.default()
    res = ctx.merkle_forest_ragged(tag, flat, off, arity=arity, want_levels=want_levels)
    return (res[0], res[1], level_offsets) if want_levels else res


def merkle4_openings(leaves, levels, indices):
    """Host-side bookkeeping (no hashing): sibling paths of the leaves at `indices` out of a built tree.
    leaves (n,4), levels = concatenated upper levels as merkle4_tree(..., want_levels=True) returns.
    Returns (siblings (m,depth,3,4) uint64, positions (m,depth) uint8); missing siblings = zero scalar."""
    leaves = _as_scalars(leaves).reshape(-1, 4)
    levels = _as_scalars(levels).reshape(-1, 4)
    per_level, cnt, off = [leaves], leaves.shape[0], 0
    while cnt > 1:
        cnt = (cnt + 3) // 4
        per_level.append(levels[off:off + cnt])
        off += cnt
    depth = len(per_level) - 1
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    sib = np.zeros((idx.shape[0], depth, 3, 4), dtype=np.uint64)
    pos = np.zeros((idx.shape[0], depth), dtype=np.uint8)
    cur = idx.copy()
    for l in range(depth):
        nodes = per_level[l]
        p = cur & 3
        pos[:, l] = p
        base = cur - p
        for m in range(idx.shape[0]):
            others = [base[m] + k for k in range(4) if k != p[m]]
            for s, j in enumerate(others):
                if j < nodes.shape[0]:
                    sib[m, l, s] = nodes[j]
        cur = cur >> 2
    return sib, pos


def forest_ragged_append(ctx, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_add, d_add_offsets, n_trees_new=None,
                         max_leaves_new=None, arity=4):
    """Leaves appended to the trees of a built forest (Context.merkle_forest_ragged_append_device): the forest = torch CUDA tensors
    as Context.merkle_forest_ragged_device took and filled them; tree t receives d_add[d_add_offsets[t]:d_add_offsets[t+1]] (d_add None:
    a compaction copy).  n_trees_new defaults to the trees d_add_offsets names, max_leaves_new to max_leaves plus the scalars of d_add (no
    append can then be too long).  Sizes and allocates the new forest and returns (d_leaves_new, d_offsets_new, d_levels_new, d_roots,
    d_n_bad (1,) int32, d_n_hashed (1,) int64), all on the device; d_leaves_new is exact-sized (old leaves plus d_add: rows past
    d_offsets_new[-1] are unused), d_levels_new holds the bound of the new shape.  No synchronisation."""
    import torch
    a = _arity("forest_ragged_append", arity)
    ctx = ctx or Context.default()
    dev = d_add_offsets.device
    n_add = _n_scalars(d_add) if d_add is not None else 0
    n_leaves = _n_scalars(d_leaves) if d_leaves is not None else 0
    if n_trees_new is None:
        n_trees_new = d_add_offsets.numel() - 1
    if max_leaves_new is None:
        max_leaves_new = max(max_leaves + n_add, 1)
    total = n_leaves + n_add
    leaves_new = torch.empty((total, 4), dtype=torch.int64, device=dev)
    offsets_new = torch.empty(n_trees_new + 1, dtype=torch.int64, device=dev)
    levels_new = torch.empty((a.forest_levels_bytes(total, n_trees_new, a.depth(max_leaves_new)) // 32, 4), dtype=torch.int64, device=dev)
    roots = torch.empty((n_trees_new, 4), dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    n_hashed = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.merkle_forest_ragged_append_device(
        a.tag() if tag is None else _as_scalars(tag).reshape(4), d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_add, d_add_offsets,
        n_trees_new, max_leaves_new, leaves_new if total else None, offsets_new, levels_new if levels_new.numel() else None, roots, n_bad, n_hashed,
        arity=arity)
    return leaves_new, offsets_new, levels_new, roots, n_bad, n_hashed


def forest_ragged_resize(ctx, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep=None, d_add=None, d_add_offsets=None,
                         n_trees_new=None, max_leaves_new=None, arity=4):
    """A built forest rolled back and forward in one call (Context.merkle_forest_ragged_resize_device): tree t keeps its first
    min(d_keep[t], n_t) leaves (d_keep: int64/uint64 on the device, -1 or any value >= n_t keeps the tree whole; None: every tree) and
    then receives d_add[d_add_offsets[t]:d_add_offsets[t+1]] (both None: a pure rollback).  n_trees_new defaults to the trees
    d_add_offsets names, else d_keep, else n_trees; smaller than n_trees it drops the trailing trees.  max_leaves_new defaults as in
    forest_ragged_append.  Sizes and allocates the new forest as forest_ragged_append does and returns the same tuple (d_leaves_new,
    d_offsets_new, d_levels_new, d_roots, d_n_bad, d_n_hashed), all on the device.  No synchronisation."""
    import torch
    a = _arity("forest_ragged_resize", arity)
    ctx = ctx or Context.default()
    if n_trees_new is None:
        named = d_add_offsets.numel() - 1 if d_add_offsets is not None else d_keep.numel() if d_keep is not None else n_trees
        n_trees_new = named
    dev = next(t for t in (d_add_offsets, d_keep, d_offsets, d_add) if t is not None).device
    if d_add_offsets is None:  # nothing appended
        if d_add is not None:
            raise ValueError("forest_ragged_resize: d_add needs d_add_offsets")
        d_add_offsets = torch.zeros(n_trees_new + 1, dtype=torch.int64, device=dev)
    n_add = _n_scalars(d_add) if d_add is not None else 0
    n_leaves = _n_scalars(d_leaves) if d_leaves is not None else 0
    if max_leaves_new is None:
        max_leaves_new = max(max_leaves + n_add, 1)
    total = n_leaves + n_add
    leaves_new = torch.empty((total, 4), dtype=torch.int64, device=dev)
    offsets_new = torch.empty(n_trees_new + 1, dtype=torch.int64, device=dev)
    levels_new = torch.empty((a.forest_levels_bytes(total, n_trees_new, a.depth(max_leaves_new)) // 32, 4), dtype=torch.int64, device=dev)
    roots = torch.empty((n_trees_new, 4), dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    n_hashed = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.merkle_forest_ragged_resize_device(
        a.tag() if tag is None else _as_scalars(tag).reshape(4), d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add, d_add_offsets,
        n_trees_new, max_leaves_new, leaves_new if total else None, offsets_new, levels_new if levels_new.numel() else None, roots, n_bad, n_hashed,
        arity=arity)
    return leaves_new, offsets_new, levels_new, roots, n_bad, n_hashed


def forest_ragged_select(ctx, forest_a, pick, forest_b=None, arity=4, leaves_cap=None):
    """Any trees of one or two built forests gathered into a new compact forest, with no digest
    (Context.merkle_forest_ragged_select_device): forest_a, forest_b = (d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_roots),
    torch CUDA tensors as Context.merkle_forest_ragged_device took and filled them; pick = the ids of the new forest's trees in order
    (a device int64 tensor, or anything numpy takes): below n_trees_a a tree of A, then a tree of B.  leaves_cap defaults to the leaves
    of both sources, enough when no tree is named twice; a pick past it is refused and counted, never written.  Sizes and allocates
    the new forest and returns (d_leaves_new, d_offsets_new, d_levels_new, d_roots, d_n_bad (1,) int32), all on the device: what
    forest_ragged_append returns for a new forest, less the digest count (there is none).  d_levels_new holds the bound of the new
    shape; max_leaves of the new forest is the larger of the two sources'.  No synchronisation."""
    import torch
    a = _arity("forest_ragged_select", arity)
    ctx = ctx or Context.default()
    dev = forest_a[0].device
    if not isinstance(pick, torch.Tensor):
        ids = np.ascontiguousarray(pick)
        if ids.dtype.kind not in "iu":
            raise ValueError("forest_ragged_select: pick must hold integers, not %s" % ids.dtype)
        pick = torch.from_numpy(ids.astype(np.uint64).view(np.int64).reshape(-1)).to(dev)
    n_pick = pick.numel()
    if leaves_cap is None:
        leaves_cap = _n_scalars(forest_a[0]) + (_n_scalars(forest_b[0]) if forest_b is not None else 0)
    if leaves_cap <= 0:
        raise ValueError("forest_ragged_select: leaves_cap must be > 0")
    max_leaves = max(forest_a[3], forest_b[3] if forest_b is not None else 0)
    leaves_new = torch.empty((leaves_cap, 4), dtype=torch.int64, device=dev)
    offsets_new = torch.empty(n_pick + 1, dtype=torch.int64, device=dev)
    levels_new = torch.empty((a.forest_levels_bytes(leaves_cap, n_pick, a.depth(max_leaves)) // 32, 4), dtype=torch.int64, device=dev)
    roots = torch.empty((n_pick, 4), dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if n_pick == 0:  # (the library enqueues nothing: the one offset is written here)
        offsets_new.zero_()
    ctx.merkle_forest_ragged_select_device(forest_a, forest_b, pick, n_pick, leaves_new, offsets_new, levels_new if levels_new.numel() else None,
                                           roots, n_bad, arity=arity)
    return leaves_new, offsets_new, levels_new, roots, n_bad


class ForestJournal:
    """what one journaled update overwrote (forest_ragged_update_journaled), on the device: ids (cap, 4) int32 {tree id, level + 1, node
    index low, high}, values (cap, 4) int64, len (1,) int64 = the entries in use; n_bad (1,) int32 and n_hashed (1,) int64 are the
    update's counters.  forest_ragged_journal_swap takes it, any number of times."""

    def __init__(self, ids, values, len, n_bad, n_hashed):  # noqa: A002 (the journal's length, as the C call names it)
        self.ids, self.values, self.len, self.n_bad, self.n_hashed = ids, values, len, n_bad, n_hashed

    @property
    def cap(self):
        return self.ids.shape[0]


def forest_ragged_update_journaled(ctx, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, tree_ids, leaf_ids, new_leaves, d_roots=None,
                                   arity=4):
    """Leaf updates of a built forest that can be undone (Context.merkle_forest_ragged_update_journaled_device): the forest = torch
    CUDA tensors as Context.merkle_forest_ragged_device took and filled them, updated in place; (tree_ids[i], leaf_ids[i]) receives
    new_leaves[i] (sequences, numpy or torch).  Allocates the journal at its bound and returns it as a ForestJournal; its counters are
    on the device.  No synchronisation."""
    import torch
    f = "forest_ragged_update_journaled"
    a = _arity(f, arity)
    ctx = ctx or Context.default()
    dev = d_leaves.device
    t = torch.as_tensor(tree_ids, device=dev).to(torch.int64).reshape(-1)
    l = torch.as_tensor(leaf_ids, device=dev).to(torch.int64).reshape(-1)
    new = new_leaves if _is_torch(new_leaves) else torch.from_numpy(np.ascontiguousarray(_as_scalars(new_leaves)).view(np.int64))
    new = new.to(dev).contiguous()
    k = t.numel()
    if l.numel() != k or _n_scalars(new) != k:
        raise ValueError("%s: %d tree ids, %d leaf ids, %d new leaves" % (f, k, l.numel(), _n_scalars(new)))
    cap = ctx.merkle_forest_ragged_journal_bound(_n_scalars(d_leaves), n_trees, max_leaves, k, arity=arity)
    j = ForestJournal(torch.empty((cap, 4), dtype=torch.int32, device=dev), torch.empty((cap, 4), dtype=torch.int64, device=dev),
                      torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                      torch.zeros(1, dtype=torch.int64, device=dev))
    ctx.merkle_forest_ragged_update_journaled_device(
        a.tag() if tag is None else _as_scalars(tag).reshape(4), d_leaves, d_offsets, n_trees, max_leaves, d_levels if a.depth(max_leaves) else None,
        (t & 0xFFFFFFFF).to(torch.int32), l, new, k, j.ids if cap else None, j.values if cap else None, cap, j.len, d_roots, j.n_bad, j.n_hashed,
        arity=arity)
    return j


def forest_ragged_journal_swap(ctx, d_leaves, d_offsets, n_trees, max_leaves, d_levels, journal, d_roots=None, arity=4):
    """The update behind `journal` (a ForestJournal) undone — or, after an undo, redone — with no hashing
    (Context.merkle_forest_ragged_journal_swap_device): the forest exactly as the update took it, changed in place; d_roots follows for
    the touched trees.  Journals stack: undo the latest first, redo the earliest first.  Returns the entries that named no node of this
    forest as a (1,) int32 device tensor: 0 for a journal used on its own forest.  No synchronisation."""
    import torch
    a = _arity("forest_ragged_journal_swap", arity)
    ctx = ctx or Context.default()
    n_bad = torch.zeros(1, dtype=torch.int32, device=d_leaves.device)
    cap = journal.cap
    ctx.merkle_forest_ragged_journal_swap_device(d_leaves, d_offsets, n_trees, max_leaves, d_levels if a.depth(max_leaves) else None,
                                                 journal.ids if cap else None, journal.values if cap else None, cap, journal.len, d_roots, n_bad,
                                                 arity=arity)
    return n_bad


class ForestFrontier:
    """A forest of append-only trees kept only as their frontiers, on the device: counts (n_trees,) int64, frontier (n_trees, bound, 4)
    int64 with bound = Context.merkle_forest_frontier_bound(max_leaves), roots (n_trees, 4) int64 — O(depth) scalars per tree
    whatever the trees hold.  ForestFrontier(ctx, n_trees, max_leaves) is a forest of empty trees; from_forest takes the state out of
    a built ragged forest; append grows the trees in place."""

    def __init__(self, ctx, n_trees, max_leaves, arity=4, device=None, counts=None, frontier=None, roots=None):
        import torch
        _arity("ForestFrontier", arity)
        self.ctx = ctx or Context.default()
        self.n_trees, self.max_leaves, self.arity = n_trees, max_leaves, arity
        dev = device if device is not None else "cuda:%d" % self.ctx.device
        bound = self.ctx.merkle_forest_frontier_bound(max_leaves, arity=arity)
        self.counts = torch.zeros(n_trees, dtype=torch.int64, device=dev) if counts is None else counts
        self.frontier = torch.zeros((n_trees, bound, 4), dtype=torch.int64, device=dev) if frontier is None else frontier
        self.roots = torch.zeros((n_trees, 4), dtype=torch.int64, device=dev) if roots is None else roots

    @classmethod
    def from_forest(cls, ctx, d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots, max_leaves=None, arity=4):
        """the state of a forest Context.merkle_forest_ragged_device built with d_levels -> (ForestFrontier, d_n_bad (1,) int32)"""
        self = cls(ctx, n_trees, max_leaves_forest if max_leaves is None else max_leaves, arity, device=d_leaves.device)
        return self, forest_frontier_extract(self.ctx, d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots, self)

    def append(self, d_add, d_add_offsets, tag=None, witnesses=None):
        """tree t receives d_add[d_add_offsets[t]:d_add_offsets[t+1]] -> (d_n_bad (1,) int32, d_n_hashed (1,) int64); with witnesses (a
        ForestWitnesses) their openings are kept current in the same call and the bad ones are counted in a third (1,) int32; no
        synchronisation"""
        return forest_frontier_append(self.ctx, tag, self, d_add, d_add_offsets, witnesses)


class ForestWitnesses:
    """The openings of k marked leaves of a ForestFrontier, kept current by ForestFrontier.append(..., witnesses=self): witness i names
    leaf leaf_ids[i] of tree tree_ids[i] (sequences, numpy or torch; kept on the device as (k,) int32 and (k,) int64).  leaves (k, 4),
    siblings (k, D, arity - 1, 4), positions (k, D) uint8 and depths (k,) uint8, D = depth(max_leaves), are the layout of
    Context.merkle_forest_ragged_openings_device.  A new one is zeroed with depth 0xFF: right for leaves that a later append brings, and
    bad until then.  Leaves that are in the trees already come from_openings of the stored forest."""

    def __init__(self, ctx, k, max_leaves, arity, tree_ids, leaf_ids, device=None):
        import torch
        a = _arity("ForestWitnesses", arity)
        self.ctx = ctx or Context.default()
        self.k, self.max_leaves, self.arity, self.depth = k, max_leaves, arity, a.depth(max_leaves)
        dev = device if device is not None else "cuda:%d" % self.ctx.device
        ids = lambda x, dtype: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.int64))).to(device=dev, dtype=dtype).contiguous()  # noqa: E731
        self.tree_ids, self.leaf_ids = ids(tree_ids, torch.int32), ids(leaf_ids, torch.int64)
        if self.tree_ids.shape != (k,) or self.leaf_ids.shape != (k,):
            raise ValueError("ForestWitnesses: tree_ids and leaf_ids must hold k = %d ids each" % k)
        self.leaves = torch.zeros((k, 4), dtype=torch.int64, device=dev)
        self.siblings = torch.zeros((k, self.depth, a.per, 4), dtype=torch.int64, device=dev)
        self.positions = torch.zeros((k, self.depth), dtype=torch.uint8, device=dev)
        self.depths = torch.full((k,), 0xFF, dtype=torch.uint8, device=dev)

    @classmethod
    def from_openings(cls, ctx, d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, tree_ids, leaf_ids, max_leaves=None, arity=4):
        """the witnesses of leaves of a forest Context.merkle_forest_ragged_device built with d_levels, at the stride of max_leaves (>=
        max_leaves_forest: the bound of the ForestFrontier that takes the forest over) -> (ForestWitnesses, d_n_bad (1,) int32)"""
        import torch
        top = max_leaves_forest if max_leaves is None else max_leaves
        self = cls(ctx, len(tree_ids), top, arity, tree_ids, leaf_ids, device=d_leaves.device)
        n_bad = torch.zeros(1, dtype=torch.int32, device=d_leaves.device)
        if self.k:
            inner = _arity("ForestWitnesses", arity).depth(max_leaves_forest)  # the openings come at the forest's own stride
            lv, sib, pos, dep, _ = self.ctx.merkle_forest_ragged_openings_device(d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels,
                                                                                 self.tree_ids, self.leaf_ids, self.k, d_n_bad=n_bad, arity=arity)
            self.leaves.copy_(lv)
            self.siblings[:, :inner] = sib
            self.positions[:, :inner] = pos
            self.depths.copy_(dep)
        return self, n_bad

    def verify(self, frontier, tag=None):
        """d_ok (k,) uint8 on the device: 1 iff witness i re-hashes to the root of ITS tree in `frontier` (a ForestFrontier)
        (Context.merkle_forest_ragged_verify_device); no synchronisation"""
        import torch
        a = _arity("ForestWitnesses.verify", self.arity)
        ok = torch.zeros(self.k, dtype=torch.uint8, device=self.depths.device)
        if self.k:
            self.ctx.merkle_forest_ragged_verify_device(a.tag() if tag is None else _as_scalars(tag).reshape(4), self.leaves,
                                                        self.siblings if self.depth else None, self.positions if self.depth else None, self.depths,
                                                        self.depth, self.tree_ids, frontier.roots, frontier.n_trees, ok, self.k, arity=self.arity)
        return ok


def forest_frontier_append(ctx, tag, state, d_add, d_add_offsets, witnesses=None):
    """Leaves appended to the trees of a ForestFrontier, in place (Context.merkle_forest_frontier_append_device): tree t receives
    d_add[d_add_offsets[t]:d_add_offsets[t+1]] (torch CUDA tensors; d_add None: nothing).  Returns (d_n_bad (1,) int32, d_n_hashed (1,)
    int64) on the device: the refused appends, whose trees are untouched, and the digests computed.  With witnesses (a ForestWitnesses
    of the same arity and max_leaves) their openings are kept current by the same call
    (Context.merkle_forest_frontier_append_witness_device) and a third tensor, d_n_bad_witness (1,) int32, follows.
    No synchronisation."""
    import torch
    a = _arity("forest_frontier_append", state.arity)
    ctx = ctx or state.ctx
    dev = state.counts.device
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    n_hashed = torch.zeros(1, dtype=torch.int64, device=dev)
    tag = a.tag() if tag is None else _as_scalars(tag).reshape(4)
    if witnesses is None:
        ctx.merkle_forest_frontier_append_device(tag, state.counts, state.frontier, state.roots, state.n_trees, state.max_leaves, d_add, d_add_offsets,
                                                 n_bad, n_hashed, arity=state.arity)
        return n_bad, n_hashed
    if witnesses.arity != state.arity or witnesses.max_leaves != state.max_leaves:
        raise ValueError("forest_frontier_append: the witnesses are of arity %d and max_leaves %d, the state of %d and %d"
                         % (witnesses.arity, witnesses.max_leaves, state.arity, state.max_leaves))
    n_bad_witness = torch.zeros(1, dtype=torch.int32, device=dev)
    w = witnesses
    ctx.merkle_forest_frontier_append_witness_device(
        tag, state.counts, state.frontier, state.roots, state.n_trees, state.max_leaves, d_add, d_add_offsets, w.tree_ids, w.leaf_ids, w.k,
        w.leaves, w.siblings if w.depth else None, w.positions if w.depth else None, w.depths, n_bad, n_hashed, n_bad_witness, arity=state.arity)
    return n_bad, n_hashed, n_bad_witness


def forest_frontier_extract(ctx, d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots, state):
    """The frontiers of a built ragged forest written into `state` (a ForestFrontier of n_trees trees with max_leaves >=
    max_leaves_forest), with no digest (Context.merkle_forest_frontier_extract_device).  Returns d_n_bad (1,) int32 on the device:
    the trees the build calls bad, which become empty ones.  No synchronisation."""
    import torch
    _arity("forest_frontier_extract", state.arity)
    ctx = ctx or state.ctx
    if state.n_trees != n_trees:
        raise ValueError("forest_frontier_extract: the state holds %d trees, the forest %d" % (state.n_trees, n_trees))
    n_bad = torch.zeros(1, dtype=torch.int32, device=state.counts.device)
    ctx.merkle_forest_frontier_extract_device(d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots, state.max_leaves, state.counts,
                                              state.frontier, state.roots, n_bad, arity=state.arity)
    return n_bad


def forest_ragged_consistency(ctx, d_leaves, d_offsets, n_trees, max_leaves, d_levels, tree_ids, old_counts, arity=4):
    """Consistency proofs out of a built ragged forest, with no digest (Context.merkle_forest_ragged_consistency_device): proof i
    shows that tree tree_ids[i], as it is now, is the tree it was at old_counts[i] leaves with leaves appended (sequences, numpy or
    torch; a (n_trees,) counts tensor of a ForestFrontier with tree_ids = arange serves as it stands).  Returns (d_new_counts (k,)
    int64, (d_leaves_out (k, 4), d_siblings (k, D, arity - 1, 4), d_positions (k, D) uint8, d_depths (k,) uint8, D), d_n_bad (1,)
    int32), all on the device: the proof tuple is what forest_consistency_verify takes.  No synchronisation."""
    import torch
    a = _arity("forest_ragged_consistency", arity)
    ctx = ctx or Context.default()
    dev = d_leaves.device
    ids = lambda x, dtype: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.int64))).to(device=dev, dtype=dtype).contiguous()  # noqa: E731
    t, n = ids(tree_ids, torch.int32), ids(old_counts, torch.int64)
    k = t.numel()
    if n.numel() != k:
        raise ValueError("forest_ragged_consistency: %d tree ids, %d old counts" % (k, n.numel()))
    D = a.depth(max_leaves)
    new_counts = torch.zeros(k, dtype=torch.int64, device=dev)
    lv = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    sib = torch.zeros((k, D, a.per, 4), dtype=torch.int64, device=dev)
    pos = torch.zeros((k, D), dtype=torch.uint8, device=dev)
    dep = torch.full((k,), 0xFF, dtype=torch.uint8, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if k:
        ctx.merkle_forest_ragged_consistency_device(d_leaves, d_offsets, n_trees, max_leaves, d_levels if D else None, t, n, k, new_counts, lv,
                                                    sib if D else None, pos if D else None, dep, n_bad, arity=arity)
    return new_counts, (lv, sib, pos, dep, D), n_bad


def forest_consistency_verify(ctx, d_old_counts, d_old_roots, d_new_counts, d_new_roots, proof, d_tree_ids=None, tag=None, arity=4):
    """Consistency proofs checked against (old count, old root, new count, new root) claims
    (Context.merkle_forest_consistency_verify_device): proof = (d_leaves, d_siblings, d_positions, d_depths, D) as
    forest_ragged_consistency returns it; claim i is element i of the four claim tensors, or element d_tree_ids[i] (int32) when given —
    then they hold one entry per tree, as the counts and roots of a ForestFrontier do.  Returns (d_ok (k,) uint8, d_old_roots_out (k, 4),
    d_new_roots_out (k, 4), d_n_hashed (1,) int64) on the device: the verdicts, the recomputed roots, the digests computed.  No
    synchronisation."""
    import torch
    a = _arity("forest_consistency_verify", arity)
    ctx = ctx or Context.default()
    lv, sib, pos, dep, D = proof
    k, dev = dep.numel(), dep.device
    ok = torch.zeros(k, dtype=torch.uint8, device=dev)
    old_out, new_out = torch.zeros((k, 4), dtype=torch.int64, device=dev), torch.zeros((k, 4), dtype=torch.int64, device=dev)
    n_hashed = torch.zeros(1, dtype=torch.int64, device=dev)
    if k:
        ctx.merkle_forest_consistency_verify_device(
            a.tag() if tag is None else _as_scalars(tag).reshape(4), d_old_counts, d_old_roots, d_new_counts, d_new_roots, lv, sib if D else None,
            pos if D else None, dep, D, k, ok, d_tree_ids, _n_scalars(d_old_roots) if d_tree_ids is not None else 0, old_out, new_out, n_hashed,
            arity=arity)
    return ok, old_out, new_out, n_hashed


def forest_ragged_anchor_openings(ctx, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, anchor_tree_ids, anchor_counts, anchor_ids,
                                  leaf_ids, arity=4):
    """Roots and openings of the trees of a built ragged forest as they WERE at earlier leaf counts
    (Context.merkle_forest_ragged_anchor_openings_device): anchor a is tree anchor_tree_ids[a] at anchor_counts[a] leaves, opening i
    is leaf leaf_ids[i] under anchor anchor_ids[i] (sequences, numpy or torch; empty leaf_ids: the roots alone).  tag = None: the arity's
    own.  Returns (d_anchor_roots (m, 4), d_anchor_depths (m,) uint8, openings, (d_n_bad_anchors, d_n_bad) (1,) int32 each, d_n_hashed
    (1,) int64), all on the device, with openings = (d_leaves_out (k, 4), d_siblings (k, D, arity - 1, 4), d_positions (k, D) uint8,
    d_depths (k,) uint8, D): merkle_forest_ragged_verify_device(tag, *openings, d_anchor_ids, d_anchor_roots, m, d_ok, k) takes it as it
    stands, and so does merkle_path_ragged_device.  No synchronisation."""
    import torch
    a = _arity("forest_ragged_anchor_openings", arity)
    ctx = ctx or Context.default()
    dev = d_leaves.device
    ids = lambda x, dtype: (x if _is_torch(x) else torch.from_numpy(np.asarray(x).astype(np.int64))).to(device=dev, dtype=dtype).contiguous()  # noqa: E731
    at, ac = ids(anchor_tree_ids, torch.int32), ids(anchor_counts, torch.int64)
    oa, ol = ids(anchor_ids, torch.int32), ids(leaf_ids, torch.int64)
    m, k = at.numel(), oa.numel()
    if ac.numel() != m or ol.numel() != k:
        raise ValueError("forest_ragged_anchor_openings: %d anchor trees, %d counts; %d anchor ids, %d leaf ids" % (m, ac.numel(), k, ol.numel()))
    D = a.depth(max_leaves)
    roots = torch.zeros((m, 4), dtype=torch.int64, device=dev)
    depths = torch.full((m,), 0xFF, dtype=torch.uint8, device=dev)
    lv = torch.zeros((k, 4), dtype=torch.int64, device=dev)
    sib = torch.zeros((k, D, a.per, 4), dtype=torch.int64, device=dev)
    pos = torch.zeros((k, D), dtype=torch.uint8, device=dev)
    dep = torch.full((k,), 0xFF, dtype=torch.uint8, device=dev)
    bad_anchors, bad = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    n_hashed = torch.zeros(1, dtype=torch.int64, device=dev)
    if m or k:
        ctx.merkle_forest_ragged_anchor_openings_device(
            a.tag() if tag is None else _as_scalars(tag).reshape(4), d_leaves, d_offsets, n_trees, max_leaves, d_levels if D else None,
            at if m else None, ac if m else None, m, oa if k else None, ol if k else None, k, roots if m else None, depths if m else None,
            lv if k else None, sib if k and D else None, pos if k and D else None, dep if k else None, bad_anchors, bad, n_hashed, arity=arity)
    return roots, depths, (lv, sib, pos, dep, D), (bad_anchors, bad), n_hashed


def merkle_multiproof(d_leaves, d_levels, indices, arity=4, ctx=None):
    """One shared proof for many leaves of ONE stored tree (Context.merkle_multiproof_device): d_leaves / d_levels = torch CUDA tensors
    as merkle4_tree(..., want_levels=True) fills them, indices = leaf positions in any order (a sequence, numpy or torch); they are
    sorted and de-duplicated on the device.  Returns (indices (k,) int32, leaves (k, 4), proof (len, 4)), all on the device — what
    merkle_multiproof_verify takes; one synchronisation, to read the proof's length.  A position outside the tree: ValueError."""
    import torch
    ctx = ctx or Context.default()
    dev = d_leaves.device
    n = _n_scalars(d_leaves)
    idx = torch.unique(torch.as_tensor(indices, device=dev).to(torch.int64).reshape(-1) & 0xFFFFFFFF).to(torch.int32)  # (sorted)
    k = idx.numel()
    if k == 0:
        raise ValueError("merkle_multiproof: no positions")
    out = torch.empty((k, 4), dtype=torch.int64, device=dev)
    proof = torch.empty((ctx.merkle_multiproof_bound(n, k, arity), 4), dtype=torch.int64, device=dev)
    meta = torch.zeros(2, dtype=torch.int64, device=dev)  # the length; the bad positions (its low 32 bits)
    ctx.merkle_multiproof_device(d_leaves, n, d_levels if n > 1 else None, idx, k, out, proof if proof.numel() else None, meta[:1],
                                 meta[1:].view(torch.int32)[:1], arity=arity)
    length, bad = (int(v) for v in meta.cpu())
    if bad:
        raise ValueError("merkle_multiproof: %d position(s) outside the tree (%d leaves)" % (bad, n))
    return idx, out, proof[:length]


def merkle_multiproof_verify(n_leaves, indices, leaves, proof, root, arity=4, tag=None, ctx=None):
    """True iff (indices, leaves, proof) — torch CUDA tensors as merkle_multiproof returns them — re-hash to `root` (4,) for a tree of
    n_leaves, every ancestor hashed once (Context.merkle_multiproof_verify_device).  Synchronises to read the verdict."""
    import torch
    ctx = ctx or Context.default()
    if tag is None:  # (an arity that is neither is refused in the name of the call below, which refused it before)
        tag = _arity("merkle_multiproof_verify_device", arity).tag()
    ok = torch.zeros(1, dtype=torch.uint8, device=leaves.device)
    proof_len = _n_scalars(proof)
    ctx.merkle_multiproof_verify_device(_as_scalars(tag).reshape(4), n_leaves, indices, leaves, indices.numel(), proof if proof_len else None,
                                        proof_len, root, ok, arity=arity)
    return bool(ok.item())


def forest_ragged_multiproof(ctx, d_leaves, d_offsets, n_trees, max_leaves, d_levels, tree_ids, leaf_ids, arity=4):
    """One shared, tree-major proof for leaves of many trees of a ragged forest (Context.merkle_forest_ragged_multiproof_device):
    d_leaves, d_offsets, n_trees, max_leaves, d_levels as merkle_forest_ragged_device took and filled them; (tree_ids[i], leaf_ids[i])
    in any order (sequences, numpy or torch): they are sorted and de-duplicated on the device.  Returns (tree_ids (k,) int32, leaf_ids
    (k,) int64, leaves (k, 4), proof (len, 4), proof_offsets (n_trees + 1,) int64), all on the device — what
    forest_ragged_multiproof_verify takes; proof[proof_offsets[t]:proof_offsets[t+1]] is tree t's single-tree proof.  One
    synchronisation, to read the proof's length.  A pair outside the forest: ValueError."""
    import torch
    f = "forest_ragged_multiproof"
    a = _arity(f, arity)
    ctx = ctx or Context.default()
    dev = d_leaves.device
    t = torch.as_tensor(tree_ids, device=dev).to(torch.int64).reshape(-1)
    l = torch.as_tensor(leaf_ids, device=dev).to(torch.int64).reshape(-1)
    if t.numel() != l.numel():
        raise ValueError("%s: %d tree ids, %d leaf ids" % (f, t.numel(), l.numel()))
    if t.numel() == 0:
        raise ValueError("%s: no pairs" % f)
    if not 0 < n_trees < 1 << 31 or not 0 < max_leaves < 1 << 32:
        raise ValueError("%s: n_trees must be in 1 .. 2^31 - 1 and max_leaves in 1 .. 2^32 - 1" % f)
    outside = int(((t < 0) | (t >= n_trees) | (l < 0) | (l >= max_leaves)).sum())
    if outside:
        raise ValueError("%s: %d pair(s) outside the forest (%d trees of at most %d leaves)" % (f, outside, n_trees, max_leaves))
    key = torch.unique((t << 32) | l)  # (sorted by tree, then leaf)
    k = key.numel()
    tid, lid = (key >> 32).to(torch.int32), key & 0xFFFFFFFF
    n_leaves = _n_scalars(d_leaves)
    bound = ctx.merkle_forest_ragged_multiproof_bound(n_leaves, n_trees, max_leaves, k, arity=arity)
    out = torch.empty((k, 4), dtype=torch.int64, device=dev)
    proof = torch.empty((bound, 4), dtype=torch.int64, device=dev)
    offs = torch.empty(n_trees + 1, dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    ctx.merkle_forest_ragged_multiproof_device(d_leaves, d_offsets, n_trees, max_leaves, d_levels if a.depth(max_leaves) else None, tid, lid, k, out,
                                               proof if bound else None, offs, n_bad, arity=arity)
    bad, length = int(n_bad.item()), int(offs[-1].item())
    if bad:
        raise ValueError("%s: %d pair(s) outside the forest (a bad tree, or a leaf id past its tree)" % (f, bad))
    return tid, lid, out, proof[:length], offs


def forest_ragged_multiproof_verify(ctx, d_offsets, n_leaves, n_trees, max_leaves, tree_ids, leaf_ids, leaves, proof, proof_offsets, d_roots,
                                    arity=4, tag=None):
    """The n_trees verdicts (a torch bool tensor on the host) of (tree_ids, leaf_ids, leaves, proof, proof_offsets) — torch CUDA tensors as
    forest_ragged_multiproof returns them — against d_roots (n_trees, 4) for a forest of the shape (d_offsets, n_leaves, n_trees,
    max_leaves), every ancestor hashed once (Context.merkle_forest_ragged_multiproof_verify_device): entry t is True iff tree t has a
    pair and its part of the proof re-hashes to d_roots[t].  Synchronises to read the verdicts."""
    import torch
    a = _arity("forest_ragged_multiproof_verify", arity)
    ctx = ctx or Context.default()
    ok = torch.zeros(n_trees, dtype=torch.uint8, device=leaves.device)
    proof_len = _n_scalars(proof)
    ctx.merkle_forest_ragged_multiproof_verify_device(
        a.tag() if tag is None else _as_scalars(tag).reshape(4), d_offsets, n_leaves, n_trees, max_leaves, tree_ids, leaf_ids, leaves,
        tree_ids.numel(), proof if proof_len else None, proof_len, proof_offsets, d_roots, ok, arity=arity)
    return ok.cpu().to(torch.bool)


def forest_range_stride(max_leaves, arity=4):
    """scalars of one row of range proofs, 2 (arity - 1) depth(max_leaves): room for the proof of any run
    (p252_merkle{4,2}_forest_range_stride)"""
    return int(_arity("forest_range_stride", arity).fn("forest_range_stride")(max_leaves))


def forest_ragged_range_proofs(ctx, d_leaves, d_offsets, n_trees, max_leaves, d_levels, tree_ids, first, lengths, arity=4):
    """The proofs of whole runs of leaves of a ragged forest (Context.merkle{4,2}_forest_ragged_range_proofs_device): d_leaves, d_offsets,
    n_trees, max_leaves, d_levels as merkle_forest_ragged_device took and filled them; run r is leaves [first[r], first[r] + lengths[r])
    of tree tree_ids[r] (sequences, numpy or torch).  Returns (tree_ids (m,) int32, first (m,) int64, leaf_offsets (m + 1,) int64,
    leaves (k, 4), proof (m, P, 4), proof_lens (m,) int32, counts (m,) int64), all on the device — what forest_range_verify takes; row r
    of the proof is the shared proof of merkle_multiproof for the positions of run r.  One synchronisation, to read the count of bad
    runs.  A run outside its tree: ValueError."""
    import torch
    f = "forest_ragged_range_proofs"
    a = _arity(f, arity)
    ctx = ctx or Context.default()
    dev = d_leaves.device
    t = torch.as_tensor(tree_ids, device=dev).to(torch.int64).reshape(-1)
    s = torch.as_tensor(first, device=dev).to(torch.int64).reshape(-1)
    n = torch.as_tensor(lengths, device=dev).to(torch.int64).reshape(-1)
    if not t.numel() == s.numel() == n.numel():
        raise ValueError("%s: %d tree ids, %d first leaves, %d lengths" % (f, t.numel(), s.numel(), n.numel()))
    m = t.numel()
    if m == 0:
        raise ValueError("%s: no runs" % f)
    outside = int(((t < 0) | (t >= n_trees) | (s < 0) | (n < 1) | (n > max_leaves)).sum())
    if outside:
        raise ValueError("%s: %d run(s) outside the forest (%d trees of at most %d leaves)" % (f, outside, n_trees, max_leaves))
    offs = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(n, 0)
    k = int(offs[-1].item())
    stride = forest_range_stride(max_leaves, arity)
    out = torch.empty((k, 4), dtype=torch.int64, device=dev)
    proof = torch.empty((m, stride, 4), dtype=torch.int64, device=dev)
    lens = torch.empty(m, dtype=torch.int32, device=dev)
    counts = torch.empty(m, dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    tid = t.to(torch.int32)
    call = ctx.merkle4_forest_ragged_range_proofs_device if a.arity == 4 else ctx.merkle2_forest_ragged_range_proofs_device
    call(d_leaves, d_offsets, n_trees, max_leaves, d_levels if stride else None, tid, s, offs, m, k, proof if stride else None, lens, counts,
         d_leaves_out=out, d_n_bad=n_bad)
    bad = int(n_bad.item())
    if bad:
        raise ValueError("%s: %d run(s) outside the forest (a bad tree, or a run past its tree's leaves)" % (f, bad))
    return tid, s, offs, out, proof, lens, counts


def forest_range_verify(ctx, tree_ids, counts, first, leaf_offsets, leaves, proof, proof_lens, d_roots, max_leaves, arity=4, tag=None):
    """The m verdicts (a torch bool tensor on the host) of (tree_ids, first, leaf_offsets, leaves, proof, proof_lens) — torch CUDA tensors
    as forest_ragged_range_proofs returns them — with the claimed leaf counts `counts` (m,) against d_roots (n_trees, 4)
    (Context.merkle{4,2}_forest_range_verify_device): entry r is True iff run r re-hashes to d_roots[tree_ids[r]].  Needs no forest.
    Synchronises to read the verdicts."""
    import torch
    a = _arity("forest_range_verify", arity)
    ctx = ctx or Context.default()
    m, k = tree_ids.numel(), _n_scalars(leaves)
    stride = _n_scalars(proof) // m if m else 0
    ok = torch.zeros(m, dtype=torch.uint8, device=leaves.device)
    call = ctx.merkle4_forest_range_verify_device if a.arity == 4 else ctx.merkle2_forest_range_verify_device
    call(a.tag() if tag is None else _as_scalars(tag).reshape(4), tree_ids, counts, first, leaf_offsets, m, max_leaves, leaves, k,
         proof if stride else None, stride, proof_lens, d_roots, _n_scalars(d_roots), ok)
    return ok.cpu().to(torch.bool)


def forest_ragged_update_sequential(ctx, d_leaves, d_offsets, n_trees, max_leaves, d_levels, tree_ids, leaf_ids, new_leaves, d_roots=None,
                                    arity=4, tag=None):
    """Leaf updates of a ragged forest applied IN ORDER, each with its witness (Context.merkle{4,2}_forest_ragged_update_sequential_device):
    d_leaves, d_offsets, n_trees, max_leaves, d_levels as merkle_forest_ragged_device took and filled them, updated in place (and d_roots
    (n_trees, 4), if given); update i writes new_leaves[i] (k, 4) to leaf leaf_ids[i] of tree tree_ids[i] (sequences, numpy or torch) and
    sees the forest as updates 0 .. i - 1 left it, so a pair may repeat.  The order the call needs — the stable sort by pair — is made
    here, on the device.  Returns (d_old_leaves (k, 4), d_siblings (k, D, arity - 1, 4), d_positions (k, D) uint8, d_depths (k,) uint8,
    d_roots_before (k, 4), d_roots_after (k, 4), D), all on the device: (old leaf, opening) re-hashes to the root before update i, (new
    leaf, the same opening) to the root after it.  One synchronisation, to read the count of bad updates.  An id outside the forest:
    ValueError before anything is enqueued; a bad tree or a leaf past its tree's leaves: ValueError after the call, which skipped that
    update alone and applied the others."""
    import torch
    f = "forest_ragged_update_sequential"
    a = _arity(f, arity)
    ctx = ctx or Context.default()
    dev = d_leaves.device
    t = torch.as_tensor(tree_ids, device=dev).to(torch.int64).reshape(-1)
    j = torch.as_tensor(leaf_ids, device=dev).to(torch.int64).reshape(-1)
    if isinstance(new_leaves, torch.Tensor):
        v = new_leaves.to(dev).contiguous()
    else:
        v = torch.from_numpy(_as_scalars(new_leaves).view(np.int64)).to(dev)
    k = t.numel()
    if k == 0:
        raise ValueError("%s: no updates" % f)
    if j.numel() != k or _n_scalars(v) != k:
        raise ValueError("%s: %d tree ids, %d leaf ids, %d new leaves" % (f, k, j.numel(), _n_scalars(v)))
    outside = int(((t < 0) | (t >= n_trees) | (j < 0) | (j >= max_leaves)).sum())
    if outside:
        raise ValueError("%s: %d update(s) outside the forest (%d trees of at most %d leaves)" % (f, outside, n_trees, max_leaves))
    # the stable sort by (tree id, leaf id): by leaf, then — stable — by tree; ties keep their index order
    by_leaf = torch.sort(j, stable=True).indices
    order = by_leaf[torch.sort(t[by_leaf], stable=True).indices].to(torch.int32)
    depth = a.depth(max_leaves)
    old = torch.empty((k, 4), dtype=torch.int64, device=dev)
    sib = torch.empty((k, depth, a.per, 4), dtype=torch.int64, device=dev)
    pos = torch.empty((k, depth), dtype=torch.uint8, device=dev)
    dep = torch.empty((k,), dtype=torch.uint8, device=dev)
    before = torch.empty((k, 4), dtype=torch.int64, device=dev)
    after = torch.empty((k, 4), dtype=torch.int64, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    call = ctx.merkle4_forest_ragged_update_sequential_device if a.arity == 4 else ctx.merkle2_forest_ragged_update_sequential_device
    call(a.tag() if tag is None else _as_scalars(tag).reshape(4), d_leaves, d_offsets, n_trees, max_leaves, d_levels if depth else None,
         t.to(torch.int32), j, v, order, k, sib if depth else None, pos if depth else None, dep, after, d_old_leaves=old, d_roots_before=before,
         d_roots=d_roots, d_n_bad=n_bad)
    bad = int(n_bad.item())
    if bad:
        raise ValueError("%s: %d update(s) outside the forest (a bad tree, or a leaf past its tree's leaves)" % (f, bad))
    return old, sib, pos, dep, before, after, depth


def _pairs_on_device(f, tree_ids, leaf_ids, ctx):
    """(d_tree_ids int32 or None, d_leaf_ids int64, k) on ctx's device: the bit patterns of uint32 tree ids and uint64 leaf ids"""
    import torch
    dev = torch.device("cuda", ctx.device)

    def words(x, wide):
        if isinstance(x, torch.Tensor):
            return x.to(dev).to(torch.int64 if wide else torch.int32).reshape(-1).contiguous()
        a = np.asarray(x)
        if a.size == 0:
            raise ValueError("%s: no pairs" % f)
        if a.dtype.kind not in "iu":
            raise ValueError("%s: ids must be integers, not %s" % (f, a.dtype))
        a = np.ascontiguousarray(a.astype(np.uint64 if wide else np.uint32).reshape(-1))
        return torch.from_numpy(a.view(np.int64 if wide else np.int32)).to(dev)
    j = words(leaf_ids, True)
    t = None if tree_ids is None else words(tree_ids, False)
    k = j.numel()
    if k == 0:
        raise ValueError("%s: no pairs" % f)
    if t is not None and t.numel() != k:
        raise ValueError("%s: %d tree ids, %d leaf ids" % (f, t.numel(), k))
    return t, j, k


def pairs_order(tree_ids, leaf_ids, ctx=None):
    """The indices 0 .. k - 1 sorted by (tree id, leaf id, index) — the stable sort by pair that
    Context.merkle{4,2}_forest_ragged_update_sequential_device takes as d_order — as an int32 tensor on the device, made by the library
    (Context.pairs_order_device).  tree_ids, leaf_ids: sequences, numpy or torch; tree_ids None: every pair is of tree 0.  Both parts
    compare as unsigned (uint32, uint64).  No synchronisation."""
    import torch
    ctx = ctx or Context.default()
    t, j, k = _pairs_on_device("pairs_order", tree_ids, leaf_ids, ctx)
    order = torch.empty(k, dtype=torch.int32, device=j.device)
    ctx.pairs_order_device(t, j, k, order)
    return order


def pairs_unique(tree_ids, leaf_ids, ctx=None):
    """The distinct pairs of (tree_ids, leaf_ids), ascending, as the shared proofs take them (Context.pairs_unique_device): returns
    (tree_ids int32 (n,), leaf_ids int64 (n,), first int32 (n,)) on the device, first[i] the lowest input index that holds pair i.
    tree_ids None: every pair is of tree 0 (the tree ids returned are zeros).  One synchronisation, to read the count."""
    import torch
    ctx = ctx or Context.default()
    t, j, k = _pairs_on_device("pairs_unique", tree_ids, leaf_ids, ctx)
    t_out = torch.empty(k, dtype=torch.int32, device=j.device)
    j_out = torch.empty(k, dtype=torch.int64, device=j.device)
    first = torch.empty(k, dtype=torch.int32, device=j.device)
    n = torch.zeros(1, dtype=torch.int64, device=j.device)
    ctx.pairs_unique_device(t, j, k, n, d_tree_ids_out=t_out, d_leaf_ids_out=j_out, d_first=first)
    n = int(n.item())
    return t_out[:n], j_out[:n], first[:n]


def merkle4_path_roots(leaves, siblings, positions, tag=None, ctx=None):
    """Roots recomputed from n openings (numpy host buffers); compare with the tree root to verify."""
    ctx = ctx or Context.default()
    tag = merkle4_tag() if tag is None else _as_scalars(tag).reshape(4)
    return ctx.merkle4_path_batch(tag, leaves, siblings, positions)
