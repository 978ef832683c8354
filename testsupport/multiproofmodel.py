"""The numpy model of the shared proof of many leaves (include/poseidon252_hip.h): of ONE tree (p252_merkle{4,2}_multiproof_device /
_verify_device) — multiproof_model, multiproof_extract, multiproof_root — and of a ragged forest
(p252_merkle{4,2}_forest_ragged_multiproof_device_into / _verify_device), a composition of the single-tree model:
P_t = multiproof_extract(tree t's leaves, tree t's levels, tree t's positions).  The tests compare the device's bytes and counts with
it; tests/test_multiproof_cpu.py and tests/test_forest_multiproof_cpu.py check the model.  No torch here."""
import numpy as np

from . import treeshape as TS


def multiproof_model(n_leaves, positions, arity):
    """the structure of the shared proof of the strictly ascending `positions` of a tree of n_leaves: (proof_nodes, S, w) with
    w[l] = nodes of level l, S[l] = the sorted nodes of level l that the verifier knows or computes (S[0] = the positions), and
    proof_nodes[l] = the nodes of level l the proof holds, in proof order (l = 0 .. depth - 1)"""
    s = np.asarray(positions, dtype=np.int64).reshape(-1)
    assert s.size and n_leaves >= 1 and int(s[0]) >= 0 and int(s[-1]) < n_leaves and bool(np.all(np.diff(s) > 0))
    S, w, proof_nodes = [s], [int(n_leaves)], []
    while w[-1] > 1:
        parents = np.unique(S[-1] // arity)
        slots = (parents[:, None] * arity + np.arange(arity)).reshape(-1)  # parent by parent, slot by slot: the visiting order
        proof_nodes.append(slots[(slots < w[-1]) & ~np.isin(slots, S[-1])])
        S.append(parents)
        w.append((w[-1] + arity - 1) // arity)
    return proof_nodes, S, w


def multiproof_counts(n_leaves, positions, arity):
    """(proof scalars, digests a verifier computes)"""
    proof_nodes, S, _ = multiproof_model(n_leaves, positions, arity)
    return int(sum(p.size for p in proof_nodes)), int(sum(s.size for s in S[1:]))


def multiproof_bound(n_leaves, k, arity):
    """p252_merkle{4,2}_multiproof_bound"""
    total, w = 0, n_leaves
    while w > 1:
        up = (w + arity - 1) // arity
        total += min((arity - 1) * min(k, up), w - min(k, w))
        w = up
    return total


def _split_levels(leaves, levels, arity):
    leaves, levels = np.asarray(leaves).reshape(-1, 4), np.asarray(levels).reshape(-1, 4)
    per_level, cnt, off = [leaves], leaves.shape[0], 0
    while cnt > 1:
        cnt = (cnt + arity - 1) // arity
        per_level.append(levels[off:off + cnt])
        off += cnt
    return per_level


def multiproof_extract(leaves, levels, positions, arity):
    """the proof (len, 4) of `positions` out of a stored tree: leaves (n, 4), levels = the upper levels bottom-up"""
    per_level = _split_levels(leaves, levels, arity)
    proof_nodes, _, _ = multiproof_model(per_level[0].shape[0], positions, arity)
    parts = [per_level[l][nodes] for l, nodes in enumerate(proof_nodes)]
    return np.concatenate(parts) if parts else np.zeros((0, 4), dtype=per_level[0].dtype)


def multiproof_root(n_leaves, positions, leaf_values, proof, arity, digest):
    """the verifier: the root that (positions, leaf_values (k, 4), proof (len, 4)) re-hash to with digest((m, arity, 4)) -> (m, 4),
    or None when the structure does not consume exactly len(proof) scalars"""
    proof_nodes, S, w = multiproof_model(n_leaves, positions, arity)
    proof = np.asarray(proof, dtype=np.uint64).reshape(-1, 4)
    if proof.shape[0] != sum(p.size for p in proof_nodes):
        return None
    vals, at = np.asarray(leaf_values, dtype=np.uint64).reshape(-1, 4), 0
    for l, nodes in enumerate(proof_nodes):
        parents = S[l + 1]
        children = np.zeros((parents.size * arity, 4), dtype=np.uint64)  # (slots at or past w[l] stay zero)
        first = parents * arity
        place = lambda c: np.searchsorted(first, c - c % arity) * arity + c % arity  # noqa: E731
        children[place(S[l])] = vals
        children[place(nodes)] = proof[at:at + nodes.size]
        at += nodes.size
        vals = np.asarray(digest(children.reshape(parents.size, arity, 4))).reshape(-1, 4)
    return vals[0]


# ---------------------------------------------------------------------------------------------- the forest
def forest_pairs_by_tree(n_trees, tree_ids, leaf_ids):
    """{t: the ascending positions asked of tree t} for strictly ascending pairs (trees without pairs are absent)"""
    tid, lid = np.asarray(tree_ids, dtype=np.int64).reshape(-1), np.asarray(leaf_ids, dtype=np.int64).reshape(-1)
    assert tid.size == lid.size and tid.size and int(tid.min()) >= 0 and int(tid.max()) < n_trees
    key = tid * (1 << 40) + lid
    assert bool(np.all(np.diff(key) > 0)), "pairs must be strictly ascending in (tree, leaf)"
    trees, first = np.unique(tid, return_index=True)
    return {int(t): part for t, part in zip(trees, np.split(lid, first[1:]))}


def forest_multiproof_counts(sizes, tree_ids, leaf_ids, arity):
    """(proof_offsets (n_trees + 1,) uint64, digests a verifier computes) of the forest proof of the pairs in trees of `sizes` leaves"""
    per_tree = forest_pairs_by_tree(len(sizes), tree_ids, leaf_ids)
    lens, hashed = np.zeros(len(sizes) + 1, dtype=np.uint64), 0
    for t, pos in per_tree.items():
        length, digests = multiproof_counts(int(sizes[t]), pos, arity)
        lens[t + 1] = length
        hashed += digests
    return np.cumsum(lens, dtype=np.uint64), hashed


def forest_multiproof_extract(leaves, offsets, levels, tree_ids, leaf_ids, arity):
    """(leaves_out (k, 4), proof (len, 4), proof_offsets (n_trees + 1,)) out of a built forest: leaves (n, 4), offsets (n_trees + 1,),
    levels = the tree-major upper levels (tree t's block after the blocks of the trees before it)"""
    leaves, levels = np.asarray(leaves).reshape(-1, 4), np.asarray(levels).reshape(-1, 4)
    off = np.asarray(offsets, dtype=np.int64)
    sizes = np.diff(off)
    lo = TS.offsets(TS.levels_len(sizes, arity), dtype=np.int64)
    per_tree = forest_pairs_by_tree(len(sizes), tree_ids, leaf_ids)
    parts, lens = [], np.zeros(len(sizes) + 1, dtype=np.uint64)
    for t in sorted(per_tree):
        p = multiproof_extract(leaves[off[t]:off[t + 1]], levels[lo[t]:lo[t + 1]], per_tree[t], arity)
        parts.append(p)
        lens[t + 1] = p.shape[0]
    proof = np.concatenate(parts) if parts else np.zeros((0, 4), dtype=leaves.dtype)
    tid, lid = np.asarray(tree_ids, dtype=np.int64).reshape(-1), np.asarray(leaf_ids, dtype=np.int64).reshape(-1)
    return leaves[off[tid] + lid], proof, np.cumsum(lens, dtype=np.uint64)


def forest_multiproof_roots(sizes, tree_ids, leaf_ids, leaf_values, proof, proof_offsets, arity, digest, reduce=None):
    """{t: the root tree t's part re-hashes to, or None when its structure does not consume exactly its part}; a one-leaf tree's root is
    reduce(its leaf) (the forest's convention: the leaf mod p)"""
    per_tree = forest_pairs_by_tree(len(sizes), tree_ids, leaf_ids)
    tid = np.asarray(tree_ids, dtype=np.int64).reshape(-1)
    vals, proof, po = np.asarray(leaf_values).reshape(-1, 4), np.asarray(proof).reshape(-1, 4), np.asarray(proof_offsets, dtype=np.int64)
    out = {}
    for t, pos in per_tree.items():
        root = multiproof_root(int(sizes[t]), pos, vals[tid == t], proof[po[t]:po[t + 1]], arity, digest)
        if root is not None and int(sizes[t]) == 1 and reduce is not None:
            root = np.asarray(reduce(np.asarray(root).reshape(1, 4))).reshape(4)
        out[t] = root
    return out


def forest_multiproof_bound(n_leaves, n_trees, max_leaves, k, arity):
    """p252_merkle{4,2}_forest_ragged_multiproof_bound"""
    if not (k and n_leaves and n_trees):
        return 0
    d = TS.depth(max_leaves, arity)
    return min(k * d * (arity - 1), n_leaves + n_leaves // (arity - 1) + n_trees * d)
