"""The numpy model of the proofs of whole runs of leaves of a ragged forest (include/poseidon252_hip.h:
p252_merkle{4,2}_forest_ragged_range_proofs_device_into / p252_merkle{4,2}_forest_range_verify_device_into; csrc/forest_range.hip).
Run [a, b) of a tree of n leaves: with a_l = a // A^l, b_l = ceil(b / A^l), w_l = ceil(n / A^l), the nodes of level l that a verifier
knows or computes are the interval [a_l, b_l), and the proof of level l is [A a_{l+1}, a_l) then [b_l, min(A b_{l+1}, w_l)).
tests/test_forest_range_cpu.py checks every function here against testsupport/multiproofmodel.py.  No torch here."""
import numpy as np

from . import treeshape as TS

BAD_LEN = 0xFFFFFFFF


def _ceil(x, d):
    return -(-x // d)


def range_model(n, a, b, arity):
    """(proof_nodes, S, w) of the run [a, b) of a tree of n leaves, as multiproofmodel.multiproof_model gives them for the positions
    a .. b - 1: w[l] = nodes of level l, S[l] = (a_l, b_l), proof_nodes[l] = the nodes of level l that the proof holds, in proof order"""
    assert n >= 1 and 0 <= a < b <= n
    S, w, proof_nodes, d = [(a, b)], [n], [], 1
    while w[-1] > 1:
        a_l, b_l = S[-1]
        up = (a // (d * arity), _ceil(b, d * arity))
        proof_nodes.append(np.concatenate([np.arange(arity * up[0], a_l), np.arange(b_l, min(arity * up[1], w[-1]))]).astype(np.int64))
        d *= arity
        S.append(up)
        w.append(_ceil(n, d))
    return proof_nodes, S, w


def range_counts(n, a, b, arity):
    """(proof scalars, digests a verifier computes)"""
    proof_nodes, S, _ = range_model(n, a, b, arity)
    return int(sum(p.size for p in proof_nodes)), int(sum(hi - lo for lo, hi in S[1:]))


def range_stride(max_leaves, arity):
    """p252_merkle{4,2}_forest_range_stride"""
    return 2 * (arity - 1) * int(TS.depth(max_leaves, arity))


def level_bound(k, m, l, arity):
    """the host's bound of the nodes that m runs of k leaves in all have on level l >= 1 together"""
    return min(k + m, k // arity ** l + 2 * m)


# ---------------------------------------------------------------------------------------------- the bad-run rule
def run_lengths(leaf_offsets, k):
    """the ragged forest's rule for tree offsets with k in the place of n_leaves (and of max_leaves): len(leaf_offsets) - 1 lengths, 0 for
    a bad run — decreasing, empty, past k, or the lengths of the runs before it (those that passed the first three) and its own above k"""
    off = [int(v) for v in np.asarray(leaf_offsets, dtype=np.uint64)]
    first = [hi - lo if lo <= hi <= k and hi > lo else 0 for lo, hi in zip(off[:-1], off[1:])]
    out, before = [], 0
    for n in first:
        out.append(n if before <= k and n <= k - before else 0)
        before += n
    return np.array(out, dtype=np.int64)


def good_runs(counts, tree_ids, first, leaf_offsets, k, n_trees, max_leaves):
    """(good (m,) bool, lengths (m,)): counts[r] = the leaf count of run r's tree (the forest's own, 0 for a bad tree; or the
    verifier's claim)"""
    lens = run_lengths(leaf_offsets, k)
    good = []
    for r, n in enumerate(lens):
        t, a, c = int(tree_ids[r]), int(first[r]), int(counts[r]) if int(tree_ids[r]) < n_trees else 0
        good.append(bool(n > 0 and t < n_trees and 1 <= c <= max_leaves and a <= c and n <= c - a))
    return np.array(good, dtype=bool), lens


# ---------------------------------------------------------------------------------------------- extraction
def _levels_of(leaves, levels, n, arity):
    per_level, off = [leaves], 0
    for w in TS.level_widths(int(n), arity):
        per_level.append(levels[off:off + w])
        off += w
    return per_level


def range_extract(leaves, offsets, levels, tree_ids, first, leaf_offsets, k, max_leaves, arity, leaves_out=None):
    """(proof (m, P, 4), proof_lens (m,) uint32, counts (m,) uint64, leaves_out (k, 4), n_bad) out of a built forest: leaves (n, 4),
    offsets (n_trees + 1,), levels = the tree-major upper levels; leaves_out starts as the given array (default zeros)"""
    leaves, levels = np.asarray(leaves).reshape(-1, 4), np.asarray(levels).reshape(-1, 4)
    off = np.asarray(offsets, dtype=np.int64)
    sizes = np.diff(off)
    lo = TS.block_starts(sizes, arity)
    m, P = len(tree_ids), range_stride(max_leaves, arity)
    per_run = [int(sizes[t]) if int(t) < len(sizes) else 0 for t in tree_ids]
    good, lens = good_runs(per_run, tree_ids, first, leaf_offsets, k, len(sizes), max_leaves)
    proof, plen = np.zeros((m, P, 4), dtype=np.uint64), np.full(m, BAD_LEN, dtype=np.uint32)
    counts = np.zeros(m, dtype=np.uint64)
    out = np.zeros((k, 4), dtype=np.uint64) if leaves_out is None else np.array(leaves_out, dtype=np.uint64)
    for r in np.nonzero(good)[0]:
        t, a, n = int(tree_ids[r]), int(first[r]), per_run[r]
        b = a + int(lens[r])
        per_level = _levels_of(leaves[off[t]:off[t + 1]], levels[lo[t]:lo[t + 1]], n, arity)
        parts = [per_level[l][nodes] for l, nodes in enumerate(range_model(n, a, b, arity)[0])]
        row = np.concatenate(parts) if parts else np.zeros((0, 4), dtype=np.uint64)
        proof[r, :row.shape[0]] = row
        plen[r], counts[r] = row.shape[0], n
        at = int(leaf_offsets[r])
        out[at:at + b - a] = leaves[off[t] + a:off[t] + b]
    return proof, plen, counts, out, int((~good).sum())


# ---------------------------------------------------------------------------------------------- verification
def range_root(n, a, leaf_values, proof, arity, digest):
    """the root that the run [a, a + len(leaf_values)) of a tree of n leaves re-hashes to with the proof row `proof` (its first
    range_counts scalars are used) and digest((m, arity, 4)) -> (m, 4); a one-leaf tree gives its leaf as it stands"""
    vals = np.asarray(leaf_values, dtype=np.uint64).reshape(-1, 4)
    proof_nodes, S, w = range_model(n, a, a + vals.shape[0], arity)
    proof, at = np.asarray(proof, dtype=np.uint64).reshape(-1, 4), 0
    for l, nodes in enumerate(proof_nodes):
        lo, hi = S[l + 1]
        children = np.zeros(((hi - lo) * arity, 4), dtype=np.uint64)  # (slots at or past w[l] stay zero)
        children[S[l][0] - lo * arity:S[l][1] - lo * arity] = vals
        children[nodes - lo * arity] = proof[at:at + nodes.size]
        at += nodes.size
        vals = np.asarray(digest(children.reshape(hi - lo, arity, 4))).reshape(-1, 4)
    return vals[0]


def range_verify(counts, tree_ids, first, leaf_offsets, k, max_leaves, leaves_in, proof, proof_lens, roots, arity, digest, reduce):
    """(ok (m,) uint8, roots_out {r: root} of the runs that pass everything but the comparison, n_hashed, n_bad): proof (m, stride, 4),
    roots (n_trees, 4); reduce((1, 4)) -> (1, 4) is the leaf mod p of a one-leaf tree"""
    proof, roots = np.asarray(proof, dtype=np.uint64), np.asarray(roots, dtype=np.uint64).reshape(-1, 4)
    leaves_in = np.asarray(leaves_in, dtype=np.uint64).reshape(-1, 4)
    m, stride = len(tree_ids), proof.shape[1]
    good, lens = good_runs(counts, tree_ids, first, leaf_offsets, k, roots.shape[0], max_leaves)
    ok, roots_out, hashed = np.zeros(m, dtype=np.uint8), {}, 0
    for r in np.nonzero(good)[0]:
        n, a, at = int(counts[r]), int(first[r]), int(leaf_offsets[r])
        length, digests = range_counts(n, a, a + int(lens[r]), arity)
        if int(proof_lens[r]) != length or length > stride:
            continue
        root = range_root(n, a, leaves_in[at:at + int(lens[r])], proof[r], arity, digest)
        if n == 1:
            root = np.asarray(reduce(root.reshape(1, 4))).reshape(4)
        hashed += digests
        roots_out[int(r)] = root
        ok[r] = np.array_equal(root, roots[int(tree_ids[r])])
    return ok, roots_out, hashed, int((~good).sum())


# ---------------------------------------------------------------------------------------------- the dense lists
def scan_bases(counts, first, lens, depth, arity):
    """(base (depth + 1, m), totals (depth + 1,)): base[l][r] = the nodes that the runs before r have on level l, counts[r] = 0 for
    a run that takes no part; a run of a tree that ends below level l has no node there"""
    m = len(counts)
    cnt = np.zeros((depth + 1, m), dtype=np.int64)
    for r in range(m):
        if int(counts[r]):
            _, S, _ = range_model(int(counts[r]), int(first[r]), int(first[r]) + int(lens[r]), arity)
            for l, (lo, hi) in enumerate(S):
                cnt[l, r] = hi - lo
    base = np.zeros_like(cnt)
    base[:, 1:] = np.cumsum(cnt, axis=1)[:, :-1]
    return base, cnt.sum(axis=1)
