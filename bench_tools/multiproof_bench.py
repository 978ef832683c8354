#!/usr/bin/env python3
"""Many leaves of ONE tree behind one shared proof (p252_merkle{4,2}_multiproof_device / _verify_device, every ancestor hashed once)
against the per-leaf calls (p252_merkle{4,2}_openings_device, p252_merkle{4,2}_verify_batch_device) on the same leaves.

  python bench_tools/multiproof_bench.py [--reps 20] [--out profiles/multiproof.txt] [--quick]

One arity-4 tree of 4^12 leaves and one arity-2 tree of 2^24 leaves; k = 2^10, 2^14, 2^17, 2^20 random distinct positions (seed 1),
sorted.  Every shape is warmed up; times are medians of --reps host wall clocks around calls that end in a device synchronise; the
two sides of a ratio alternate in the one process; every multiproof is verified (ok = 1, root = the tree's) and its length and digest
count are compared with the numpy model below before it is timed; the shader clock is probed before and after.
Prints one line per workload, writes them to --out, and prints a JSON summary last.

The numpy model of the proof format (include/poseidon252_hip.h) is here too — multiproof_model, multiproof_extract, multiproof_root —
for the tests to compare the device's bytes and counts with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def tree_device(ctx, arity, tag, d_leaves, n, d_root, d_levels):
    """p252_merkle{4,2}_tree_device on torch's current stream (the Python mirror has the arity-4 call only)"""
    import ctypes
    from poseidon252_amd import _lib
    from poseidon252_amd.hash import _stream
    L = _lib.lib()
    fn = L.p252_merkle4_tree_device if arity == 4 else L.p252_merkle2_tree_device
    tp = np.ascontiguousarray(tag, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    ctx._check(fn(ctx._h, tp, d_leaves.data_ptr(), n, d_root.data_ptr(), d_levels.data_ptr() if d_levels is not None else None, _stream(ctx)))


def _once_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _alternate(fns, reps):
    """medians (ms) of the callables, run in turn `reps` times"""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ts[i].append(_once_ms(fn))
    return [float(np.median(t)) for t in ts]


def _clock_mhz(ctx):
    """shader clock of one probe wave (MHz), or None"""
    import torch
    try:
        t = ctx.clock_probe(spin_us=1000)
        torch.cuda.synchronize()
        return round(ctx.clock_probe_result(t)["shader_ghz"] * 1e3, 1)
    except Exception:  # (a measurement aid only)
        return None


def _tree(ctx, arity, n, say, reps, ks):
    import torch
    from poseidon252_amd import merkle as M
    dev = torch.device("cuda:0")
    tag = M.merkle4_tag() if arity == 4 else M.merkle2_tag()
    d = torch.randint(0, 1 << 60, (n, 4), dtype=torch.int64, device=dev)
    root = torch.empty(4, dtype=torch.int64, device=dev)
    lv = torch.empty((M.levels_len(n, arity), 4), dtype=torch.int64, device=dev)
    tree_device(ctx, arity, tag, d, n, root, lv)
    rows = []
    for k in ks:
        pos = np.sort(np.random.default_rng(1).choice(n, k, replace=False)).astype(np.uint32)
        d_idx = torch.from_numpy(pos.view(np.int32)).to(dev)
        want_len, want_hashed = multiproof_counts(n, pos, arity)
        bound = ctx.merkle_multiproof_bound(n, k, arity)
        out = torch.empty((k, 4), dtype=torch.int64, device=dev)
        proof = torch.empty((bound, 4), dtype=torch.int64, device=dev)
        plen, hashed = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        ok, root_out = torch.zeros(1, dtype=torch.uint8, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        extract = lambda: ctx.merkle_multiproof_device(d, n, lv, d_idx, k, out, proof, plen, arity=arity)  # noqa: E731
        extract()
        length = int(plen)
        verify = lambda: ctx.merkle_multiproof_verify_device(tag, n, d_idx, out, k, proof, length, root, ok, d_root_out=root_out,  # noqa: E731
                                                             d_n_hashed=hashed, arity=arity)
        verify()
        torch.cuda.synchronize()
        good = length == want_len and int(hashed) == want_hashed and int(ok) == 1 and bool(torch.equal(root_out, root))
        # the per-leaf calls on the same leaves
        o_l, o_s, o_p, depth = ctx.merkle4_openings_device(d, n, lv, d_idx, k, arity=arity)
        bufs = (o_l, o_s, o_p, torch.zeros(1, dtype=torch.int32, device=dev))
        openings = lambda: ctx.merkle4_openings_device(d, n, lv, d_idx, k, out=bufs, arity=arity)  # noqa: E731
        oks = torch.zeros(k, dtype=torch.uint8, device=dev)
        batch = lambda: ctx.merkle_verify_batch_device(tag, o_l, o_s, o_p, depth, root, oks, k, arity=arity)  # noqa: E731
        batch()
        torch.cuda.synchronize()
        good = good and int(oks.sum()) == k
        t_open, t_extract = _alternate([openings, extract], reps)
        t_batch, t_verify = _alternate([batch, verify], reps)
        per_leaf_scalars, per_leaf_digests = k * depth * (arity - 1), k * depth
        rows.append({"arity": arity, "leaves": n, "k": k, "openings_ms": t_open, "multiproof_ms": t_extract, "extract_ratio": t_open / t_extract,
                     "verify_batch_ms": t_batch, "multiproof_verify_ms": t_verify, "verify_ratio": t_batch / t_verify,
                     "siblings_bytes": per_leaf_scalars * 32, "proof_bytes": length * 32, "bytes_ratio": per_leaf_scalars / max(length, 1),
                     "digests_per_leaf": per_leaf_digests, "digests_once": int(hashed), "digest_ratio": per_leaf_digests / int(hashed),
                     "bound": bound, "agrees_with_model": good})
        say("arity %d, %d leaves, k = 2^%d: extract openings %.3f ms (%d B)  multiproof %.3f ms (%d B; bound %d B)  ratio %.2f (bytes %.2f)  |  "
            "verify_batch %.3f ms (%d digests)  multiproof_verify %.3f ms (%d digests)  ratio %.2f (digests %.2f)  agrees with the model %s"
            % (arity, n, int(np.log2(k)), t_open, per_leaf_scalars * 32, t_extract, length * 32, bound * 32, t_open / t_extract,
               per_leaf_scalars / max(length, 1), t_batch, per_leaf_digests, t_verify, int(hashed), t_batch / t_verify,
               per_leaf_digests / int(hashed), good))
        del out, proof, o_l, o_s, o_p, bufs
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiproof.txt"), help="where the workload lines are written")
    ap.add_argument("--quick", action="store_true", help="small shapes (4^8 and 2^16 leaves): a check of the tool, not a measurement")
    ap.add_argument("--only", type=int, default=0, help="one k of one arity-4 tree only (for a profiler run)")
    a = ap.parse_args()
    import poseidon252_amd as P
    ctx = P.Context(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    res = {"reps": a.reps, "clock_mhz_before": _clock_mhz(ctx)}
    say("python bench_tools/multiproof_bench.py --reps %d%s   shader clock before: %s MHz" % (a.reps, " --quick" if a.quick else "", res["clock_mhz_before"]))
    ks = [1 << 6, 1 << 10, 1 << 14] if a.quick else [1 << 10, 1 << 14, 1 << 17, 1 << 20]
    if a.only:
        res["rows"] = _tree(ctx, 4, 4 ** 12, say, a.reps, [a.only])
    else:
        res["rows"] = _tree(ctx, 4, 4 ** 8 if a.quick else 4 ** 12, say, a.reps, ks)
        res["rows"] += _tree(ctx, 2, 2 ** 16 if a.quick else 2 ** 24, say, a.reps, ks)
    res["clock_mhz_after"] = _clock_mhz(ctx)
    say("shader clock after: %s MHz" % res["clock_mhz_after"])
    if not a.only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
