"""Round 5: the asynchronous builders are re-entrant across STREAMS of one context (the reference is
re-entrant by construction: `const` tables, borrows only — src/hash.rs:92-96); library-owned copies of secrets are wiped (the
reference builds with `zeroize`, Cargo.toml:14; src/encryption.rs:62-95); Hash::finalize_truncated (src/hash.rs:164-183, 203-210)
is ONE launch — the digest kernels' own output stage — asserted on a kernel trace."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.forest import _np as _host, _torch as _dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- item 2: streams of ONE context
def test_two_root_only_builds_on_two_streams_of_one_context(gpu_ctx, oracle_mod):
    """two DIFFERENT 4^8-leaf root-only builds issued back to back on two torch streams of ONE context, 50 times: round 4 shared
    one ping-pong scratch per context between them (api.cpp d_lvl) and returned wrong roots, silently"""
    import torch
    import poseidon252_amd as P
    tag = P.merkle4_tag()
    n = 4 ** 8
    la, lb = oracle_mod.fill_random(0x51, n), oracle_mod.fill_random(0x52, n)
    ea, eb = oracle_mod.merkle4_tree(tag, la)[0], oracle_mod.merkle4_tree(tag, lb)[0]
    da, db = _dev(la), _dev(lb)
    ra = torch.zeros((50, 4), dtype=torch.int64, device="cuda:0")
    rb = torch.zeros((50, 4), dtype=torch.int64, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for i in range(50):
        with torch.cuda.stream(s1):
            gpu_ctx.merkle4_tree_device(tag, da, n, ra[i], None)
        with torch.cuda.stream(s2):
            gpu_ctx.merkle4_tree_device(tag, db, n, rb[i], None)
    torch.cuda.synchronize()
    assert np.array_equal(_host(ra), np.tile(ea, (50, 1))), "stream 1's roots differ from the oracle's"
    assert np.array_equal(_host(rb), np.tile(eb, (50, 1))), "stream 2's roots differ from the oracle's"


def test_more_streams_than_scratch_pairs_and_forests(gpu_ctx, oracle_mod):
    """six streams on one context (the context keeps four scratch pairs: the fifth and sixth stream take over the least recently
    used pair behind an event), trees of different sizes and a forest in the mix, three rounds: every root equals the oracle's"""
    import torch
    import poseidon252_amd as P
    tag = P.merkle4_tag()
    sizes = [4 ** 7, 4 ** 6, 4 ** 7, 5000, 4 ** 5, 4 ** 7]
    leaves = [oracle_mod.fill_random(0x60 + i, m) for i, m in enumerate(sizes)]
    exp = [oracle_mod.merkle4_tree(tag, lv)[0] for lv in leaves]
    d = [_dev(lv) for lv in leaves]
    streams = [torch.cuda.Stream() for _ in sizes]
    roots = torch.zeros((3, len(sizes), 4), dtype=torch.int64, device="cuda:0")
    per, n_trees = 4 ** 4, 64
    fl = oracle_mod.fill_random(0x6f, per * n_trees)
    d_fl = _dev(fl)
    f_roots = torch.zeros((3, n_trees, 4), dtype=torch.int64, device="cuda:0")
    fs = torch.cuda.Stream()
    torch.cuda.synchronize()
    for rnd in range(3):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                gpu_ctx.merkle4_tree_device(tag, d[i], sizes[i], roots[rnd, i], None)
        with torch.cuda.stream(fs):
            gpu_ctx.merkle4_forest_device(tag, d_fl, n_trees, per, f_roots[rnd])
    torch.cuda.synchronize()
    got = _host(roots).reshape(3, len(sizes), 4)
    for rnd in range(3):
        for i in range(len(sizes)):
            assert np.array_equal(got[rnd, i], exp[i]), (rnd, i)
    fr = _host(f_roots).reshape(3, n_trees, 4)
    for t in (0, 17, n_trees - 1):
        e = oracle_mod.merkle4_tree(tag, fl[t * per:(t + 1) * per])[0]
        assert all(np.array_equal(fr[rnd, t], e) for rnd in range(3)), t


def test_sharded_builds_of_one_communicator_on_two_streams(gpu_ctx, oracle_mod):
    """a communicator's d_sub / d_roots / d_top are one set: builds queued on two streams are ordered by an event, never concurrent
     — world = 1 on the real backend, two different leaf sets, 20 times"""
    import torch
    import poseidon252_amd as P
    from poseidon252_amd import comm as C
    tag = P.merkle4_tag()
    n = 4 ** 7
    la, lb = oracle_mod.fill_random(0x71, n), oracle_mod.fill_random(0x72, n)
    ea, eb = oracle_mod.merkle4_tree(tag, la)[0], oracle_mod.merkle4_tree(tag, lb)[0]
    da, db = _dev(la), _dev(lb)
    ctx = P.Context(0)
    c = C.Comm.create_rank(ctx, 0, 1, lambda b: b)
    ra = torch.zeros((20, 4), dtype=torch.int64, device="cuda:0")
    rb = torch.zeros((20, 4), dtype=torch.int64, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for i in range(20):
        with torch.cuda.stream(s1):
            c.merkle4_tree_sharded_device(tag, da, n, ra[i])
        with torch.cuda.stream(s2):
            c.merkle4_tree_sharded_device(tag, db, n, rb[i])
    torch.cuda.synchronize()
    assert np.array_equal(_host(ra), np.tile(ea, (20, 1))) and np.array_equal(_host(rb), np.tile(eb, (20, 1)))
    c.destroy()
    ctx.close()


# ---------------------------------------------------------------------------------------------- item 3: secret hygiene
@pytest.mark.parametrize("n,length", [(300, 2), (5000, 7), (70000, 42)])  # 70,000 x 42 scalars: through the staging lanes, several chunks
def test_host_encrypt_and_decrypt_leave_nothing_in_the_context(oracle_mod, n, length):
    """shared secrets, nonces and plaintexts of p252_encrypt_batch / p252_decrypt_batch (host buffers) are copied into the
    context's device scratch or its page-locked staging lanes: both are zero again when the call returns"""
    import poseidon252_amd as P
    from poseidon252_amd import encryption as Enc
    ctx = P.Context(0)
    try:
        assert ctx.scratch_residue() == 0  # a fresh context owns nothing yet
        msgs = oracle_mod.fill_random(0x81 + n, n * length).reshape(n, length, 4)
        secrets = oracle_mod.fill_random(0x82 + n, n * 2).reshape(n, 2, 4)
        nonces = oracle_mod.fill_random(0x83 + n, n).reshape(n, 4)
        ciphers = Enc.encrypt_batch(msgs, secrets, nonces, ctx=ctx)
        assert ctx.scratch_residue() == 0, "encrypt left data in library-owned buffers"  # (the call table holds kind/len words, nothing of the caller's: not counted since ABI 8)
        back, ok = Enc.decrypt_batch(ciphers, secrets, nonces, ctx=ctx)
        assert ctx.scratch_residue() == 0, "decrypt left data in library-owned buffers"
        assert bool(np.all(ok)) and np.array_equal(back.reshape(msgs.shape), msgs)
        idx = np.arange(0, n, max(1, n // 64))
        tag = Enc.encryption_tag(length)
        assert np.array_equal(np.asarray(ciphers).reshape(n, length + 1, 4)[idx],
                              oracle_mod.encrypt_batch(tag, np.ascontiguousarray(msgs[idx]), np.ascontiguousarray(secrets[idx]), np.ascontiguousarray(nonces[idx])))
        # hashing calls do not wipe (their inputs are public): the scratch holds data until p252_wipe / p252_destroy
        hb = P.HashBatch(P.Domain.Other, 5, ctx=ctx)
        hb.digest(oracle_mod.fill_random(0x84, 5 * 2000).reshape(2000, 5, 4))
        assert ctx.scratch_residue() > 2000 * 5 * 16
        ctx.wipe()
        assert ctx.scratch_residue() == 0
        # ... and the context works as before after a wipe (the call table is uploaded again)
        assert np.array_equal(Enc.encrypt_batch(msgs[:50], secrets[:50], nonces[:50], ctx=ctx), ciphers[:50])
    finally:
        ctx.close()


def test_wipe_covers_level_scratch_and_staging_lanes(oracle_mod):
    import torch
    import poseidon252_amd as P
    ctx = P.Context(0)
    try:
        tag = P.merkle4_tag()
        lv = oracle_mod.fill_random(0x91, 4 ** 7)
        root = torch.zeros(4, dtype=torch.int64, device="cuda:0")
        ctx.merkle4_tree_device(tag, _dev(lv), 4 ** 7, root, None)  # root-only: the levels ping-pong in context-owned scratch
        torch.cuda.synchronize()
        big = oracle_mod.fill_random(0x92, 4 * (1 << 19)).reshape(-1, 4, 4)  # 64 MiB of pageable input: staging lanes
        P.HashBatch(P.Domain.Merkle4, 4, ctx=ctx).digest(big)
        assert ctx.scratch_residue() > (4 ** 6) * 16
        ctx.wipe()
        assert ctx.scratch_residue() == 0
        assert np.array_equal(_host(root), oracle_mod.merkle4_tree(tag, lv)[0])
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- item 5: fused truncation
@pytest.mark.parametrize("domain,item_len,out_len,n", [("Merkle4", 4, 1, 3000), ("Merkle4", 4, 1, 70000), ("Merkle2", 2, 1, 9000),
                                                       ("Other", 5, 1, 300),   # tests/hash.rs:188-203: 5 inputs, truncated
                                                       ("Other", 5, 1, 20000), ("Other", 42, 5, 9001), ("Other", 3, 7, 100), ("Other", 42, 5, 64)])
def test_digest_truncated_is_the_fused_output_stage(gpu_ctx, oracle_mod, domain, item_len, out_len, n):
    """every kernel family's truncating build (lane groups, one lane; whole-line fetches; single-permutation digests) against the
    oracle's rule applied to the oracle's digests, host and device buffers, and against the two-launch form"""
    import torch
    import poseidon252_amd as P
    hb = P.HashBatch(getattr(P.Domain, domain), item_len, output_len=out_len, ctx=gpu_ctx)
    m = oracle_mod.fill_random(0xa0 + n + item_len, n * item_len).reshape(n, item_len, 4)
    full = oracle_mod.hash_batch(hb.tag, m, item_len, hb.out_len, threads=8).reshape(-1, 4)
    exp = np.stack([oracle_mod.truncate250(v) for v in full]).reshape(n, hb.out_len, 4)
    assert np.array_equal(hb.digest_truncated(m), exp)
    d = hb.digest_truncated(_dev(m))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d).reshape(exp.shape), exp)
    two = hb.digest(_dev(m))
    gpu_ctx.truncate250_device(two, two, two.numel() // 4)
    torch.cuda.synchronize()
    assert torch.equal(two, d)
    for v in _host(d).reshape(-1, 4)[:50]:  # the definition: a value below 2^250
        assert oracle_mod.limbs_to_int(v) < (1 << 250)


def test_truncated_edge_values(gpu_ctx, oracle_mod):
    """outputs whose canonical value has bits above 2^250 set / is tiny: the mask and the Montgomery-form drop on special inputs
    (the all-zero message, p - 1 everywhere)"""
    import poseidon252_amd as P
    hb = P.HashBatch(P.Domain.Merkle4, 4, ctx=gpu_ctx)
    specials = np.stack([np.stack([oracle_mod.mont_from_int(v)] * 4) for v in (0, 1, oracle_mod.P - 1, 1 << 250, (1 << 254) + 12345)])
    m = np.concatenate([specials, oracle_mod.fill_random(0xb1, 4 * 27).reshape(27, 4, 4)])
    full = oracle_mod.hash_batch(hb.tag, m, 4, 1).reshape(-1, 4)
    got = hb.digest_truncated(m).reshape(-1, 4)
    for g, f in zip(got, full):
        canonical = oracle_mod.limbs_to_int(f) * pow(1 << 256, -1, oracle_mod.P) % oracle_mod.P
        assert oracle_mod.limbs_to_int(g) == canonical & ((1 << 250) - 1)


def test_digest_truncated_on_device_tensors_issues_one_kernel(gpu_ctx, tmp_path):
    """VERDICT r4 item 5, the kernel-trace assertion: HashBatch.digest_truncated on device tensors = ONE kernel of this library
    (the truncating build of the digest kernel), no k_to_canonical, for both the single-permutation and the sponge family"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        pytest.skip("rocprofv3 not on this box")
    script = tmp_path / "one_launch.py"
    script.write_text(
        "import sys; sys.path.insert(0, %r)\n"
        "import torch, poseidon252_amd as P\n"
        "from poseidon252_amd import synth\n"
        "ctx = P.Context(0)\n"
        "a = synth.splitmix_scalars(1, 4 << 15, torch.device('cuda:0'))\n"
        "b = synth.splitmix_scalars(2, 42 << 14, torch.device('cuda:0'))\n"
        "torch.cuda.synchronize()\n"
        "P.HashBatch(P.Domain.Merkle4, 4, ctx=ctx).digest_truncated(a)\n"
        "P.HashBatch(P.Domain.Other, 42, output_len=5, ctx=ctx).digest_truncated(b)\n"
        "torch.cuda.synchronize()\n" % ROOT)
    out = tmp_path / "trace"
    env = dict(os.environ, TMPDIR="/tmp")
    r = subprocess.run([rocprof, "--kernel-trace", "--output-format", "csv", "-d", str(out), "-o", "kt", "--", sys.executable, str(script)],
                       cwd="/tmp", env=env, capture_output=True, timeout=600)
    files = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    if r.returncode != 0 and not files:  # the PROFILER could not run here (no counters / permissions): nothing was learnt about the library
        pytest.skip("rocprofv3 could not trace on this box: " + r.stderr.decode()[-300:])
    assert r.returncode == 0 and files, r.stderr.decode()[-2000:]
    import csv
    names = [row["Kernel_Name"] for f in files for row in csv.DictReader(open(f))]
    ours = [n for n in names if "p252" in n]
    hashing = [n for n in ours if "k_synth" not in n and "splitmix" not in n]
    assert len(hashing) == 2, hashing
    assert sum("k_merkle4_trunc" in n for n in hashing) == 1 and sum("k_sponge_lines_trunc" in n for n in hashing) == 1, hashing
    assert not any("k_to_canonical" in n for n in names)


# ---------------------------------------------------------------------------------------------- HIP graphs
def test_device_entry_points_capture_into_a_hip_graph(gpu_ctx, oracle_mod):
    """the `_device` entry points only enqueue kernels on the stream they are given, so a caller can capture them into a hipGraph
    (here through torch.cuda.CUDAGraph, which captures torch's current stream — the stream the binding launches on) and replay the
    graph on new data: digests (both kernel families), a 42 -> 5 sponge, the truncated form, a tree build with caller-owned levels
    and a root-only one (its per-stream scratch exists after the warm-up call, so the capture allocates nothing).  Replays on fresh
    inputs equal the oracle."""
    import torch
    import poseidon252_amd as P
    tag4 = P.merkle4_tag()
    hb5 = P.HashBatch(P.Domain.Other, 42, output_len=5, ctx=gpu_ctx)
    n_small, n_big, n_sp, n_leaves = 3000, 20000, 9000, 4 ** 6
    d_small = torch.zeros((n_small, 4, 4), dtype=torch.int64, device="cuda:0")
    d_big = torch.zeros((n_big, 4, 4), dtype=torch.int64, device="cuda:0")
    d_sp = torch.zeros((n_sp, 42, 4), dtype=torch.int64, device="cuda:0")
    d_lv = torch.zeros((n_leaves, 4), dtype=torch.int64, device="cuda:0")
    o_small = torch.zeros((n_small, 4), dtype=torch.int64, device="cuda:0")
    o_big = torch.zeros((n_big, 4), dtype=torch.int64, device="cuda:0")
    o_trunc = torch.zeros((n_big, 4), dtype=torch.int64, device="cuda:0")
    o_sp = torch.zeros((n_sp, 5, 4), dtype=torch.int64, device="cuda:0")
    o_root = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    o_levels = torch.zeros((P.levels_len(n_leaves), 4), dtype=torch.int64, device="cuda:0")
    o_root2 = torch.zeros(4, dtype=torch.int64, device="cuda:0")

    def work():
        gpu_ctx.hash_batch_device(tag4, d_small, 4, 1, o_small, n_small)
        gpu_ctx.hash_batch_device(tag4, d_big, 4, 1, o_big, n_big)
        gpu_ctx.hash_batch_device(tag4, d_big, 4, 1, o_trunc, n_big, truncated=True)
        gpu_ctx.hash_batch_device(hb5.tag, d_sp, 42, 5, o_sp, n_sp)
        gpu_ctx.merkle4_tree_device(tag4, d_lv, n_leaves, o_root, o_levels)
        gpu_ctx.merkle4_tree_device(tag4, d_lv, n_leaves, o_root2, None)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (warm-up outside the capture, as torch asks)
        work()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        work()
    for rep in range(3):
        xs = oracle_mod.fill_random(0xd0 + rep, 4 * n_small).reshape(n_small, 4, 4)
        xb = oracle_mod.fill_random(0xd4 + rep, 4 * n_big).reshape(n_big, 4, 4)
        sp = oracle_mod.fill_random(0xd8 + rep, 42 * n_sp).reshape(n_sp, 42, 4)
        lv = oracle_mod.fill_random(0xdc + rep, n_leaves)
        for dst, src in ((d_small, xs), (d_big, xb), (d_sp, sp), (d_lv, lv)):
            dst.copy_(_dev(src).view(dst.shape))
        for o in (o_small, o_big, o_trunc, o_sp, o_root, o_levels, o_root2):
            o.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(o_small), oracle_mod.hash_batch(tag4, xs, 4, 1, threads=8).reshape(-1, 4)), rep
        eb = oracle_mod.hash_batch(tag4, xb, 4, 1, threads=8).reshape(-1, 4)
        assert np.array_equal(_host(o_big), eb), rep
        assert np.array_equal(_host(o_trunc), P.truncate250(eb)), rep
        idx = np.arange(0, n_sp, 37)
        assert np.array_equal(_host(o_sp).reshape(n_sp, 5, 4)[idx], oracle_mod.hash_batch(hb5.tag, np.ascontiguousarray(sp[idx]), 42, 5, threads=8)), rep
        e_root, e_levels, _ = oracle_mod.merkle4_tree(tag4, lv, want_levels=True)
        assert np.array_equal(_host(o_root), e_root) and np.array_equal(_host(o_levels), e_levels) and np.array_equal(_host(o_root2), e_root), rep


# ---------------------------------------------------------------------------------------------- Opening::verify in bulk
@pytest.mark.parametrize("arity,n_leaves,k", [(4, 4 ** 7, 20000), (4, 5001, 3000), (2, 2 ** 12, 5000), (2, 70001, 20000), (4, 1, 3)])
def test_verify_batch_flags_exactly_the_tampered_openings(gpu_ctx, oracle_mod, arity, n_leaves, k):
    """p252_merkle{4,2}_verify_batch_device — `Opening::verify` of the downstream poseidon-merkle consumer (AGENTS.md:62-66) for k openings
    against ONE root: build (all levels) -> extract -> tamper with a known subset (a sibling limb, the leaf, a position byte) -> verify,
    all on the device.  The flags are exactly the untouched openings; the oracle's re-hash of a sample agrees opening by opening; and
    the call on two streams of one context at once gives the same flags (the recomputed roots live in per-stream scratch)."""
    import torch
    import poseidon252_amd as P
    tag = P.merkle4_tag() if arity == 4 else P.compute_tag(P.Domain.Merkle2, [2], 1)
    lv = oracle_mod.fill_random(0xe0 + n_leaves + arity, n_leaves)
    root, levels = (gpu_ctx.merkle4_tree if arity == 4 else gpu_ctx.merkle2_tree)(tag, lv, want_levels=True)
    assert np.array_equal(root, (oracle_mod.merkle4_tree if arity == 4 else oracle_mod.merkle2_tree)(tag, lv)[0])
    d_lv = _dev(lv)
    d_levels = _dev(levels if levels.shape[0] else np.zeros((1, 4), dtype=np.uint64))
    d_root = _dev(root)
    rng = np.random.default_rng(n_leaves + arity)
    idx = rng.integers(0, n_leaves, size=k).astype(np.int32)
    out, sib, pos, depth = gpu_ctx.merkle4_openings_device(d_lv, n_leaves, d_levels, torch.from_numpy(idx).to("cuda:0"), k, check=True, arity=arity)
    ok = torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    gpu_ctx.merkle_verify_batch_device(tag, out, sib, pos, depth, d_root, ok, k, arity=arity)
    torch.cuda.synchronize()
    assert bool(ok.all()), "an untouched opening of the tree does not verify"
    # tamper: every 7th opening, by one of three means
    bad = np.arange(0, k, 7)
    h_out, h_sib, h_pos = out.cpu().numpy().copy(), sib.cpu().numpy().copy(), pos.cpu().numpy().copy()
    for j, i in enumerate(bad):
        kind = j % 3 if depth else 1
        if kind == 0:
            h_sib.reshape(k, -1)[i, (j * 5) % h_sib.reshape(k, -1).shape[1]] ^= 1  # one bit of one limb of one sibling
        elif kind == 1:
            h_out[i, 0] ^= 1 << 7  # the leaf
        else:
            h_pos[i, j % depth] ^= 1  # the path turns the other way at one level
    t_out, t_sib, t_pos = torch.from_numpy(h_out).to("cuda:0"), torch.from_numpy(h_sib).to("cuda:0"), torch.from_numpy(h_pos).to("cuda:0")
    ok2 = torch.ones(k, dtype=torch.uint8, device="cuda:0")
    ok3 = torch.ones(k, dtype=torch.uint8, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        gpu_ctx.merkle_verify_batch_device(tag, t_out, t_sib, t_pos, depth, d_root, ok2, k, arity=arity)
    with torch.cuda.stream(s2):  # (the untouched arrays on a second stream at the same time: all ones)
        gpu_ctx.merkle_verify_batch_device(tag, out, sib, pos, depth, d_root, ok3, k, arity=arity)
    torch.cuda.synchronize()
    expect = np.ones(k, dtype=np.uint8)
    expect[bad] = 0
    got = ok2.cpu().numpy()
    # (a flipped position bit whose sibling equals the path's node would still verify: cannot happen with random leaves)
    assert np.array_equal(got, expect), (np.nonzero(got != expect)[0][:10], depth)
    assert bool(ok3.all())
    if arity == 4 and depth:  # the oracle re-hashes a sample of the tampered openings: equal to the root exactly where the flag is set
        sample = np.arange(0, k, max(1, k // 60))
        o_roots = oracle_mod.merkle4_path_batch(tag, np.ascontiguousarray(h_out.view(np.uint64)[sample]),
                                                np.ascontiguousarray(h_sib.view(np.uint64).reshape(k, depth, 3, 4)[sample]), np.ascontiguousarray(h_pos[sample]))
        assert np.array_equal((o_roots == root.reshape(1, 4)).all(axis=1).astype(np.uint8), got[sample])
