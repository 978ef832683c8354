"""Parity tests proper (-m gpu): the HIP path, called through the C ABI, against the KAT-pinned oracle
on the same seeded inputs and against the committed golden fixtures — bit-exact (limb equality).
Shapes follow the reference's tests: tests/hash.rs (3/5/15 inputs; 3->3, 5->2, 4->7 outputs),
src/hades.rs KAT, README doctest properties, BASELINE.json configs at full size via
size-independent properties."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "vectors.json")))
KAT = json.load(open(os.path.join(HERE, "golden", "hades_kat.json")))


def limbs(hexlist):
    return np.array([int(h, 16) for h in hexlist], dtype=np.uint64)


def test_native_extension_loaded(gpu_ctx):
    """the GPU tests run on the in-tree HIP library, not on anything else"""
    from poseidon252_amd import _lib
    maps = open("/proc/self/maps").read()
    assert os.path.basename(_lib.LIB_PATH) in maps


# ---------------------------------------------------------------- permutation
def test_permute_matches_oracle(gpu_ctx, oracle_mod):
    st = oracle_mod.fill_random(1, 5 * 3001).reshape(3001, 5, 4)  # ragged: not a multiple of the block size
    assert np.array_equal(gpu_ctx.permute_batch(st), oracle_mod.permute_batch(st))


def test_permute_golden_and_special(gpu_ctx, oracle_mod):
    g = GOLD["permute"]
    st = oracle_mod.fill_random(g["seed"], 5 * g["n"]).reshape(g["n"], 5, 4)
    assert np.array_equal(gpu_ctx.permute_batch(st).reshape(-1), limbs(g["out"]))
    special = np.zeros((3, 5, 4), dtype=np.uint64)
    special[1] = np.stack([oracle_mod.mont_from_int(17)] * 5)  # hades_det input, scalar.rs:87-92
    special[2] = np.stack([oracle_mod.mont_from_int(i) for i in range(5)])
    out = gpu_ctx.permute_batch(special)
    assert np.array_equal(out.reshape(-1), limbs(GOLD["permute_special"]["out"]))
    # SURVEY A.2 model-derived canonical values
    for row, key in zip(out, ["0,0,0,0,0", "17,17,17,17,17", "0,1,2,3,4"]):
        assert ["%064x" % oracle_mod.int_from_mont(v) for v in row] == KAT["model_derived_permutations_be_hex"][key]


def test_permute_edge_values(gpu_ctx, oracle_mod):
    P = oracle_mod.P
    vals = [0, 1, P - 1, P - 2, (P - 1) // 2, 1 << 254, (1 << 255) % P, pow(2, -256, P)]
    e = np.stack([oracle_mod.mont_from_int(v) for v in vals] + [oracle_mod.int_to_limbs(P - 1), oracle_mod.int_to_limbs(1)])
    rng = np.random.default_rng(5)
    st = e[rng.integers(0, len(e), size=(500, 5))]
    assert np.array_equal(gpu_ctx.permute_batch(st), oracle_mod.permute_batch(st))


def test_empty_and_single(gpu_ctx, oracle_mod):
    assert gpu_ctx.permute_batch(np.zeros((0, 5, 4), dtype=np.uint64)).shape == (0, 5, 4)
    tag = oracle_mod.tag(0, [4], 1)
    assert gpu_ctx.hash_batch(tag, np.zeros((0, 4, 4), dtype=np.uint64), 4, 1).shape == (0, 1, 4)
    one = oracle_mod.fill_random(9, 4).reshape(1, 4, 4)
    assert np.array_equal(gpu_ctx.hash_batch(tag, one, 4, 1), oracle_mod.hash_batch(tag, one, 4, 1))


# ---------------------------------------------------------------- the reference KAT, on the GPU
@pytest.mark.parametrize("n", [3, 4, 5, 6, 8, 10])
def test_reference_kat_on_gpu(gpu_ctx, oracle_mod, n):
    """src/hades.rs:94-162 through the HIP sponge: tag = 0, message = inputs[..n] ++ [one]"""
    ins = [int.from_bytes(bytes.fromhex(h), "little") for h in KAT["inputs_le_hex"]][:n] + [1]
    msg = np.stack([oracle_mod.mont_from_int(v) for v in ins])[None]
    out = gpu_ctx.hash_batch(np.zeros(4, dtype=np.uint64), msg, n + 1, 1)[0, 0]
    assert "%064x" % oracle_mod.int_from_mont(out) == KAT["expected_be_hex"][str(n)]


# ---------------------------------------------------------------- sponge
@pytest.mark.parametrize("in_len,out_len", [(4, 1), (2, 1), (3, 1), (5, 1), (15, 1), (3, 3), (5, 2), (4, 7), (42, 5), (42, 1),
                                            (1, 1), (8, 4), (9, 9), (16, 8), (1, 13)])
def test_hash_batch_matches_oracle(gpu_ctx, oracle_mod, in_len, out_len):
    tag = oracle_mod.fill_random(1000 + in_len, 1)[0]  # arbitrary capacity element: the tag is an input
    n = 777
    m = oracle_mod.fill_random(100 * in_len + out_len, n * in_len).reshape(n, in_len, 4)
    assert np.array_equal(gpu_ctx.hash_batch(tag, m, in_len, out_len), oracle_mod.hash_batch(tag, m, in_len, out_len))


def test_hash_golden(gpu_ctx, oracle_mod):
    for c in GOLD["hash"]:
        tag = limbs(c["tag_UNPINNED"])
        m = oracle_mod.fill_random(c["seed"], c["n"] * c["in_len"]).reshape(c["n"], c["in_len"], 4)
        assert np.array_equal(gpu_ctx.hash_batch(tag, m, c["in_len"], c["out_len"]).reshape(-1), limbs(c["out"])), c


def test_invalid_patterns_return_error_codes(gpu_ctx):
    import poseidon252_amd as P
    z = np.zeros((4, 4), dtype=np.uint64)
    with pytest.raises(P.InvalidIOPattern):
        gpu_ctx.hash_batch(z[0], z[None], 4, 0)
    with pytest.raises(P.InvalidIOPattern):
        gpu_ctx.hash_batch(z[0], z[:0], 0, 1)
    with pytest.raises(ValueError):
        gpu_ctx.merkle4_tree(z[0], z[:0])


# ---------------------------------------------------------------- Hash / HashBatch mirror (reads like tests/hash.rs + README)
def test_misaligned_device_pointers_are_refused(gpu_ctx, oracle_mod):
    """the kernels use 16-byte accesses: a device pointer 8 bytes off (a Rust BlsScalar is only 8-byte aligned, but a
    device array of them never starts there) must come back as an error, not as a GPU fault"""
    import torch
    tag = oracle_mod.tag(0, [4], 1)
    buf = torch.zeros(4 * 64 * 4 + 1, dtype=torch.int64, device="cuda")
    out = torch.zeros(64 * 4 + 1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        gpu_ctx.hash_batch_device(tag, buf[1:], 4, 1, out, 64)
    with pytest.raises(ValueError):
        gpu_ctx.hash_batch_device(tag, buf, 4, 1, out[1:], 64)
    with pytest.raises(ValueError):
        gpu_ctx.permute_batch_device(buf[1:], buf, 32)
    # the binding's own checks: a strided view, a view too short for the call, a tensor on another device.  Every view starts
    # inside a buffer that holds what the call would touch, so a missing check would stay inside the allocation.
    wide = torch.zeros((2 * 64 * 4, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="d_in is not contiguous"):
        gpu_ctx.hash_batch_device(tag, wide[::2], 4, 1, out, 64)
    with pytest.raises(ValueError, match="d_out is not contiguous"):
        gpu_ctx.hash_batch_device(tag, buf, 4, 1, wide[:128, :2], 64)
    with pytest.raises(ValueError, match="d_in holds 8064 bytes, the call touches 8192"):
        gpu_ctx.hash_batch_device(tag, buf[:4 * 63 * 4], 4, 1, out, 64)
    with pytest.raises(ValueError, match="d_out holds 2016 bytes"):
        gpu_ctx.hash_batch_device(tag, buf, 4, 1, out[:63 * 4], 64)
    with pytest.raises(ValueError, match="d_root holds 16 bytes"):
        gpu_ctx.merkle4_tree_device(tag, buf, 64, out[:2])
    if torch.cuda.device_count() > 1:
        other = torch.zeros_like(buf, device="cuda:1")
        with pytest.raises(ValueError, match="d_in is on cuda:1, the context is on cuda:0"):
            gpu_ctx.hash_batch_device(tag, other, 4, 1, out, 64)
    gpu_ctx.hash_batch_device(tag, buf[4:], 4, 1, out[4:], 63)  # whole-scalar offsets are fine
    torch.cuda.synchronize()
    exp = oracle_mod.hash_batch(tag, np.zeros((63, 4, 4), dtype=np.uint64), 4, 1).reshape(-1)
    assert np.array_equal(out[4:4 + 63 * 4].cpu().numpy().view(np.uint64), exp)  # and the context still works


def test_hash_api_like_reference_tests(gpu_ctx, oracle_mod):
    import poseidon252_amd as P
    # tests/hash.rs shapes: 3 / 5 / 15 inputs, default output_len
    for n_in in (3, 5, 15):
        inp = oracle_mod.fill_random(0xbeef + n_in, n_in)
        d = P.Hash.digest(P.Domain.Other, inp, ctx=gpu_ctx)
        assert d.shape == (1, 4)
        assert np.array_equal(d, oracle_mod.hash_batch(oracle_mod.tag(3, [n_in], 1), inp[None], n_in, 1)[0])
    # multi-output (3,3), (5,2), (4,7)  — tests/hash.rs:277-292
    for n_in, n_out in [(3, 3), (5, 2), (4, 7)]:
        inp = oracle_mod.fill_random(0xbeef + 16 * n_in + n_out, n_in)
        h = P.Hash.new(P.Domain.Other, ctx=gpu_ctx)
        h.output_len(n_out)
        h.update(inp)
        out = h.finalize()
        assert out.shape == (n_out, 4)
        assert np.array_equal(out, oracle_mod.hash_batch(oracle_mod.tag(3, [n_in], n_out), inp[None], n_in, n_out)[0])
    # README.md:31-51: chunked update == one-shot digest; Merkle4 digest != Other digest on the same 4 inputs
    inp = oracle_mod.fill_random(0xc10d, 42)
    h = P.Hash.new(P.Domain.Other, ctx=gpu_ctx)
    h.update(inp[:3])
    h.update(inp[3:])
    assert np.array_equal(h.finalize(), P.Hash.digest(P.Domain.Other, inp, ctx=gpu_ctx))
    four = inp[:4]
    assert not np.array_equal(P.Hash.digest(P.Domain.Merkle4, four, ctx=gpu_ctx), P.Hash.digest(P.Domain.Other, four, ctx=gpu_ctx))
    # Merkle4 digest == perm([tag, x0..x3])[1]  
    tag = oracle_mod.tag(0, [4], 1)
    st = np.concatenate([tag[None], four])[None]
    assert np.array_equal(P.Hash.digest(P.Domain.Merkle4, four, ctx=gpu_ctx)[0], gpu_ctx.permute_batch(st)[0, 1])
    # truncated variant (hash.rs:164-183)
    t = P.Hash.digest_truncated(P.Domain.Other, inp[:5], ctx=gpu_ctx)
    assert np.array_equal(t[0], oracle_mod.truncate250(P.Hash.digest(P.Domain.Other, inp[:5], ctx=gpu_ctx)[0]))
    # panics of the reference -> exceptions
    with pytest.raises(P.IOPatternViolation):
        P.Hash.digest(P.Domain.Merkle4, inp[:3], ctx=gpu_ctx)


def test_hashbatch_host_and_device_buffers(gpu_ctx, oracle_mod):
    import torch
    import poseidon252_amd as P
    hb = P.HashBatch(P.Domain.Merkle4, 4, ctx=gpu_ctx)
    x = oracle_mod.fill_random(42, 4 * 5000).reshape(5000, 4, 4)
    exp = oracle_mod.hash_batch(hb.tag, x, 4, 1)
    assert np.array_equal(hb.digest(x), exp)
    d = torch.from_numpy(x.view(np.int64)).cuda()
    out = hb.digest(d)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), exp)
    # inputs are borrowed, never mutated (hash.rs:94,118-120)
    assert np.array_equal(d.cpu().numpy().view(np.uint64), x)
    hb5 = P.HashBatch(P.Domain.Other, 42, output_len=5, ctx=gpu_ctx)
    m = oracle_mod.fill_random(43, 42 * 300).reshape(300, 42, 4)
    assert np.array_equal(hb5.digest(m), oracle_mod.hash_batch(hb5.tag, m, 42, 5))


# ---------------------------------------------------------------- Merkle tree
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 21, 64, 255, 256, 257, 1000, 4096, 4097])
def test_tree_matches_oracle(gpu_ctx, oracle_mod, n):
    tag = oracle_mod.tag(0, [4], 1)
    lv = oracle_mod.fill_random(7 + n, n)
    root, levels = gpu_ctx.merkle4_tree(tag, lv, want_levels=True)
    oroot, olevels, _ = oracle_mod.merkle4_tree(tag, lv, want_levels=True)
    assert np.array_equal(root, oroot) and np.array_equal(levels, olevels)
    assert np.array_equal(gpu_ctx.merkle4_tree(tag, lv), oroot)  # scratch (ping-pong) path


def test_tree_golden(gpu_ctx, oracle_mod):
    tag = oracle_mod.tag(0, [4], 1)
    for t in GOLD["merkle4_tree"]:
        root = gpu_ctx.merkle4_tree(tag, oracle_mod.fill_random(t["seed"], t["n_leaves"]))
        assert np.array_equal(root, limbs(t["root"]))


def test_tree_device_api_and_subtree_composition(gpu_ctx, oracle_mod):
    """config-5 structure at small scale: 8 complete subtrees -> 8 roots -> top of tree"""
    import torch
    import poseidon252_amd as P
    tag = oracle_mod.tag(0, [4], 1)
    lv = oracle_mod.fill_random(0x77, 8 * 256)
    d = torch.from_numpy(lv.view(np.int64)).cuda()
    full = P.merkle4_tree(d, tag=tag, ctx=gpu_ctx)
    roots = torch.stack([P.merkle4_tree(d[i * 256:(i + 1) * 256].contiguous(), tag=tag, ctx=gpu_ctx) for i in range(8)])
    top = P.merkle4_tree(roots.contiguous(), tag=tag, ctx=gpu_ctx)
    torch.cuda.synchronize()
    assert torch.equal(full, top)
    assert np.array_equal(full.cpu().numpy().view(np.uint64), oracle_mod.merkle4_tree(tag, lv)[0])


# ---------------------------------------------------------------- BASELINE.json full sizes via size-independent properties
def test_config2_full_size_properties(gpu_ctx, oracle_mod):
    """2^20 Merkle4 digests: (a) a digest does not depend on its position or on the batch it is in
    (shard consistency), (b) an oracle spot check over a strided sample, (c) determinism."""
    import torch
    n = 1 << 20
    tag = oracle_mod.tag(0, [4], 1)
    h = oracle_mod.fill_random(0xc10d, 4 * n).reshape(n, 4, 4)
    d_in = torch.from_numpy(h.view(np.int64)).cuda()
    d_out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    gpu_ctx.hash_batch_device(tag, d_in, 4, 1, d_out, n)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    idx = np.arange(0, n, 4099)
    assert np.array_equal(out[idx], oracle_mod.hash_batch(tag, h[idx], 4, 1).reshape(-1, 4))
    # shard consistency: hashing a permuted / shifted sub-batch gives the same digests
    lo, hi = 123457, 123457 + 70001
    assert np.array_equal(gpu_ctx.hash_batch(tag, h[lo:hi], 4, 1).reshape(-1, 4), out[lo:hi])
    d_out2 = torch.empty_like(d_out)
    gpu_ctx.hash_batch_device(tag, d_in, 4, 1, d_out2, n)
    torch.cuda.synchronize()
    assert torch.equal(d_out, d_out2)
    assert all(oracle_mod.lib().p252o_is_reduced(out[i].ctypes.data_as(oracle_mod._u64p)) for i in idx)


def test_config3_tree_properties(gpu_ctx, oracle_mod):
    """2^20-leaf tree (config 3's structure, 1/16 of its size to keep the suite short): every level is
    the digest of the level below — verified with the oracle on a random sample of nodes per level —
    and the root equals the tree over the level-k nodes (subtree composition)."""
    import torch
    n = 1 << 20
    tag = oracle_mod.tag(0, [4], 1)
    lv = oracle_mod.fill_random(0x3333, n)
    d = torch.from_numpy(lv.view(np.int64)).cuda()
    from poseidon252_amd import levels_len
    d_levels = torch.empty((levels_len(n), 4), dtype=torch.int64, device="cuda")
    d_root = torch.empty(4, dtype=torch.int64, device="cuda")
    gpu_ctx.merkle4_tree_device(tag, d, n, d_root, d_levels)
    torch.cuda.synchronize()
    levels = d_levels.cpu().numpy().view(np.uint64)
    below, off, cnt = lv, 0, n // 4
    rng = np.random.default_rng(1)
    while cnt >= 1:
        cur = levels[off:off + cnt]
        idx = rng.integers(0, cnt, size=min(cnt, 64))
        exp = oracle_mod.hash_batch(tag, below.reshape(-1, 4, 4)[idx], 4, 1).reshape(-1, 4)
        assert np.array_equal(cur[idx], exp)
        below, off, cnt = cur, off + cnt, cnt // 4
    assert np.array_equal(d_root.cpu().numpy().view(np.uint64), levels[-1])
    d_root2 = torch.empty(4, dtype=torch.int64, device="cuda")
    gpu_ctx.merkle4_tree_device(tag, d, n, d_root2, None)
    torch.cuda.synchronize()
    assert torch.equal(d_root, d_root2)


def test_config4_sponge_full_width_sample(gpu_ctx, oracle_mod):
    """Domain::Other, 42 scalars -> 5 outputs (config 4) on 2^15 messages, oracle on a strided sample"""
    import poseidon252_amd as P
    n = 1 << 15
    hb = P.HashBatch(P.Domain.Other, 42, output_len=5, ctx=gpu_ctx)
    m = oracle_mod.fill_random(0x4444, 42 * n).reshape(n, 42, 4)
    out = hb.digest(m)
    idx = np.arange(0, n, 257)
    assert np.array_equal(out[idx], oracle_mod.hash_batch(hb.tag, m[idx], 42, 5))
    # output_len=1 is a prefix of output_len=5 only if the tags agree — they do not (io-pattern is in the tag)
    hb1 = P.HashBatch(P.Domain.Other, 42, output_len=1, ctx=gpu_ctx)
    assert not np.array_equal(hb1.digest(m[:4])[:, 0], out[:4, 0])
    assert np.array_equal(gpu_ctx.hash_batch(hb.tag, m[:4], 42, 1)[:, 0], out[:4, 0])  # same tag: squeeze order is a prefix


def test_tables_roundtrip_and_broadcast_equivalence(gpu_ctx):
    t = gpu_ctx.tables_export()
    assert t.dtype == np.int32 and np.abs(t.astype(np.int64)).max() <= 1 << 28
    gpu_ctx.tables_import(t)
    assert np.array_equal(gpu_ctx.tables_export(), t)
    # a table that is not the one the library derives from its own arc.bin / mds.bin is refused: it would
    # bypass the Cauchy-structure and column-bound checks of p252_create and give silently wrong digests
    bad = t.copy()
    bad[100] ^= 1
    with pytest.raises(ValueError):
        gpu_ctx.tables_import(bad)
    assert np.array_equal(gpu_ctx.tables_export(), t)  # the device table is untouched


def test_adversarial_noncanonical_limbs_on_gpu(gpu_ctx, oracle_mod):
    """same adversarial patterns as tests/test_host_arith.py, on the GPU, against the big-int model"""
    import random
    import pymodel
    P = pymodel.P
    C, M = pymodel.load_constants()
    Rinv = pow(1 << 256, -1, P)
    pats = [(1 << 256) - 1, (1 << 255) + 12345, P, P + 1, 2 * P - 1, int("55" * 32, 16), int("aa" * 32, 16),
            sum(((1 << 29) - 1) << (29 * i) for i in range(8)) | (((1 << 24) - 1) << 232)]
    rng = random.Random(4)
    states = [[rng.choice(pats) for _ in range(5)] for _ in range(12)] + [[pats[0]] * 5]
    st = np.array([[oracle_mod.int_to_limbs(v) for v in s] for s in states], dtype=np.uint64)
    out = gpu_ctx.permute_batch(st)
    for s, o in zip(states, out):
        assert [oracle_mod.int_from_mont(x) for x in o] == pymodel.perm_reference([v * Rinv % P for v in s], C, M)
    # sponge with a saturating tag and message: 9 inputs, 6 outputs
    msg = st[:9, 0]
    got = gpu_ctx.hash_batch(st[0, 1], msg[None], 9, 6)[0]
    exp = pymodel.sponge(states[0][1] * Rinv % P, [s[0] * Rinv % P for s in states[:9]], 6, perm=lambda x: pymodel.perm_reference(x, C, M))
    assert [oracle_mod.int_from_mont(x) for x in got] == exp


def test_tree_with_padded_narrow_levels_is_bit_identical(gpu_ctx, oracle_mod):
    """the narrow levels of a large tree are computed redundantly on every SIMD (k_merkle4_pad: lane i hashes node
    i mod n) to hold the chip's power state; forced on for SMALL trees here (P252_TREE_PAD_LANES is read once per
    process, hence the subprocess): roots and all levels equal the oracle's, arity 4 and 2"""
    import subprocess, sys
    code = r'''
import numpy as np, oracle, poseidon252_amd as P
ctx = P.Context(0)
tag = P.merkle4_tag()
for n in (1, 2, 5, 64, 1000, 4096, 70000):
    lv = oracle.fill_random(900 + n, n)
    root, levels = P.merkle4_tree(lv, tag=tag, ctx=ctx, want_levels=True)
    o_root, o_levels, _ = oracle.merkle4_tree(tag, lv, want_levels=True)
    assert np.array_equal(root, o_root) and np.array_equal(levels, o_levels), n
    tag2 = oracle.tag(1, [2], 1)
    root2, levels2 = ctx.merkle2_tree(tag2, lv[:min(n, 3000)], want_levels=True)
    o2 = oracle.merkle2_tree(tag2, lv[:min(n, 3000)], want_levels=True)
    assert np.array_equal(root2, o2[0]) and np.array_equal(levels2, o2[1]), n
print("PAD OK")
'''
    import os
    # 65538 / 16386: NOT multiples of the lane groups' 8 / 4 — the launcher rounds up to whole groups (a partial
    # last group exchanged with lanes that had left the kernel and stored a garbage digest beside the right one)
    for lanes in ("16384", "65538", "16386", "9"):
        env = dict(os.environ, P252_TREE_PAD_LANES=lanes)
        out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), env=env, capture_output=True, timeout=600)
        assert out.returncode == 0 and b"PAD OK" in out.stdout, lanes + ": " + out.stdout.decode() + out.stderr.decode()


def test_library_loaded_before_torch_leaves_torch_usable():
    """PyTorch-ROCm bundles its own HIP runtime under the SONAME the library links to; whichever copy is loaded first
    serves the whole process.  Loading this library first must not leave a later `import torch` without devices
    (poseidon252_amd/_lib.py loads torch's copy first when torch is installed)."""
    import subprocess, sys
    code = r'''
import sys
import numpy as np
import oracle, poseidon252_amd as P
assert "torch" not in sys.modules
ctx = P.Context(0)
x = oracle.fill_random(1, 4 * 100).reshape(100, 4, 4)
tag = P.merkle4_tag()
a = ctx.hash_batch(tag, x, 4, 1)
import torch
assert torch.cuda.is_available() and torch.cuda.device_count() >= 1
d = torch.from_numpy(x.view(np.int64)).cuda()
b = P.HashBatch(P.Domain.Merkle4, 4, ctx=ctx).digest(d)
torch.cuda.synchronize()
assert np.array_equal(b.cpu().numpy().view(np.uint64).reshape(-1), a.reshape(-1))
print("ORDER OK")
'''
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, timeout=600)
    assert out.returncode == 0 and b"ORDER OK" in out.stdout, out.stdout.decode() + out.stderr.decode()[-3000:]
