"""Edge values for every hashing entry point: ONE pattern set (PATTERNS), ONE seeded generator (edge_scalars), and the matrix of
rows (ROWS) that tests/test_edge_values_gpu.py checks against the oracle and tests/helpers/edge_matrix_driver.py runs under the
kernel tracer.  A plain helper module, imported as pymodel and primcases are.

An edge value is a 256-bit limb pattern V — what lies in memory where a BlsScalar in Montgomery form is expected: 0, 1, p - 1,
patterns at and above p up to 2^256 - 1, saturated 29- and 32-bit digits.  The rule the rows check (include/poseidon252_hip.h,
"Scalars"): a value that is hashed, absorbed, added or subtracted counts as V mod p; a value that is COMPARED (the stored MAC of a
cipher, the expected root of a verification) is compared as the 32 bytes it is; every output is reduced.  So every row hands the
GPU `raw`, the oracle `reduced` = raw mod p, and asks for the same bytes.

A row is data: its name, the callable that makes the GPU calls (and, when asked, the oracle's and the comparison), and the names
of the kernels its sizes select under the default environment (launch_merkle4, coop8 and the launchers in csrc/*.hip decide)."""
import os
import re
import time

import numpy as np

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P = oracle.P
R = oracle.R
M256 = (1 << 256) - 1
M64 = (1 << 64) - 1
UNREDUCED_TAG = (1 << 256) - 5  # the second tag of every row that takes one: a word above 2p
ORACLE_THREADS = 16


# ---------------------------------------------------------------------------------------------- the patterns
def _patterns():
    def mont(v):
        return (v % P) * R % P
    d29 = (1 << 29) - 1
    saturated = sum(d29 << (29 * i) for i in range(8)) | (((1 << 24) - 1) << 232)  # every 29-bit digit of the nine full
    fives, tens = int("55" * 32, 16), int("aa" * 32, 16)
    pats = []
    # the lists of test_gpu_coop.py, test_gpu_parity.py and test_host_arith.py (limb patterns, and Montgomery forms of values)
    pats += [M256, (1 << 255) + 12345, P, P + 1, 2 * P - 1, 2 * P + 7, (4 * P + 3) & M256, fives, tens, 0, 1, P - 1, saturated,
             (1 << 256) - (1 << 200), P - (1 << 200), (1 << 254) + 12345]
    pats += [mont(v) for v in (0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, (1 << 255) % P, 1 << 254, (1 << 29) - 1, 1 << 29,
                               (1 << 232) - 1, 1 << 232, pow(2, -256, P), pow(2, 256, P), pow(3, 200, P), 17)]
    # around 0, p, 2p and 2^256
    pats += [0, 1, 2, P - 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, M256, (1 << 256) - (1 << 32), 1 << 255, 1 << 254]
    pats += [(P - 1) // 2, (M256 // P) * P]  # (the largest multiple of p below 2^256)
    pats += [R % P, R * R % P, (P - R) % P]  # the Montgomery images of 1, R and -1
    for i in range(9):  # digit boundaries of the kernels' 29-bit representation
        pats += [(1 << (29 * i)) & M256, ((1 << (29 * i)) - 1) & M256, (d29 << (29 * i)) & M256]
    for i in range(1, 8):  # and of the 32-bit words the scalars are loaded as
        pats += [1 << (32 * i), (1 << (32 * i)) - 1]
    pats += [fives, tens, saturated]
    seen, out = set(), []
    for v in pats:
        assert 0 <= v <= M256
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


PATTERNS = _patterns()
_PAT_RAW = np.array([[(v >> (64 * i)) & M64 for i in range(4)] for v in PATTERNS], dtype=np.uint64)
_PAT_RED = np.array([[((v % P) >> (64 * i)) & M64 for i in range(4)] for v in PATTERNS], dtype=np.uint64)
_BIG = np.array([k for k, v in enumerate(PATTERNS) if v >= P], dtype=np.int64)  # the patterns whose limbs are >= p


def limbs(v):
    return np.array([(v >> (64 * i)) & M64 for i in range(4)], dtype=np.uint64)


def _shape(shape):
    return (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)


def edge_draw(seed, shape):
    """(raw, reduced, index): as edge_scalars, and index (shape) = the entry of PATTERNS a scalar holds, -1 for a random scalar"""
    shape = _shape(shape)
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    rnd = oracle.fill_random(seed, n)
    m = (n + 1) // 2  # about half of the scalars are patterns
    n_big = (m + 2) // 3  # at least a third of those from the patterns >= p; the others walk through ALL patterns in turn
    ids = np.concatenate([np.resize(rng.permutation(_BIG), n_big), np.resize(rng.permutation(len(PATTERNS)), m - n_big)])
    ids = ids[rng.permutation(m)]
    slots = rng.permutation(n)[:m]  # a seeded permutation, not blocks: neighbouring lanes differ
    index = np.full(n, -1, dtype=np.int64)
    index[slots] = ids
    raw, red = rnd.copy(), rnd.copy()
    raw[slots] = _PAT_RAW[ids]
    red[slots] = _PAT_RED[ids]
    return raw.reshape(shape + (4,)), red.reshape(shape + (4,)), index.reshape(shape)


def edge_scalars(seed, shape):
    """(raw, reduced): two uint64 limb arrays of shape + (4,).  raw mixes PATTERNS with oracle.fill_random scalars — about half
    are patterns, at least a third of those >= p, laid out by a seeded permutation; reduced = raw mod p, limb for limb."""
    raw, red, _ = edge_draw(seed, shape)
    return raw, red


# ---------------------------------------------------------------------------------------------- 256-bit numpy arithmetic
def _add_const(a, c):
    """a + c over (..., 4) uint64 limbs -> (the sum mod 2^256, the carry out as bool)"""
    a = np.asarray(a, dtype=np.uint64)
    out = np.empty_like(a)
    carry = np.zeros(a.shape[:-1], dtype=np.uint64)
    for i in range(4):
        ci = np.uint64((c >> (64 * i)) & M64)
        s = a[..., i] + ci
        c1 = s < ci
        s2 = s + carry
        c2 = s2 < carry
        out[..., i] = s2
        carry = (c1 | c2).astype(np.uint64)
    return out, carry.astype(bool)


def is_reduced(a):
    """elementwise V < p over (..., 4) uint64 limbs (oracle p252o_is_reduced, vectorised; test_edgecases_cpu.py compares the two)"""
    a = np.asarray(a, dtype=np.uint64)
    lt = np.zeros(a.shape[:-1], dtype=bool)
    eq = np.ones(a.shape[:-1], dtype=bool)
    for i in (3, 2, 1, 0):
        pi = np.uint64((P >> (64 * i)) & M64)
        lt |= eq & (a[..., i] < pi)
        eq &= a[..., i] == pi
    return lt


def reduce_mod_p(a):
    """V mod p over (..., 4) uint64 limbs (V < 2^256 < 3p: two conditional subtractions)"""
    a = np.array(a, dtype=np.uint64)
    for _ in range(2):
        dif, _ = _add_const(a, (1 << 256) - P)  # V - p mod 2^256
        a = np.where(is_reduced(a)[..., None], a, dif)
    return a


def unreduced_twin(x):
    """for canonical x: the other limb pattern of the same residue — x + 2p where that fits below 2^256, else x + p"""
    x = np.asarray(x, dtype=np.uint64)
    assert is_reduced(x).all()
    two, over = _add_const(x, 2 * P)
    one, _ = _add_const(x, P)
    return np.where(over[..., None], one, two)


def plus_p(x):
    """canonical x -> the limbs of x + p (another 32 bytes of the same residue: what a comparison must NOT accept)"""
    x = np.asarray(x, dtype=np.uint64)
    assert is_reduced(x).all()
    return _add_const(x, P)[0]


# ---------------------------------------------------------------------------------------------- the run of a row
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def _empty(*shape):
    import torch
    return torch.empty(shape, dtype=torch.int64, device="cuda:0")


class Run:
    """what a row's callable gets: the context, and whether to compare (check=False: the GPU side alone, for the kernel tracer)"""

    def __init__(self, ctx, check=True):
        self.ctx, self.check = ctx, check

    def sync(self):
        import torch
        torch.cuda.synchronize()

    def tags(self, real):
        """the two tags of a row as (what the GPU gets, what the oracle gets): the domain's own, and an unreduced word"""
        real = np.ascontiguousarray(real, dtype=np.uint64).reshape(4)
        return [(real, real), (limbs(UNREDUCED_TAG), limbs(UNREDUCED_TAG % P))]

    def same(self, got, want, what=""):
        """exact equality with the oracle's scalars, every output canonical"""
        got = _host(got) if not isinstance(got, np.ndarray) else got
        want = np.asarray(want, dtype=np.uint64)
        got = got.reshape(want.shape)
        assert is_reduced(got).all(), "%s: an output scalar is not reduced" % what
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(-1, 4).any(axis=1))[0]
            raise AssertionError("%s: %d of %d scalars differ from the oracle, first at %d" % (what, bad.size, got.size // 4, int(bad[0])))


def _mtag(arity):
    return oracle.tag(0, [4], 1) if arity == 4 else oracle.tag(1, [2], 1)


def _pmap(fn, items):
    """fn over items on ORACLE_THREADS host threads (the oracle's C calls release the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    oracle.permute_batch(np.zeros((1, 5, 4), dtype=np.uint64))  # (its constants: loaded once, before the threads start)
    with ThreadPoolExecutor(ORACLE_THREADS) as pool:
        return list(pool.map(fn, items))


def oracle_tree(tag_red, red, arity):
    """(root, levels bottom-up) as oracle.merkle{4,2}_tree(..., want_levels=True) gives them, level by level through the threaded
    oracle.hash_batch (test_edgecases_cpu.py compares the two): missing children are the zero scalar, one leaf is its own root"""
    cur = np.asarray(red, dtype=np.uint64).reshape(-1, 4)
    levels = []
    while cur.shape[0] > 1:
        n = (cur.shape[0] + arity - 1) // arity
        ch = np.zeros((n * arity, 4), dtype=np.uint64)
        ch[:cur.shape[0]] = cur
        cur = oracle.hash_batch(tag_red, ch.reshape(n, arity, 4), arity, 1, threads=ORACLE_THREADS).reshape(n, 4)
        levels.append(cur)
    return cur[0].copy(), (np.concatenate(levels) if levels else np.zeros((0, 4), dtype=np.uint64))


def _otree(arity):
    return oracle.merkle4_tree if arity == 4 else oracle.merkle2_tree


def _truncated(x):
    x = np.asarray(x, dtype=np.uint64)
    return np.stack([oracle.truncate250(v) for v in x.reshape(-1, 4)]).reshape(x.shape)


def _tree_device(ctx, arity, tag, d_leaves, n, d_root, d_levels):
    from testsupport.device import tree_device  # p252_merkle{4,2}_tree_device on the current stream
    tree_device(ctx, arity, tag, d_leaves, n, d_root, d_levels)


def _levels_len(n, arity):
    from poseidon252_amd import levels_len
    return levels_len(n, arity)


# ---------------------------------------------------------------------------------------------- single-permutation digests
def digests(run, n, truncated=False, seed=0x1000):
    """hash_batch(tag, x, 4 | 2, 1) on device tensors, both arities, both tags"""
    raw, red, _ = edge_draw(seed + n, (n, 4))
    d = _dev(raw)
    for arity in (4, 2):
        x = d[:, :arity].contiguous()
        x_red = np.ascontiguousarray(red[:, :arity])
        for tag, tag_red in run.tags(_mtag(arity)):
            out = _empty(n, 4)
            run.ctx.hash_batch_device(tag, x, arity, 1, out, n, truncated=truncated)
            run.sync()
            if run.check:
                want = oracle.hash_batch(tag_red, x_red, arity, 1, threads=ORACLE_THREADS).reshape(n, 4)
                run.same(out, _truncated(want) if truncated else want, "digest n=%d arity=%d" % (n, arity))


def trees(run, arity, n, seed=0x2000):
    """p252_merkle{4,2}_tree_device with caller-owned levels and root-only, both tags"""
    raw, red, _ = edge_draw(seed + arity, (n,))
    d = _dev(raw)
    for tag, tag_red in run.tags(_mtag(arity)):
        root, root_only, lv = _empty(4), _empty(4), _empty(_levels_len(n, arity), 4)
        _tree_device(run.ctx, arity, tag, d, n, root, lv)
        _tree_device(run.ctx, arity, tag, d, n, root_only, None)
        run.sync()
        if run.check:
            o_root, o_levels = oracle_tree(tag_red, red, arity)
            run.same(lv, o_levels, "tree levels arity=%d" % arity)
            run.same(root, o_root, "tree root")
            run.same(root_only, o_root, "tree root (scratch levels)")


def tree4(run):
    trees(run, 4, 65541)  # level 1: 16,386 nodes, the last with one child


def tree2(run):
    trees(run, 2, 32771)  # level 1: 16,386 nodes, the last with one child


def forest_equal(run, n_trees=64, per=64, seed=0x2100):
    """merkle4_forest_device: 64 complete trees of 4^3 leaves, one launch per level across all of them"""
    raw, red, _ = edge_draw(seed, (n_trees * per,))
    d = _dev(raw)
    per_tree = _levels_len(per, 4)
    for tag, tag_red in run.tags(_mtag(4)):
        roots, lv, roots_only = _empty(n_trees, 4), _empty(n_trees * per_tree, 4), _empty(n_trees, 4)
        run.ctx.merkle4_forest_device(tag, d, n_trees, per, roots, lv)
        run.ctx.merkle4_forest_device(tag, d, n_trees, per, roots_only, None)
        run.sync()
        if run.check:
            built = _pmap(lambda t: oracle.merkle4_tree(tag_red, red[t * per:(t + 1) * per], want_levels=True), range(n_trees))
            run.same(roots, np.stack([b[0] for b in built]), "forest roots")
            run.same(roots_only, np.stack([b[0] for b in built]), "forest roots (scratch levels)")
            want, off, cnt = [], 0, per
            while cnt > 1:  # level-major: level l of every tree, tree by tree
                cnt //= 4
                want += [b[1][off:off + cnt] for b in built]
                off += cnt
            run.same(lv, np.concatenate(want), "forest levels")


def permutations(run, n, seed=0x3000):
    raw, red, _ = edge_draw(seed + n, (n, 5))
    d, out = _dev(raw), _empty(n, 5, 4)
    run.ctx.permute_batch_device(d, out, n)
    run.sync()
    if run.check:
        run.same(out, oracle.permute_batch(red), "permute n=%d" % n)


# ---------------------------------------------------------------------------------------------- sponges
def sponges(run, n, shapes, truncated=False, seed=0x4000):
    for in_len, out_len in shapes:
        raw, red, _ = edge_draw(seed + 64 * in_len + out_len + n, (n, in_len))
        d = _dev(raw)
        assert d.data_ptr() % 64 == 0  # (k_sponge_lines takes messages that start on a 64-byte boundary)
        for tag, tag_red in run.tags(oracle.tag(3, [in_len], out_len)):
            out = _empty(n, out_len, 4)
            run.ctx.hash_batch_device(tag, d, in_len, out_len, out, n, truncated=truncated)
            run.sync()
            if run.check:
                want = oracle.hash_batch(tag_red, red, in_len, out_len, threads=ORACLE_THREADS)
                run.same(out, _truncated(want) if truncated else want, "sponge n=%d %d->%d" % (n, in_len, out_len))


# ---------------------------------------------------------------------------------------------- openings re-hashed
def rehash(tag_red, arity, leaves, sib, pos, depths=None):
    """roots of openings, level by level through oracle.hash_batch (opening i stops after depths[i] levels) — on reduced values; the
    re-hash itself is testsupport/soundness.py's, the one numpy model of an opening"""
    from testsupport.soundness import rehash as model_rehash
    return model_rehash(lambda ch: oracle.hash_batch(tag_red, ch, arity, 1, threads=ORACLE_THREADS), arity, leaves, sib, pos, depths)


def paths(run, n, depth, arity, seed=0x5000):
    """p252_merkle{4,2}_path_batch_device: leaves AND siblings are edge values"""
    raw, red, _ = edge_draw(seed + 100 * depth + arity + n, (n, 1 + depth * (arity - 1)))
    pos = np.random.default_rng(seed + depth).integers(0, arity, size=(n, depth), dtype=np.uint8)
    d_leaves, d_sib, d_pos = _dev(raw[:, 0]), _dev(raw[:, 1:]), _dev(pos)
    assert d_sib.data_ptr() % 128 == 0 and d_pos.data_ptr() % 4 == 0  # (what k_merkle4_path_lines asks of its buffers)
    call = run.ctx.merkle4_path_batch_device if arity == 4 else run.ctx.merkle2_path_batch_device
    for tag, tag_red in run.tags(_mtag(arity)):
        roots = _empty(n, 4)
        call(tag, d_leaves, d_sib, d_pos, depth, roots, n)
        run.sync()
        if run.check:
            sib_red = red[:, 1:].reshape(n, depth, arity - 1, 4)
            want = rehash(tag_red, arity, red[:, 0], sib_red, pos)
            if arity == 4:  # the oracle's own opening call, on the rows of the last blocks
                top = slice(max(0, n - 200), n)
                assert np.array_equal(want[top], oracle.merkle4_path_batch(tag_red, red[top, 0], sib_red[top], pos[top]))
            run.same(roots, want, "paths n=%d depth=%d arity=%d" % (n, depth, arity))


def verify_batch(run, arity, n_leaves, k=9000, seed=0x5800):
    """openings extracted from a stored tree over edge leaves, re-hashed and compared with ONE root (k_compare_roots): every opening
    verifies, still does with every leaf and sibling replaced by its unreduced twin, and none does against root + p"""
    import torch
    raw, red, _ = edge_draw(seed + arity, (n_leaves,))
    d, tag = _dev(raw), _mtag(arity)
    root, lv = _empty(4), _empty(_levels_len(n_leaves, arity), 4)
    _tree_device(run.ctx, arity, tag, d, n_leaves, root, lv)
    idx = np.random.default_rng(seed).integers(0, n_leaves, size=k).astype(np.uint32)
    idx[:2] = (0, n_leaves - 1)
    o_l, o_s, o_p, depth = run.ctx.merkle4_openings_device(d, n_leaves, lv, _dev(idx), k, arity=arity)
    ok = torch.full((3, k), 7, dtype=torch.uint8, device="cuda:0")
    run.ctx.merkle_verify_batch_device(tag, o_l, o_s, o_p, depth, root, ok[0], k, arity=arity)
    run.sync()
    if not run.check:
        return
    o_root = oracle_tree(tag, red, arity)[0]
    run.same(root, o_root, "tree root")
    assert np.array_equal(_host(o_l), raw[idx])  # (extraction copies bytes)
    t_l, t_s = _dev(unreduced_twin(reduce_mod_p(_host(o_l)))), _dev(unreduced_twin(reduce_mod_p(_host(o_s))))
    run.ctx.merkle_verify_batch_device(tag, t_l, t_s, o_p, depth, root, ok[1], k, arity=arity)
    run.ctx.merkle_verify_batch_device(tag, o_l, o_s, o_p, depth, _dev(plus_p(o_root)), ok[2], k, arity=arity)
    run.sync()
    got = _host(ok)
    assert (got[0] == 1).all() and (got[1] == 1).all(), "an opening of the tree's own leaves does not verify"
    assert (got[2] == 0).all(), "root + p was accepted as the root"


# ---------------------------------------------------------------------------------------------- encryption
CRYPT_CAP = 1024  # the oracle encrypts item by item: it checks the LAST rows of a large batch (the last partial wave among them)


def crypt(run, n, seed=0x6000):
    """encrypt / decrypt, STREAM and DUPLEX, lengths 1, 4, 5, 9: messages, both secret scalars and the nonces are edge values"""
    import torch
    from poseidon252_amd import encryption as E
    top = slice(max(0, n - CRYPT_CAP), n)
    for variant in (E.STREAM, E.DUPLEX):
        for length in (1, 4, 5, 9):
            raw, red, index = edge_draw(seed + 16 * length + variant + n, (n, length + 3))
            if n * (length + 3) >= 4 * len(PATTERNS) * 3:  # the capped part still holds every pattern
                assert set(range(len(PATTERNS))) <= set(index[top].reshape(-1).tolist())
            d_msg, d_sec, d_non = _dev(raw[:, :length]), _dev(raw[:, length:length + 2]), _dev(raw[:, length + 2])
            m_red, s_red, n_red = red[top, :length], red[top, length:length + 2], red[top, length + 2]
            for tag, tag_red in run.tags(oracle.encryption_tag(length, variant)):
                d_c = _empty(n, length + 1, 4)
                E.encrypt_batch_device(d_msg, d_sec, d_non, length, d_c, n, ctx=run.ctx, tag=tag, variant=variant)
                d_back, d_ok = _empty(n, length, 4), torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
                E.decrypt_batch_device(d_c, d_sec, d_non, length, d_back, d_ok, n, ctx=run.ctx, tag=tag, variant=variant)
                run.sync()
                if not run.check:
                    continue
                what = "crypt n=%d length=%d variant=%d" % (n, length, variant)
                cipher = _host(d_c)
                assert is_reduced(cipher).all(), what
                parts = np.array_split(np.arange(m_red.shape[0]), ORACLE_THREADS)
                want = np.concatenate(_pmap(lambda q: oracle.encrypt_batch(tag_red, m_red[q], s_red[q], n_red[q], variant=variant), parts))
                run.same(cipher[top], want, what)
                o_back, o_ok = oracle.decrypt_batch(tag_red, want[-64:], s_red[-64:], n_red[-64:], variant=variant)
                assert o_ok.all() and np.array_equal(o_back, m_red[-64:])  # (the oracle's own decryption: the messages it was given)
                run.same(_host(d_back)[top], m_red, what + " (decrypt)")
                assert (_host(d_ok) == 1).all(), what
                # the message elements of the cipher as their unreduced twins, the MAC as stored: the same messages, ok = 1
                twin = cipher.copy()
                twin[:, :length] = unreduced_twin(cipher[:, :length])
                E.decrypt_batch_device(_dev(twin), d_sec, d_non, length, d_back, d_ok, n, ctx=run.ctx, tag=tag, variant=variant)
                run.sync()
                run.same(_host(d_back)[top], m_red, what + " (decrypt of unreduced cipher elements)")
                assert (_host(d_ok) == 1).all(), what + ": an unreduced cipher element failed the MAC"
                # then the MAC as MAC + p: the same residue, other bytes — refused, the messages as before
                twin[:, length] = plus_p(cipher[:, length])
                E.decrypt_batch_device(_dev(twin), d_sec, d_non, length, d_back, d_ok, n, ctx=run.ctx, tag=tag, variant=variant)
                run.sync()
                run.same(_host(d_back)[top], m_red, what + " (decrypt under MAC + p)")
                assert (_host(d_ok) == 0).all(), what + ": MAC + p was accepted as the MAC"


# ---------------------------------------------------------------------------------------------- messages of different lengths
RAGGED_MAX_LEN = 23
RAGGED_UNREDUCED = (3, 8, 13, 18, 23)  # the lengths whose tag is the unreduced word


def ragged(run, n, out_len=2, seed=0x7000):
    """p252_hash_ragged[_truncated]_device: lengths 0 .. 23 mixed (0: a bad message, a zero row), one tag per length"""
    import torch
    rng = np.random.default_rng(seed + n)
    lens = rng.integers(0, RAGGED_MAX_LEN + 1, size=n)
    lens[:RAGGED_MAX_LEN + 1] = np.arange(RAGGED_MAX_LEN + 1)
    rng.shuffle(lens)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens.astype(np.uint64), out=off[1:])
    raw, red, _ = edge_draw(seed + n + 1, (int(off[-1]),))
    tags_red = np.stack([oracle.tag(3, [L], out_len) for L in range(1, RAGGED_MAX_LEN + 1)])
    tags = tags_red.copy()
    for L in RAGGED_UNREDUCED:
        tags[L - 1], tags_red[L - 1] = limbs(UNREDUCED_TAG), limbs(UNREDUCED_TAG % P)
    d_tags, d_in, d_off = _dev(tags), _dev(raw), _dev(off)
    start = off[:-1].astype(np.int64)
    for truncated in (False, True):
        out = torch.full((n, out_len, 4), -1, dtype=torch.int64, device="cuda:0")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        run.ctx.hash_ragged_device(d_tags, RAGGED_MAX_LEN, d_in, d_off, out_len, out, n, d_n_bad=bad, truncated=truncated)
        run.sync()
        if not run.check:
            continue
        want = np.zeros((n, out_len, 4), dtype=np.uint64)
        for L in range(1, RAGGED_MAX_LEN + 1):
            sel = np.nonzero(lens == L)[0]
            x = red[start[sel][:, None] + np.arange(L)[None, :]]
            h = oracle.hash_batch(tags_red[L - 1], x, L, out_len, threads=ORACLE_THREADS)
            want[sel] = _truncated(h) if truncated else h
        run.same(out, want, "ragged n=%d truncated=%s" % (n, truncated))
        assert int(bad) == int((lens == 0).sum())


# ---------------------------------------------------------------------------------------------- forests of trees of different sizes
FOREST_MAX_LEAVES = 40


class Forest:
    """a forest of n_trees trees of 1 .. 40 edge leaves on the device, built with caller-owned tree-major levels"""

    def __init__(self, run, arity, n_trees, seed=0x8000):
        import torch
        from poseidon252_amd.hash import _ARITIES
        self.run, self.arity, self.n_trees, self.tag = run, arity, n_trees, _mtag(arity)
        rng = np.random.default_rng(seed + arity + n_trees)
        self.sizes = rng.integers(1, FOREST_MAX_LEAVES + 1, size=n_trees)
        self.sizes[:FOREST_MAX_LEAVES] = np.arange(1, FOREST_MAX_LEAVES + 1)  # every size, trees of ONE leaf among them
        rng.shuffle(self.sizes)
        self.off = np.zeros(n_trees + 1, dtype=np.uint64)
        np.cumsum(self.sizes.astype(np.uint64), out=self.off[1:])
        self.n_leaves = int(self.off[-1])
        self.raw, self.red, _ = edge_draw(seed + 7 * arity + n_trees, (self.n_leaves,))
        self.lo = np.concatenate([[0], np.cumsum([_levels_len(int(s), arity) for s in self.sizes])]).astype(np.int64)
        self.d, self.d_off = _dev(self.raw), _dev(self.off)
        bound = self.n_leaves // (arity - 1) + n_trees * _ARITIES[arity].depth(FOREST_MAX_LEAVES)
        self.d_lv = torch.full((bound, 4), -1, dtype=torch.int64, device="cuda:0")
        self.d_roots = torch.full((n_trees, 4), -1, dtype=torch.int64, device="cuda:0")
        self.build(self.tag, self.d_roots, self.d_lv)

    def build(self, tag, d_roots, d_lv):
        import torch
        bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        self.run.ctx.merkle_forest_ragged_device(tag, self.d, self.d_off, self.n_trees, FOREST_MAX_LEAVES, d_roots, d_lv, bad, arity=self.arity)
        return bad

    def oracle_build(self, tag_red, red):
        """(roots (n_trees, 4), the tree-major levels) of the oracle's single-tree builds over the reduced leaves"""
        built = _pmap(lambda t: _otree(self.arity)(tag_red, red[int(self.off[t]):int(self.off[t + 1])], want_levels=True), range(self.n_trees))
        return np.stack([b[0] for b in built]), np.concatenate([b[1] for b in built])

    def same_as_oracle(self, tag_red, red, d_roots, d_lv, what):
        roots, levels = self.oracle_build(tag_red, red)
        self.run.same(d_roots, roots, what + " roots")
        if d_lv is not None:
            self.run.same(_host(d_lv)[:levels.shape[0]], levels, what + " levels")
        return roots


def forest_build(run, arity, n_trees):
    """p252_merkle{4,2}_forest_ragged_device, with levels and root-only, both tags: every root and every tree's level block"""
    f = Forest(run, arity, n_trees)
    for tag, tag_red in run.tags(f.tag):
        roots, roots_only, lv = _empty(n_trees, 4), _empty(n_trees, 4), _empty(f.d_lv.shape[0], 4)
        bad = f.build(tag, roots, lv)
        bad2 = f.build(tag, roots_only, None)
        run.sync()
        if run.check:
            assert int(bad) == 0 and int(bad2) == 0
            want = f.same_as_oracle(tag_red, f.red, roots, lv, "forest arity=%d trees=%d" % (arity, n_trees))
            run.same(roots_only, want, "forest roots (scratch levels)")


def forest_update(run, arity, n_trees, k, seed=0x8800):
    """p252_merkle{4,2}_forest_ragged_update_device: k new edge leaves under k DISTINCT parents (and in every one-leaf tree)"""
    import torch
    f = Forest(run, arity, n_trees)
    rng = np.random.default_rng(seed + arity + k)
    parents = (f.sizes + arity - 1) // arity
    tid = np.repeat(np.arange(n_trees), np.where(f.sizes > 1, parents, 0))
    node = np.concatenate([np.arange(p) for p, s in zip(parents, f.sizes) if s > 1])
    pick = rng.permutation(tid.size)[:k]
    tid, node = tid[pick], node[pick]
    lid = np.minimum(node * arity + rng.integers(0, arity, size=tid.size), f.sizes[tid] - 1)  # one child of each picked parent
    ones = np.nonzero(f.sizes == 1)[0]
    tid, lid = np.concatenate([tid, ones]), np.concatenate([lid, np.zeros(ones.size, dtype=np.int64)])
    new_raw, new_red, _ = edge_draw(seed + 3 * arity + k, (tid.size,))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    hashed = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    run.ctx.merkle_forest_ragged_update_device(f.tag, f.d, f.d_off, n_trees, FOREST_MAX_LEAVES, f.d_lv, _dev(tid.astype(np.uint32)),
                                               _dev(lid.astype(np.uint64)), _dev(new_raw), tid.size, d_roots=f.d_roots, d_n_bad=bad,
                                               d_n_hashed=hashed, arity=arity)
    run.sync()
    if not run.check:
        return
    at = f.off[tid].astype(np.int64) + lid
    raw, red = f.raw.copy(), f.red.copy()
    raw[at], red[at] = new_raw, new_red
    assert int(bad) == 0 and int(hashed) >= k
    assert np.array_equal(_host(f.d), raw), "the leaves do not hold the bytes handed in"
    f.same_as_oracle(f.tag, red, f.d_roots, f.d_lv, "forest update arity=%d k=%d" % (arity, k))


def forest_openings(run, arity, n_trees=3000, k=9000, seed=0x9000):
    """openings out of the forest, re-hashed for their own depths (k_path_ragged) and verified against the root of their tree
    (k_compare_roots_gather): all verify, still do as unreduced twins, none does against root + p"""
    import torch
    f = Forest(run, arity, n_trees)
    rng = np.random.default_rng(seed + arity)
    tid = rng.integers(0, n_trees, size=k)
    tid[:FOREST_MAX_LEAVES] = np.argsort(f.sizes, kind="stable")[:FOREST_MAX_LEAVES]  # (the smallest trees: those of one leaf)
    lid = (rng.integers(0, 1 << 30, size=k) % f.sizes[tid]).astype(np.uint64)
    d_tid = _dev(tid.astype(np.uint32))
    o_l, o_s, o_p, o_d, D = run.ctx.merkle_forest_ragged_openings_device(f.d, f.d_off, n_trees, FOREST_MAX_LEAVES, f.d_lv, d_tid, _dev(lid), k,
                                                                         arity=arity)
    back = _empty(k, 4)
    ok = torch.full((3, k), 7, dtype=torch.uint8, device="cuda:0")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    run.ctx.merkle_path_ragged_device(f.tag, o_l, o_s, o_p, o_d, D, back, k, d_n_bad=bad, arity=arity)
    run.ctx.merkle_forest_ragged_verify_device(f.tag, o_l, o_s, o_p, o_d, D, d_tid, f.d_roots, n_trees, ok[0], k, arity=arity)
    run.sync()
    if not run.check:
        return
    roots = f.same_as_oracle(f.tag, f.red, f.d_roots, f.d_lv, "forest arity=%d" % arity)
    assert int(bad) == 0
    depths = _host(o_d).astype(np.int64)
    assert depths.min() == 0 and depths.max() == D  # mixed depths, one-leaf trees among them
    run.same(back, roots[tid], "forest openings re-hashed")
    sib, pos = _host(o_s).reshape(k, D, arity - 1, 4), _host(o_p).reshape(k, D)
    assert np.array_equal(rehash(f.tag, arity, reduce_mod_p(_host(o_l)), reduce_mod_p(sib), pos, depths), roots[tid])
    t_l, t_s = _dev(unreduced_twin(reduce_mod_p(_host(o_l)))), _dev(unreduced_twin(reduce_mod_p(sib)))
    run.ctx.merkle_forest_ragged_verify_device(f.tag, t_l, t_s, o_p, o_d, D, d_tid, f.d_roots, n_trees, ok[1], k, arity=arity)
    run.ctx.merkle_forest_ragged_verify_device(f.tag, o_l, o_s, o_p, o_d, D, d_tid, _dev(plus_p(roots)), n_trees, ok[2], k, arity=arity)
    run.sync()
    got = _host(ok)
    assert (got[0] == 1).all() and (got[1] == 1).all(), "an opening of the forest's own leaves does not verify"
    assert (got[2] == 0).all(), "root + p was accepted as a root"


# ---------------------------------------------------------------------------------------------- one stored tree: updates, shared proofs
def tree_update(run, k, n=4 ** 8, seed=0xA000):
    """merkle4_update_device on a 4^8-leaf tree over edge leaves: k distinct positions get new edge leaves"""
    raw, red, _ = edge_draw(seed, (n,))
    d, tag = _dev(raw), _mtag(4)
    root, lv = _empty(4), _empty(_levels_len(n, 4), 4)
    run.ctx.merkle4_tree_device(tag, d, n, root, lv)
    idx = np.random.default_rng(seed + k).permutation(n)[:k].astype(np.uint32)
    new_raw, new_red, _ = edge_draw(seed + k, (k,))
    run.ctx.merkle4_update_device(tag, d, n, lv, _dev(idx), _dev(new_raw), k, d_root=root)
    run.sync()
    if run.check:
        raw, red = raw.copy(), red.copy()
        raw[idx], red[idx] = new_raw, new_red
        assert np.array_equal(_host(d), raw), "the leaves do not hold the bytes handed in"
        o_root, o_levels = oracle_tree(tag, red, 4)
        run.same(lv, o_levels, "update k=%d levels" % k)
        run.same(root, o_root, "update k=%d root" % k)


def multiproof(run, arity, n, k, seed=0xB000):
    """one shared proof of k sorted leaves of a tree over edge leaves: the proof is the numpy model's (multiproofmodel.py), it
    verifies, still does with its leaves and nodes as unreduced twins, and does not against root + p"""
    import torch
    from testsupport.multiproofmodel import multiproof_extract
    raw, red, _ = edge_draw(seed + arity, (n,))
    d, tag = _dev(raw), _mtag(arity)
    root, lv = _empty(4), _empty(_levels_len(n, arity), 4)
    _tree_device(run.ctx, arity, tag, d, n, root, lv)
    pos = np.sort(np.random.default_rng(seed + k).permutation(n)[:k])
    pos[0], pos[-1] = 0, n - 1
    d_idx = _dev(pos.astype(np.uint32))
    out, proof = _empty(k, 4), _empty(run.ctx.merkle_multiproof_bound(n, k, arity), 4)
    plen, bad = torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    run.ctx.merkle_multiproof_device(d, n, lv, d_idx, k, out, proof, plen, d_n_bad=bad, arity=arity)
    length = int(plen)
    ok = torch.full((3,), 7, dtype=torch.uint8, device="cuda:0")
    root_out = _empty(3, 4)

    def verify(i, leaves, nodes, expected):
        run.ctx.merkle_multiproof_verify_device(tag, n, d_idx, leaves, k, nodes[:length] if length else None, length, expected, ok[i:i + 1],
                                                d_root_out=root_out[i], arity=arity)
    verify(0, out, proof, root)
    run.sync()
    if not run.check:
        return
    o_root, o_levels = oracle_tree(tag, red, arity)
    run.same(lv, o_levels, "tree levels")
    run.same(root, o_root, "tree root")
    want = multiproof_extract(raw, o_levels, pos, arity)  # (extraction copies bytes: the leaves as handed in)
    assert int(bad) == 0 and length == want.shape[0]
    assert np.array_equal(_host(proof)[:length], want) and np.array_equal(_host(out), raw[pos])
    verify(1, _dev(unreduced_twin(red[pos])), _dev(unreduced_twin(reduce_mod_p(want))) if length else proof, root)
    verify(2, out, proof, _dev(plus_p(o_root)))
    run.sync()
    got = _host(ok)
    assert got[0] == 1 and got[1] == 1, "the shared proof of the tree's own leaves does not verify"
    assert got[2] == 0, "root + p was accepted as the root"
    run.same(root_out, np.stack([o_root] * 3), "multiproof roots")


# ---------------------------------------------------------------------------------------------- the matrix
class Row:
    def __init__(self, name, fn, kernels, coop=False, pad=False):
        """coop: a lane-group-sized row, run again on the one-lane kernels (P252_COOP_MAX_NODES=0); pad: run again with
        P252_TREE_PAD_LANES=65538 (k_merkle4_pad)"""
        self.name, self.fn, self.kernels, self.coop, self.pad = name, fn, tuple(kernels), coop, pad

    def __call__(self, run):
        t0 = time.perf_counter()
        self.fn(run)
        return time.perf_counter() - t0

    def __repr__(self):
        return self.name


ROWS = [
    Row("digest_16385", lambda r: digests(r, 16385), ["k_merkle4_lat"]),
    Row("digest_131073", lambda r: digests(r, 131073), ["k_merkle4"]),  # three waves per SIMD
    Row("digest_trunc_9", lambda r: (digests(r, 9, truncated=True), digests(r, 1200, truncated=True)), ["k_merkle4_coop8_trunc"], coop=True),
    Row("digest_trunc_8193", lambda r: digests(r, 8193, truncated=True), ["k_merkle4_trunc"]),
    Row("tree4_65541", tree4, ["k_merkle4_lat", "k_merkle4_coop"], pad=True),
    Row("tree2_32771", tree2, ["k_merkle4_lat", "k_merkle4_coop"], pad=True),
    Row("forest_64x64", forest_equal, ["k_merkle4_coop"]),
    Row("permute_8193", lambda r: permutations(r, 8193), ["k_permute"]),
    Row("permute_300", lambda r: permutations(r, 300), ["k_permute_coop"], coop=True),
    Row("sponge_8193", lambda r: sponges(r, 8193, [(5, 2)]), ["k_sponge"]),
    Row("sponge_lines_8193", lambda r: sponges(r, 8193, [(42, 5), (4, 7)]), ["k_sponge_lines"]),
    Row("sponge_300", lambda r: sponges(r, 300, [(9, 6), (1, 13)]), ["k_sponge_coop"], coop=True),
    Row("sponge_trunc_8193", lambda r: sponges(r, 8193, [(5, 1)], truncated=True), ["k_sponge_trunc"]),
    Row("sponge_lines_trunc_8193", lambda r: sponges(r, 8193, [(42, 5)], truncated=True), ["k_sponge_lines_trunc"]),
    Row("sponge_trunc_300", lambda r: sponges(r, 300, [(5, 1), (42, 5)], truncated=True), ["k_sponge_coop_trunc"], coop=True),
    Row("paths_300_d5", lambda r: paths(r, 300, 5, 4), ["k_merkle4_path_coop"], coop=True),
    Row("paths_8193_d5", lambda r: paths(r, 8193, 5, 4), ["k_merkle4_path"]),
    Row("paths_8193_d4_d12", lambda r: (paths(r, 8193, 4, 4), paths(r, 8193, 12, 4)), ["k_merkle4_path_lines"]),
    Row("paths2_8193_d9", lambda r: paths(r, 8193, 9, 2), ["k_merkle2_path"]),
    Row("verify_batch", lambda r: (verify_batch(r, 4, 4 ** 8), verify_batch(r, 2, 2 ** 14)), ["k_merkle4_path_lines", "k_merkle2_path", "k_compare_roots"]),
    Row("crypt_64", lambda r: crypt(r, 64), ["k_crypt_coop"], coop=True),
    Row("crypt_8193", lambda r: crypt(r, 8193), ["k_crypt"]),
    Row("ragged_100", lambda r: ragged(r, 100), ["k_sponge_ragged_coop", "k_sponge_ragged_coop_trunc"], coop=True),
    Row("ragged_8193", lambda r: ragged(r, 8193), ["k_sponge_ragged", "k_sponge_ragged_trunc"]),
    Row("forest4_3000", lambda r: forest_build(r, 4, 3000), ["k_fr_digest"]),
    Row("forest2_3000", lambda r: forest_build(r, 2, 3000), ["k_fr_digest"]),
    Row("forest_50", lambda r: (forest_build(r, 4, 50), forest_build(r, 2, 50)), ["k_fr_digest_coop"], coop=True),
    Row("forest_update4_9000", lambda r: forest_update(r, 4, 3000, 9000), ["k_fu_digest"]),
    Row("forest_update2_9000", lambda r: forest_update(r, 2, 3000, 9000), ["k_fu_digest"]),
    Row("forest_update_100", lambda r: (forest_update(r, 4, 3000, 100), forest_update(r, 2, 3000, 100)), ["k_fu_digest_coop"], coop=True),
    Row("tree_update_20000", lambda r: tree_update(r, 20000), ["k_merkle4_update"]),
    Row("tree_update_300", lambda r: tree_update(r, 300), ["k_merkle4_update_coop"], coop=True),
    Row("forest_openings4", lambda r: forest_openings(r, 4), ["k_path_ragged", "k_compare_roots_gather"]),
    Row("forest_openings2", lambda r: forest_openings(r, 2), ["k_path_ragged", "k_compare_roots_gather"]),
    Row("multiproof4_20000", lambda r: multiproof(r, 4, 4 ** 8, 20000), ["k_mp_digest"]),
    # (a level of a 2^14-leaf tree holds at most 8,192 parents — the lane groups' size: 2^16 leaves reach k_mp_digest<2>)
    Row("multiproof2_20000", lambda r: multiproof(r, 2, 2 ** 16, 20000), ["k_mp_digest"]),
    Row("multiproof_200", lambda r: (multiproof(r, 4, 4 ** 8, 200), multiproof(r, 2, 2 ** 14, 200)), ["k_mp_digest_coop"], coop=True),
]
BY_NAME = {r.name: r for r in ROWS}
# the environment-switched children of test_edge_values_gpu.py: what they set, the rows they run, the kernels those reach there
CHILDREN = {
    "pad": ({"P252_TREE_PAD_LANES": "65538"}, [r.name for r in ROWS if r.pad], ["k_merkle4_pad"]),
    "one_lane": ({"P252_COOP_MAX_NODES": "0"}, [r.name for r in ROWS if r.coop],
                 ["k_merkle4_trunc", "k_permute", "k_sponge", "k_sponge_trunc", "k_sponge_lines_trunc", "k_merkle4_path",
                  "k_crypt", "k_sponge_ragged", "k_sponge_ragged_trunc", "k_fr_digest", "k_fu_digest", "k_merkle4_update", "k_mp_digest"]),
}


def named_kernels():
    """every kernel some row names: the default-environment rows and the two children"""
    names = {k for r in ROWS for k in r.kernels}
    for _, _, kernels in CHILDREN.values():
        names |= set(kernels)
    return names


def kernel_in_trace(kernel, traced):
    """kernel (a function name) is one of the traced names (demangled `p252::k_x<..>(..)`, bare, or mangled)"""
    bare = re.compile(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(kernel))
    mangled = "%d%s" % (len(kernel), kernel)
    return any((n.startswith("_Z") and mangled in n) or bare.search(n) for n in traced)


# ---------------------------------------------------------------------------------------------- the library's hashing kernels
def _functions(text):
    """(qualifier, name, body) of every __global__ / __device__ function defined in a HIP source (comments stripped)"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for m in re.finditer(r"__(global|device)__", text):
        i, depth, last_open, params_at = m.end(), 0, -1, -1
        while i < len(text) and not (depth == 0 and text[i] in "{;"):
            if text[i] == "(":
                if depth == 0:
                    last_open = i
                depth += 1
            elif text[i] == ")":
                depth -= 1
                if depth == 0:
                    params_at = last_open
            i += 1
        if i >= len(text) or text[i] == ";" or params_at < 0:
            continue
        name = re.search(r"([A-Za-z_]\w*)\s*$", text[m.end():params_at])
        j, braces = i, 0
        while j < len(text):
            braces += (text[j] == "{") - (text[j] == "}")
            j += 1
            if braces == 0:
                break
        if name:
            out.append((m.group(1), name.group(1), text[i:j]))
    return out


def hashing_kernels(csrc=os.path.join(ROOT, "poseidon252_amd", "csrc")):
    """the __global__ functions of csrc/*.hip that run the permutation: a hades_permute* / node_digest_coop call in their body or in
    a function of the same file that they call.  primtest.hip's k_pt_* (the per-primitive harness) are left out by name."""
    kernels = set()
    for fname in sorted(os.listdir(csrc)):
        if not fname.endswith(".hip"):
            continue
        funcs = _functions(open(os.path.join(csrc, fname)).read())
        hashing, grew = set(), True
        while grew:
            grew = False
            for _, name, body in funcs:
                if name in hashing:
                    continue
                calls = r"\b(hades_permute\w*|node_digest_coop%s)\s*[<(]" % "".join("|" + re.escape(h) for h in sorted(hashing))
                if re.search(calls, body):
                    hashing.add(name)
                    grew = True
        kernels |= {name for q, name, _ in funcs if q == "global" and name in hashing and not name.startswith("k_pt_")}
    return kernels
