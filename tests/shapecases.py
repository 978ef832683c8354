"""Message shapes for the three kernel families whose control flow depends on a SHAPE parameter — the sponge (in_len, out_len), the
cipher (len, variant) and the opening re-hash (depth, arity): the shape lists (SPONGE_SHAPES, CRYPT_CASES, PATH_CASES), a plain
Python restatement of the dispatch (which kernel a call reaches, and which class of the kernel's shape-dependent branching a lane
falls in), and the runner that pushes a list through the device entry points and compares EVERY output row with the oracle.
tests/test_shape_sweep_cpu.py proves against the model that the lists reach every class; tests/test_shape_sweep_gpu.py runs them
on the lane-group kernels, and through tests/helpers/shape_sweep_driver.py on the one-lane, whole-line and block-by-block builds.
A plain helper module, imported as edgecases and forestwalk are: the lists and the model need numpy alone, the runner a context.

The values are plain random scalars (tests/edgecases.py is the sweep along the VALUE axis); everything here is byte equality."""
import hashlib
import os
import time

import numpy as np

import oracle
from edgecases import ORACLE_THREADS, _dev, _host, _mtag, _pmap, _truncated, rehash

STREAM, DUPLEX = 0, 1  # P252_CRYPT_STREAM / P252_CRYPT_DUPLEX (include/poseidon252_hip.h)

# ---------------------------------------------------------------------------------------------- the shape lists
# hash_batch_device sends (4, 1) and (2, 1) to the single-permutation digest kernels (api.cpp hash_batch_device_impl: launch_merkle4),
# never to a sponge kernel: they are not sponge shapes, and tests/edgecases.py's digest rows own them
DIGEST_SHAPES = ((4, 1), (2, 1))
# in_len 1 .. 18: every residue mod 4 with 1, 2, 3, 4 and 5 absorb blocks, and the even lengths 2 .. 18 that the whole-line kernel
# takes (2 and 4: one block, a message that ends in the line it starts in); out_len 1 .. 9: every residue mod 4 with 1 and 2
# squeeze blocks, and 9: a third block.  in_len 40 .. 44: the long messages of config 4 (42) and its neighbours of every residue,
# at out_len 1, 4, 5, 8 (a partial and a full block, one and two of them)
SPONGE_SHAPES = tuple((i, o) for i in range(1, 19) for o in range(1, 10) if (i, o) not in DIGEST_SHAPES) + \
    tuple((i, o) for i in (40, 41, 42, 43, 44) for o in (1, 4, 5, 8))
SPONGE_LAYOUTS = (0, 32, 64)  # the byte offset of message 0 in its 128-byte line: as allocated; block by block; whole lines, phases exchanged
RAGGED_IN_LENS = tuple(range(1, 19))  # hash_ragged_device on n messages of ONE length: the bytes of hash_batch_device
RAGGED_OUT_LEN = 5  # (two squeeze blocks, the second partial)
# len 1 .. 18: every residue mod 4 (where the last permutation inside the message falls, and the lane that holds the last element)
# with one to five chunks of DUPLEX; 41, 42, 43: the lengths of the reference's own tests and their neighbours
CRYPT_LENS = tuple(range(1, 19)) + (41, 42, 43)
CRYPT_CASES = tuple((v, ln) for v in (STREAM, DUPLEX) for ln in CRYPT_LENS)
# depth 0 (p252_merkle{4,2}_path_batch_device accept it: the leaf is the root; tests/test_shape_sweep_gpu.py pins that), 1, both
# neighbours of 4, 8 and 12, and 16 and 20: the whole-line kernel fetches the position bytes of 16 levels at a time
PATH_DEPTHS = tuple(range(0, 14)) + (16, 20)
PATH_CASES = tuple((a, d) for a in (4, 2) for d in PATH_DEPTHS)
PATH_LAYOUTS = ("aligned", "siblings+32", "positions+1")  # as allocated; siblings one scalar into a line; positions at an odd address

N_LANE_GROUPS = 70  # eight lanes per message: eight messages fill a wave; 70 leave a partial group of waves and a partial wave
N_ONE_LANE = 323    # one lane per message: one full block of 256, one full wave, three lanes


# ---------------------------------------------------------------------------------------------- the dispatch model
def environment():
    """(coop_max_nodes, line_fetch) as the library reads them, once per process (kernels.hip coop_max_nodes, line_fetch)"""
    e = os.environ.get("P252_COOP_MAX_NODES")
    f = os.environ.get("P252_LINE_FETCH")
    return (int(e) if e else 16384), not (f and f[0] == "0")


def coop8(n, coop_max=16384):
    """kernels.h coop8: the batch runs on lane groups"""
    return n <= coop_max and n * 8 <= 65536


def sponge_kernel(n, in_len, out_len, offset, truncated, coop_max=16384, line_fetch=True):
    """the kernel hash_batch_device launches (api.cpp hash_batch_device_impl, kernels.hip launch_sponge); offset: the address of
    the input mod 128"""
    assert (in_len, out_len) not in DIGEST_SHAPES
    if coop8(n, coop_max):
        name = "k_sponge_coop"
    elif line_fetch and in_len % 2 == 0 and offset % 64 == 0:
        name = "k_sponge_lines"
    else:
        name = "k_sponge"
    return name + ("_trunc" if truncated else "")


def sponge_lane(in_len, out_len, offset, idx, lines):
    """what sponge_body<LINES> derives for lane idx: sh (scalars into its line), tail_half, the trip at which `parked` first turns
    true (None: never), the absorb and squeeze block counts"""
    absorb_blocks, squeeze_blocks = (in_len + 3) // 4, (out_len + 3) // 4
    sh = ((offset + idx * in_len * 32) >> 5) & 3 if lines else 0
    tail_half = lines and ((sh + in_len) & 3) == 2 and in_len >= 2
    parked = next((it for it in range(absorb_blocks) if tail_half and it * 4 + sh + 4 > in_len), None)
    return {"sh": sh, "tail_half": tail_half, "parked": parked, "absorb_blocks": absorb_blocks, "squeeze_blocks": squeeze_blocks}


def sponge_class(in_len, out_len, offset, idx, lines):
    """the class of a lane's path through sponge_body.  Block by block: (in_len mod 4, absorb blocks 1 | 2 | 3 = more, out_len mod 4,
    squeeze blocks).  Whole lines: the same with the line phase, tail_half and the trip of `parked` ('first', 'later', None)."""
    lane = sponge_lane(in_len, out_len, offset, idx, lines)
    out = (out_len % 4, min(lane["squeeze_blocks"], 3))
    if not lines:
        return (in_len % 4, min(lane["absorb_blocks"], 3)) + out
    parked = None if lane["parked"] is None else "first" if lane["parked"] == 0 else "later"
    return (in_len % 4, lane["sh"], min(lane["absorb_blocks"], 3), lane["tail_half"], parked) + out


def ragged_sponge_kernel(n, truncated, coop_max=16384):
    """ragged.hip launch_hash_ragged"""
    return ("k_sponge_ragged_coop" if coop8(n, coop_max) else "k_sponge_ragged") + ("_trunc" if truncated else "")


def crypt_program(variant, length):
    """api.cpp crypt_program: the sponge calls of one encryption as (kind, count); kinds as in kernels.hip k_crypt"""
    prog = [(0, 2), (1, 1)]
    if variant == STREAM:
        prog += [(2, length), (3, length)]
    else:
        left = length
        while left:
            c = min(left, 4)
            prog += [(2, c), (3, c)]
            left -= c
    return prog + [(4, 1)]


def crypt_walk(variant, length):
    """k_crypt's walk over the call table: one (kind, position, permutes first) per element"""
    pos_absorb = pos_squeeze = 0
    walk = []
    for kind, cnt in crypt_program(variant, length):
        is_absorb = kind in (0, 1, 3)
        for _ in range(cnt):
            permutes = (pos_absorb if is_absorb else pos_squeeze) == 4
            if permutes:
                pos_absorb = 0
                if not is_absorb:
                    pos_squeeze = 0
            if is_absorb:
                walk.append((kind, pos_absorb, permutes))
                pos_absorb += 1
            else:
                walk.append((kind, pos_squeeze, permutes))
                pos_squeeze += 1
        if is_absorb:
            pos_squeeze = 4
    return walk


def crypt_class(variant, length):
    """(variant, len mod 4, permutations inside the message 1 | 2 | 3 = more, the MAC squeeze permutes)"""
    walk = crypt_walk(variant, length)
    inside = sum(1 for kind, _, permutes in walk if kind in (2, 3) and permutes)
    return (variant, length % 4, min(inside, 3), walk[-1][2])


def crypt_kernel(n, coop_max=16384):
    """kernels.hip launch_crypt (both template forms: encrypt and decrypt)"""
    return "k_crypt_coop" if coop8(n, coop_max) else "k_crypt"


def path_kernel(arity, n, depth, layout, coop_max=16384, line_fetch=True):
    """kernels.hip launch_merkle4_path / merkle2.hip launch_merkle2_path (arity 2: one kernel at every size)"""
    if arity == 2:
        return "k_merkle2_path"
    if coop8(n, coop_max):
        return "k_merkle4_path_coop"
    lines = line_fetch and depth != 0 and depth % 4 == 0 and layout == "aligned"  # siblings on a line, positions on a word
    return "k_merkle4_path_lines" if lines else "k_merkle4_path"


def path_class(depth):
    """(depth mod 4, groups of four levels 0 | 1 | 2 = more): depth 0 is (0, 0), depth 1 is (1, 0)"""
    return (depth % 4, min(depth // 4, 2))


def path_lines_class(depth):
    """the whole-line kernel: (position words in use 1 .. 4, a second fetch of position words)"""
    return (min(depth // 4, 4), depth > 16)


FAMILIES = ("sponge", "crypt", "paths")
WHOLE = (0, 1)  # a part (i, k) of a family's list is every k-th case from the i-th on: children that must stay short run a part each


def family_cases(family, part=WHOLE):
    """the cases of one family's sweep, or a part of them: for the sponge (the shapes, the lengths of the ragged equivalence)"""
    i, k = part
    if family == "sponge":
        return SPONGE_SHAPES[i::k], RAGGED_IN_LENS[i::k]
    return {"crypt": CRYPT_CASES, "paths": PATH_CASES}[family][i::k]


def predicted_kernels(family, n, coop_max=None, line_fetch=None, part=WHOLE):
    """every kernel the sweep of `family` at n launches under (coop_max, line_fetch) — default: this process's environment"""
    env = environment()
    coop_max = env[0] if coop_max is None else coop_max
    line_fetch = env[1] if line_fetch is None else line_fetch
    cases = family_cases(family, part)
    if family == "sponge":
        names = {sponge_kernel(n, i, o, off, t, coop_max, line_fetch) for i, o in cases[0] for off in SPONGE_LAYOUTS for t in (False, True)}
        return names | {ragged_sponge_kernel(n, t, coop_max) for t in (False, True) if cases[1]}
    if family == "crypt":
        return {crypt_kernel(n, coop_max) for _ in cases}
    return {path_kernel(a, n, d, lay, coop_max, line_fetch) for a, d in cases for lay in PATH_LAYOUTS} | ({"k_path_ragged"} if cases else set())


def expected_rows(family, n, part=WHOLE):
    """the output rows the sweep of `family` at n compares (what a report must count: an empty sweep is no sweep)"""
    cases = family_cases(family, part)
    if family == "sponge":
        return n * (len(cases[0]) * len(SPONGE_LAYOUTS) * 2 + len(cases[1]) * 2)
    if family == "crypt":
        return n * len(cases) * 3  # ciphers, messages back, messages of the tampered copy
    return n * len(cases) * (len(PATH_LAYOUTS) + 1)


# ---------------------------------------------------------------------------------------------- big-integer references
def bigint_encrypt(variant, tag, message, secret, nonce, perm):
    """the big-integer state machine of tests/pymodel.py (its one copy)"""
    from pymodel import _bigint_encrypt
    return _bigint_encrypt(variant, tag, message, secret, nonce, perm)


# ---------------------------------------------------------------------------------------------- the runner
class Sweep:
    """one run of shapes through a context: counts the rows compared, digests every output, notes the kernels the model expects.
    check=False: the GPU side alone (for the kernel tracer)"""

    def __init__(self, ctx, n, check=True):
        self.ctx, self.n, self.check = ctx, n, check
        self.rows, self.sha, self.kernels = 0, hashlib.sha256(), set()
        self.coop_max, self.line_fetch = environment()

    def sync(self):
        import torch
        torch.cuda.synchronize()

    def same(self, got, want, what, rows=None):
        """every row of a device output against the oracle's; the bytes go into the digest"""
        got = _host(got)
        self.sha.update(np.ascontiguousarray(got).tobytes())
        if not self.check:
            return
        want = np.asarray(want, dtype=got.dtype)
        got = got.reshape(want.shape)
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(want.shape[0], -1).any(axis=1))[0]
            raise AssertionError("%s: %d of %d rows differ from the oracle, first at %d" % (what, bad.size, want.shape[0], int(bad[0])))
        self.rows += want.shape[0] if rows is None else rows


def _at_offset(scalars, offset):
    """the scalars (.., 4) uint64 on the device, flat, with scalar 0 at `offset` bytes into a 128-byte line"""
    import torch
    flat = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    k = offset // 32
    buf = torch.zeros((flat.shape[0] + k + 1, 4), dtype=torch.int64, device="cuda:0")
    assert buf.data_ptr() % 128 == 0
    view = buf[k:k + flat.shape[0]]
    view.copy_(torch.from_numpy(flat.view(np.int64)))
    assert view.is_contiguous() and (view.numel() == 0 or view.data_ptr() % 128 == offset)
    return view


def _guarded(n, *shape):
    """an output of n rows and one more that no kernel may touch, all ones"""
    import torch
    return torch.full((n + 1,) + shape, -1, dtype=torch.int64, device="cuda:0")


def _untouched(out, n, what):
    assert bool((out[n:] == -1).all()), what + ": a store past the last row"


def sponge_shape(sw, in_len, out_len, seed=0x51000):
    """one (in_len, out_len) through hash_batch_device: three layouts, plain and truncated"""
    n = sw.n
    msgs = oracle.fill_random(seed + 64 * in_len + out_len, n * in_len).reshape(n, in_len, 4)
    tag = oracle.tag(3, [in_len], out_len)
    want = want_trunc = None
    if sw.check:
        want = oracle.hash_batch(tag, msgs, in_len, out_len, threads=ORACLE_THREADS)
        want_trunc = _truncated(want)
    for offset in SPONGE_LAYOUTS:
        d = _at_offset(msgs, offset)
        for truncated in (False, True):
            out = _guarded(n, out_len, 4)
            sw.ctx.hash_batch_device(tag, d, in_len, out_len, out, n, truncated=truncated)
            sw.sync()
            what = "sponge n=%d %d->%d at +%d B%s" % (n, in_len, out_len, offset, " truncated" if truncated else "")
            sw.same(out[:n], want_trunc if truncated else want, what)
            _untouched(out, n, what)
            sw.kernels.add(sponge_kernel(n, in_len, out_len, offset, truncated, sw.coop_max, sw.line_fetch))


def sponge_ragged_equivalence(sw, in_len, out_len=RAGGED_OUT_LEN, seed=0x52000):
    """hash_ragged_device on n messages that all have in_len scalars, with that length's tag: the bytes of hash_batch_device"""
    import torch
    n = sw.n
    msgs = oracle.fill_random(seed + in_len, n * in_len).reshape(n, in_len, 4)
    tags = np.stack([oracle.tag(3, [L], out_len) for L in range(1, in_len + 1)])
    d, d_tags = _dev(msgs.reshape(-1, 4)), _dev(tags)
    d_off = torch.arange(0, (n + 1) * in_len, in_len, dtype=torch.int64, device="cuda:0")
    for truncated in (False, True):
        fixed, rag = _guarded(n, out_len, 4), _guarded(n, out_len, 4)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        sw.ctx.hash_batch_device(tags[in_len - 1], d, in_len, out_len, fixed, n, truncated=truncated)
        sw.ctx.hash_ragged_device(d_tags, in_len, d, d_off, out_len, rag, n, d_n_bad=bad, truncated=truncated)
        sw.sync()
        what = "ragged sponge n=%d %d->%d%s" % (n, in_len, out_len, " truncated" if truncated else "")
        sw.same(rag[:n], _host(fixed[:n]), what)
        _untouched(rag, n, what)
        if sw.check:
            assert int(bad) == 0, what
        sw.kernels.add(ragged_sponge_kernel(n, truncated, sw.coop_max))


def tampered(cipher):
    """a copy of the ciphers (n, len + 1, 4) in which row i has one bit flipped in element i mod (len + 1): with n > len every
    element index, the MAC included, is hit by some row"""
    bad = cipher.copy()
    rows = np.arange(bad.shape[0])
    bad[rows, rows % bad.shape[1], 1] ^= np.uint64(4)
    return bad


def _oracle_encrypt(tag, msgs, secrets, nonces, variant):
    """oracle.encrypt_batch, which works item by item, on ORACLE_THREADS host threads"""
    parts = [q for q in np.array_split(np.arange(msgs.shape[0]), ORACLE_THREADS) if q.size]
    return np.concatenate(_pmap(lambda q: oracle.encrypt_batch(tag, msgs[q], secrets[q], nonces[q], variant=variant), parts))


def _oracle_decrypt(tag, ciphers, secrets, nonces, variant):
    """oracle.decrypt_batch likewise: (messages, ok)"""
    parts = [q for q in np.array_split(np.arange(ciphers.shape[0]), ORACLE_THREADS) if q.size]
    done = _pmap(lambda q: oracle.decrypt_batch(tag, ciphers[q], secrets[q], nonces[q], variant=variant), parts)
    return np.concatenate([d[0] for d in done]), np.concatenate([d[1] for d in done])


def crypt_case(sw, variant, length, seed=0x53000):
    """one (variant, len) through encrypt / decrypt_batch_device: the ciphers, the messages back, and a tampered copy"""
    import torch
    from poseidon252_amd import encryption as E
    n = sw.n
    assert n > length
    s = seed + 16 * length + variant
    msgs = oracle.fill_random(s, n * length).reshape(n, length, 4)
    secrets, nonces = oracle.fill_random(s + 1, 2 * n).reshape(n, 2, 4), oracle.fill_random(s + 2, n)
    tag = oracle.encryption_tag(length, variant)
    d_msg, d_sec, d_non = _dev(msgs), _dev(secrets), _dev(nonces)
    what = "crypt n=%d len=%d variant=%d" % (n, length, variant)
    d_c = _guarded(n, length + 1, 4)
    E.encrypt_batch_device(d_msg, d_sec, d_non, length, d_c, n, ctx=sw.ctx, tag=tag, variant=variant)
    d_back, d_ok = _guarded(n, length, 4), torch.full((n + 1,), 7, dtype=torch.uint8, device="cuda:0")
    E.decrypt_batch_device(d_c, d_sec, d_non, length, d_back, d_ok, n, ctx=sw.ctx, tag=tag, variant=variant)
    sw.sync()
    cipher = _host(d_c[:n]).copy()
    sw.same(d_c[:n], _oracle_encrypt(tag, msgs, secrets, nonces, variant) if sw.check else None, what)
    sw.same(d_back[:n], msgs, what + " (decrypt)")
    sw.sha.update(_host(d_ok).tobytes())
    assert not sw.check or (_host(d_ok)[:n] == 1).all(), what + ": a cipher of the library's own was refused"
    bad = tampered(cipher)
    d_back2, d_ok2 = _guarded(n, length, 4), torch.full((n + 1,), 7, dtype=torch.uint8, device="cuda:0")
    E.decrypt_batch_device(_dev(bad), d_sec, d_non, length, d_back2, d_ok2, n, ctx=sw.ctx, tag=tag, variant=variant)
    sw.sync()
    o_back = o_ok = None
    if sw.check:
        o_back, o_ok = _oracle_decrypt(tag, bad, secrets, nonces, variant)
        assert not o_ok.all()  # (the oracle refuses tampered rows at all)
        got_ok = _host(d_ok2)[:n]
        assert np.array_equal(got_ok == 1, o_ok) and np.isin(got_ok, (0, 1)).all(), what + ": not the rows the oracle refuses"
        acc = np.nonzero(o_ok)[0]
        assert np.array_equal(_host(d_back2[:n])[acc], o_back[acc]), what + ": an accepted row differs from the oracle"
    # (refused rows too: the oracle writes the message it recovers whatever the MAC says, as the kernel does)
    sw.same(d_back2[:n], o_back, what + " (decrypt of the tampered copy)")
    sw.sha.update(_host(d_ok2).tobytes())
    for out in (d_c, d_back, d_back2):
        _untouched(out, n, what)
    assert int(d_ok[n]) == 7 and int(d_ok2[n]) == 7, what + ": a flag past the last row"
    sw.kernels.add(crypt_kernel(n, sw.coop_max))


def path_case(sw, arity, depth, seed=0x54000):
    """one (arity, depth) through merkle{4,2}_path_batch_device in three layouts, and through merkle_path_ragged_device with every
    opening at that depth and a stride of that depth"""
    import torch
    n, per = sw.n, arity - 1
    s = seed + 100 * depth + arity
    leaves = oracle.fill_random(s, n)
    sib = oracle.fill_random(s + 1, n * depth * per).reshape(n, depth, per, 4)
    pos = np.random.default_rng(s).integers(0, arity, size=(n, depth), dtype=np.uint8)
    tag = _mtag(arity)
    want = None
    if sw.check:
        want = rehash(tag, arity, leaves, sib, pos)
        if depth == 0:  # no level: the leaf is the root
            assert np.array_equal(want, leaves)
        elif arity == 4:  # the oracle's own opening call, every row
            assert np.array_equal(want, oracle.merkle4_path_batch(tag, leaves, sib, pos))
    d_leaves, d_pos = _dev(leaves), _dev(pos.reshape(-1))
    d_sib = {0: _at_offset(sib, 0), 32: _at_offset(sib, 32)}
    d_pos_odd = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda:0"), d_pos])[1:]
    assert d_pos.data_ptr() % 4 == 0 and (depth == 0 or d_pos_odd.data_ptr() % 2 == 1)
    call = sw.ctx.merkle4_path_batch_device if arity == 4 else sw.ctx.merkle2_path_batch_device
    for layout, d_s, d_p in (("aligned", d_sib[0], d_pos), ("siblings+32", d_sib[32], d_pos), ("positions+1", d_sib[0], d_pos_odd)):
        roots = _guarded(n, 4)
        call(tag, d_leaves, d_s, d_p, depth, roots, n)
        sw.sync()
        what = "paths n=%d depth=%d arity=%d %s" % (n, depth, arity, layout)
        sw.same(roots[:n], want, what)
        _untouched(roots, n, what)
        sw.kernels.add(path_kernel(arity, n, depth, layout, sw.coop_max, sw.line_fetch))
    roots = _guarded(n, 4)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_depths = torch.full((n,), depth, dtype=torch.uint8, device="cuda:0")
    sw.ctx.merkle_path_ragged_device(tag, d_leaves, d_sib[0], d_pos, d_depths, depth, roots, n, d_n_bad=bad, arity=arity)
    sw.sync()
    what = "ragged paths n=%d depth=%d arity=%d" % (n, depth, arity)
    sw.same(roots[:n], want, what)
    _untouched(roots, n, what)
    assert not sw.check or int(bad) == 0, what
    sw.kernels.add("k_path_ragged")


def run_family(sw, family, part=WHOLE):
    """the list of one family, or a part of it; returns the seconds it took"""
    t0 = time.perf_counter()
    cases = family_cases(family, part)
    if family == "sponge":
        for in_len, out_len in cases[0]:
            sponge_shape(sw, in_len, out_len)
        for in_len in cases[1]:
            sponge_ragged_equivalence(sw, in_len)
    elif family == "crypt":
        for variant, length in cases:
            crypt_case(sw, variant, length)
    else:
        assert family == "paths"
        for arity, depth in cases:
            path_case(sw, arity, depth)
    return time.perf_counter() - t0
