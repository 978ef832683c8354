"""Host-side mirror of the reference's public hash API over the C ABI.

Mirrors, name for name, `dusk_poseidon::{Domain, Hash}` (src/hash.rs:21-211, re-exported at
src/lib.rs:19-22) and adds the batched sibling `HashBatch` that the GPU needs.  The reference is a
Rust crate; no Rust toolchain exists in this image, so this mirror is Python over ctypes (the Rust
binding a maintainer would add is in INTEGRATION.md).  All hashing happens in
libposeidon252_hip.so on the GPU — a missing extension or GPU raises, nothing falls back to a CPU.

Scalars are numpy uint64 arrays whose last axis is the 4 little-endian limbs of a `BlsScalar`
(Montgomery form, exactly the reference's memory layout), or torch CUDA tensors of the same bytes.
"""
import ctypes
import enum
import inspect

import numpy as np

from . import _lib
from ._lib import _u64p, _u8p

__all__ = ["Domain", "Hash", "HashBatch", "RaggedHashBatch", "Context", "Error", "IOPatternViolation", "InvalidIOPattern",
           "HADES_WIDTH", "compute_tag"]

HADES_WIDTH = 5  # dusk_poseidon::HADES_WIDTH, src/lib.rs:17


class Error(Exception):
    """dusk_poseidon::Error (src/error.rs:9-29) — only the variants the hash path can produce."""


class IOPatternViolation(Error):
    """Error::IOPatternViolation (src/error.rs:12-14): Merkle domain with the wrong arity (hash.rs:70-78)."""


class InvalidIOPattern(Error):
    """Error::InvalidIOPattern (src/error.rs:16-17): empty input / zero-length chunk / zero outputs."""


class DeviceError(RuntimeError):
    """HIP failure or no device: there is no CPU fallback."""


def _raise(rc, ctx_handle=None, global_err=False):
    """global_err: the failing call had no context (p252_comm_unique_id, p252_comm_backend) — its message is p252_last_error(NULL)"""
    msg = _lib.lib().p252_last_error(ctx_handle).decode() if (ctx_handle is not None or global_err) else ""
    if rc == _lib.ERR_IO_PATTERN_VIOLATION:
        raise IOPatternViolation("io-pattern should be valid: IOPatternViolation " + msg)
    if rc == _lib.ERR_INVALID_IO_PATTERN:
        raise InvalidIOPattern("at this point the io-pattern is valid: InvalidIOPattern " + msg)
    if rc == _lib.ERR_INVALID_ARGUMENT:
        raise ValueError("poseidon252_hip: invalid argument " + msg)
    raise DeviceError("poseidon252_hip error %d: %s" % (rc, msg))


class Domain(enum.IntEnum):
    """`enum Domain` (src/hash.rs:21-36), discriminants in declaration order."""
    Merkle4 = 0
    Merkle2 = 1
    Encryption = 2
    Other = 3

    def separator(self):
        """`From<Domain> for u64` (src/hash.rs:38-56)."""
        out = ctypes.c_uint64(0)
        rc = _lib.lib().p252_domain_separator(int(self), ctypes.byref(out))
        if rc:
            _raise(rc)
        return out.value

    def __int__(self):
        return self.value


def check_io_pattern(domain, absorb_lens, output_len):
    """`io_pattern()` (src/hash.rs:62-85) + dusk-safe's validation; raises like Hash::finalize panics."""
    lens = (ctypes.c_size_t * max(1, len(absorb_lens)))(*absorb_lens)
    rc = _lib.lib().p252_check_io_pattern(int(domain), lens, len(absorb_lens), output_len)
    if rc:
        _raise(rc)


def compute_tag(domain, absorb_lens, output_len):
    """Safe::tag for this io-pattern (scalar.rs:29-31).  UNPINNED recipe — see DESIGN.md; Rust callers
    pass the value from the real crates instead (every entry point accepts `tag=`)."""
    lens = (ctypes.c_size_t * max(1, len(absorb_lens)))(*absorb_lens)
    out = np.empty(4, dtype=np.uint64)
    rc = _lib.lib().p252_tag(int(domain), lens, len(absorb_lens), output_len, _ptr(out))
    if rc:
        _raise(rc)
    return out


def _as_scalars(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.shape[-1] != 4:
        raise ValueError("scalar arrays need a trailing axis of 4 u64 limbs")
    return a


def _ptr(a, kind=_u64p):
    """C pointer to a C-contiguous numpy array (the pointer holds a reference to the array)"""
    return a.ctypes.data_as(kind)


def _tag(tag):
    return _ptr(_as_scalars(tag).reshape(4))


def _host_out(call, out, n_scalars):
    """a caller-provided host output buffer: C-contiguous uint64, exactly n_scalars scalars"""
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint64 and out.flags.c_contiguous and out.size == n_scalars * 4):
        raise ValueError("%s: out must be a C-contiguous uint64 array of %d scalars" % (call, n_scalars))
    return out


def _dev_ptr(ctx, call, arg, t, need, elem=0, null_ok=False):
    """the device address the C call `call` takes for argument `arg`: t must be a contiguous torch CUDA tensor on ctx's device
    holding at least the `need` bytes the call touches (and, if `elem` is given, of elem-byte elements), else ValueError — the
    library can only check alignment, and a host pointer or a short view would reach a kernel.  null_ok: None passes as NULL.
    Reads metadata only (no synchronisation, no allocation): these calls are captured into graphs."""
    if t is None and null_ok:
        return None
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a torch tensor, not %s" % (call, arg, type(t).__name__))
    if not t.is_cuda:
        raise ValueError("%s: %s is on %s, not on the GPU" % (call, arg, t.device))
    if t.get_device() != ctx.device:
        raise ValueError("%s: %s is on cuda:%d, the context is on cuda:%d" % (call, arg, t.get_device(), ctx.device))
    if not t.is_contiguous():
        raise ValueError("%s: %s is not contiguous" % (call, arg))
    if elem and t.element_size() != elem:
        raise ValueError("%s: %s needs %d-byte elements, not %d" % (call, arg, elem, t.element_size()))
    if t.numel() * t.element_size() < need:
        raise ValueError("%s: %s holds %d bytes, the call touches %d" % (call, arg, t.numel() * t.element_size(), need))
    return t.data_ptr()


def _dev_ptrs(ctxs, call, arg, ts, needs):
    """_dev_ptr for each context of a multi-device call: ts[i] on ctxs[i]'s device, needs[i] bytes -> a void* array"""
    if len(ts) != len(ctxs) or len(needs) != len(ctxs):
        raise ValueError("%s: %d contexts, %d tensors in %s, %d sizes" % (call, len(ctxs), len(ts), arg, len(needs)))
    return (ctypes.c_void_p * len(ctxs))(*[_dev_ptr(c, call, "%s[%d]" % (arg, i), ts[i], needs[i]) for i, c in enumerate(ctxs)])


def _stream(ctx):
    """the current torch stream of ctx's device: where the *_device calls launch"""
    import torch
    return torch.cuda.current_stream(ctx.device).cuda_stream


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _n_scalars(t):  # the BlsScalars a tensor holds
    return t.numel() * t.element_size() // 32


def levels_len(n_leaves, arity=4):  # (public as merkle.levels_len) a tree's upper levels in scalars, as p252_merkle{4,2}_levels_len
    total, c = 0, n_leaves
    while c > 1:
        c = (c + arity - 1) // arity
        total += c
    return total


class _Arity:
    """One supported Merkle arity: its C entry points p252_merkle<arity>_<stem> (named once, from _lib.PROTOTYPES; looked up in the
    library of each call, which tests and P252_LIB_PATH replace), the siblings per level `per`, the domain of its node hash."""

    def __init__(self, arity, domain):
        self.arity, self.per, self.domain = arity, arity - 1, domain
        prefix = "p252_merkle%d_" % arity
        self._names = {name[len(prefix):]: name for name in _lib.PROTOTYPES if name.startswith(prefix)}

    def fn(self, stem):
        return getattr(_lib.lib(), self._names[stem])

    def depth(self, n_leaves):
        return int(self.fn("depth")(n_leaves))

    def levels_len(self, n_leaves):
        return int(self.fn("levels_len")(n_leaves))

    def forest_levels_bytes(self, n_leaves, n_trees, depth):  # of a ragged forest's d_levels: a bound, the offsets are never read back
        return (n_leaves // self.per + n_trees * depth) * 32

    def tag(self):
        return compute_tag(self.domain, [self.arity], 1)


_ARITIES = {4: _Arity(4, Domain.Merkle4), 2: _Arity(2, Domain.Merkle2)}


def _arity(f, arity):
    if arity not in (2, 4):
        raise ValueError("%s: arity must be 4 or 2, not %r" % (f, arity))
    return _ARITIES[arity]


def _offsets_fit(prefix, off, flat, holds):
    if off.shape[0] and int(off[-1]) > flat.shape[0]:
        raise ValueError("%soffsets reach past the %d %s given" % (prefix, flat.shape[0], holds))


def _ragged_items(items, prefix, noun, holds, empty, strict=False):
    """(flat (S, 4) uint64, offsets (n + 1,) uint64, lengths (n,) int64) of a list of (n_i, 4) arrays or of a (flat, offsets) pair with
    item i = flat[offsets[i]:offsets[i+1]].  Refused, in this order: decreasing offsets, offsets past flat (ValueError: prefix, the items
    named by `noun`, flat by what it `holds`), an empty item (empty = exception type, prefix); strict: first, arrays other than (u)int64."""
    def ints(a, what):
        if strict and np.asarray(a).dtype not in (np.uint64, np.int64):
            raise ValueError("%s%s must be uint64 or int64, not %s" % (prefix, what, np.asarray(a).dtype))
        return a
    if isinstance(items, tuple):
        flat, off = items
        flat = _as_scalars(ints(flat, "the " + holds)).reshape(-1, 4)
        off = np.ascontiguousarray(ints(off, "the offsets"), dtype=np.uint64).reshape(-1)
        if strict and off.shape[0] == 0:
            raise ValueError("%soffsets need n_%ss + 1 entries" % (prefix, noun))
        lens = off[1:].astype(np.int64) - off[:-1].astype(np.int64)
        if (lens < 0).any():
            raise ValueError("%soffsets decrease at %s %d" % (prefix, noun, int(np.argmax(lens < 0))))
        _offsets_fit(prefix, off, flat, holds)
    else:
        parts = [_as_scalars(ints(m, "%s %d" % (noun, i))).reshape(-1, 4) for i, m in enumerate(items)]
        lens = np.array([p.shape[0] for p in parts], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        flat = np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), dtype=np.uint64)
    if (lens == 0).any():
        raise empty[0]("%s%s %d is empty" % (empty[1], noun, int(np.argmax(lens == 0))))
    return flat, off, lens


class Context:
    """One `p252_ctx`: bound to one HIP device (one process per GPU)."""

    _default = {}

    def __init__(self, device=0):
        L = _lib.lib()
        h = ctypes.c_void_p()
        rc = L.p252_create(int(device), ctypes.byref(h))
        if rc:
            raise DeviceError("p252_create(device=%d) failed (%d): %s" % (device, rc, L.p252_last_error(None).decode()))
        self._h = h
        self.device = int(device)

    @classmethod
    def default(cls, device=None):
        if device is None:
            device = 0
            try:
                import torch
                if torch.cuda.is_available():
                    device = torch.cuda.current_device()
            except ImportError:
                pass
        if device not in cls._default:
            cls._default[device] = cls(device)
        return cls._default[device]

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().p252_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            _raise(rc, self._h)

    # ---- host buffers ----
    def permute_batch(self, states):
        """n x [BlsScalar; 5] -> n permuted states (Safe::permute, scalar.rs:25-27)."""
        s = _as_scalars(states).reshape(-1, 5, 4)
        out = np.empty_like(s)
        self._check(_lib.lib().p252_permute_batch(self._h, _ptr(s), _ptr(out), s.shape[0]))
        return out

    def sync(self, stream=None):
        """wait for `stream` (a torch stream; default: the current one) — p252_sync; raises DeviceError if a sharded tree build of this
        context's communicator met a failed peer since the last check (comm.Comm.check)"""
        self._check(_lib.lib().p252_sync(self._h, stream.cuda_stream if stream is not None else _stream(self)))

    def wipe(self):
        """clear every scratch buffer the context owns (p252_wipe: device scratch, level scratch, staging lanes).  The host-buffer
        encrypt / decrypt calls and close() do this themselves (the reference builds with `zeroize`, Cargo.toml:14)."""
        self._check(_lib.lib().p252_wipe(self._h))

    def trim(self):
        """give the grow-only scratch back (p252_trim: waits for the device, wipes, frees; the next call allocates again) — the
        reference holds no state at all (hash.rs:92-96)"""
        self._check(_lib.lib().p252_trim(self._h))

    def scratch_residue(self):
        """diagnostics: non-zero bytes in the context's scratch buffers (p252_scratch_residue)"""
        n = ctypes.c_uint64(0)
        self._check(_lib.lib().p252_scratch_residue(self._h, ctypes.byref(n)))
        return int(n.value)

    def hash_batch(self, tag, messages, in_len, out_len, out=None, truncated=False):
        """truncated=True: Hash::finalize_truncated's raw limbs (hash.rs:164-183), produced by the digest kernel's output stage"""
        m = _as_scalars(messages)
        if in_len <= 0:
            self._check(_lib.ERR_INVALID_IO_PATTERN)
        m = m.reshape(-1, in_len, 4)
        if out is None:
            out = np.empty((m.shape[0], max(out_len, 0), 4), dtype=np.uint64)
        else:  # caller-provided (e.g. pinned) output buffer
            out = _host_out("hash_batch", out, m.shape[0] * out_len).reshape(m.shape[0], out_len, 4)
        fn = _lib.lib().p252_hash_batch_truncated if truncated else _lib.lib().p252_hash_batch
        self._check(fn(self._h, _tag(tag), _ptr(m), in_len, out_len, _ptr(out), m.shape[0]))
        return out

    def hash_ragged(self, tags, flat, offsets, out_len, truncated=False):
        """n messages of different lengths (p252_hash_ragged[_truncated]): message i = flat[offsets[i]:offsets[i+1]], tags[L-1] = the
        tag of a message of length L (max_len = len(tags)).  Host numpy buffers -> (n, out_len, 4); the library checks every length
        (zero -> InvalidIOPattern; decreasing offsets or a length above max_len -> ValueError) before it launches anything."""
        t = _as_scalars(tags).reshape(-1, 4)
        x = _as_scalars(flat).reshape(-1, 4)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        n = max(off.shape[0] - 1, 0)
        if n:
            _offsets_fit("hash_ragged: ", off, x, "scalars")
        out = np.empty((n, max(out_len, 0), 4), dtype=np.uint64)
        fn = _lib.lib().p252_hash_ragged_truncated if truncated else _lib.lib().p252_hash_ragged
        self._check(fn(self._h, _ptr(t), t.shape[0], _ptr(x), _ptr(off), out_len, _ptr(out), n))
        return out

    def crypt_ragged(self, decrypt, variant, tags, flat, offsets, secrets, nonces):
        """n messages of different lengths encrypted or decrypted from host buffers (p252_{encrypt,decrypt}_ragged): offsets are the
        n + 1 MESSAGE offsets in both directions; message i = messages[offsets[i]:offsets[i+1]], its cipher the L_i + 1 scalars at
        ciphers[offsets[i] + i:].  tags[L-1] = the tag of a message of length L (max_len = len(tags)).  flat = the messages
        (encrypt) or the ciphers (decrypt) -> the other side, and the (n,) uint8 flags on decrypt.  The library checks every length
        before it launches anything and clears its copies of what it was handed before it returns."""
        f = "decrypt_ragged" if decrypt else "encrypt_ragged"
        t = _as_scalars(tags).reshape(-1, 4)
        x = _as_scalars(flat).reshape(-1, 4)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        n = max(off.shape[0] - 1, 0)
        sec = _as_scalars(secrets).reshape(-1, 2, 4)
        non = _as_scalars(nonces).reshape(-1, 4)
        if sec.shape[0] != n or non.shape[0] != n:
            raise ValueError("%s: %d messages, %d secrets, %d nonces" % (f, n, sec.shape[0], non.shape[0]))
        total = int(off[-1]) if n else 0
        if n and total + (n if decrypt else 0) > x.shape[0]:
            raise ValueError("%s: offsets reach past the %d scalars given" % (f, x.shape[0]))
        out = np.empty((total + (0 if decrypt else n), 4), dtype=np.uint64)
        if decrypt:
            ok = np.zeros(n, dtype=np.uint8)
            self._check(_lib.lib().p252_decrypt_ragged(self._h, int(variant), _ptr(t), t.shape[0], _ptr(x), _ptr(off), _ptr(sec), _ptr(non),
                                                       _ptr(out), _ptr(ok, _lib._u8p), n))
            return out, ok
        self._check(_lib.lib().p252_encrypt_ragged(self._h, int(variant), _ptr(t), t.shape[0], _ptr(x), _ptr(off), _ptr(sec), _ptr(non),
                                                   _ptr(out), n))
        return out

    def merkle4_tree(self, tag, leaves, want_levels=False):
        return self._tree(_ARITIES[4], tag, leaves, want_levels)

    def merkle2_tree(self, tag, leaves, want_levels=False):
        """arity-2 tree over Hash::digest(Domain::Merkle2, [c0, c1]) nodes (hash.rs:27-31)"""
        return self._tree(_ARITIES[2], tag, leaves, want_levels)

    def _tree(self, a, tag, leaves, want_levels):
        lv = _as_scalars(leaves).reshape(-1, 4)
        root = np.empty(4, dtype=np.uint64)
        levels = np.empty((a.levels_len(lv.shape[0]), 4), dtype=np.uint64) if want_levels else None
        self._check(a.fn("tree")(self._h, _tag(tag), _ptr(lv), lv.shape[0], _ptr(root), _ptr(levels) if want_levels else None))
        return (root, levels) if want_levels else root

    # ---- device buffers (torch CUDA tensors on the context's device; asynchronous on torch's current stream there) ----
    def permute_batch_device(self, d_states, d_out, n):
        f = "permute_batch_device"
        self._check(_lib.lib().p252_permute_batch_device(self._h, _dev_ptr(self, f, "d_states", d_states, n * 160),
                                                         _dev_ptr(self, f, "d_out", d_out, n * 160), n, _stream(self)))

    def hash_batch_device(self, tag, d_in, in_len, out_len, d_out, n, truncated=False):
        """truncated=True: p252_hash_batch_truncated_device — finalize_truncated's raw limbs from the SAME launch (hash.rs:164-183)"""
        f = "hash_batch_device"
        fn = _lib.lib().p252_hash_batch_truncated_device if truncated else _lib.lib().p252_hash_batch_device
        self._check(fn(self._h, _tag(tag), _dev_ptr(self, f, "d_in", d_in, n * in_len * 32), in_len, out_len,
                       _dev_ptr(self, f, "d_out", d_out, n * out_len * 32), n, _stream(self)))

    def hash_ragged_device(self, d_tags, max_len, d_in, d_offsets, out_len, d_out, n, d_n_bad=None, truncated=False):
        """p252_hash_ragged[_truncated]_device on torch's current stream: d_offsets = n + 1 int64/uint64 scalar indices, d_tags =
        max_len scalars (tags[L-1] for length L), d_out (n, out_len, 4).  Bad messages (empty, longer than max_len, decreasing
        offsets) get zero rows and increment d_n_bad (a zeroed device int32/uint32, optional) — nothing is checked on the host
        (so the extent of d_in, which the offsets give, is not checked either)."""
        f = "hash_ragged_device"
        fn = _lib.lib().p252_hash_ragged_truncated_device if truncated else _lib.lib().p252_hash_ragged_device
        self._check(fn(self._h, _dev_ptr(self, f, "d_tags", d_tags, max_len * 32), max_len, _dev_ptr(self, f, "d_in", d_in, 0),
                       _dev_ptr(self, f, "d_offsets", d_offsets, (n + 1) * 8, elem=8), out_len,
                       _dev_ptr(self, f, "d_out", d_out, n * out_len * 32), n,
                       _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def encrypt_ragged_device(self, variant, d_tags, max_len, d_messages, n_scalars, d_offsets, d_secrets, d_nonces, d_ciphers, n, d_n_bad=None):
        """p252_encrypt_ragged_device_into on torch's current stream: d_offsets = n + 1 int64/uint64 MESSAGE offsets, d_tags = max_len
        scalars (tags[L-1] for length L), d_messages n_scalars scalars, d_ciphers n_scalars + n (the cipher of message i at
        offsets[i] + i).  A bad message (empty, longer than max_len, decreasing offsets, an end past n_scalars) leaves its output
        untouched and increments d_n_bad (a zeroed device int32/uint32, optional); nothing is checked on the host."""
        f = "encrypt_ragged_device"
        self._check(_lib.lib().p252_encrypt_ragged_device_into(
            self._h, int(variant), _dev_ptr(self, f, "d_tags", d_tags, max_len * 32), max_len,
            _dev_ptr(self, f, "d_messages", d_messages, n_scalars * 32), n_scalars, _dev_ptr(self, f, "d_offsets", d_offsets, (n + 1) * 8, elem=8),
            _dev_ptr(self, f, "d_secrets", d_secrets, n * 64), _dev_ptr(self, f, "d_nonces", d_nonces, n * 32),
            _dev_ptr(self, f, "d_ciphers", d_ciphers, (n_scalars + n) * 32), n, _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True),
            _stream(self)))

    def decrypt_ragged_device(self, variant, d_tags, max_len, d_ciphers, n_scalars, d_offsets, d_secrets, d_nonces, d_messages, d_ok, n,
                              d_n_bad=None):
        """p252_decrypt_ragged_device_into: the layout of encrypt_ragged_device read the other way; d_ok = n uint8 flags (1 = the MAC
        verified; 0 = DecryptionFailed with that message unspecified, or a bad message, whose output is untouched)"""
        f = "decrypt_ragged_device"
        self._check(_lib.lib().p252_decrypt_ragged_device_into(
            self._h, int(variant), _dev_ptr(self, f, "d_tags", d_tags, max_len * 32), max_len,
            _dev_ptr(self, f, "d_ciphers", d_ciphers, (n_scalars + n) * 32), n_scalars, _dev_ptr(self, f, "d_offsets", d_offsets, (n + 1) * 8, elem=8),
            _dev_ptr(self, f, "d_secrets", d_secrets, n * 64), _dev_ptr(self, f, "d_nonces", d_nonces, n * 32),
            _dev_ptr(self, f, "d_messages", d_messages, n_scalars * 32), _dev_ptr(self, f, "d_ok", d_ok, n, elem=1), n,
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def merkle4_tree_device(self, tag, d_leaves, n_leaves, d_root, d_levels=None):
        f = "merkle4_tree_device"
        L = _lib.lib()
        levels = L.p252_merkle4_levels_len(n_leaves) * 32 if d_levels is not None else 0
        self._check(L.p252_merkle4_tree_device(self._h, _tag(tag), _dev_ptr(self, f, "d_leaves", d_leaves, n_leaves * 32), n_leaves,
                                               _dev_ptr(self, f, "d_root", d_root, 32),
                                               _dev_ptr(self, f, "d_levels", d_levels, levels, null_ok=True), _stream(self)))

    def merkle4_forest(self, tag, leaves, leaves_per_tree):
        """host leaves (numpy, pageable is fine) -> roots (n_trees, 4) numpy: p252_merkle4_forest hashes the first level while the
        leaves stream in through the staging lanes, then the upper levels once across all trees"""
        lv = _as_scalars(leaves).reshape(-1, 4)
        if leaves_per_tree < 1 or lv.shape[0] % leaves_per_tree:
            raise ValueError("forest: %d leaves are not a whole number of %d-leaf trees" % (lv.shape[0], leaves_per_tree))
        n_trees = lv.shape[0] // leaves_per_tree
        roots = np.empty((n_trees, 4), dtype=np.uint64)
        self._check(_lib.lib().p252_merkle4_forest(self._h, _tag(tag), _ptr(lv), n_trees, leaves_per_tree, _ptr(roots)))
        return roots

    def merkle4_forest_device(self, tag, d_leaves, n_trees, leaves_per_tree, d_roots, d_levels=None, arity=4):
        """n_trees independent complete 4^k-leaf trees, tree-major in d_leaves: one launch per level across ALL trees
        (p252_merkle4_forest_device); d_roots (n_trees, 4); d_levels: level-major, n_trees * levels_len(leaves_per_tree) scalars"""
        f = "merkle4_forest_device"
        a = _arity(f, arity)
        levels = n_trees * a.levels_len(leaves_per_tree) * 32 if d_levels is not None else 0
        fn = a.fn("forest_device")
        self._check(fn(self._h, _tag(tag), _dev_ptr(self, f, "d_leaves", d_leaves, n_trees * leaves_per_tree * 32), n_trees, leaves_per_tree,
                       _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32), _dev_ptr(self, f, "d_levels", d_levels, levels, null_ok=True),
                       _stream(self)))

    def merkle_forest_ragged(self, tag, flat, offsets, arity=4, want_levels=False):
        """trees of different sizes from host buffers (p252_merkle{4,2}_forest_ragged): tree t = flat[offsets[t]:offsets[t+1]].
        Returns roots (n_trees, 4) and, with want_levels, the tree-major levels (sum of levels_len(n_t) scalars).  The library
        checks every tree first (empty, decreasing offsets -> ValueError)."""
        a = _arity("merkle_forest_ragged", arity)
        x = _as_scalars(flat).reshape(-1, 4)
        off = np.ascontiguousarray(offsets, dtype=np.uint64).reshape(-1)
        n = max(off.shape[0] - 1, 0)
        if n:
            _offsets_fit("merkle_forest_ragged: ", off, x, "scalars")
        lens = off[1:].astype(np.int64) - off[:-1].astype(np.int64)
        n_levels = sum(a.levels_len(int(c)) for c in lens if c > 0) if want_levels else 0
        roots = np.empty((n, 4), dtype=np.uint64)
        levels = np.empty((n_levels, 4), dtype=np.uint64) if want_levels else None
        self._check(a.fn("forest_ragged")(self._h, _tag(tag), _ptr(x), _ptr(off), n, _ptr(roots), _ptr(levels) if n_levels else None))
        return (roots, levels) if want_levels else roots

    def merkle_forest_ragged_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_roots, d_levels=None, d_n_bad=None, arity=4):
        """p252_merkle{4,2}_forest_ragged_device on torch's current stream: tree t = d_leaves[d_offsets[t]:d_offsets[t+1]]
        (d_offsets: n_trees + 1 int64/uint64 scalar indices; n_leaves = the scalars d_leaves holds).  d_roots (n_trees, 4);
        d_levels (tree-major) must hold the bound n_leaves // (arity - 1) + n_trees * depth(max_leaves) scalars, as the offsets
        are never read back to the host.  Bad trees get zero roots and increment d_n_bad (a zeroed device int32/uint32,
        optional)."""
        f = "merkle_forest_ragged_device"
        a = _arity(f, arity)
        leaves = _dev_ptr(self, f, "d_leaves", d_leaves, 0)
        n_leaves = _n_scalars(d_leaves)
        need = a.forest_levels_bytes(n_leaves, n_trees, a.depth(max_leaves)) if d_levels is not None else 0
        fn = a.fn("forest_ragged_device")
        self._check(fn(self._h, _tag(tag), leaves, n_leaves, _dev_ptr(self, f, "d_offsets", d_offsets, (n_trees + 1) * 8, elem=8),
                       n_trees, max_leaves, _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32),
                       _dev_ptr(self, f, "d_levels", d_levels, need, null_ok=True),
                       _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def _built_forest(self, f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels):
        """the six leading C arguments of a call that takes a forest merkle_forest_ragged_device built with d_levels (leaves, n_leaves,
        offsets, n_trees, max_leaves, levels), and depth(max_leaves): d_levels must hold the build's bound, None only at depth 0"""
        leaves = _dev_ptr(self, f, "d_leaves", d_leaves, 32)
        n_leaves = _n_scalars(d_leaves)
        depth = a.depth(max_leaves)
        offsets = _dev_ptr(self, f, "d_offsets", d_offsets, (n_trees + 1) * 8, elem=8)
        levels = _dev_ptr(self, f, "d_levels", d_levels, a.forest_levels_bytes(n_leaves, n_trees, depth), null_ok=depth == 0)
        return (leaves, n_leaves, offsets, n_trees, max_leaves, levels), depth

    def merkle_forest_ragged_openings_device(self, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, k,
                                             out=None, d_n_bad=None, arity=4):
        """openings out of a forest merkle_forest_ragged_device built with d_levels (p252_merkle{4,2}_forest_ragged_openings_device):
        opening i = leaf d_leaf_ids[i] (int64/uint64, a position inside the tree) of tree d_tree_ids[i] (int32/uint32); d_leaves,
        d_offsets, n_trees, max_leaves, d_levels exactly as the build took them.  Returns (d_leaves_out (k,4), d_siblings
        (k,D,arity-1,4), d_positions (k,D) uint8, d_depths (k,) uint8, D) with D = depth(max_leaves); rows at or past d_depths[i]
        are zero, a bad opening is all zero with depth 0xFF and counted in d_n_bad (a zeroed device int32/uint32, optional).
        out = (d_leaves_out, d_siblings, d_positions, d_depths) writes into caller-owned tensors (no allocation per call)."""
        import torch
        f = "merkle_forest_ragged_openings_device"
        a = _arity(f, arity)
        forest, depth = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
        tree_ids = _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4)
        leaf_ids = _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8)
        if out is not None:
            lv, sib, pos, dep = out
        else:
            dev = d_leaves.device
            lv = torch.empty((k, 4), dtype=torch.int64, device=dev)
            sib = torch.empty((k, depth, a.per, 4), dtype=torch.int64, device=dev)
            pos = torch.empty((k, depth), dtype=torch.uint8, device=dev)
            dep = torch.empty((k,), dtype=torch.uint8, device=dev)
        self._check(a.fn("forest_ragged_openings_device")(
            self._h, *forest, tree_ids, leaf_ids, k,
            _dev_ptr(self, f, "d_leaves_out", lv, k * 32), _dev_ptr(self, f, "d_siblings", sib, k * depth * 32 * a.per) if depth else None,
            _dev_ptr(self, f, "d_positions", pos, k * depth, elem=1) if depth else None, _dev_ptr(self, f, "d_depths", dep, k, elem=1),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))
        return lv, sib, pos, dep, depth

    def _ragged_opening_ptrs(self, f, a, d_leaves, d_siblings, d_positions, d_depths, stride_depth, k):
        if not 0 <= stride_depth <= 64:
            raise ValueError("%s: stride_depth must be in 0 .. 64, not %r" % (f, stride_depth))
        return (_dev_ptr(self, f, "d_leaves", d_leaves, k * 32),
                _dev_ptr(self, f, "d_siblings", d_siblings, k * stride_depth * a.per * 32) if stride_depth else None,
                _dev_ptr(self, f, "d_positions", d_positions, k * stride_depth, elem=1) if stride_depth else None,
                _dev_ptr(self, f, "d_depths", d_depths, k, elem=1))

    def merkle_path_ragged_device(self, tag, d_leaves, d_siblings, d_positions, d_depths, stride_depth, d_roots, k, d_n_bad=None, arity=4):
        """re-hash of k openings of DIFFERENT depths (p252_merkle{4,2}_path_ragged_device): d_roots[i] from the first d_depths[i]
        (uint8) levels of opening i in the layout merkle_forest_ragged_openings_device writes, at stride stride_depth.  A depth
        above the stride (0xFF: a bad opening) gives a zero root and is counted in d_n_bad (zeroed device int32/uint32, optional)."""
        f = "merkle_path_ragged_device"
        a = _arity(f, arity)
        leaves, sib, pos, dep = self._ragged_opening_ptrs(f, a, d_leaves, d_siblings, d_positions, d_depths, stride_depth, k)
        fn = a.fn("path_ragged_device")
        self._check(fn(self._h, _tag(tag), leaves, sib, pos, dep, stride_depth, _dev_ptr(self, f, "d_roots", d_roots, k * 32), k,
                       _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def merkle_forest_ragged_verify_device(self, tag, d_leaves, d_siblings, d_positions, d_depths, stride_depth, d_tree_ids, d_roots,
                                           n_trees, d_ok, k, arity=4):
        """`Opening::verify` across a forest (p252_merkle{4,2}_forest_ragged_verify_device): d_ok[i] (uint8) = 1 iff opening i is
        well-formed and re-hashes to d_roots[d_tree_ids[i]], the root of ITS tree; k bytes come back"""
        f = "merkle_forest_ragged_verify_device"
        a = _arity(f, arity)
        leaves, sib, pos, dep = self._ragged_opening_ptrs(f, a, d_leaves, d_siblings, d_positions, d_depths, stride_depth, k)
        fn = a.fn("forest_ragged_verify_device")
        self._check(fn(self._h, _tag(tag), leaves, sib, pos, dep, stride_depth, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4),
                       _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32, null_ok=n_trees == 0), n_trees,
                       _dev_ptr(self, f, "d_ok", d_ok, k, elem=1), k, _stream(self)))

    def merkle_forest_ragged_update_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids,
                                           d_new_leaves, k, d_roots=None, d_n_bad=None, d_n_hashed=None, arity=4):
        """k leaf updates anywhere in a forest merkle_forest_ragged_device built with d_levels, in one call
        (p252_merkle{4,2}_forest_ragged_update_device): update i writes d_new_leaves[i] to leaf d_leaf_ids[i] (int64/uint64, a position
        inside the tree) of tree d_tree_ids[i] (int32/uint32), then every dirty ancestor is re-hashed ONCE, in place; d_leaves,
        d_offsets, n_trees, max_leaves, d_levels exactly as the build took them.  d_roots (n_trees, 4; optional) is rewritten for
        the touched trees only.  A bad update writes nothing and is counted in d_n_bad (a zeroed device int32/uint32, optional);
        d_n_hashed (a zeroed device int64/uint64, optional) grows by the number of digests computed."""
        f = "merkle_forest_ragged_update_device"
        a = _arity(f, arity)
        forest, _ = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
        self._check(a.fn("forest_ragged_update_device")(
            self._h, _tag(tag), *forest, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4),
            _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8),
            _dev_ptr(self, f, "d_new_leaves", d_new_leaves, k * 32), k, _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32, null_ok=True),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True), _stream(self)))

    # ---- the update with a journal, and the swap that undoes and redoes it (p252_merkle{4,2}_forest_ragged_journal_*, _update_journaled_device_into;
    # csrc/forest_journal.hip) ----
    def merkle_forest_ragged_journal_bound(self, n_leaves, n_trees, max_leaves, k, arity=4):
        """the most journal entries one journaled update of k leaves writes (p252_merkle{4,2}_forest_ragged_journal_bound): the capacity
        merkle_forest_ragged_update_journaled_device asks of its journal"""
        return int(_arity("merkle_forest_ragged_journal_bound", arity).fn("forest_ragged_journal_bound")(n_leaves, n_trees, max_leaves, k))

    def merkle_forest_ragged_update_journaled_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids,
                                                     d_new_leaves, k, d_journal_ids, d_journal_values, journal_cap, d_journal_len,
                                                     d_roots=None, d_n_bad=None, d_n_hashed=None, arity=4):
        """merkle_forest_ragged_update_device keeping a journal of every leaf and node it overwrites
        (p252_merkle{4,2}_forest_ragged_update_journaled_device_into; pass the tag of that arity): the update's arguments with its
        meaning, except that of a (tree, leaf) pair given several times exactly one update is applied, whole, and the others are dropped
        without a count.  The journal is the caller's: d_journal_ids (journal_cap x 4 int32/uint32), d_journal_values (journal_cap
        scalars), d_journal_len (one device int64/uint64, set by the call); journal_cap >= merkle_forest_ragged_journal_bound(..), else
        the library refuses the call.  merkle_forest_ragged_journal_swap_device plays it back."""
        f = "merkle_forest_ragged_update_journaled_device"
        a = _arity(f, arity)
        forest, _ = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
        self._check(a.fn("forest_ragged_update_journaled_device_into")(
            self._h, _tag(tag), *forest, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4),
            _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8),
            _dev_ptr(self, f, "d_new_leaves", d_new_leaves, k * 32), k, _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32, null_ok=True),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True),
            _dev_ptr(self, f, "d_journal_ids", d_journal_ids, journal_cap * 16, elem=4, null_ok=journal_cap == 0),
            _dev_ptr(self, f, "d_journal_values", d_journal_values, journal_cap * 32, null_ok=journal_cap == 0), journal_cap,
            _dev_ptr(self, f, "d_journal_len", d_journal_len, 8, elem=8), _stream(self)))

    def merkle_forest_ragged_journal_swap_device(self, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_journal_ids, d_journal_values,
                                                 journal_cap, d_journal_len, d_roots=None, d_n_bad=None, arity=4):
        """the journal of merkle_forest_ragged_update_journaled_device played back (p252_merkle{4,2}_forest_ragged_journal_swap_device_into;
        no tag, nothing is hashed): each of the first min(d_journal_len, journal_cap) entries changes places with the node it names, so
        one call undoes the update byte for byte and a second one redoes it; d_roots (n_trees, 4; optional) follows for the touched
        trees.  The forest arguments exactly as the update took them — a journal is void on any other shape.  An entry that names no
        node of this forest writes nothing and is counted in d_n_bad (a zeroed device int32/uint32, optional)."""
        f = "merkle_forest_ragged_journal_swap_device"
        a = _arity(f, arity)
        forest, _ = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
        self._check(a.fn("forest_ragged_journal_swap_device_into")(
            self._h, *forest, _dev_ptr(self, f, "d_journal_ids", d_journal_ids, journal_cap * 16, elem=4, null_ok=journal_cap == 0),
            _dev_ptr(self, f, "d_journal_values", d_journal_values, journal_cap * 32, null_ok=journal_cap == 0), journal_cap,
            _dev_ptr(self, f, "d_journal_len", d_journal_len, 8, elem=8), _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32, null_ok=True),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def merkle_forest_ragged_append_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_add, d_add_offsets, n_trees_new,
                                           max_leaves_new, d_leaves_new, d_offsets_new, d_levels_new, d_roots, d_n_bad=None, d_n_hashed=None,
                                           arity=4):
        """leaves appended to the trees of a forest merkle_forest_ragged_device built with d_levels, written INTO a new compact forest
        (p252_merkle{4,2}_forest_ragged_append_device_into; pass the tag of that arity): d_leaves, d_offsets, n_trees, max_leaves, d_levels
        exactly as the build took them (read-only; None when n_trees == 0); tree t of the n_trees_new >= n_trees new trees receives
        d_add[d_add_offsets[t]:d_add_offsets[t+1]] (n_trees_new + 1 int64/uint64; d_add None: a compaction copy).  Written: d_leaves_new
        (its length is the capacity, at least the old leaves plus d_add), d_offsets_new (n_trees_new + 1), d_levels_new (the bound of
        merkle_forest_ragged_device for the new shape), d_roots (n_trees_new, 4) — byte for byte a fresh build of the new forest,
        with the unchanged nodes moved and only the others hashed.  A refused append or an empty new tree is counted in d_n_bad (a
        zeroed device int32/uint32, optional); d_n_hashed (a zeroed device int64/uint64, optional) receives the digests computed."""
        self._forest_ragged_regrow("merkle_forest_ragged_append_device", arity, False, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels,
                                   None, d_add, d_add_offsets, n_trees_new, max_leaves_new, d_leaves_new, d_offsets_new, d_levels_new, d_roots,
                                   d_n_bad, d_n_hashed)

    def merkle_forest_ragged_resize_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add, d_add_offsets,
                                           n_trees_new, max_leaves_new, d_leaves_new, d_offsets_new, d_levels_new, d_roots, d_n_bad=None,
                                           d_n_hashed=None, arity=4):
        """such a forest rolled back and forward in one call (p252_merkle{4,2}_forest_ragged_resize_device_into; pass the tag of that
        arity): the append above after tree t was cut to its first min(d_keep[t], n_t) leaves.  d_keep = n_trees_new int64/uint64 on the
        device (-1, i.e. UINT64_MAX, or any value >= n_t keeps the tree whole; None keeps every tree whole).  n_trees_new may be smaller
        than n_trees: the trailing trees are dropped.  d_add None: a pure rollback, at most one node per tree and level hashed.  A refused
        append still leaves its tree cut.  Everything else, the sizes of the outputs included, as merkle_forest_ragged_append_device."""
        self._forest_ragged_regrow("merkle_forest_ragged_resize_device", arity, True, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels,
                                   d_keep, d_add, d_add_offsets, n_trees_new, max_leaves_new, d_leaves_new, d_offsets_new, d_levels_new, d_roots,
                                   d_n_bad, d_n_hashed)

    def _forest_ragged_regrow(self, f, arity, resize, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_keep, d_add, d_add_offsets,
                              n_trees_new, max_leaves_new, d_leaves_new, d_offsets_new, d_levels_new, d_roots, d_n_bad, d_n_hashed):
        """the append and the resize: one set of checks; the resize's C call takes d_keep after d_levels"""
        a = _arity(f, arity)
        stem = "forest_ragged_resize_device_into" if resize else "forest_ragged_append_device_into"
        keep = (_dev_ptr(self, f, "d_keep", d_keep, n_trees_new * 8, elem=8, null_ok=True),) if resize else ()
        none = n_trees == 0  # no old forest
        leaves = _dev_ptr(self, f, "d_leaves", d_leaves, 0, null_ok=none)
        n_leaves = _n_scalars(d_leaves) if d_leaves is not None else 0
        add = _dev_ptr(self, f, "d_add", d_add, 0, null_ok=True)
        n_add = _n_scalars(d_add) if d_add is not None else 0
        depth, depth_new = a.depth(max_leaves) if not none else 0, a.depth(max_leaves_new)
        leaves_new = _dev_ptr(self, f, "d_leaves_new", d_leaves_new, (n_leaves + n_add) * 32, null_ok=n_leaves + n_add == 0)
        levels_need = a.forest_levels_bytes(n_leaves + n_add, n_trees_new, depth_new)
        levels_new = _dev_ptr(self, f, "d_levels_new", d_levels_new, levels_need, null_ok=depth_new == 0)
        self._check(a.fn(stem)(
            self._h, _tag(tag), leaves, n_leaves, _dev_ptr(self, f, "d_offsets", d_offsets, (n_trees + 1) * 8, elem=8, null_ok=none), n_trees,
            max_leaves, _dev_ptr(self, f, "d_levels", d_levels, a.forest_levels_bytes(n_leaves, n_trees, depth), null_ok=depth == 0),
            *keep, add, n_add, _dev_ptr(self, f, "d_add_offsets", d_add_offsets, (n_trees_new + 1) * 8, elem=8), n_trees_new, max_leaves_new,
            leaves_new, _n_scalars(d_leaves_new) if d_leaves_new is not None else 0,
            _dev_ptr(self, f, "d_offsets_new", d_offsets_new, (n_trees_new + 1) * 8, elem=8),
            levels_new, _n_scalars(d_levels_new) if d_levels_new is not None else levels_need // 32,  # (no level: nothing is written)
            _dev_ptr(self, f, "d_roots", d_roots, n_trees_new * 32), _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True), _stream(self)))

    def merkle_forest_ragged_select_device(self, forest_a, forest_b, d_pick, n_pick, d_leaves_new, d_offsets_new, d_levels_new, d_roots_new,
                                           d_n_bad=None, arity=4):
        """any trees of one or two built forests gathered INTO a new compact forest, with no digest
        (p252_merkle{4,2}_forest_ragged_select_device_into; arity 2: the level layout of merkle2 trees).  forest_a, forest_b =
        (d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_roots), each exactly what merkle_forest_ragged_device took and filled
        (read-only); forest_b may be None.  d_pick = n_pick int64/uint64 ids on the device: below n_trees_a a tree of A, then a tree of B;
        any order, repeats allowed.  Written: d_leaves_new (its length is leaves_cap), d_offsets_new (n_pick + 1), d_levels_new (at least
        the bound of merkle_forest_ragged_device for leaves_cap leaves, n_pick trees and the larger max_leaves), d_roots_new (n_pick, 4)
        — byte for byte a fresh build of the new forest.  A pick out of range, of a bad tree, or past leaves_cap (and every non-empty
        one after it) becomes an empty tree and is counted in d_n_bad (a zeroed device int32/uint32, optional)."""
        f = "merkle_forest_ragged_select_device"
        a = _arity(f, arity)

        def source(which, forest):
            """the seven C arguments of one source forest, and its byte ranges"""
            if forest is None:
                return (None, 0, None, 0, 0, None, None), 0, []
            if len(forest) != 6:
                raise ValueError("%s: forest_%s must be (d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_roots)" % (f, which))
            d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_roots = forest
            if n_trees <= 0 or max_leaves <= 0:
                raise ValueError("%s: forest_%s needs n_trees and max_leaves > 0" % (f, which))
            leaves = _dev_ptr(self, f, "d_leaves_" + which, d_leaves, 32)
            n_leaves = _n_scalars(d_leaves)
            depth = a.depth(max_leaves)
            sizes = ((n_trees + 1) * 8, a.forest_levels_bytes(n_leaves, n_trees, depth), n_trees * 32)
            ptrs = (leaves, n_leaves, _dev_ptr(self, f, "d_offsets_" + which, d_offsets, sizes[0], elem=8), n_trees, max_leaves,
                    _dev_ptr(self, f, "d_levels_" + which, d_levels, sizes[1], null_ok=depth == 0),
                    _dev_ptr(self, f, "d_roots_" + which, d_roots, sizes[2]))
            ranges = [("d_leaves_" + which, leaves, n_leaves * 32), ("d_offsets_" + which, ptrs[2], sizes[0]),
                      ("d_levels_" + which, ptrs[5], sizes[1]), ("d_roots_" + which, ptrs[6], sizes[2])]
            return ptrs, max_leaves, ranges

        if forest_a is None:
            raise ValueError("%s: forest_a is required" % f)
        args_a, max_a, in_a = source("a", forest_a)
        args_b, max_b, in_b = source("b", forest_b)
        if n_pick < 0:
            raise ValueError("%s: n_pick must be >= 0" % f)
        pick = _dev_ptr(self, f, "d_pick", d_pick, n_pick * 8, elem=8, null_ok=n_pick == 0)
        depth = a.depth(max(max_a, max_b))
        leaves_new = _dev_ptr(self, f, "d_leaves_new", d_leaves_new, 32)
        leaves_cap = _n_scalars(d_leaves_new)
        levels_need = a.forest_levels_bytes(leaves_cap, n_pick, depth)
        levels_new = _dev_ptr(self, f, "d_levels_new", d_levels_new, levels_need, null_ok=depth == 0)
        levels_cap = _n_scalars(d_levels_new) if d_levels_new is not None else levels_need // 32  # (no level: nothing is written)
        offsets_new = _dev_ptr(self, f, "d_offsets_new", d_offsets_new, (n_pick + 1) * 8, elem=8)
        roots_new = _dev_ptr(self, f, "d_roots_new", d_roots_new, n_pick * 32)
        n_bad = _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True)
        # no output may overlap an input or another output (the library refuses it too: all sizes are known here)
        outs = [("d_leaves_new", leaves_new, leaves_cap * 32), ("d_offsets_new", offsets_new, (n_pick + 1) * 8),
                ("d_levels_new", levels_new, levels_cap * 32), ("d_roots_new", roots_new, n_pick * 32), ("d_n_bad", n_bad, 4)]
        ins = in_a + in_b + [("d_pick", pick, n_pick * 8)]
        for i, (name, p, size) in enumerate(outs):
            for other, q, size_q in ins + outs[:i]:
                if p and q and size and size_q and p < q + size_q and q < p + size:
                    raise ValueError("%s: %s overlaps %s" % (f, name, other))
        self._check(a.fn("forest_ragged_select_device_into")(self._h, *args_a, *args_b, pick, n_pick, leaves_new, leaves_cap, offsets_new,
                                                             levels_new, levels_cap, roots_new, n_bad, _stream(self)))

    # ---- the order and the distinct (tree id, leaf id) pairs that the sequential updates and the shared proofs take (csrc/pairs.hip) ----
    def pairs_order_device(self, d_tree_ids, d_leaf_ids, k, d_order, stream=None):
        """d_order (k,) int32/uint32 = the indices 0 .. k - 1 sorted by (tree id, leaf id, index): the stable sort by pair, on the
        device (p252_pairs_order_device_into) — what merkle{4,2}_forest_ragged_update_sequential_device takes.  d_leaf_ids (k,)
        int64/uint64; d_tree_ids (k,) int32/uint32, or None: every pair is of tree 0.  Both parts compare as unsigned.  Asynchronous
        on `stream` (a torch stream; default the current one), no synchronisation: the call can be captured into a graph."""
        f = "pairs_order_device"
        self._check(_lib.lib().p252_pairs_order_device_into(
            self._h, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8), k, _dev_ptr(self, f, "d_order", d_order, k * 4, elem=4),
            stream.cuda_stream if stream is not None else _stream(self)))

    def pairs_unique_device(self, d_tree_ids, d_leaf_ids, k, d_n_unique, d_tree_ids_out=None, d_leaf_ids_out=None, d_indices_out=None,
                            d_first=None, stream=None):
        """the distinct pairs of (d_tree_ids, d_leaf_ids), ascending, into the first d_n_unique[0] entries of every output given
        (p252_pairs_unique_device_into): d_tree_ids_out (k,) int32/uint32 and d_leaf_ids_out (k,) int64/uint64 the pair, d_indices_out
        (k,) int32/uint32 the low word of its leaf id (the positions merkle_multiproof_device takes), d_first (k,) int32/uint32 the
        lowest input index that holds it.  d_n_unique: a device int64/uint64, always written; entries at and past it are left alone.
        d_tree_ids may be None: every pair is of tree 0.  Asynchronous on `stream` (default the current one)."""
        f = "pairs_unique_device"
        self._check(_lib.lib().p252_pairs_unique_device_into(
            self._h, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8), k,
            _dev_ptr(self, f, "d_tree_ids_out", d_tree_ids_out, k * 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_leaf_ids_out", d_leaf_ids_out, k * 8, elem=8, null_ok=True),
            _dev_ptr(self, f, "d_indices_out", d_indices_out, k * 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_first", d_first, k * 4, elem=4, null_ok=True), _dev_ptr(self, f, "d_n_unique", d_n_unique, 8, elem=8),
            stream.cuda_stream if stream is not None else _stream(self)))

    # ---- truncated outputs on the device, batched Merkle openings ----
    def truncate250_device(self, d_scalars, d_out, n):
        f = "truncate250_device"
        self._check(_lib.lib().p252_truncate250_device(self._h, _dev_ptr(self, f, "d_scalars", d_scalars, n * 32),
                                                       _dev_ptr(self, f, "d_out", d_out, n * 32), n, _stream(self)))

    def merkle4_update_device(self, tag, d_leaves, n_leaves, d_levels, d_indices, d_new_leaves, k, d_root=None, check=False):
        """incremental update of a stored tree: d_leaves[d_indices[i]] = d_new_leaves[i] (k distinct positions, int32/uint32
        tensor) and every ancestor in d_levels (the layout merkle4_tree_device fills) re-hashed; d_root gets the new root.
        Positions >= n_leaves are skipped by the kernels.  check=True (a debugging aid: it synchronises) raises ValueError
        when the list holds an out-of-range or a repeated position."""
        f = "merkle4_update_device"
        L = _lib.lib()
        leaves = _dev_ptr(self, f, "d_leaves", d_leaves, n_leaves * 32)
        levels = _dev_ptr(self, f, "d_levels", d_levels, L.p252_merkle4_levels_len(n_leaves) * 32, null_ok=n_leaves == 1)
        indices = _dev_ptr(self, f, "d_indices", d_indices, k * 4, elem=4) if k else None
        new_leaves = _dev_ptr(self, f, "d_new_leaves", d_new_leaves, k * 32) if k else None
        root = _dev_ptr(self, f, "d_root", d_root, 32, null_ok=True)
        if check and k:
            import torch
            idx = d_indices[:k].to(torch.int64) & 0xFFFFFFFF
            if int(idx.max()) >= n_leaves:
                raise ValueError("merkle4_update: position %d is outside the tree (%d leaves)" % (int(idx.max()), n_leaves))
            if int(torch.unique(idx).numel()) != k:
                raise ValueError("merkle4_update: the positions are not distinct")
        self._check(L.p252_merkle4_update_device(self._h, _tag(tag), leaves, n_leaves, levels, indices, new_leaves, k, root, _stream(self)))

    # ---- the canonical byte format (BlsScalar::to_bytes / from_bytes) on device-resident arrays ----
    def to_bytes_device(self, d_scalars, d_bytes, n):
        f = "to_bytes_device"
        self._check(_lib.lib().p252_to_bytes_device(self._h, _dev_ptr(self, f, "d_scalars", d_scalars, n * 32),
                                                    _dev_ptr(self, f, "d_bytes", d_bytes, n * 32), n, _stream(self)))

    def from_bytes_device(self, d_bytes, d_scalars, n, d_ok=None):
        f = "from_bytes_device"
        self._check(_lib.lib().p252_from_bytes_device(self._h, _dev_ptr(self, f, "d_bytes", d_bytes, n * 32),
                                                      _dev_ptr(self, f, "d_scalars", d_scalars, n * 32),
                                                      _dev_ptr(self, f, "d_ok", d_ok, n, null_ok=True), n, _stream(self)))

    def merkle4_path_batch(self, tag, leaves, siblings, positions):
        """leaves (n,4) u64; siblings (n,depth,3,4) u64; positions (n,depth) u8 in 0..3 -> roots (n,4)"""
        lv = _as_scalars(leaves).reshape(-1, 4)
        n = lv.shape[0]
        pos = np.ascontiguousarray(positions, dtype=np.uint8).reshape(n, -1)
        depth = pos.shape[1]
        sib = _as_scalars(siblings).reshape(n, depth, 3, 4) if depth else np.zeros((n, 0, 3, 4), dtype=np.uint64)
        roots = np.empty((n, 4), dtype=np.uint64)
        self._check(_lib.lib().p252_merkle4_path_batch(self._h, _tag(tag), _ptr(lv), _ptr(sib), _ptr(pos, _u8p), depth, _ptr(roots), n))
        return roots

    def merkle4_openings_device(self, d_leaves, n_leaves, d_levels, d_indices, k, check=False, out=None, arity=4):
        """openings of a stored tree, extracted on the device (p252_merkle4_openings_device): d_indices = k leaf positions (int32 /
        uint32 torch tensor).  Returns (d_leaves_out (k,4), d_siblings (k,depth,3,4), d_positions (k,depth) uint8, depth) — what
        merkle4_path_batch_device takes.  check=True: raises if a position lies outside the tree (they yield zero openings);
        out = (d_leaves_out, d_siblings, d_positions, d_n_bad) to write into caller-owned tensors (no allocation per call).
        arity=2: a Merkle2 tree (p252_merkle2_openings_device): one sibling per level, d_siblings (k,depth,1,4)."""
        import torch
        f = "merkle4_openings_device"
        a = _arity(f, arity)
        depth = a.depth(n_leaves)
        leaves = _dev_ptr(self, f, "d_leaves", d_leaves, n_leaves * 32)
        levels = _dev_ptr(self, f, "d_levels", d_levels, a.levels_len(n_leaves) * 32) if depth else None
        indices = _dev_ptr(self, f, "d_indices", d_indices, k * 4, elem=4)
        if out is not None:
            out, sib, pos, bad = out
        else:
            dev = d_leaves.device
            out = torch.empty((k, 4), dtype=torch.int64, device=dev)
            sib = torch.empty((k, depth, a.per, 4), dtype=torch.int64, device=dev)
            pos = torch.empty((k, depth), dtype=torch.uint8, device=dev)
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self._check(a.fn("openings_device")(
            self._h, leaves, n_leaves, levels, indices, k, _dev_ptr(self, f, "d_leaves_out", out, k * 32),
            _dev_ptr(self, f, "d_siblings", sib, k * depth * 32 * a.per) if depth else None,
            _dev_ptr(self, f, "d_positions", pos, k * depth) if depth else None, _dev_ptr(self, f, "d_n_bad", bad, 4), _stream(self)))
        if check and int(bad.item()):
            raise ValueError("merkle4_openings: %d position(s) outside the tree" % int(bad.item()))
        return out, sib, pos, depth

    # ---- many leaves of ONE stored tree behind one shared proof (p252_merkle{4,2}_multiproof_*; csrc/multiproof.hip) ----
    def merkle_multiproof_bound(self, n_leaves, k, arity=4):
        """upper bound, in scalars, of the shared proof of k leaves of a tree of n_leaves (p252_merkle{4,2}_multiproof_bound)"""
        return int(_arity("merkle_multiproof_bound", arity).fn("multiproof_bound")(n_leaves, k))

    def merkle_multiproof_device(self, d_leaves, n_leaves, d_levels, d_indices, k, d_leaves_out, d_proof, d_proof_len, d_n_bad=None,
                                 arity=4):
        """one shared proof for k leaves of a tree stored as merkle{4,2}_tree_device filled it (p252_merkle{4,2}_multiproof_device; no
        hashing): d_indices = k STRICTLY ASCENDING positions (int32/uint32), d_leaves_out (k, 4) receives the leaves, d_proof the
        proof — its capacity is the tensor's length, nothing is written past it (None: capacity 0, to learn the length) — and
        d_proof_len (one int64/uint64) the scalars the proof needs.  A position outside the tree or not above its predecessor is
        counted in d_n_bad (a zeroed device int32/uint32, optional) and makes the length 0.  Asynchronous on the current stream."""
        f = "merkle_multiproof_device"
        a = _arity(f, arity)
        levels = levels_len(n_leaves, arity)
        proof_cap = _n_scalars(d_proof) if hasattr(d_proof, "element_size") else 0
        fn = a.fn("multiproof_device")
        self._check(fn(self._h, _dev_ptr(self, f, "d_leaves", d_leaves, n_leaves * 32), n_leaves,
                       _dev_ptr(self, f, "d_levels", d_levels, levels * 32, null_ok=levels == 0),
                       _dev_ptr(self, f, "d_indices", d_indices, k * 4, elem=4), k, _dev_ptr(self, f, "d_leaves_out", d_leaves_out, k * 32),
                       _dev_ptr(self, f, "d_proof", d_proof, proof_cap * 32, null_ok=True), proof_cap,
                       _dev_ptr(self, f, "d_proof_len", d_proof_len, 8, elem=8),
                       _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def merkle_multiproof_verify_device(self, tag, n_leaves, d_indices, d_leaves_in, k, d_proof, proof_len, d_root, d_ok, d_root_out=None,
                                        d_n_hashed=None, d_n_bad=None, arity=4):
        """checks such a proof with every ancestor hashed ONCE (p252_merkle{4,2}_multiproof_verify_device; tag = that arity's Merkle
        tag): d_ok (one uint8) = 1 iff no position is bad, the structure that (n_leaves, d_indices) define consumes exactly
        proof_len scalars of d_proof (None when proof_len == 0), and the recomputed root equals d_root.  Optional outputs: d_root_out
        (4,) the recomputed root, d_n_hashed (one int64/uint64) the digests computed, d_n_bad (a zeroed int32/uint32) the bad
        positions.  Asynchronous on the current stream."""
        f = "merkle_multiproof_verify_device"
        fn = _arity(f, arity).fn("multiproof_verify_device")
        self._check(fn(self._h, _tag(tag), n_leaves, _dev_ptr(self, f, "d_indices", d_indices, k * 4, elem=4),
                       _dev_ptr(self, f, "d_leaves_in", d_leaves_in, k * 32), k,
                       _dev_ptr(self, f, "d_proof", d_proof, proof_len * 32, null_ok=proof_len == 0), proof_len,
                       _dev_ptr(self, f, "d_root", d_root, 32), _dev_ptr(self, f, "d_ok", d_ok, 1, elem=1),
                       _dev_ptr(self, f, "d_root_out", d_root_out, 32, null_ok=True),
                       _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True),
                       _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    # ---- a forest kept only as its frontiers (p252_merkle{4,2}_forest_frontier_*; csrc/forest_frontier.hip) ----
    def merkle_forest_frontier_bound(self, max_leaves, arity=4):
        """scalars of one tree's frontier, (depth(max_leaves) + 1) * (arity - 1) (p252_merkle{4,2}_forest_frontier_bound)"""
        return int(_arity("merkle_forest_frontier_bound", arity).fn("forest_frontier_bound")(max_leaves))

    def merkle_forest_frontier_append_device(self, tag, d_counts, d_frontier, d_roots, n_trees, max_leaves, d_add, d_add_offsets,
                                             d_n_bad=None, d_n_hashed=None, arity=4):
        """leaves appended to n_trees trees that are kept only as their frontiers, IN PLACE
        (p252_merkle{4,2}_forest_frontier_append_device_into; pass the tag of that arity): d_counts (n_trees int64/uint64), d_frontier
        (n_trees x merkle_forest_frontier_bound(max_leaves) scalars) and d_roots (n_trees, 4) are the state — all zero for empty trees;
        tree t receives d_add[d_add_offsets[t]:d_add_offsets[t+1]] (n_trees + 1 int64/uint64; d_add None: nothing appended).  Afterwards
        d_roots[t] is the root of all leaves tree t was ever given.  A refused append leaves its tree untouched and is counted in
        d_n_bad (a zeroed device int32/uint32, optional); d_n_hashed (a zeroed device int64/uint64, optional) receives the digests
        computed.  Asynchronous on the current stream."""
        f = "merkle_forest_frontier_append_device"
        a = _arity(f, arity)
        stride = (a.depth(max_leaves) + 1) * a.per if max_leaves else 0  # p252_merkle{4,2}_forest_frontier_bound
        self._check(a.fn("forest_frontier_append_device_into")(
            self._h, _tag(tag), _dev_ptr(self, f, "d_counts", d_counts, n_trees * 8, elem=8),
            _dev_ptr(self, f, "d_frontier", d_frontier, n_trees * stride * 32), _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32), n_trees,
            max_leaves, _dev_ptr(self, f, "d_add", d_add, 0, null_ok=True), _n_scalars(d_add) if d_add is not None else 0,
            _dev_ptr(self, f, "d_add_offsets", d_add_offsets, (n_trees + 1) * 8, elem=8),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True),
            _stream(self)))

    def merkle_forest_frontier_append_witness_device(self, tag, d_counts, d_frontier, d_roots, n_trees, max_leaves, d_add, d_add_offsets,
                                                     d_wit_tree_ids, d_wit_leaf_ids, k, d_wit_leaves, d_wit_siblings, d_wit_positions,
                                                     d_wit_depths, d_n_bad=None, d_n_hashed=None, d_n_bad_witness=None, arity=4):
        """merkle_forest_frontier_append_device keeping the openings of k marked leaves current, IN PLACE
        (p252_merkle{4,2}_forest_frontier_append_witness_device_into; pass the tag of that arity): witness i names leaf d_wit_leaf_ids[i]
        (int64/uint64) of tree d_wit_tree_ids[i] (int32/uint32); d_wit_leaves (k, 4), d_wit_siblings (k, D, arity-1, 4), d_wit_positions
        (k, D) uint8 and d_wit_depths (k,) uint8 with D = depth(max_leaves) are what merkle_forest_ragged_openings_device writes at that
        stride.  A witness of a leaf below the tree's old count must be its opening at that count and becomes its opening in the grown
        tree; one of a leaf this call appends is written whole; one that names no leaf becomes all zero with depth 0xFF and is counted in
        d_n_bad_witness (a zeroed device int32/uint32, optional).  The siblings and positions may be None when D == 0.  Every good
        witness verifies against d_roots (merkle_forest_ragged_verify_device).  Asynchronous on the current stream."""
        f = "merkle_forest_frontier_append_witness_device"
        a = _arity(f, arity)
        depth = a.depth(max_leaves)
        stride = (depth + 1) * a.per if max_leaves else 0  # p252_merkle{4,2}_forest_frontier_bound
        none = k == 0  # (the plain call: no witness buffer is looked at)
        self._check(a.fn("forest_frontier_append_witness_device_into")(
            self._h, _tag(tag), _dev_ptr(self, f, "d_counts", d_counts, n_trees * 8, elem=8),
            _dev_ptr(self, f, "d_frontier", d_frontier, n_trees * stride * 32), _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32), n_trees,
            max_leaves, _dev_ptr(self, f, "d_add", d_add, 0, null_ok=True), _n_scalars(d_add) if d_add is not None else 0,
            _dev_ptr(self, f, "d_add_offsets", d_add_offsets, (n_trees + 1) * 8, elem=8),
            _dev_ptr(self, f, "d_wit_tree_ids", d_wit_tree_ids, k * 4, elem=4, null_ok=none),
            _dev_ptr(self, f, "d_wit_leaf_ids", d_wit_leaf_ids, k * 8, elem=8, null_ok=none), k,
            _dev_ptr(self, f, "d_wit_leaves", d_wit_leaves, k * 32, null_ok=none),
            _dev_ptr(self, f, "d_wit_siblings", d_wit_siblings, k * depth * a.per * 32, null_ok=none or depth == 0),
            _dev_ptr(self, f, "d_wit_positions", d_wit_positions, k * depth, elem=1, null_ok=none or depth == 0),
            _dev_ptr(self, f, "d_wit_depths", d_wit_depths, k, elem=1, null_ok=none),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True),
            _dev_ptr(self, f, "d_n_bad_witness", d_n_bad_witness, 4, elem=4, null_ok=True), _stream(self)))

    def merkle_forest_frontier_extract_device(self, d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels, d_roots_forest, max_leaves,
                                              d_counts, d_frontier, d_roots, d_n_bad=None, arity=4):
        """the frontier state of a forest merkle_forest_ragged_device built with d_levels
        (p252_merkle{4,2}_forest_frontier_extract_device_into; no hashing): d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels,
        d_roots_forest exactly as the build took and filled them; writes d_counts (n_trees), d_frontier (n_trees x
        merkle_forest_frontier_bound(max_leaves), max_leaves >= max_leaves_forest) and d_roots (n_trees, 4).  A bad tree becomes an empty
        one and is counted in d_n_bad (a zeroed device int32/uint32, optional)."""
        f = "merkle_forest_frontier_extract_device"
        a = _arity(f, arity)
        forest, _ = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves_forest, d_levels)
        stride = (a.depth(max_leaves) + 1) * a.per if max_leaves else 0  # p252_merkle{4,2}_forest_frontier_bound
        self._check(a.fn("forest_frontier_extract_device_into")(
            self._h, *forest, _dev_ptr(self, f, "d_roots_forest", d_roots_forest, n_trees * 32), max_leaves,
            _dev_ptr(self, f, "d_counts", d_counts, n_trees * 8, elem=8), _dev_ptr(self, f, "d_frontier", d_frontier, n_trees * stride * 32),
            _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32), _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    # ---- consistency proofs: a grown tree extends its old root (p252_merkle{4,2}_forest_ragged_consistency_device_into,
    # _forest_consistency_verify_device_into; csrc/forest_consistency.hip) ----
    def merkle_forest_ragged_consistency_device(self, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_old_counts, k,
                                                d_new_counts_out, d_leaves_out, d_siblings, d_positions, d_depths, d_n_bad=None, arity=4):
        """k consistency proofs out of a forest merkle_forest_ragged_device built with d_levels
        (p252_merkle{4,2}_forest_ragged_consistency_device_into; no hashing): proof i shows that tree d_tree_ids[i] (int32/uint32), now of
        n_t leaves, is the tree it was at d_old_counts[i] (int64/uint64) leaves with leaves appended.  It is the opening of leaf index
        n of the tree, in the layout merkle_forest_ragged_openings_device writes at D = depth(max_leaves): d_leaves_out (k, 4),
        d_siblings (k, D, arity-1, 4), d_positions (k, D) uint8, d_depths (k,) uint8; d_new_counts_out (k,) receives n_t.  n == n_t: all
        zero with the depth of n_t.  A tree id out of range, a bad tree, n == 0 or n > n_t: all zero, depth 0xFF, new count 0, counted
        in d_n_bad (a zeroed device int32/uint32, optional).  The siblings and positions may be None when D == 0."""
        f = "merkle_forest_ragged_consistency_device"
        a = _arity(f, arity)
        forest, depth = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
        self._check(a.fn("forest_ragged_consistency_device_into")(
            self._h, *forest, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4),
            _dev_ptr(self, f, "d_old_counts", d_old_counts, k * 8, elem=8), k,
            _dev_ptr(self, f, "d_new_counts_out", d_new_counts_out, k * 8, elem=8), _dev_ptr(self, f, "d_leaves_out", d_leaves_out, k * 32),
            _dev_ptr(self, f, "d_siblings", d_siblings, k * depth * a.per * 32, null_ok=depth == 0),
            _dev_ptr(self, f, "d_positions", d_positions, k * depth, elem=1, null_ok=depth == 0),
            _dev_ptr(self, f, "d_depths", d_depths, k, elem=1), _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def merkle_forest_consistency_verify_device(self, tag, d_old_counts, d_old_roots, d_new_counts, d_new_roots, d_leaves, d_siblings,
                                                d_positions, d_depths, stride_depth, k, d_ok, d_tree_ids=None, n_trees=0,
                                                d_old_roots_out=None, d_new_roots_out=None, d_n_hashed=None, arity=4):
        """k consistency proofs checked against their claims (p252_merkle{4,2}_forest_consistency_verify_device_into; pass the tag of
        that arity): d_ok[i] (uint8) = 1 iff the opening i (the layout above, at stride_depth rows) re-hashes to the new root and its
        left siblings alone to the old root, with its slots the digits of the old count.  Without d_tree_ids claim i is element i of
        d_old_counts, d_old_roots, d_new_counts, d_new_roots (k entries each); with d_tree_ids (int32/uint32) they hold n_trees entries
        and claim i is element d_tree_ids[i] — so the counts and roots of a ForestFrontier are the old claims as they stand.
        d_old_roots_out / d_new_roots_out (k, 4; optional) receive the recomputed roots, d_n_hashed (a zeroed device int64/uint64,
        optional) grows by the digests computed.  Asynchronous on the current stream."""
        f = "merkle_forest_consistency_verify_device"
        a = _arity(f, arity)
        leaves, sib, pos, dep = self._ragged_opening_ptrs(f, a, d_leaves, d_siblings, d_positions, d_depths, stride_depth, k)
        claims = n_trees if d_tree_ids is not None else k
        self._check(a.fn("forest_consistency_verify_device_into")(
            self._h, _tag(tag), _dev_ptr(self, f, "d_old_counts", d_old_counts, claims * 8, elem=8, null_ok=claims == 0),
            _dev_ptr(self, f, "d_old_roots", d_old_roots, claims * 32, null_ok=claims == 0),
            _dev_ptr(self, f, "d_new_counts", d_new_counts, claims * 8, elem=8, null_ok=claims == 0),
            _dev_ptr(self, f, "d_new_roots", d_new_roots, claims * 32, null_ok=claims == 0), leaves, sib, pos, dep, stride_depth, k,
            _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4, null_ok=True), n_trees, _dev_ptr(self, f, "d_ok", d_ok, k, elem=1),
            _dev_ptr(self, f, "d_old_roots_out", d_old_roots_out, k * 32, null_ok=True),
            _dev_ptr(self, f, "d_new_roots_out", d_new_roots_out, k * 32, null_ok=True),
            _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True), _stream(self)))

    # ---- anchors: roots and openings of a forest's trees as they were at earlier leaf counts
    # (p252_merkle{4,2}_forest_ragged_anchor_openings_device_into; csrc/forest_anchor.hip) ----
    def merkle_forest_ragged_anchor_openings_device(self, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_anchor_tree_ids,
                                                    d_anchor_counts, m, d_anchor_ids, d_leaf_ids, k, d_anchor_roots, d_anchor_depths,
                                                    d_leaves_out=None, d_siblings=None, d_positions=None, d_depths=None,
                                                    d_n_bad_anchors=None, d_n_bad=None, d_n_hashed=None, arity=4):
        """m anchors and k openings against them out of a forest merkle_forest_ragged_device built with d_levels
        (p252_merkle{4,2}_forest_ragged_anchor_openings_device_into; pass the tag of that arity).  Anchor a is tree d_anchor_tree_ids[a]
        (int32/uint32) as it was at d_anchor_counts[a] (int64/uint64) leaves: d_anchor_roots (m, 4) receives the root a fresh build of
        those leaves returns, d_anchor_depths (m,) uint8 its depth.  Opening i is leaf d_leaf_ids[i] (int64/uint64) under anchor
        d_anchor_ids[i] (int32/uint32), written in the layout of merkle_forest_ragged_openings_device at D = depth(max_leaves):
        d_leaves_out (k, 4), d_siblings (k, D, arity-1, 4), d_positions (k, D) uint8, d_depths (k,) uint8 — what that call writes on a
        fresh build of the tree's first c leaves, so merkle_forest_ragged_verify_device takes them with d_tree_ids = d_anchor_ids, d_roots =
        d_anchor_roots, n_trees = m.  A bad anchor (unknown or bad tree, count 0 or above n_t): a zero root, depth 0xFF, counted in
        d_n_bad_anchors; a bad opening (anchor id >= m, a bad anchor, leaf id >= count): zeros, depth 0xFF, counted in d_n_bad (zeroed
        device int32/uint32, optional).  d_n_hashed (a zeroed device int64/uint64, optional) grows by the digests the anchors need.
        k == 0: the roots alone, the opening tensors may be None; the siblings and positions may be None when D == 0.  Asynchronous on
        the current stream."""
        f = "merkle_forest_ragged_anchor_openings_device"
        a = _arity(f, arity)
        forest, depth = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
        self._check(a.fn("forest_ragged_anchor_openings_device_into")(
            self._h, _tag(tag), *forest, _dev_ptr(self, f, "d_anchor_tree_ids", d_anchor_tree_ids, m * 4, elem=4, null_ok=m == 0),
            _dev_ptr(self, f, "d_anchor_counts", d_anchor_counts, m * 8, elem=8, null_ok=m == 0), m,
            _dev_ptr(self, f, "d_anchor_ids", d_anchor_ids, k * 4, elem=4, null_ok=k == 0),
            _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8, null_ok=k == 0), k,
            _dev_ptr(self, f, "d_anchor_roots", d_anchor_roots, m * 32, null_ok=m == 0),
            _dev_ptr(self, f, "d_anchor_depths", d_anchor_depths, m, elem=1, null_ok=m == 0),
            _dev_ptr(self, f, "d_leaves_out", d_leaves_out, k * 32, null_ok=k == 0),
            _dev_ptr(self, f, "d_siblings", d_siblings, k * depth * a.per * 32, null_ok=k == 0 or depth == 0),
            _dev_ptr(self, f, "d_positions", d_positions, k * depth, elem=1, null_ok=k == 0 or depth == 0),
            _dev_ptr(self, f, "d_depths", d_depths, k, elem=1, null_ok=k == 0),
            _dev_ptr(self, f, "d_n_bad_anchors", d_n_bad_anchors, 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True),
            _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True), _stream(self)))

    # ---- the shared proof across a ragged forest (p252_merkle{4,2}_forest_ragged_multiproof_*; csrc/forest_multiproof.hip) ----
    def merkle_forest_ragged_multiproof_bound(self, n_leaves, n_trees, max_leaves, k, arity=4):
        """upper bound, in scalars, of the shared proof of k pairs of a ragged forest (p252_merkle{4,2}_forest_ragged_multiproof_bound)"""
        a = _arity("merkle_forest_ragged_multiproof_bound", arity)
        return int(a.fn("forest_ragged_multiproof_bound")(n_leaves, n_trees, max_leaves, k))

    def merkle_forest_ragged_multiproof_device(self, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids, k,
                                               d_leaves_out, d_proof, d_proof_offsets, d_n_bad=None, arity=4):
        """one shared, tree-major proof for k (tree id, leaf id) pairs anywhere in a forest merkle_forest_ragged_device built with d_levels
        (p252_merkle{4,2}_forest_ragged_multiproof_device_into; no hashing): d_leaves, d_offsets, n_trees, max_leaves, d_levels exactly as the
        build took them; d_tree_ids (int32/uint32) and d_leaf_ids (int64/uint64) STRICTLY ASCENDING in (tree, leaf).  d_leaves_out (k, 4)
        receives the leaves, d_proof the proof — its capacity is the tensor's length, nothing is written past it (None: capacity 0) —
        and d_proof_offsets (n_trees + 1 int64/uint64) where each tree's single-tree proof starts, the last entry the length the
        proof needs.  A bad pair is counted in d_n_bad (a zeroed device int32/uint32, optional) and makes every offset 0.
        Asynchronous on the current stream."""
        f = "merkle_forest_ragged_multiproof_device"
        a = _arity(f, arity)
        forest, _ = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
        proof_cap = _n_scalars(d_proof) if hasattr(d_proof, "element_size") else 0
        self._check(a.fn("forest_ragged_multiproof_device_into")(
            self._h, *forest, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4),
            _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8), k,
            _dev_ptr(self, f, "d_leaves_out", d_leaves_out, k * 32), _dev_ptr(self, f, "d_proof", d_proof, proof_cap * 32, null_ok=True),
            proof_cap, _dev_ptr(self, f, "d_proof_offsets", d_proof_offsets, (n_trees + 1) * 8, elem=8),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def merkle_forest_ragged_multiproof_verify_device(self, tag, d_offsets, n_leaves, n_trees, max_leaves, d_tree_ids, d_leaf_ids, d_leaves_in,
                                                      k, d_proof, proof_len, d_proof_offsets, d_roots, d_ok, d_roots_out=None,
                                                      d_n_hashed=None, d_n_bad=None, arity=4):
        """checks such a proof with every ancestor hashed ONCE (p252_merkle{4,2}_forest_ragged_multiproof_verify_device_into; pass the tag
        of that arity); needs neither leaves nor levels: d_offsets and n_leaves, n_trees, max_leaves as the build took them, the pairs and
        d_leaves_in (k, 4) as extraction returned them, proof_len scalars of d_proof (None when 0), d_proof_offsets (n_trees + 1),
        d_roots (n_trees, 4).  d_ok[t] (n_trees uint8) = 1 iff tree t has a pair, no pair is bad, its offsets are in order and inside
        proof_len, its structure consumes exactly its part and the recomputed root equals d_roots[t].  Optional outputs: d_roots_out
        (n_trees, 4) the recomputed roots, d_n_hashed (one int64/uint64) the digests computed, d_n_bad (a zeroed int32/uint32) the bad
        pairs.  Asynchronous on the current stream."""
        f = "merkle_forest_ragged_multiproof_verify_device"
        a = _arity(f, arity)
        self._check(a.fn("forest_ragged_multiproof_verify_device_into")(
            self._h, _tag(tag), _dev_ptr(self, f, "d_offsets", d_offsets, (n_trees + 1) * 8, elem=8), n_leaves, n_trees, max_leaves,
            _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4), _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8),
            _dev_ptr(self, f, "d_leaves_in", d_leaves_in, k * 32), k,
            _dev_ptr(self, f, "d_proof", d_proof, proof_len * 32, null_ok=proof_len == 0), proof_len,
            _dev_ptr(self, f, "d_proof_offsets", d_proof_offsets, (n_trees + 1) * 8, elem=8),
            _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32), _dev_ptr(self, f, "d_ok", d_ok, n_trees, elem=1),
            _dev_ptr(self, f, "d_roots_out", d_roots_out, n_trees * 32, null_ok=True),
            _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True),
            _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))

    def merkle_path_batch_device(self, tag, d_leaves, d_siblings, d_positions, depth, d_roots, n, arity=4):
        """re-hash of n openings of one depth (p252_merkle{4,2}_path_batch_device; pass the tag of that arity): d_siblings
        (n,depth,arity-1,4), for arity 2 also (n,depth,4); d_positions (n,depth) in 0..arity-1"""
        f = "merkle_path_batch_device"
        a = _arity(f, arity)
        self._check(a.fn("path_batch_device")(self._h, _tag(tag), _dev_ptr(self, f, "d_leaves", d_leaves, n * 32),
            _dev_ptr(self, f, "d_siblings", d_siblings, n * depth * a.per * 32) if depth else None,
            _dev_ptr(self, f, "d_positions", d_positions, n * depth) if depth else None, depth,
            _dev_ptr(self, f, "d_roots", d_roots, n * 32), n, _stream(self)))

    def merkle_verify_batch_device(self, tag, d_leaves, d_siblings, d_positions, depth, d_root, d_ok, n, arity=4):
        """`Opening::verify` in bulk (the downstream poseidon-merkle verifier, AGENTS.md:62-66): d_ok[i] (uint8) = 1 iff opening i
        re-hashes to the ONE root at d_root — p252_merkle{4,2}_verify_batch_device; n bytes come back instead of n x 32"""
        f = "merkle_verify_batch_device"
        a = _arity(f, arity)
        self._check(a.fn("verify_batch_device")(self._h, _tag(tag), _dev_ptr(self, f, "d_leaves", d_leaves, n * 32),
            _dev_ptr(self, f, "d_siblings", d_siblings, n * depth * a.per * 32) if depth else None,
            _dev_ptr(self, f, "d_positions", d_positions, n * depth) if depth else None, depth,
            _dev_ptr(self, f, "d_root", d_root, 32), _dev_ptr(self, f, "d_ok", d_ok, n), n, _stream(self)))

    # ---- measurement aid: the shader clock (bench.py) ----
    def clock_probe(self, spin_us=1000, stream=None):
        """launches the one-wave clock probe (p252_clock_probe_device) on `stream` (a torch.cuda.Stream; default: the current
        one) and returns the device tensor it fills; read it with `clock_probe_result` after synchronising"""
        import torch
        stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(stream):  # the buffer is zeroed on the probe's own stream: ordered before the kernel
            out = torch.zeros(6, dtype=torch.int64, device="cuda:%d" % self.device)
        self._check(_lib.lib().p252_clock_probe_device(self._h, out.data_ptr(), int(spin_us), ctypes.c_void_p(stream.cuda_stream)))
        return out

    @staticmethod
    def clock_probe_result(t, realtime_hz=100e6):
        """{shader_ghz, interval_us, cycles_per_dependent_add}: the shader clock over the probe's interval"""
        m0, r0, mc, m1, r1, _ = [int(v) for v in t.cpu().tolist()]
        ticks = max(1, r1 - r0)
        return {"shader_ghz": (m1 - m0) / ticks * realtime_hz / 1e9, "interval_us": ticks / realtime_hz * 1e6,
                "cycles_per_dependent_add": (mc - m0) / 1024.0}

    # ---- constant table exchange ----
    def tables_export(self):
        size = _lib.lib().p252_tables_size()
        buf = np.empty(size // 4, dtype=np.int32)
        self._check(_lib.lib().p252_tables_export(self._h, _ptr(buf, ctypes.c_void_p), size))
        return buf

    def tables_import(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.int32)
        self._check(_lib.lib().p252_tables_import(self._h, _ptr(buf, ctypes.c_void_p), buf.nbytes))


# the calls that are also published per arity: Context.merkle4_<stem> and Context.merkle2_<stem> (bench.py, the per-call tests and the
# bench tools call them) are Context.merkle_<stem>(..., arity=4) and (..., arity=2)
_PER_ARITY_STEMS = (
    "forest_ragged_journal_bound", "forest_ragged_update_journaled_device", "forest_ragged_journal_swap_device",
    "forest_ragged_append_device", "forest_ragged_resize_device", "forest_ragged_select_device",
    "forest_frontier_bound", "forest_frontier_append_device", "forest_frontier_append_witness_device", "forest_frontier_extract_device",
    "forest_ragged_consistency_device", "forest_consistency_verify_device", "forest_ragged_anchor_openings_device",
    "forest_ragged_multiproof_bound", "forest_ragged_multiproof_device", "forest_ragged_multiproof_verify_device",
    "path_batch_device")


def _publish_per_arity(cls, stems):
    def forwarder(unified, arity):
        def call(self, *args, **kw):
            return unified(self, *args, arity=arity, **kw)
        return call
    for stem in stems:
        unified = getattr(cls, "merkle_" + stem)
        sig = inspect.signature(unified)
        sig = sig.replace(parameters=[p for p in sig.parameters.values() if p.name != "arity"])
        for arity in (4, 2):
            call = forwarder(unified, arity)
            call.__name__ = "merkle%d_%s" % (arity, stem)
            call.__qualname__ = "%s.%s" % (cls.__qualname__, call.__name__)
            call.__doc__ = "%s.%s(..., arity=%d): see there" % (cls.__qualname__, unified.__name__, arity)
            call.__signature__ = sig
            setattr(cls, call.__name__, call)


_publish_per_arity(Context, _PER_ARITY_STEMS)


# ---- whole runs of leaves of a ragged forest (p252_merkle{4,2}_forest_ragged_range_proofs_device_into, _forest_range_verify_device_into;
# csrc/forest_range.hip): Context.merkle4_<call> and Context.merkle2_<call> take no arity=, each pair is made from one private
# implementation; the arity-taking forms are merkle.forest_ragged_range_proofs / merkle.forest_range_verify ----
def _forest_ragged_range_proofs_device(self, a, f, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_first, d_leaf_offsets, m, k,
                                       d_proof, d_proof_lens, d_counts_out, d_leaves_out=None, d_n_bad=None):
    forest, depth = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
    stride = 2 * a.per * depth  # p252_merkle{4,2}_forest_range_stride
    self._check(a.fn("forest_ragged_range_proofs_device_into")(
        self._h, *forest, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, m * 4, elem=4), _dev_ptr(self, f, "d_first", d_first, m * 8, elem=8),
        _dev_ptr(self, f, "d_leaf_offsets", d_leaf_offsets, (m + 1) * 8, elem=8), m, k,
        _dev_ptr(self, f, "d_leaves_out", d_leaves_out, k * 32, null_ok=True),
        _dev_ptr(self, f, "d_proof", d_proof, m * stride * 32, null_ok=stride == 0),
        _dev_ptr(self, f, "d_proof_lens", d_proof_lens, m * 4, elem=4), _dev_ptr(self, f, "d_counts_out", d_counts_out, m * 8, elem=8),
        _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _stream(self)))


def _forest_range_verify_device(self, a, f, tag, d_tree_ids, d_counts, d_first, d_leaf_offsets, m, max_leaves, d_leaves_in, k, d_proof,
                                proof_stride, d_proof_lens, d_roots, n_trees, d_ok, d_roots_out=None, d_n_hashed=None, d_n_bad=None):
    self._check(a.fn("forest_range_verify_device_into")(
        self._h, _tag(tag), _dev_ptr(self, f, "d_tree_ids", d_tree_ids, m * 4, elem=4), _dev_ptr(self, f, "d_counts", d_counts, m * 8, elem=8),
        _dev_ptr(self, f, "d_first", d_first, m * 8, elem=8), _dev_ptr(self, f, "d_leaf_offsets", d_leaf_offsets, (m + 1) * 8, elem=8), m,
        max_leaves, _dev_ptr(self, f, "d_leaves_in", d_leaves_in, k * 32), k,
        _dev_ptr(self, f, "d_proof", d_proof, m * proof_stride * 32, null_ok=proof_stride == 0), proof_stride,
        _dev_ptr(self, f, "d_proof_lens", d_proof_lens, m * 4, elem=4), _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32), n_trees,
        _dev_ptr(self, f, "d_ok", d_ok, m, elem=1), _dev_ptr(self, f, "d_roots_out", d_roots_out, m * 32, null_ok=True),
        _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True), _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True),
        _stream(self)))


_RANGE_DOCS = {
    "forest_ragged_range_proofs_device":
        """the proofs of m whole runs of leaves out of a forest merkle_forest_ragged_device built with d_levels
        (p252_merkle%d_forest_ragged_range_proofs_device_into; no hashing): d_leaves, d_offsets, n_trees, max_leaves, d_levels exactly as the
        build took and filled them.  Run r is leaves [d_first[r], d_first[r] + len) of tree d_tree_ids[r] (int32/uint32; d_first
        int64/uint64) with len = d_leaf_offsets[r + 1] - d_leaf_offsets[r] (m + 1 int64/uint64, k leaves in all).  Row r of d_proof
        (m, P, 4), P = 2 (arity - 1) depth(max_leaves), receives the proof and zeros behind it, d_proof_lens (m,) int32/uint32 its
        length, d_counts_out (m,) int64/uint64 the tree's leaf count, d_leaves_out (k, 4; optional) the runs' leaves at their offsets.
        A bad run: a zero row, length 0xFFFFFFFF, count 0, counted in d_n_bad (a zeroed device int32/uint32, optional).  d_levels and
        d_proof may be None when max_leaves == 1.  Asynchronous on the current stream.""",
    "forest_range_verify_device":
        """checks such proofs against the claimed leaf counts alone (p252_merkle%d_forest_range_verify_device_into; pass the tag of that
        arity): d_ok[r] (m uint8) = 1 iff run r is good against d_counts[r] (m int64/uint64, in 1 .. max_leaves), d_proof_lens[r] is
        the closed-form length and at most proof_stride, and the run's leaves — d_leaves_in (k, 4) at d_leaf_offsets[r] — and row r of
        d_proof (m, proof_stride, 4) re-hash to d_roots[d_tree_ids[r]] (n_trees, 4).  Optional outputs: d_roots_out (m, 4) the
        recomputed roots, d_n_hashed (one int64/uint64) the digests computed, d_n_bad (a zeroed int32/uint32) the bad runs.  d_proof
        may be None when proof_stride == 0.  Asynchronous on the current stream."""}


def _publish_pairs(cls, impls, docs):
    """Context.merkle4_<stem> and Context.merkle2_<stem>, neither taking arity=, from one private implementation per stem"""
    def bound(impl, a, name):
        def call(self, *args, **kw):
            return impl(self, a, name, *args, **kw)
        return call
    for stem, impl in impls:
        sig = inspect.signature(impl)
        sig = sig.replace(parameters=[p for p in sig.parameters.values() if p.name not in ("a", "f")])
        for arity in (4, 2):
            name = "merkle%d_%s" % (arity, stem)
            call = bound(impl, _ARITIES[arity], name)
            call.__name__ = name
            call.__qualname__ = "%s.%s" % (cls.__qualname__, name)
            call.__doc__ = docs[stem] % arity
            call.__signature__ = sig
            setattr(cls, name, call)


_publish_pairs(Context, (("forest_ragged_range_proofs_device", _forest_ragged_range_proofs_device),
                         ("forest_range_verify_device", _forest_range_verify_device)), _RANGE_DOCS)


# ---- leaf updates of a ragged forest applied in order, each with its witness (p252_merkle{4,2}_forest_ragged_update_sequential_device_into;
# csrc/forest_sequential.hip): published as the range calls are, one private implementation per pair; the arity-taking form is
# merkle.forest_ragged_update_sequential ----
def _forest_ragged_update_sequential_device(self, a, f, tag, d_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids,
                                            d_new_leaves, d_order, k, d_siblings, d_positions, d_depths, d_roots_after, d_old_leaves=None,
                                            d_roots_before=None, d_roots=None, d_n_bad=None, d_n_hashed=None):
    forest, depth = self._built_forest(f, a, d_leaves, d_offsets, n_trees, max_leaves, d_levels)
    self._check(a.fn("forest_ragged_update_sequential_device_into")(
        self._h, _tag(tag), *forest, _dev_ptr(self, f, "d_tree_ids", d_tree_ids, k * 4, elem=4),
        _dev_ptr(self, f, "d_leaf_ids", d_leaf_ids, k * 8, elem=8), _dev_ptr(self, f, "d_new_leaves", d_new_leaves, k * 32),
        _dev_ptr(self, f, "d_order", d_order, k * 4, elem=4), k, _dev_ptr(self, f, "d_old_leaves", d_old_leaves, k * 32, null_ok=True),
        _dev_ptr(self, f, "d_siblings", d_siblings, k * depth * a.per * 32, null_ok=depth == 0),
        _dev_ptr(self, f, "d_positions", d_positions, k * depth, elem=1, null_ok=depth == 0),
        _dev_ptr(self, f, "d_depths", d_depths, k, elem=1), _dev_ptr(self, f, "d_roots_before", d_roots_before, k * 32, null_ok=True),
        _dev_ptr(self, f, "d_roots_after", d_roots_after, k * 32), _dev_ptr(self, f, "d_roots", d_roots, n_trees * 32, null_ok=True),
        _dev_ptr(self, f, "d_n_bad", d_n_bad, 4, elem=4, null_ok=True), _dev_ptr(self, f, "d_n_hashed", d_n_hashed, 8, elem=8, null_ok=True),
        _stream(self)))


_SEQUENTIAL_DOC = """k leaf updates of a forest merkle_forest_ragged_device built with d_levels, applied IN ORDER in one call, each with
    its witness (p252_merkle%d_forest_ragged_update_sequential_device_into; pass the tag of that arity): update i writes d_new_leaves[i]
    (k, 4) to leaf d_leaf_ids[i] (int64/uint64) of tree d_tree_ids[i] (int32/uint32) and sees the forest as updates 0 .. i - 1 left it;
    the same pair may occur any number of times.  d_order (k,) int32/uint32 is the indices sorted by (tree id, leaf id, index) — the
    stable sort by pair; the library checks it and sorts nothing.  The witness of update i, at stride D = depth(max_leaves): d_siblings
    (k, D, arity - 1, 4) and d_positions (k, D) uint8 the leaf's opening in the state just before the update, d_depths (k,) uint8,
    d_roots_after (k, 4) the tree's root just after it; optional d_old_leaves (k, 4) the leaf it replaces, d_roots_before (k, 4).  The
    forest is updated in place: afterwards a fresh build of the final leaves; d_roots (n_trees, 4; optional) is rewritten for the trees
    that received a good update.  A bad update is skipped: zero rows, depth 0xFF, zero roots, counted in d_n_bad (a zeroed device
    int32/uint32, optional).  An invalid order: every depth 0xFF, d_n_bad += k, nothing else written.  d_n_hashed (a zeroed device
    int64/uint64, optional) grows by depth(n_t) per good update.  d_levels, d_siblings and d_positions may be None when max_leaves == 1.
    Asynchronous on the current stream."""


_publish_pairs(Context, (("forest_ragged_update_sequential_device", _forest_ragged_update_sequential_device),),
               {"forest_ragged_update_sequential_device": _SEQUENTIAL_DOC})


class PinnedScalars:
    """n_scalars BlsScalars in page-locked host memory (p252_host_alloc); `.array` is a numpy view
    (n_scalars, 4) uint64.  Host-buffer entry points fed from/into such buffers copy at PCIe speed."""

    def __init__(self, n_scalars):
        nbytes = max(1, int(n_scalars)) * 32
        self._ptr = _lib.lib().p252_host_alloc(nbytes)
        if not self._ptr:
            raise MemoryError("p252_host_alloc(%d) failed" % nbytes)
        buf = (ctypes.c_uint64 * (nbytes // 8)).from_address(self._ptr)
        self.array = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4)[:n_scalars]

    def free(self):
        if getattr(self, "_ptr", None):
            self.array = None
            _lib.lib().p252_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class registered:
    """`with registered(array):` page-locks a numpy array the caller owns for the duration of the block
    (p252_host_register / p252_host_unregister): host-buffer calls on it then copy at PCIe speed."""

    def __init__(self, array):
        if not array.flags["C_CONTIGUOUS"]:
            raise ValueError("registered: the array is not C-contiguous")
        self._a = array

    def __enter__(self):
        rc = _lib.lib().p252_host_register(self._a.ctypes.data, self._a.nbytes)
        if rc:
            _raise(rc)
        return self._a

    def __exit__(self, *exc):
        _lib.lib().p252_host_unregister(self._a.ctypes.data)
        return False


def truncate250(scalars):
    """finalize_truncated's post-processing (hash.rs:164-183): raw limbs for JubJubScalar::from_raw."""
    s = _as_scalars(scalars)
    out = np.empty_like(s)
    rc = _lib.lib().p252_truncate250(_ptr(s), _ptr(out), s.size // 4)
    if rc:
        _raise(rc)
    return out


def to_bytes(scalars):
    """`BlsScalar::to_bytes` for an array of scalars: (n,4) u64 Montgomery limbs -> (n,32) u8, the little-endian bytes of the
    canonical values (host-side; `Context.to_bytes_device` for device-resident arrays)"""
    s = _as_scalars(scalars).reshape(-1, 4)
    out = np.empty((s.shape[0], 32), dtype=np.uint8)
    rc = _lib.lib().p252_to_bytes(_ptr(s), _ptr(out, _u8p), s.shape[0])
    if rc:
        _raise(rc)
    return out


def from_bytes(data):
    """`BlsScalar::from_bytes` for n records of 32 little-endian bytes -> ((n,4) u64 Montgomery limbs, ok (n,) bool);
    ok[i] False = the value is not below p (from_bytes fails there; the limbs are those of the value mod p)"""
    b = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1, 32)
    out = np.empty((b.shape[0], 4), dtype=np.uint64)
    ok = np.zeros(b.shape[0], dtype=np.uint8)
    rc = _lib.lib().p252_from_bytes(_ptr(b, _u8p), _ptr(out), _ptr(ok, _u8p), b.shape[0])
    if rc:
        _raise(rc)
    return out, ok.astype(bool)


class Hash:
    """`dusk_poseidon::Hash` (src/hash.rs:87-211): one message, absorbed in chunks, squeezed once.

    `tag=` overrides the capacity element (pass BlsScalar::hash_to_scalar output from the real crates)."""

    def __init__(self, domain, ctx=None, tag=None):  # Hash::new, hash.rs:98-105
        self.domain = Domain(domain)
        self.input = []
        self._output_len = 1
        self._ctx = ctx
        self._tag = tag

    @classmethod
    def new(cls, domain, **kw):
        return cls(domain, **kw)

    def output_len(self, output_len):  # hash.rs:111-115: honoured only for Domain::Other and > 0
        if self.domain == Domain.Other and output_len > 0:
            self._output_len = output_len

    def update(self, scalars):  # hash.rs:118-120
        self.input.append(_as_scalars(scalars).reshape(-1, 4))

    def finalize(self, truncated=False):  # hash.rs:128-155
        lens = [c.shape[0] for c in self.input]
        check_io_pattern(self.domain, lens, self._output_len)  # raises where the reference panics
        tag = self._tag if self._tag is not None else compute_tag(self.domain, lens, self._output_len)
        msg = np.concatenate(self.input, axis=0)
        ctx = self._ctx or Context.default()
        return ctx.hash_batch(tag, msg[None], msg.shape[0], self._output_len, truncated=truncated)[0]

    def finalize_truncated(self):  # hash.rs:164-183 — truncated by the digest kernel's output stage (one launch)
        return self.finalize(truncated=True)

    @classmethod
    def digest(cls, domain, scalars, **kw):  # hash.rs:191-195
        h = cls(domain, **kw)
        h.update(scalars)
        return h.finalize()

    @classmethod
    def digest_truncated(cls, domain, scalars, **kw):  # hash.rs:203-210
        h = cls(domain, **kw)
        h.update(scalars)
        return h.finalize_truncated()


class HashBatch:
    """Batched sibling of `Hash`: n independent messages with one io-pattern, one kernel launch.

    hb = HashBatch(Domain.Merkle4, item_len=4); digests = hb.digest(scalars)   # (n,4,4) -> (n,1,4)
    Per item the result equals Hash::digest(domain, item) — same validation, same tag, same order."""

    def __init__(self, domain, item_len, output_len=1, ctx=None, tag=None):
        self.domain = Domain(domain)
        self.item_len = int(item_len)
        self.out_len = int(output_len) if (self.domain == Domain.Other and output_len > 0) else 1  # hash.rs:111-115
        check_io_pattern(self.domain, [self.item_len], self.out_len)
        self.tag = _as_scalars(tag).reshape(4) if tag is not None else compute_tag(self.domain, [self.item_len], self.out_len)
        self._ctx = ctx

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = Context.default()
        return self._ctx

    def digest(self, scalars, out=None, truncated=False):
        if _is_torch(scalars):
            import torch
            n = _n_scalars(scalars) // self.item_len
            if out is None:
                out = torch.empty((n, self.out_len, 4), dtype=torch.int64, device=scalars.device)
            self.ctx.hash_batch_device(self.tag, scalars, self.item_len, self.out_len, out, n, truncated=truncated)
            return out
        return self.ctx.hash_batch(self.tag, scalars, self.item_len, self.out_len, out=out, truncated=truncated)

    def digest_truncated(self, scalars, out=None):
        """Hash::digest_truncated (hash.rs:203-210) per item, host or device buffers: ONE kernel launch — the digest kernel's
        output stage canonicalises, masks to 250 bits and stores the raw limbs JubJubScalar::from_raw receives"""
        return self.digest(scalars, out=out, truncated=True)


_RAGGED_TAGS = {}  # (domain, out_len, max_len) -> host tag table; (domain, out_len, max_len, device) -> device tensor


def ragged_tags(domain, out_len, max_len):
    """the tag table of a ragged call: row L-1 = compute_tag(domain, [L], out_len) for L = 1 .. max_len (cached)"""
    key = (int(domain), int(out_len), int(max_len))
    t = _RAGGED_TAGS.get(key)
    if t is None:
        t = np.stack([compute_tag(domain, [L], out_len) for L in range(1, max_len + 1)])
        _RAGGED_TAGS[key] = t
    return t


class RaggedHashBatch:
    """n messages of DIFFERENT lengths in one call: per message the result equals Hash::digest(domain, message) (hash.rs:191-195).

    rb = RaggedHashBatch(Domain.Other, output_len=1)
    rb.digest([m0, m1, ...])               # list of (L_i, 4) uint64 arrays -> (n, output_len, 4)
    rb.digest((flat, offsets))             # message i = flat[offsets[i]:offsets[i+1]]
    rb.digest((d_flat, d_offsets), max_len=64)   # torch CUDA tensors: the device path, asynchronous, returns a device tensor
    Lengths are checked on the host path (a zero-length message raises InvalidIOPattern, as Hash::finalize panics); on the device
    path bad messages get zero rows and increment `d_n_bad` when given.  The Merkle domains have one fixed length: HashBatch."""

    def __init__(self, domain=Domain.Other, output_len=1, ctx=None):
        self.domain = Domain(domain)
        if self.domain in (Domain.Merkle4, Domain.Merkle2):
            raise IOPatternViolation("io-pattern should be valid: IOPatternViolation — %s messages have one fixed length; use HashBatch"
                                     % self.domain.name)
        self.out_len = int(output_len) if (self.domain == Domain.Other and output_len > 0) else 1  # hash.rs:111-115
        self._ctx = ctx

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = Context.default()
        return self._ctx

    def tags(self, max_len):
        return ragged_tags(self.domain, self.out_len, max_len)

    def _device_tags(self, max_len, device):
        import torch
        key = (int(self.domain), self.out_len, int(max_len), str(device))
        t = _RAGGED_TAGS.get(key)
        if t is None:
            t = torch.from_numpy(self.tags(max_len).view(np.int64)).to(device)
            _RAGGED_TAGS[key] = t
        return t

    @staticmethod
    def _host_messages(messages):
        """-> (flat (S, 4), offsets (n + 1,) uint64, the longest length), validated like check_io_pattern (an empty absorb: hash.rs:134-137)"""
        flat, off, lens = _ragged_items(messages, "poseidon252_hip: invalid argument — ", "message", "scalars",
                                        (InvalidIOPattern, "at this point the io-pattern is valid: InvalidIOPattern — "))
        return flat, off, (int(lens.max()) if lens.size else 0)

    def digest(self, messages, max_len=None, out=None, d_n_bad=None, truncated=False):
        if isinstance(messages, tuple) and _is_torch(messages[0]):
            import torch
            d_in, d_off = messages
            if max_len is None:
                raise ValueError("RaggedHashBatch.digest: the device path needs max_len= (offsets are never read back to the host)")
            n = d_off.numel() - 1
            if out is None:
                out = torch.empty((n, self.out_len, 4), dtype=torch.int64, device=d_in.device)
            self.ctx.hash_ragged_device(self._device_tags(max_len, d_in.device), max_len, d_in, d_off, self.out_len, out, n,
                                        d_n_bad=d_n_bad, truncated=truncated)
            return out
        flat, off, longest = self._host_messages(messages)
        if off.shape[0] <= 1:
            return np.empty((0, self.out_len, 4), dtype=np.uint64)
        max_len = longest if max_len is None else int(max_len)
        if longest > max_len:
            raise ValueError("poseidon252_hip: invalid argument — a message of %d scalars is longer than max_len = %d" % (longest, max_len))
        return self.ctx.hash_ragged(self.tags(max_len), flat, off, self.out_len, truncated=truncated)

    def digest_truncated(self, messages, max_len=None, out=None, d_n_bad=None):
        """Hash::digest_truncated per message (hash.rs:203-210): the raw limbs from the sponge's own output stage (one launch)"""
        return self.digest(messages, max_len=max_len, out=out, d_n_bad=d_n_bad, truncated=True)
