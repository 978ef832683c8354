"""Host-side mirror of `dusk_poseidon::{encrypt, decrypt}` (src/encryption.rs:62-95), single and batched.

The reference wraps `dusk_safe::encrypt/decrypt` with `ScalarPermutation`, `Domain::Encryption` and the
two coordinates of a JubJub shared point as the secret.  dusk-safe is not vendored in the reference and
its tests only check round trips and failures (tests/encryption.rs:30-115), so the construction is UNPINNED at
the byte level.  The library interprets the literal sponge-call sequence; `variant` picks it:
  STREAM (default)  [Absorb(2), Absorb(1), Squeeze(len), Absorb(len), Squeeze(1)] — dusk-safe's encrypt as recollected
  DUPLEX            [Absorb(2), Absorb(1), {Squeeze(c), Absorb(c)}*, Squeeze(1)], c = min(4, remaining)
(identical for len <= 4).  cipher[i] = message[i] + mask[i], cipher[len] = MAC.  All hashing happens on the GPU.

shared_secret: (2,4) uint64 — the (u, v) coordinates of the shared JubJubAffine as BlsScalars
               (encryption.rs:66-69: `shared_secret.get_u(), shared_secret.get_v()`); nonce: (4,) uint64.
"""
import numpy as np

from . import _lib
from ._lib import _u8p
from .hash import Context, Error, _as_scalars, _dev_ptr, _ptr, _raise, _stream, _tag

STREAM, DUPLEX = 0, 1  # P252_CRYPT_STREAM / P252_CRYPT_DUPLEX (include/poseidon252_hip.h)


class DecryptionFailed(Error):
    """Error::DecryptionFailed (src/error.rs:27-29)"""


def encryption_tag(message_len, variant=STREAM):
    """Safe::tag of the encryption io-pattern for a message of `message_len` scalars.  UNPINNED recipe."""
    out = np.empty(4, dtype=np.uint64)
    rc = _lib.lib().p252_encryption_tag(int(variant), int(message_len), _ptr(out))
    if rc:
        _raise(rc)
    return out


def encrypt_batch(messages, shared_secrets, nonces, ctx=None, tag=None, variant=STREAM):
    """messages (n,len,4), shared_secrets (n,2,4), nonces (n,4) -> ciphers (n,len+1,4)"""
    secrets = _as_scalars(shared_secrets).reshape(-1, 2, 4)
    n = secrets.shape[0]
    msgs = _as_scalars(messages).reshape(n, -1, 4) if n else _as_scalars(messages).reshape(0, 1, 4)
    non = _as_scalars(nonces).reshape(n, 4)
    ln = msgs.shape[1]
    ctx = ctx or Context.default()
    tag = encryption_tag(ln, variant) if tag is None else tag
    out = np.empty((n, ln + 1, 4), dtype=np.uint64)
    ctx._check(_lib.lib().p252_encrypt_batch(ctx._h, int(variant), _tag(tag), _ptr(msgs), _ptr(secrets), _ptr(non), ln, _ptr(out), n))
    return out


def decrypt_batch(ciphers, shared_secrets, nonces, ctx=None, tag=None, variant=STREAM):
    """ciphers (n,len+1,4) -> (messages (n,len,4), ok (n,) bool); ok[i] False = DecryptionFailed for item i"""
    secrets = _as_scalars(shared_secrets).reshape(-1, 2, 4)
    n = secrets.shape[0]
    cph = _as_scalars(ciphers).reshape(n, -1, 4)
    non = _as_scalars(nonces).reshape(n, 4)
    ln = cph.shape[1] - 1
    ctx = ctx or Context.default()
    if ln < 1:
        ctx._check(_lib.ERR_INVALID_IO_PATTERN)
    tag = encryption_tag(ln, variant) if tag is None else tag
    out = np.empty((n, ln, 4), dtype=np.uint64)
    ok = np.zeros(n, dtype=np.uint8)
    ctx._check(_lib.lib().p252_decrypt_batch(ctx._h, int(variant), _tag(tag), _ptr(cph), _ptr(secrets), _ptr(non), ln, _ptr(out),
                                             _ptr(ok, _u8p), n))
    return out, ok.astype(bool)


def encrypt(message, shared_secret, nonce, ctx=None, tag=None, variant=STREAM):
    """`dusk_poseidon::encrypt` (encryption.rs:62-76): Vec<BlsScalar> of message.len() + 1"""
    m = _as_scalars(message).reshape(-1, 4)
    return encrypt_batch(m[None], _as_scalars(shared_secret).reshape(1, 2, 4), _as_scalars(nonce).reshape(1, 4), ctx=ctx, tag=tag, variant=variant)[0]


def decrypt(cipher, shared_secret, nonce, ctx=None, tag=None, variant=STREAM):
    """`dusk_poseidon::decrypt` (encryption.rs:81-95): the message, or raises DecryptionFailed"""
    c = _as_scalars(cipher).reshape(-1, 4)
    msg, ok = decrypt_batch(c[None], _as_scalars(shared_secret).reshape(1, 2, 4), _as_scalars(nonce).reshape(1, 4), ctx=ctx, tag=tag, variant=variant)
    if not ok[0]:
        raise DecryptionFailed("DecryptionFailed")
    return msg[0]


def encrypt_batch_device(d_messages, d_secrets, d_nonces, message_len, d_ciphers, n, ctx=None, tag=None, variant=STREAM):
    """device-resident variant (torch CUDA tensors of int64 limbs): messages n*len, secrets n*2, nonces n scalars in,
    ciphers n*(len+1) scalars out; asynchronous on torch's current stream"""
    ctx, f = ctx or Context.default(), "encrypt_batch_device"
    ctx._check(_lib.lib().p252_encrypt_batch_device(
        ctx._h, int(variant), _tag(encryption_tag(message_len, variant) if tag is None else tag),
        _dev_ptr(ctx, f, "d_messages", d_messages, n * message_len * 32), _dev_ptr(ctx, f, "d_secrets", d_secrets, n * 64),
        _dev_ptr(ctx, f, "d_nonces", d_nonces, n * 32), message_len,
        _dev_ptr(ctx, f, "d_ciphers", d_ciphers, n * (message_len + 1) * 32), n, _stream(ctx)))


def decrypt_batch_device(d_ciphers, d_secrets, d_nonces, message_len, d_messages, d_ok, n, ctx=None, tag=None, variant=STREAM):
    """device-resident variant: d_ok is a uint8 tensor of n flags (0 = DecryptionFailed for that item)"""
    ctx, f = ctx or Context.default(), "decrypt_batch_device"
    ctx._check(_lib.lib().p252_decrypt_batch_device(
        ctx._h, int(variant), _tag(encryption_tag(message_len, variant) if tag is None else tag),
        _dev_ptr(ctx, f, "d_ciphers", d_ciphers, n * (message_len + 1) * 32), _dev_ptr(ctx, f, "d_secrets", d_secrets, n * 64),
        _dev_ptr(ctx, f, "d_nonces", d_nonces, n * 32), message_len, _dev_ptr(ctx, f, "d_messages", d_messages, n * message_len * 32),
        _dev_ptr(ctx, f, "d_ok", d_ok, n), n, _stream(ctx)))


# ---- messages of different lengths in one call (p252_{encrypt,decrypt}_ragged*) ----
RAGGED_MAX_LEN = 2048  # P252_CRYPT_RAGGED_MAX_LEN (include/poseidon252_hip.h): the longest message of a ragged call

_TAGS = {}  # (variant, max_len) -> host tag table


def encryption_tags(max_len, variant=STREAM):
    """the tag table of a ragged call (p252_encryption_tags): row L-1 = encryption_tag(L, variant) for L = 1 .. max_len (cached)"""
    key = (int(variant), int(max_len))
    t = _TAGS.get(key)
    if t is None:
        if not 0 <= key[1] < 2 ** 63:
            _raise(_lib.ERR_INVALID_ARGUMENT)
        t = np.empty((min(key[1], RAGGED_MAX_LEN + 1), 4), dtype=np.uint64)  # (the library refuses 0 and more than the cap)
        rc = _lib.lib().p252_encryption_tags(key[0], key[1], _ptr(t) if t.size else None)
        if rc:
            _raise(rc)
        _TAGS[key] = t
    return t


def _ragged_messages(call, items):
    """(flat, offsets, lengths) of a list of (L_i, 4) arrays or of a (flat, offsets) pair; an empty message raises InvalidIOPattern"""
    from .hash import InvalidIOPattern, _ragged_items
    return _ragged_items(items, "poseidon252_hip: invalid argument — %s: " % call, "message", "scalars",
                         (InvalidIOPattern, "at this point the io-pattern is valid: InvalidIOPattern — %s: " % call))


def _ragged_result(items, flat, off, extra):
    """the result in the form the caller gave: a list of arrays for a list, (flat, offsets) for a pair; extra = 1: the cipher side"""
    if isinstance(items, tuple):
        return flat, off
    return [flat[int(off[i]) + extra * i:int(off[i + 1]) + extra * (i + 1)] for i in range(off.shape[0] - 1)]


def _max_len(call, lens, max_len):
    longest = int(lens.max()) if lens.size else 0
    max_len = max(longest, 1) if max_len is None else int(max_len)
    if longest > max_len:
        raise ValueError("poseidon252_hip: invalid argument — %s: a message of %d scalars is longer than max_len = %d" % (call, longest, max_len))
    return max_len


def encrypt_ragged(messages, shared_secrets, nonces, ctx=None, tags=None, variant=STREAM, max_len=None):
    """n messages of DIFFERENT lengths encrypted in one call: messages = a list of (L_i, 4) arrays, or (flat, offsets) with message i =
    flat[offsets[i]:offsets[i+1]]; shared_secrets (n,2,4), nonces (n,4).  Returns the ciphers in the same form: a list of (L_i + 1, 4)
    arrays, or (flat_ciphers, offsets) with the cipher of message i at flat_ciphers[offsets[i] + i : offsets[i+1] + i + 1] (the
    MESSAGE offsets serve both sides).  Each cipher equals encrypt(message_i, ...).  Lengths up to RAGGED_MAX_LEN."""
    flat, off, lens = _ragged_messages("encrypt_ragged", messages)
    if off.shape[0] <= 1:
        return _ragged_result(messages, np.empty((0, 4), dtype=np.uint64), off, 1)
    max_len = _max_len("encrypt_ragged", lens, max_len)
    ctx = ctx or Context.default()
    out = ctx.crypt_ragged(False, variant, encryption_tags(max_len, variant) if tags is None else tags, flat, off, shared_secrets, nonces)
    return _ragged_result(messages, out, off, 1)


def decrypt_ragged(ciphers, shared_secrets, nonces, ctx=None, tags=None, variant=STREAM, max_len=None):
    """the inverse of encrypt_ragged: ciphers = a list of (L_i + 1, 4) arrays, or (flat_ciphers, offsets) in the layout encrypt_ragged
    returns (offsets = the MESSAGE offsets).  Returns (messages in the same form, ok (n,) bool); ok[i] False = DecryptionFailed for
    message i, whose content is then unspecified."""
    from .hash import InvalidIOPattern
    if isinstance(ciphers, tuple):
        flat = _as_scalars(ciphers[0]).reshape(-1, 4)
        off = np.ascontiguousarray(ciphers[1], dtype=np.uint64).reshape(-1)
        lens = off[1:].astype(np.int64) - off[:-1].astype(np.int64)
        if (lens < 0).any():
            raise ValueError("poseidon252_hip: invalid argument — decrypt_ragged: offsets decrease at message %d" % int(np.argmax(lens < 0)))
        if (lens == 0).any():
            raise InvalidIOPattern("at this point the io-pattern is valid: InvalidIOPattern — decrypt_ragged: message %d is empty" % int(np.argmax(lens == 0)))
    else:
        parts = [_as_scalars(c).reshape(-1, 4) for c in ciphers]
        lens = np.array([p.shape[0] - 1 for p in parts], dtype=np.int64)
        if (lens < 1).any():
            raise InvalidIOPattern("at this point the io-pattern is valid: InvalidIOPattern — decrypt_ragged: message %d is empty" % int(np.argmax(lens < 1)))
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        flat = np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), dtype=np.uint64)
    if off.shape[0] <= 1:
        return _ragged_result(ciphers, np.empty((0, 4), dtype=np.uint64), off, 0), np.zeros(0, dtype=bool)
    max_len = _max_len("decrypt_ragged", lens, max_len)
    ctx = ctx or Context.default()
    out, ok = ctx.crypt_ragged(True, variant, encryption_tags(max_len, variant) if tags is None else tags, flat, off, shared_secrets, nonces)
    return _ragged_result(ciphers, out, off, 0), ok.astype(bool)


def decrypt_ragged_checked(ciphers, shared_secrets, nonces, ctx=None, tags=None, variant=STREAM, max_len=None):
    """decrypt_ragged returning the messages alone, or raising DecryptionFailed (naming the first message) if any MAC failed —
    what `decrypt` is to `decrypt_batch`"""
    msgs, ok = decrypt_ragged(ciphers, shared_secrets, nonces, ctx=ctx, tags=tags, variant=variant, max_len=max_len)
    if not ok.all():
        raise DecryptionFailed("DecryptionFailed: message %d" % int(np.argmin(ok)))
    return msgs


def _device_tags(ctx, max_len, variant, device):
    import torch
    key = (int(variant), int(max_len), str(device))
    t = _TAGS.get(key)
    if t is None:
        t = torch.from_numpy(encryption_tags(max_len, variant).view(np.int64)).to(device)
        _TAGS[key] = t
    return t


def encrypt_ragged_device(d_messages, d_offsets, d_secrets, d_nonces, d_ciphers, n, max_len, n_scalars=None, d_n_bad=None, ctx=None, d_tags=None,
                          variant=STREAM):
    """device-resident variant (torch CUDA tensors of int64 limbs), asynchronous on torch's current stream: d_offsets = n + 1 MESSAGE
    offsets, d_messages n_scalars scalars (default: all it holds), d_ciphers n_scalars + n scalars, cipher i at offsets[i] + i.
    max_len is required (the offsets are never read back); d_tags defaults to a cached device copy of encryption_tags(max_len)."""
    ctx = ctx or Context.default()
    n_scalars = d_messages.numel() * d_messages.element_size() // 32 if n_scalars is None else n_scalars
    ctx.encrypt_ragged_device(variant, _device_tags(ctx, max_len, variant, d_messages.device) if d_tags is None else d_tags, max_len, d_messages,
                              n_scalars, d_offsets, d_secrets, d_nonces, d_ciphers, n, d_n_bad=d_n_bad)


def decrypt_ragged_device(d_ciphers, d_offsets, d_secrets, d_nonces, d_messages, d_ok, n, max_len, n_scalars=None, d_n_bad=None, ctx=None,
                          d_tags=None, variant=STREAM):
    """device-resident variant: the layout of encrypt_ragged_device read the other way (n_scalars = the scalars of the MESSAGE side,
    default: all d_messages holds); d_ok is a uint8 tensor of n flags (0 = DecryptionFailed, or a bad message)"""
    ctx = ctx or Context.default()
    n_scalars = d_messages.numel() * d_messages.element_size() // 32 if n_scalars is None else n_scalars
    ctx.decrypt_ragged_device(variant, _device_tags(ctx, max_len, variant, d_ciphers.device) if d_tags is None else d_tags, max_len, d_ciphers,
                              n_scalars, d_offsets, d_secrets, d_nonces, d_messages, d_ok, n, d_n_bad=d_n_bad)
