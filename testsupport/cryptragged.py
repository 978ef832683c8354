"""What the tests of the ragged encryption calls (p252_{encrypt,decrypt}_ragged*) share: the layout, the oracle run per length, a
numpy model of the schedule (csrc/crypt_ragged.h; its kernels in csrc/ragged.hip), and the device round trip."""
import numpy as np

CAP = 2048  # P252_CRYPT_RAGGED_MAX_LEN
SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)
SYMBOLS = {"p252_encryption_tags": 3, "p252_encrypt_ragged_device_into": 13, "p252_decrypt_ragged_device_into": 14, "p252_encrypt_ragged": 10,
           "p252_decrypt_ragged": 11}


def offsets_of(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lens, dtype=np.uint64), out=off[1:])
    return off


def case(oracle_mod, seed, lens):
    """(flat messages (S, 4), offsets (n + 1,), secrets (n, 2, 4), nonces (n, 4)) of random canonical scalars"""
    off = offsets_of(lens)
    n = len(lens)
    return (oracle_mod.fill_random(seed, int(off[-1])), off, oracle_mod.fill_random(seed + 1000, 2 * n).reshape(n, 2, 4),
            oracle_mod.fill_random(seed + 2000, n))


def cipher_rows(off, i):
    """the rows of message i's cipher in the cipher-side array: L_i + 1 scalars at offsets[i] + i"""
    return slice(int(off[i]) + i, int(off[i + 1]) + i + 1)


def bad_messages(off, max_len, n_scalars):
    """the device calls' rule: empty or decreasing, longer than max_len, or ending past the array"""
    a, b = off[:-1].astype(np.int64), off[1:].astype(np.int64)
    return (b <= a) | (b - a > max_len) | (b > n_scalars)


def oracle_ciphers(oracle_mod, flat, off, secrets, nonces, variant, rows=None):
    """the cipher-side array of the messages `rows` (default: all; the others' regions stay zero), the oracle run once per length"""
    n = off.size - 1
    lens = (off[1:] - off[:-1]).astype(np.int64)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = np.zeros((int(off[-1]) + n, 4), dtype=np.uint64)
    for L in np.unique(lens[rows]):
        sel = rows[lens[rows] == L]
        x = np.stack([flat[int(off[r]):int(off[r]) + int(L)] for r in sel])
        c = oracle_mod.encrypt_batch(oracle_mod.encryption_tag(int(L), variant), x, secrets[sel], nonces[sel], variant)
        for k, r in enumerate(sel):
            out[cipher_rows(off, r)] = c[k]
    return out


# ---- the schedule (csrc/crypt_ragged.h, the k_crypt_ragged_* kernels of csrc/ragged.hip), restated ----
def group(coop):
    return 8 if coop else 64


def slot_bound(n, max_len, coop):
    g = group(coop)
    return (n + (g - 1) * (max_len + 1) + g - 1) // g * g


def schedule(off, max_len, n_scalars, coop):
    """the order array the sort kernels leave (within a bucket: ascending message index; the device's order there depends on
    atomic timing): bucket L = the messages of length L, bucket 0 the bad ones, buckets descending with 0 last, every bucket's size
    rounded up to the group, sentinels in between and behind"""
    n = off.size - 1
    g = group(coop)
    lens = (off[1:].astype(np.int64) - off[:-1].astype(np.int64))
    bucket = np.where(bad_messages(off, max_len, n_scalars), 0, lens)
    order = np.full(slot_bound(n, max_len, coop), SENTINEL, dtype=np.uint64)
    at = 0
    for b in list(range(max_len, 0, -1)) + [0]:
        ids = np.nonzero(bucket == b)[0]
        order[at:at + ids.size] = ids
        at += (ids.size + g - 1) // g * g
    assert at <= order.size
    return order, bucket


# ---- the device round trip ----
def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def device_encrypt(ctx, flat, off, secrets, nonces, variant, max_len, prefill=0, d_bad=None, n_scalars=None):
    """p252_encrypt_ragged_device_into over host arrays -> the cipher-side array (n_scalars + n, 4), pre-filled with `prefill` limbs"""
    import torch
    from poseidon252_amd import encryption as E
    n = off.size - 1
    S = flat.shape[0] if n_scalars is None else n_scalars
    d_c = torch.full((S + n, 4), prefill, dtype=torch.int64, device="cuda")
    E.encrypt_ragged_device(to_dev(flat), to_dev(off), to_dev(secrets), to_dev(nonces), d_c, n, max_len, n_scalars=S, d_n_bad=d_bad, ctx=ctx,
                            variant=variant)
    return d_c.cpu().numpy().view(np.uint64)


def device_decrypt(ctx, ciphers, off, secrets, nonces, variant, max_len, n_scalars, prefill=0, d_bad=None):
    """p252_decrypt_ragged_device_into over host arrays -> (message-side array (n_scalars, 4) pre-filled with `prefill`, ok (n,) uint8
    pre-filled with 7)"""
    import torch
    from poseidon252_amd import encryption as E
    n = off.size - 1
    d_m = torch.full((n_scalars, 4), prefill, dtype=torch.int64, device="cuda")
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    E.decrypt_ragged_device(to_dev(ciphers), to_dev(off), to_dev(secrets), to_dev(nonces), d_m, d_ok, n, max_len, n_scalars=n_scalars, d_n_bad=d_bad,
                            ctx=ctx, variant=variant)
    return d_m.cpu().numpy().view(np.uint64), d_ok.cpu().numpy()


def round_trip(ctx, oracle_mod, variant, lens, seed, max_len):
    """encrypt equals the oracle, decrypt restores the messages with every flag 1 -> (case, ciphers)"""
    flat, off, sec, non = case(oracle_mod, seed, lens)
    got = device_encrypt(ctx, flat, off, sec, non, variant, max_len)
    assert np.array_equal(got, oracle_ciphers(oracle_mod, flat, off, sec, non, variant))
    back, ok = device_decrypt(ctx, got, off, sec, non, variant, max_len, flat.shape[0])
    assert np.array_equal(back, flat) and (ok == 1).all()
    return (flat, off, sec, non), got


def shuffled(seed, lens):
    lens = list(lens)
    np.random.default_rng(seed).shuffle(lens)
    return lens
