"""The Python binding's two tables of truth, checked without a GPU: every ctypes prototype in _lib.PROTOTYPES against
include/poseidon252_hip.h, and every function that hands a device pointer to the library refusing a CPU tensor with a
ValueError before the library is reached (a host pointer in a kernel is a GPU memory fault, not an exception)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from helpers.binding import _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401


def _c_kind(ctype):
    if ctype.endswith("*"):
        return "pointer"
    return {"int": "int32", "unsigned": "uint32", "size_t": "size_t", "void": None}[ctype]


def _ctypes_kind(t):
    if t is None:
        return None
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int: "int32", ctypes.c_uint: "uint32", ctypes.c_size_t: "size_t"}[t]


def test_prototypes_match_the_header():
    """a wrong argtypes entry silently truncates a size_t or a pointer: each argument's kind and the return kind must be the header's"""
    import gen_rust_sys
    from poseidon252_amd import _lib
    _, protos = gen_rust_sys.parse_header()
    assert sorted(name for name, _, _ in protos) == sorted(_lib.PROTOTYPES) == sorted(_lib.ABI_SYMBOLS)
    for name, ret, params in protos:
        argtypes, restype = _lib.PROTOTYPES[name]
        argtypes = argtypes or []
        assert len(argtypes) == len(params), name
        for (pname, ctype), t in zip(params, argtypes):
            assert _c_kind(ctype) == _ctypes_kind(t), "%s(%s): %s bound as %s" % (name, pname, ctype, t.__name__)
        assert _c_kind(ret) == _ctypes_kind(restype), "%s returns %s, bound as %s" % (name, ret, restype)


def arity_cases(c):
    """{method of Context that takes arity=: (the stem of its C entry points p252_merkle{4,2}_<stem>, the call, its arguments)}.  A
    forest's d_leaves is 16 scalars long, which sets the bound of its d_levels: 16 // (arity - 1) + n_trees * depth scalars."""
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    forest = dict(d_leaves=dev(), d_offsets=dev(), d_levels=dev(n=256))
    opening = dict(d_leaves=dev(), d_siblings=dev(), d_positions=dev(u8), d_depths=dev(u8))
    return {
        "merkle4_forest_device": ("forest_device", lambda a, arity: c.merkle4_forest_device(
            tag, a["d_leaves"], 2, 4, a["d_roots"], a["d_levels"], arity=arity), dict(d_leaves=dev(), d_roots=dev(), d_levels=dev())),
        "merkle_forest_ragged": ("forest_ragged", lambda a, arity: c.merkle_forest_ragged(
            tag, np.zeros((6, 4), np.uint64), np.array([0, 2, 6], np.uint64), arity=arity, want_levels=True), {}),  # (host buffers)
        "merkle_forest_ragged_device": ("forest_ragged_device", lambda a, arity: c.merkle_forest_ragged_device(
            tag, a["d_leaves"], a["d_offsets"], 2, 4, a["d_roots"], a["d_levels"], a["d_n_bad"], arity=arity),
            dict(forest, d_roots=dev(), d_n_bad=dev(i32))),
        "merkle_forest_ragged_openings_device": ("forest_ragged_openings_device", lambda a, arity: c.merkle_forest_ragged_openings_device(
            a["d_leaves"], a["d_offsets"], 2, 4, a["d_levels"], a["d_tree_ids"], a["d_leaf_ids"], 2, out=a["out"], d_n_bad=a["d_n_bad"],
            arity=arity), dict(forest, d_tree_ids=dev(i32), d_leaf_ids=dev(), out=(dev(), dev(), dev(u8), dev(u8)), d_n_bad=dev(i32))),
        "merkle_path_ragged_device": ("path_ragged_device", lambda a, arity: c.merkle_path_ragged_device(
            tag, a["d_leaves"], a["d_siblings"], a["d_positions"], a["d_depths"], 2, a["d_roots"], 2, a["d_n_bad"], arity=arity),
            dict(opening, d_roots=dev(), d_n_bad=dev(i32))),
        "merkle_forest_ragged_verify_device": ("forest_ragged_verify_device", lambda a, arity: c.merkle_forest_ragged_verify_device(
            tag, a["d_leaves"], a["d_siblings"], a["d_positions"], a["d_depths"], 2, a["d_tree_ids"], a["d_roots"], 2, a["d_ok"], 2,
            arity=arity), dict(opening, d_tree_ids=dev(i32), d_roots=dev(), d_ok=dev(u8))),
        "merkle_forest_ragged_update_device": ("forest_ragged_update_device", lambda a, arity: c.merkle_forest_ragged_update_device(
            tag, a["d_leaves"], a["d_offsets"], 2, 4, a["d_levels"], a["d_tree_ids"], a["d_leaf_ids"], a["d_new_leaves"], 2, a["d_roots"],
            a["d_n_bad"], a["d_n_hashed"], arity=arity),
            dict(forest, d_tree_ids=dev(i32), d_leaf_ids=dev(), d_new_leaves=dev(), d_roots=dev(), d_n_bad=dev(i32), d_n_hashed=dev())),
        "merkle4_openings_device": ("openings_device", lambda a, arity: c.merkle4_openings_device(
            a["d_leaves"], 16, a["d_levels"], a["d_indices"], 2, out=a["out"], arity=arity),
            dict(d_leaves=dev(), d_levels=dev(), d_indices=dev(i32), out=(dev(), dev(), dev(), dev(i32)))),
        "merkle_multiproof_bound": ("multiproof_bound", lambda a, arity: c.merkle_multiproof_bound(16, 2, arity=arity), {}),  # (no buffer)
        "merkle_multiproof_device": ("multiproof_device", lambda a, arity: c.merkle_multiproof_device(
            a["d_leaves"], 16, a["d_levels"], a["d_indices"], 2, a["d_leaves_out"], a["d_proof"], a["d_proof_len"], a["d_n_bad"], arity=arity),
            dict(d_leaves=dev(), d_levels=dev(), d_indices=dev(i32), d_leaves_out=dev(), d_proof=dev(), d_proof_len=dev(), d_n_bad=dev(i32))),
        "merkle_multiproof_verify_device": ("multiproof_verify_device", lambda a, arity: c.merkle_multiproof_verify_device(
            tag, 16, a["d_indices"], a["d_leaves_in"], 2, a["d_proof"], 4, a["d_root"], a["d_ok"], a["d_root_out"], a["d_n_hashed"],
            a["d_n_bad"], arity=arity), dict(d_indices=dev(i32), d_leaves_in=dev(), d_proof=dev(), d_root=dev(), d_ok=dev(u8),
                                             d_root_out=dev(), d_n_hashed=dev(), d_n_bad=dev(i32))),
        "merkle_verify_batch_device": ("verify_batch_device", lambda a, arity: c.merkle_verify_batch_device(
            tag, a["d_leaves"], a["d_siblings"], a["d_positions"], 2, a["d_root"], a["d_ok"], 2, arity=arity),
            dict(d_leaves=dev(), d_siblings=dev(), d_positions=dev(), d_root=dev(), d_ok=dev())),
    }


def cases():
    """(the C entry point, the call, its arguments): every function that hands a device pointer to the library; those that take
    arity= (arity_cases: two of them pass host buffers or none) once per arity, under that arity's symbol"""
    from poseidon252_amd import encryption, multi
    from poseidon252_amd.comm import Comm, merkle4_tree_multi_device_resident
    c, ctx2 = _no_device_context(), _no_device_context()
    tag = np.zeros(4, dtype=np.uint64)
    i32 = torch.int32
    by_arity = [("p252_merkle%d_%s" % (arity, stem), lambda a, call=call, arity=arity: call(a, arity), args)
                for arity in (4, 2) for stem, call, args in arity_cases(c).values()]
    return by_arity + [
        ("p252_permute_batch_device", lambda a: c.permute_batch_device(a["d_states"], a["d_out"], 2),
         dict(d_states=dev(), d_out=dev())),
        ("p252_hash_batch_device", lambda a: c.hash_batch_device(tag, a["d_in"], 4, 1, a["d_out"], 2),
         dict(d_in=dev(), d_out=dev())),
        ("p252_hash_ragged_device", lambda a: c.hash_ragged_device(a["d_tags"], 2, a["d_in"], a["d_offsets"], 1, a["d_out"], 2, a["d_n_bad"]),
         dict(d_tags=dev(), d_in=dev(), d_offsets=dev(), d_out=dev(), d_n_bad=dev(i32))),
        ("p252_hash_ragged_truncated_device",
         lambda a: c.hash_ragged_device(a["d_tags"], 2, a["d_in"], a["d_offsets"], 1, a["d_out"], 2, a["d_n_bad"], truncated=True),
         dict(d_tags=dev(), d_in=dev(), d_offsets=dev(), d_out=dev(), d_n_bad=dev(i32))),
        ("p252_merkle4_tree_device", lambda a: c.merkle4_tree_device(tag, a["d_leaves"], 16, a["d_root"], a["d_levels"]),
         dict(d_leaves=dev(), d_root=dev(), d_levels=dev())),
        ("p252_merkle4_forest_device", lambda a: c.merkle4_forest_device(tag, a["d_leaves"], 2, 4, a["d_roots"], a["d_levels"]),  # (the default)
         dict(d_leaves=dev(), d_roots=dev(), d_levels=dev())),
        ("p252_truncate250_device", lambda a: c.truncate250_device(a["d_scalars"], a["d_out"], 2),
         dict(d_scalars=dev(), d_out=dev())),
        ("p252_merkle4_update_device",
         lambda a: c.merkle4_update_device(tag, a["d_leaves"], 16, a["d_levels"], a["d_indices"], a["d_new_leaves"], 2, a["d_root"]),
         dict(d_leaves=dev(), d_levels=dev(), d_indices=dev(i32), d_new_leaves=dev(), d_root=dev())),
        ("p252_to_bytes_device", lambda a: c.to_bytes_device(a["d_scalars"], a["d_bytes"], 2),
         dict(d_scalars=dev(), d_bytes=dev())),
        ("p252_from_bytes_device", lambda a: c.from_bytes_device(a["d_bytes"], a["d_scalars"], 2, a["d_ok"]),
         dict(d_bytes=dev(), d_scalars=dev(), d_ok=dev())),
        ("p252_merkle4_openings_device", lambda a: c.merkle4_openings_device(a["d_leaves"], 16, a["d_levels"], a["d_indices"], 2, out=a["out"]),
         dict(d_leaves=dev(), d_levels=dev(), d_indices=dev(i32), out=(dev(), dev(), dev(), dev(i32)))),
        ("p252_merkle2_path_batch_device",
         lambda a: c.merkle2_path_batch_device(tag, a["d_leaves"], a["d_siblings"], a["d_positions"], 2, a["d_roots"], 2),
         dict(d_leaves=dev(), d_siblings=dev(), d_positions=dev(), d_roots=dev())),
        ("p252_merkle4_path_batch_device",
         lambda a: c.merkle4_path_batch_device(tag, a["d_leaves"], a["d_siblings"], a["d_positions"], 2, a["d_roots"], 2),
         dict(d_leaves=dev(), d_siblings=dev(), d_positions=dev(), d_roots=dev())),
        ("p252_merkle4_verify_batch_device",
         lambda a: c.merkle_verify_batch_device(tag, a["d_leaves"], a["d_siblings"], a["d_positions"], 2, a["d_root"], a["d_ok"], 2),
         dict(d_leaves=dev(), d_siblings=dev(), d_positions=dev(), d_root=dev(), d_ok=dev())),
        ("p252_encrypt_batch_device",
         lambda a: encryption.encrypt_batch_device(a["d_messages"], a["d_secrets"], a["d_nonces"], 2, a["d_ciphers"], 2, ctx=c),
         dict(d_messages=dev(), d_secrets=dev(), d_nonces=dev(), d_ciphers=dev())),
        ("p252_decrypt_batch_device",
         lambda a: encryption.decrypt_batch_device(a["d_ciphers"], a["d_secrets"], a["d_nonces"], 2, a["d_messages"], a["d_ok"], 2, ctx=c),
         dict(d_ciphers=dev(), d_secrets=dev(), d_nonces=dev(), d_messages=dev(), d_ok=dev())),
        ("p252_hash_batch_multi_device", lambda a: multi.hash_batch_multi_device([c, ctx2], tag, a["d_ins"], 4, 1, a["d_outs"], [2, 2]),
         dict(d_ins=[dev(), dev()], d_outs=[dev(), dev()])),
        ("p252_merkle4_tree_multi_device", lambda a: multi.merkle4_tree_multi_device([c, ctx2], tag, a["d_leaves"], 4),
         dict(d_leaves=[dev(), dev()])),
        ("p252_merkle4_tree_sharded_device", lambda a: Comm(None, c).merkle4_tree_sharded_device(tag, a["d_leaves"], 16, a["d_root"]),
         dict(d_leaves=dev(), d_root=dev())),
        ("p252_merkle4_tree_multi_device_resident",
         lambda a: merkle4_tree_multi_device_resident([c, ctx2], tag, a["d_leaves"], 4, a["d_roots"]),
         dict(d_leaves=[dev(), dev()], d_roots=[dev(), dev()])),
    ]


# the tensors of cases(): 67 in the rows that take an arity, once per arity, and 73 in the others (the 68 of the round-5 surface and
# the 5 of hash_ragged_device with truncated=True)
N_REFUSED = 2 * 67 + 73


def test_every_device_pointer_refuses_a_cpu_tensor(recorder):
    n_refused = 0
    for symbol, call, args in cases():
        call(args)  # the control: with every tensor "on the device" the call reaches the library, once
        assert recorder.calls == [symbol], (symbol, recorder.calls)
        del recorder.calls[:]
        for where, bad in with_cpu_tensor(args):
            with pytest.raises(ValueError, match="is on cpu") as e:
                call(bad)
            # the message names the argument (the entries of openings' out= by their own names: d_leaves_out, d_siblings, ...)
            assert where + " is on cpu" in str(e.value) or where.startswith("out["), (symbol, where, str(e.value))
            assert recorder.calls == [], (symbol, where, recorder.calls)
            n_refused += 1
    assert n_refused >= N_REFUSED


def test_every_arity_parameter_refuses_what_is_not_4_or_2(recorder):
    """every method of Context with an arity= parameter (found by its signature, so that a new one cannot be forgotten) raises the
    one ValueError for an arity that is neither, before it looks at a tensor and before the library is reached"""
    import inspect
    from poseidon252_amd import Context
    calls = arity_cases(_no_device_context())
    methods = [name for name, m in inspect.getmembers(Context, inspect.isfunction) if "arity" in inspect.signature(m).parameters]
    assert sorted(m for m in methods if not m.startswith("_")) == sorted(calls) and len(calls) == 12, (methods, sorted(calls))
    for name, (stem, call, args) in calls.items():
        cpu = {k: None for k in args}  # no tensor at all: the arity is refused first
        for arity in (3, 0, 8, None):
            for a in (args, cpu):
                with pytest.raises(ValueError, match="%s: arity must be 4 or 2, not %r" % (name, arity)):
                    call(a, arity)
    assert recorder.calls == []


def test_refusals_survive_python_O():
    """the checks are not asserts: `python -O` keeps them"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import torch\n"
            "from poseidon252_amd import _lib, hash as H\n"
            "assert sys.flags.optimize  # (stripped, like every assert here)\n"
            "class NoLibrary:\n"
            "    def __getattr__(self, name):\n"
            "        def call(*a):\n"
            "            raise SystemExit('the library was reached: ' + name)\n"
            "        return call\n"
            "_lib._lib = NoLibrary()\n"
            "ctx = H.Context.__new__(H.Context); ctx._h = None; ctx.device = 0\n"
            "try:\n"
            "    ctx.truncate250_device(torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), 2)\n"
            "except ValueError as e:\n"
            "    print('REFUSED', sys.flags.optimize, e)\n" % ROOT)
    out = subprocess.run([sys.executable, "-O", "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "REFUSED 1 truncate250_device: d_scalars is on cpu" in out.stdout, (out.stdout, out.stderr)
