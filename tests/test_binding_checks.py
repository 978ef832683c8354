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
from helpers.binding import HOST_HELPERS, _no_device_context, dev, recorder, with_cpu_tensor  # noqa: E402,F401


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


def per_arity_cases():
    """{stem of a call that Context publishes as merkle_<stem>(..., arity=) and as merkle{4,2}_<stem>: (the stem of its C entry points,
    its positional arguments out of the tensors, the tensors)}: 2 trees of at most 4 leaves, k = m = 2, the sizes of the per-call tests"""
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    forest = dict(d_leaves=dev(), d_offsets=dev(), d_levels=dev(n=256))
    built = lambda a: (a["d_leaves"], a["d_offsets"], 2, 4, a["d_levels"])  # noqa: E731
    journal = dict(d_journal_ids=dev(i32), d_journal_values=dev(), d_journal_len=dev())
    new = dict(d_leaves_new=dev(n=128), d_offsets_new=dev(), d_levels_new=dev(n=256))
    grown = dict(forest, d_add=dev(), d_add_offsets=dev(), **new, d_roots=dev(), d_n_bad=dev(i32), d_n_hashed=dev())
    grow = lambda a: (a["d_add"], a["d_add_offsets"], 2, 8, a["d_leaves_new"], a["d_offsets_new"], a["d_levels_new"], a["d_roots"],  # noqa: E731
                      a["d_n_bad"], a["d_n_hashed"])
    source = lambda a, w: (a["d_leaves_" + w], a["d_offsets_" + w], 2, 4, a["d_levels_" + w], a["d_roots_" + w])  # noqa: E731
    sources = {"%s_%s" % (k, w): dev(n=256 if k == "d_levels" else 64) for w in "ab" for k in ("d_leaves", "d_offsets", "d_levels", "d_roots")}
    state = dict(d_counts=dev(), d_frontier=dev(), d_roots=dev())
    frontier = lambda a: (tag, a["d_counts"], a["d_frontier"], a["d_roots"], 2, 4, a["d_add"], a["d_add_offsets"])  # noqa: E731
    opening = dict(d_siblings=dev(), d_positions=dev(u8), d_depths=dev(u8))
    return {
        "forest_ragged_journal_bound": ("forest_ragged_journal_bound", lambda a: (16, 2, 4, 2), {}),  # (no buffer)
        "forest_ragged_update_journaled_device": ("forest_ragged_update_journaled_device_into", lambda a: (
            tag, *built(a), a["d_tree_ids"], a["d_leaf_ids"], a["d_new_leaves"], 2, a["d_journal_ids"], a["d_journal_values"], 4,
            a["d_journal_len"], a["d_roots"], a["d_n_bad"], a["d_n_hashed"]),
            dict(forest, d_tree_ids=dev(i32), d_leaf_ids=dev(), d_new_leaves=dev(), **journal, d_roots=dev(), d_n_bad=dev(i32), d_n_hashed=dev())),
        "forest_ragged_journal_swap_device": ("forest_ragged_journal_swap_device_into", lambda a: (
            *built(a), a["d_journal_ids"], a["d_journal_values"], 4, a["d_journal_len"], a["d_roots"], a["d_n_bad"]),
            dict(forest, **journal, d_roots=dev(), d_n_bad=dev(i32))),
        "forest_ragged_append_device": ("forest_ragged_append_device_into", lambda a: (tag, *built(a), *grow(a)), grown),
        "forest_ragged_resize_device": ("forest_ragged_resize_device_into", lambda a: (tag, *built(a), a["d_keep"], *grow(a)),
                                        dict(grown, d_keep=dev())),
        "forest_ragged_select_device": ("forest_ragged_select_device_into", lambda a: (
            source(a, "a"), source(a, "b"), a["d_pick"], 2, a["d_leaves_new"], a["d_offsets_new"], a["d_levels_new"], a["d_roots_new"], a["d_n_bad"]),
            dict(sources, d_pick=dev(), **new, d_roots_new=dev(), d_n_bad=dev(i32))),
        "forest_frontier_bound": ("forest_frontier_bound", lambda a: (4,), {}),  # (no buffer)
        "forest_frontier_append_device": ("forest_frontier_append_device_into", lambda a: (*frontier(a), a["d_n_bad"], a["d_n_hashed"]),
                                          dict(state, d_add=dev(), d_add_offsets=dev(), d_n_bad=dev(i32), d_n_hashed=dev())),
        "forest_frontier_append_witness_device": ("forest_frontier_append_witness_device_into", lambda a: (
            *frontier(a), a["d_wit_tree_ids"], a["d_wit_leaf_ids"], 2, a["d_wit_leaves"], a["d_wit_siblings"], a["d_wit_positions"],
            a["d_wit_depths"], a["d_n_bad"], a["d_n_hashed"], a["d_n_bad_witness"]),
            dict(state, d_add=dev(), d_add_offsets=dev(), d_wit_tree_ids=dev(i32), d_wit_leaf_ids=dev(), d_wit_leaves=dev(), d_wit_siblings=dev(),
                 d_wit_positions=dev(u8), d_wit_depths=dev(u8), d_n_bad=dev(i32), d_n_hashed=dev(), d_n_bad_witness=dev(i32))),
        "forest_frontier_extract_device": ("forest_frontier_extract_device_into", lambda a: (
            *built(a), a["d_roots_forest"], 4, a["d_counts"], a["d_frontier"], a["d_roots"], a["d_n_bad"]),
            dict(forest, d_roots_forest=dev(), **state, d_n_bad=dev(i32))),
        "forest_ragged_consistency_device": ("forest_ragged_consistency_device_into", lambda a: (
            *built(a), a["d_tree_ids"], a["d_old_counts"], 2, a["d_new_counts_out"], a["d_leaves_out"], a["d_siblings"], a["d_positions"],
            a["d_depths"], a["d_n_bad"]),
            dict(forest, d_tree_ids=dev(i32), d_old_counts=dev(), d_new_counts_out=dev(), d_leaves_out=dev(), **opening, d_n_bad=dev(i32))),
        "forest_consistency_verify_device": ("forest_consistency_verify_device_into", lambda a: (
            tag, a["d_old_counts"], a["d_old_roots"], a["d_new_counts"], a["d_new_roots"], a["d_leaves"], a["d_siblings"], a["d_positions"],
            a["d_depths"], 2, 2, a["d_ok"], a["d_tree_ids"], 2, a["d_old_roots_out"], a["d_new_roots_out"], a["d_n_hashed"]),
            dict(d_old_counts=dev(), d_old_roots=dev(), d_new_counts=dev(), d_new_roots=dev(), d_leaves=dev(), **opening, d_ok=dev(u8),
                 d_tree_ids=dev(i32), d_old_roots_out=dev(), d_new_roots_out=dev(), d_n_hashed=dev())),
        "forest_ragged_anchor_openings_device": ("forest_ragged_anchor_openings_device_into", lambda a: (
            tag, *built(a), a["d_anchor_tree_ids"], a["d_anchor_counts"], 2, a["d_anchor_ids"], a["d_leaf_ids"], 2, a["d_anchor_roots"],
            a["d_anchor_depths"], a["d_leaves_out"], a["d_siblings"], a["d_positions"], a["d_depths"], a["d_n_bad_anchors"], a["d_n_bad"],
            a["d_n_hashed"]),
            dict(forest, d_anchor_tree_ids=dev(i32), d_anchor_counts=dev(), d_anchor_ids=dev(i32), d_leaf_ids=dev(), d_anchor_roots=dev(),
                 d_anchor_depths=dev(u8), d_leaves_out=dev(), **opening, d_n_bad_anchors=dev(i32), d_n_bad=dev(i32), d_n_hashed=dev())),
        "forest_ragged_multiproof_bound": ("forest_ragged_multiproof_bound", lambda a: (16, 2, 4, 2), {}),  # (no buffer)
        "forest_ragged_multiproof_device": ("forest_ragged_multiproof_device_into", lambda a: (
            *built(a), a["d_tree_ids"], a["d_leaf_ids"], 2, a["d_leaves_out"], a["d_proof"], a["d_proof_offsets"], a["d_n_bad"]),
            dict(forest, d_tree_ids=dev(i32), d_leaf_ids=dev(), d_leaves_out=dev(), d_proof=dev(), d_proof_offsets=dev(), d_n_bad=dev(i32))),
        "forest_ragged_multiproof_verify_device": ("forest_ragged_multiproof_verify_device_into", lambda a: (
            tag, a["d_offsets"], 16, 2, 4, a["d_tree_ids"], a["d_leaf_ids"], a["d_leaves_in"], 2, a["d_proof"], 4, a["d_proof_offsets"],
            a["d_roots"], a["d_ok"], a["d_roots_out"], a["d_n_hashed"], a["d_n_bad"]),
            dict(d_offsets=dev(), d_tree_ids=dev(i32), d_leaf_ids=dev(), d_leaves_in=dev(), d_proof=dev(), d_proof_offsets=dev(), d_roots=dev(),
                 d_ok=dev(u8), d_roots_out=dev(), d_n_hashed=dev(), d_n_bad=dev(i32))),
        "path_batch_device": ("path_batch_device", lambda a: (tag, a["d_leaves"], a["d_siblings"], a["d_positions"], 2, a["d_roots"], 2),
                              dict(d_leaves=dev(), d_siblings=dev(), d_positions=dev(), d_roots=dev())),
    }


def arity_cases(c):
    """{method of Context that takes arity=: (the stem of its C entry points p252_merkle{4,2}_<stem>, the call, its arguments)}.  A
    forest's d_leaves is 16 scalars long, which sets the bound of its d_levels: 16 // (arity - 1) + n_trees * depth scalars."""
    tag = np.zeros(4, dtype=np.uint64)
    i32, u8 = torch.int32, torch.uint8
    forest = dict(d_leaves=dev(), d_offsets=dev(), d_levels=dev(n=256))
    opening = dict(d_leaves=dev(), d_siblings=dev(), d_positions=dev(u8), d_depths=dev(u8))
    published = {"merkle_" + stem: (c_stem, lambda a, arity, m=getattr(c, "merkle_" + stem), p=positional: m(*p(a), arity=arity), tensors)
                 for stem, (c_stem, positional, tensors) in per_arity_cases().items()}
    return {
        **published,
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


# the tensors of cases(): in the rows that take an arity, once per arity, the 67 of the twelve older methods and those of
# per_arity_cases() in its order (the three _bound rows have none); 73 in the others (the 68 of the round-5 surface and the 5 of
# hash_ragged_device with truncated=True)
N_REFUSED = 2 * (67 + (0 + 12 + 8 + 11 + 12 + 14 + 0 + 7 + 14 + 8 + 11 + 13 + 16 + 0 + 9 + 11 + 4)) + 73


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
    assert sorted(m for m in methods if not m.startswith("_")) == sorted(calls) and len(calls) == 29, (methods, sorted(calls))
    for name, (stem, call, args) in calls.items():
        cpu = {k: None for k in args}  # no tensor at all: the arity is refused first
        for arity in (3, 0, 8, None):
            for a in (args, cpu):
                with pytest.raises(ValueError, match="%s: arity must be 4 or 2, not %r" % (name, arity)):
                    call(a, arity)
    assert recorder.calls == []


def test_per_arity_names_are_the_arity_methods(recorder, monkeypatch):
    """Context.merkle{4,2}_<stem>, made from one table, is merkle_<stem>(..., arity=): a function with that signature less arity=, which
    hands the same arguments to the same C symbol, p252_merkle<arity>_<C stem>, and takes no arity= of its own"""
    import inspect
    from poseidon252_amd import Context, _lib, hash as H
    seen = []

    class Spy:
        def __getattr__(self, name):
            if name in HOST_HELPERS:
                return getattr(recorder.real, name)
            return lambda *a: seen.append((name, tuple(ctypes.cast(v, ctypes.c_void_p).value if isinstance(v, ctypes._Pointer) else v
                                                       for v in a))) or 0
    monkeypatch.setattr(_lib, "_lib", Spy())
    c, rows = _no_device_context(), per_arity_cases()
    assert sorted(rows) == sorted(H._PER_ARITY_STEMS) and len(rows) == 17
    for stem, (c_stem, positional, tensors) in rows.items():
        unified = getattr(Context, "merkle_" + stem)
        params = list(inspect.signature(unified).parameters.values())
        assert params[-1].name == "arity" and params[-1].default == 4, stem
        for arity in (4, 2):
            name = "merkle%d_%s" % (arity, stem)
            m = getattr(Context, name)
            assert inspect.isfunction(m) and m.__name__ == name and m.__qualname__ == "Context." + name and "merkle_" + stem in m.__doc__
            assert list(inspect.signature(m).parameters.values()) == params[:-1], name
            getattr(c, name)(*positional(tensors))
            unified(c, *positional(tensors), arity=arity)
            assert len(seen) == 2 and seen[0] == seen[1] and seen[0][0] == "p252_merkle%d_%s" % (arity, c_stem), (name, seen)
            del seen[:]
            with pytest.raises(TypeError, match="arity"):
                getattr(c, name)(*positional(tensors), arity=arity)
            assert seen == []


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
