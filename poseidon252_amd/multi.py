"""Multi-device entry points of the C ABI (p252_*_multi): an array of contexts, one per GPU, sharded inside the library
 — what a Rust / C caller uses to get the 8-GPU path without Python or torch.distributed.  The Python
multi-GPU driver of bench.py is poseidon252_amd/distributed.py (one process per GPU); this module only binds the ABI."""
import ctypes

import numpy as np

from . import _lib
from .hash import _as_scalars, _dev_ptrs, _host_out, _ptr, _raise, _tag


def _ctx_array(ctxs):
    return (ctypes.c_void_p * len(ctxs))(*[c._h for c in ctxs])


def _check(ctxs, rc):
    if rc:
        _raise(rc, ctxs[0]._h if ctxs else None)


def hash_batch_multi(ctxs, tag, messages, in_len, out_len, out=None):
    """n messages of in_len scalars -> (n, out_len, 4); contiguous shards over `ctxs` (p252_hash_batch_multi)"""
    x = _as_scalars(messages).reshape(-1, in_len, 4) if in_len else _as_scalars(messages).reshape(0, 1, 4)
    n = x.shape[0]
    if out is None:
        out = np.empty((n, max(out_len, 1), 4), dtype=np.uint64)
    else:
        _host_out("hash_batch_multi", out, n * out_len)
    _check(ctxs, _lib.lib().p252_hash_batch_multi(_ctx_array(ctxs), len(ctxs), _tag(tag), _ptr(x), in_len, out_len, _ptr(out), n))
    return out


def merkle4_tree_multi(ctxs, tag, leaves):
    """root of the arity-4 tree over `leaves` (n_ctx * 4^k of them), one complete subtree per context"""
    lv = _as_scalars(leaves).reshape(-1, 4)
    root = np.empty(4, dtype=np.uint64)
    _check(ctxs, _lib.lib().p252_merkle4_tree_multi(_ctx_array(ctxs), len(ctxs), _tag(tag), _ptr(lv), lv.shape[0], _ptr(root)))
    return root


def hash_batch_multi_device(ctxs, tag, d_ins, in_len, out_len, d_outs, counts, streams=None):
    """device-resident shards (torch CUDA tensors, one per context, on its device); asynchronous"""
    f, k = "hash_batch_multi_device", len(ctxs)
    ins = _dev_ptrs(ctxs, f, "d_ins", d_ins, [c * in_len * 32 for c in counts])
    outs = _dev_ptrs(ctxs, f, "d_outs", d_outs, [c * out_len * 32 for c in counts])
    cnt = (ctypes.c_size_t * k)(*counts)
    sts = (ctypes.c_void_p * k)(*streams) if streams is not None else None
    _check(ctxs, _lib.lib().p252_hash_batch_multi_device(_ctx_array(ctxs), k, _tag(tag), ins, in_len, out_len, outs, cnt, sts))


def merkle4_tree_multi_device(ctxs, tag, d_leaves, leaves_per_ctx):
    ptrs = _dev_ptrs(ctxs, "merkle4_tree_multi_device", "d_leaves", d_leaves, [leaves_per_ctx * 32] * len(ctxs))
    root = np.empty(4, dtype=np.uint64)
    _lib.prefer_torch_rccl()  # (contexts on distinct devices exchange their roots over RCCL: one copy per process)
    _check(ctxs, _lib.lib().p252_merkle4_tree_multi_device(_ctx_array(ctxs), len(ctxs), _tag(tag), ptrs, leaves_per_ctx, _ptr(root)))
    return root
