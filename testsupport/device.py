"""The one device call that the tests and the bench tools both make past the Python mirror."""
import numpy as np


def tree_device(ctx, arity, tag, d_leaves, n, d_root, d_levels):
    """p252_merkle{4,2}_tree_device on torch's current stream (the Python mirror has the arity-4 call only)"""
    import ctypes
    from poseidon252_amd import _lib
    from poseidon252_amd.hash import _stream
    L = _lib.lib()
    fn = L.p252_merkle4_tree_device if arity == 4 else L.p252_merkle2_tree_device
    tp = np.ascontiguousarray(tag, dtype=np.uint64).ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    ctx._check(fn(ctx._h, tp, d_leaves.data_ptr(), n, d_root.data_ptr(), d_levels.data_ptr() if d_levels is not None else None, _stream(ctx)))
