"""ctypes binding of libposeidon252_hip.so (include/poseidon252_hip.h).

The extension is mandatory: a missing library raises ImportError-like RuntimeError at first use and
a missing GPU makes Context() raise — there is no CPU path behind this package.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# P252_LIB_PATH: developer switch to A/B-test alternative builds of the SAME HIP library (kernel variants)
LIB_PATH = os.environ.get("P252_LIB_PATH") or os.path.join(HERE, "libposeidon252_hip.so")

OK = 0
ERR_IO_PATTERN_VIOLATION = -1
ERR_INVALID_IO_PATTERN = -2
ERR_INVALID_ARGUMENT = -3
ERR_HIP = -4
ERR_NO_DEVICE = -5
ERR_COMM = -6
COMM_ID_BYTES = 128

ABI_VERSION = 9  # include/poseidon252_hip.h P252_ABI_VERSION this binding was written against

_int, _uint, _sz, _vp, _str = ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_szp = ctypes.POINTER(ctypes.c_size_t)
_vpp = ctypes.POINTER(ctypes.c_void_p)


def _f(*argtypes, ret=_int):
    """(argtypes, restype) of one C entry point; a (void) function keeps argtypes None"""
    return list(argtypes) or None, ret


# the C prototypes of every symbol include/poseidon252_hip.h declares, in its order (tests check the .so exports all of them and
# compare each argument list with the header).  Device buffers and streams are void*: the binding passes integer addresses.
PROTOTYPES = {
    "p252_device_count": _f(),
    "p252_create": _f(_int, _vpp),
    "p252_destroy": _f(_vp, ret=None),
    "p252_last_error": _f(_vp, ret=_str),
    "p252_permute_batch": _f(_vp, _u64p, _u64p, _sz),
    "p252_hash_batch": _f(_vp, _u64p, _u64p, _sz, _sz, _u64p, _sz),
    "p252_hash_batch_truncated": _f(_vp, _u64p, _u64p, _sz, _sz, _u64p, _sz),
    "p252_merkle4_tree": _f(_vp, _u64p, _u64p, _sz, _u64p, _u64p),
    "p252_merkle4_levels_len": _f(_sz, ret=_sz),
    "p252_merkle2_tree": _f(_vp, _u64p, _u64p, _sz, _u64p, _u64p),
    "p252_merkle2_levels_len": _f(_sz, ret=_sz),
    "p252_host_alloc": _f(_sz, ret=_vp),
    "p252_host_free": _f(_vp, ret=None),
    "p252_host_register": _f(_vp, _sz),
    "p252_host_unregister": _f(_vp),
    "p252_permute_batch_device": _f(_vp, _vp, _vp, _sz, _vp),
    "p252_hash_batch_device": _f(_vp, _u64p, _vp, _sz, _sz, _vp, _sz, _vp),
    "p252_hash_batch_truncated_device": _f(_vp, _u64p, _vp, _sz, _sz, _vp, _sz, _vp),
    "p252_hash_ragged_device": _f(_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp),
    "p252_hash_ragged_truncated_device": _f(_vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp),
    "p252_hash_ragged": _f(_vp, _u64p, _sz, _u64p, _u64p, _sz, _u64p, _sz),
    "p252_hash_ragged_truncated": _f(_vp, _u64p, _sz, _u64p, _u64p, _sz, _u64p, _sz),
    "p252_merkle4_tree_device": _f(_vp, _u64p, _vp, _sz, _vp, _vp, _vp),
    "p252_merkle2_tree_device": _f(_vp, _u64p, _vp, _sz, _vp, _vp, _vp),
    "p252_sync": _f(_vp, _vp),
    "p252_wipe": _f(_vp),
    "p252_scratch_residue": _f(_vp, _u64p),
    "p252_trim": _f(_vp),
    "p252_truncate250_device": _f(_vp, _vp, _vp, _sz, _vp),
    "p252_merkle4_update_device": _f(_vp, _u64p, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp),
    "p252_merkle4_update_checked_device": _f(_vp, _u64p, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp),
    "p252_to_bytes_device": _f(_vp, _vp, _vp, _sz, _vp),
    "p252_from_bytes_device": _f(_vp, _vp, _vp, _vp, _sz, _vp),
    "p252_merkle4_path_batch": _f(_vp, _u64p, _u64p, _u64p, _u8p, _sz, _u64p, _sz),
    "p252_merkle4_path_batch_device": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _vp, _sz, _vp),
    "p252_encryption_tag": _f(_int, _sz, _u64p),
    "p252_encrypt_batch": _f(_vp, _int, _u64p, _u64p, _u64p, _u64p, _sz, _u64p, _sz),
    "p252_decrypt_batch": _f(_vp, _int, _u64p, _u64p, _u64p, _u64p, _sz, _u64p, _u8p, _sz),
    "p252_encrypt_batch_device": _f(_vp, _int, _u64p, _vp, _vp, _vp, _sz, _vp, _sz, _vp),
    "p252_decrypt_batch_device": _f(_vp, _int, _u64p, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp),
    "p252_encryption_tags": _f(_int, _sz, _u64p),
    "p252_encrypt_ragged_device_into": _f(_vp, _int, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp),
    "p252_decrypt_ragged_device_into": _f(_vp, _int, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp),
    "p252_encrypt_ragged": _f(_vp, _int, _u64p, _sz, _u64p, _u64p, _u64p, _u64p, _u64p, _sz),
    "p252_decrypt_ragged": _f(_vp, _int, _u64p, _sz, _u64p, _u64p, _u64p, _u64p, _u64p, _u8p, _sz),
    "p252_merkle4_depth": _f(_sz, ret=_sz),
    "p252_merkle4_openings_device": _f(_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_depth": _f(_sz, ret=_sz),
    "p252_merkle2_openings_device": _f(_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_path_batch_device": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _vp, _sz, _vp),
    "p252_merkle4_verify_batch_device": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp),
    "p252_merkle2_verify_batch_device": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp),
    "p252_merkle4_forest_device": _f(_vp, _u64p, _vp, _sz, _sz, _vp, _vp, _vp),
    "p252_merkle4_forest": _f(_vp, _u64p, _u64p, _sz, _sz, _u64p),
    "p252_merkle2_forest_device": _f(_vp, _u64p, _vp, _sz, _sz, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_device": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_device": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged": _f(_vp, _u64p, _u64p, _u64p, _sz, _u64p, _u64p),
    "p252_merkle2_forest_ragged": _f(_vp, _u64p, _u64p, _u64p, _sz, _u64p, _u64p),
    "p252_merkle4_forest_ragged_openings_device": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_openings_device": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_path_ragged_device": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp),
    "p252_merkle2_path_ragged_device": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp),
    "p252_merkle4_forest_ragged_verify_device": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp),
    "p252_merkle2_forest_ragged_verify_device": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp),
    "p252_merkle4_forest_ragged_update_device": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_update_device": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_journal_bound": _f(_sz, _sz, _sz, _sz, ret=_sz),
    "p252_merkle2_forest_ragged_journal_bound": _f(_sz, _sz, _sz, _sz, ret=_sz),
    "p252_merkle4_forest_ragged_update_journaled_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp),
    "p252_merkle2_forest_ragged_update_journaled_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp),
    "p252_merkle4_forest_ragged_journal_swap_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_journal_swap_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_append_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_append_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_resize_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_resize_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_select_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_select_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp),
    "p252_merkle4_multiproof_bound": _f(_sz, _sz, ret=_sz),
    "p252_merkle2_multiproof_bound": _f(_sz, _sz, ret=_sz),
    "p252_merkle4_multiproof_device": _f(_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp),
    "p252_merkle2_multiproof_device": _f(_vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp),
    "p252_merkle4_multiproof_verify_device": _f(_vp, _u64p, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_multiproof_verify_device": _f(_vp, _u64p, _sz, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_multiproof_bound": _f(_sz, _sz, _sz, _sz, ret=_sz),
    "p252_merkle2_forest_ragged_multiproof_bound": _f(_sz, _sz, _sz, _sz, ret=_sz),
    "p252_merkle4_forest_ragged_multiproof_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_multiproof_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_multiproof_verify_device_into": _f(_vp, _u64p, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_multiproof_verify_device_into": _f(_vp, _u64p, _vp, _sz, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_frontier_bound": _f(_sz, ret=_sz),
    "p252_merkle2_forest_frontier_bound": _f(_sz, ret=_sz),
    "p252_merkle4_forest_frontier_append_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_frontier_append_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_frontier_append_witness_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_frontier_append_witness_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_frontier_extract_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_frontier_extract_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_consistency_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_consistency_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_consistency_verify_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_consistency_verify_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_anchor_openings_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_anchor_openings_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_range_stride": _f(_sz, ret=_sz),
    "p252_merkle2_forest_range_stride": _f(_sz, ret=_sz),
    "p252_merkle4_forest_ragged_range_proofs_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_range_proofs_device_into": _f(_vp, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_range_verify_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_range_verify_device_into": _f(_vp, _u64p, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle4_forest_ragged_update_sequential_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_merkle2_forest_ragged_update_sequential_device_into": _f(_vp, _u64p, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_pairs_order_device_into": _f(_vp, _vp, _vp, _sz, _vp, _vp),
    "p252_pairs_unique_device_into": _f(_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp),
    "p252_hash_batch_multi": _f(_vpp, _sz, _u64p, _u64p, _sz, _sz, _u64p, _sz),
    "p252_hash_batch_multi_device": _f(_vpp, _sz, _u64p, _vpp, _sz, _sz, _vpp, _szp, _vpp),
    "p252_merkle4_tree_multi": _f(_vpp, _sz, _u64p, _u64p, _sz, _u64p),
    "p252_merkle4_tree_multi_device": _f(_vpp, _sz, _u64p, _vpp, _sz, _u64p),
    "p252_merkle4_tree_multi_device_resident": _f(_vpp, _sz, _u64p, _vpp, _sz, _vpp, _vpp),
    "p252_comm_unique_id": _f(_vp, _sz),
    "p252_comm_create_rank": _f(_vp, _vp, _sz, _int, _int, _vpp),
    "p252_comm_create_all": _f(_vpp, _sz, _vpp),
    "p252_comm_destroy": _f(_vp, ret=None),
    "p252_comm_rank": _f(_vp),
    "p252_comm_size": _f(_vp),
    "p252_comm_check": _f(_vp, _vp),
    "p252_comm_backend": _f(_str, _sz),
    "p252_merkle4_tree_sharded_device": _f(_vp, _u64p, _vp, _sz, _vp, _vp),
    "p252_tables_size": _f(ret=_sz),
    "p252_tables_export": _f(_vp, _vp, _sz),
    "p252_tables_import": _f(_vp, _vp, _sz),
    "p252_domain_separator": _f(_int, _u64p),
    "p252_check_io_pattern": _f(_int, _szp, _sz, _sz),
    "p252_tag": _f(_int, _szp, _sz, _sz, _u64p),
    "p252_truncate250": _f(_u64p, _u64p, _sz),
    "p252_to_bytes": _f(_u64p, _u8p, _sz),
    "p252_from_bytes": _f(_u8p, _u64p, _u8p, _sz),
    "p252_clock_probe_device": _f(_vp, _vp, _uint, _vp),
    "p252_staging_lanes": _f(_sz),
    "p252_abi_version": _f(),
    "p252_version": _f(ret=_str),
}
ABI_SYMBOLS = tuple(PROTOTYPES)
_lib = None


class ExtensionMissing(RuntimeError):
    pass


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own copy of the HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7 —
    the same SONAME as /opt/rocm/lib's, which libposeidon252_hip.so links to), and the first copy of a SONAME loaded into a
    process serves everyone.  Loaded after `import torch`, this library runs on torch's copy: what every test and bench
    does.  Loaded BEFORE torch it would pull in the system copy, and a later `import torch` would then run on a runtime it
    was not built against (observed: "RuntimeError: No HIP GPUs are available").  So when torch is installed but not yet
    imported, load its runtime first — the order of imports then no longer matters.  P252_SYSTEM_HIP_RUNTIME=1 opts out
    (a process that will never use torch)."""
    import sys
    if "torch" in sys.modules or os.environ.get("P252_SYSTEM_HIP_RUNTIME") == "1":
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    if spec is None or not spec.origin:
        return None
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    try:
        ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except OSError:
        return None
    # (RCCL needs no such care since ABI 8: the library does not link it and, on its first communicator call, takes the copy the
    # process already holds — torch's, once torch is imported — csrc/rccl_dyn.hpp)
    return path


def prefer_torch_rccl():
    """Called by the communicator wrappers (comm.py, multi.py) before their first call.  The library resolves RCCL on first use and
    takes a copy the process already holds (csrc/rccl_dyn.hpp) — after `import torch` that is torch's bundled one.  BEFORE torch is
    imported it would load the system copy, and a later `import torch` would then be served that copy under the same SONAME instead of
    the one it was built against; so when torch is installed but not yet imported, map its librccl first (locally, NOT RTLD_GLOBAL:
    a globally visible librccl ahead of `import torch` makes the process abort at exit, tests/test_comm_forest.py).  C and Rust
    callers need none of this: they have one RCCL, the one the resolver finds.  P252_RCCL_PATH / P252_SYSTEM_HIP_RUNTIME=1 opt out."""
    import sys
    if "torch" in sys.modules or os.environ.get("P252_RCCL_PATH") or os.environ.get("P252_SYSTEM_HIP_RUNTIME") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    rccl = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so")
    if os.path.exists(rccl):
        try:
            ctypes.CDLL(rccl)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExtensionMissing(
            "%s not found: build it with `python -m poseidon252_amd.build` "
            "(hipcc --offload-arch=gfx950).  poseidon252_amd has no CPU fallback." % LIB_PATH)
    _preload_torch_hip_runtime()
    L = ctypes.CDLL(LIB_PATH)
    if not os.environ.get("P252_LIB_PATH"):
        # FIRST thing after loading: argument lists changed between versions under unchanged names, and a stale
        # build (*.so is git-ignored, so it survives a checkout) lacks the newer symbols — setting their argtypes below would
        # raise a raw "undefined symbol" AttributeError before any version check could speak
        if hasattr(L, "p252_abi_version"):
            L.p252_abi_version.restype = ctypes.c_int
            have = L.p252_abi_version()
        else:
            have = None
        if have != ABI_VERSION:
            raise ExtensionMissing("%s implements ABI version %s, this binding needs %d: rebuild it (python -m poseidon252_amd.build)"
                                   % (LIB_PATH, have, ABI_VERSION))
    if os.environ.get("P252_LIB_PATH"):
        # developer A/B switch only: an OLDER build of the library may lack entry points added since; give those a stub
        # that fails loudly when called, so that the benchmarks of the entry points it does have can still be compared
        class _Tolerant:
            def __init__(self, lib):
                self.__dict__["_l"] = lib

            def __getattr__(self, name):
                try:
                    return getattr(self._l, name)
                except AttributeError:
                    class _Missing:
                        argtypes = restype = None

                        def __call__(self, *a):
                            raise ExtensionMissing("%s is not exported by %s" % (name, LIB_PATH))
                    m = _Missing()
                    self.__dict__[name] = m
                    return m
        L = _Tolerant(L)
    for name, (argtypes, restype) in PROTOTYPES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            # entry points added within one ABI version (additive): a build from before them reports the right version but
            # lacks the symbol — name it instead of a raw AttributeError
            raise ExtensionMissing("%s does not export %s, which this binding declares: it is a stale build — rebuild it "
                                   "(python -m poseidon252_amd.build)" % (LIB_PATH, name)) from None
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L
