"""poseidon252_amd — MI355X-native batched Poseidon252 (Hades width-5 + SAFE sponge, BLS12-381 scalar
field), a drop-in for the native path of dusk-network/Poseidon252 (`dusk_poseidon::Hash` / `Domain`).

Product code path: hash.py -> ctypes -> libposeidon252_hip.so (csrc/api.cpp) -> kernels.hip (gfx950).
Nothing in this package imports oracle/ or computes hashes on the CPU.
"""
from .hash import (Context, DeviceError, Domain, Error, Hash, HashBatch, HADES_WIDTH, InvalidIOPattern,
                   IOPatternViolation, RaggedHashBatch, check_io_pattern, compute_tag, from_bytes, to_bytes, truncate250)
from .merkle import merkle4_tree, merkle4_forest, merkle4_tag, merkle_forest_ragged, levels_len, merkle_multiproof, merkle_multiproof_verify, forest_ragged_append, forest_ragged_resize, forest_ragged_select, forest_ragged_update_journaled, forest_ragged_journal_swap, ForestJournal, forest_ragged_multiproof, forest_ragged_multiproof_verify, ForestFrontier, ForestWitnesses, forest_frontier_append, forest_frontier_extract, forest_ragged_consistency, forest_consistency_verify, forest_ragged_anchor_openings, forest_ragged_range_proofs, forest_range_verify, forest_range_stride, forest_ragged_update_sequential, pairs_order, pairs_unique
from .encryption import (DecryptionFailed, decrypt, decrypt_batch, decrypt_ragged, decrypt_ragged_checked, decrypt_ragged_device, encrypt, encrypt_batch,
                         encrypt_ragged, encrypt_ragged_device, encryption_tag, encryption_tags)

__all__ = ["Context", "DeviceError", "Domain", "Error", "Hash", "HashBatch", "RaggedHashBatch", "HADES_WIDTH", "InvalidIOPattern",
           "IOPatternViolation", "check_io_pattern", "compute_tag", "truncate250", "from_bytes", "to_bytes", "merkle4_tree", "merkle4_tag",
           "levels_len", "merkle4_forest", "merkle_forest_ragged", "merkle_multiproof", "merkle_multiproof_verify", "forest_ragged_append", "forest_ragged_resize", "forest_ragged_select", "forest_ragged_update_journaled", "forest_ragged_journal_swap", "ForestJournal",
           "forest_ragged_multiproof", "forest_ragged_multiproof_verify", "ForestFrontier", "ForestWitnesses", "forest_frontier_append", "forest_frontier_extract", "forest_ragged_consistency",
           "forest_consistency_verify", "forest_ragged_anchor_openings", "forest_ragged_range_proofs", "forest_range_verify", "forest_range_stride", "forest_ragged_update_sequential", "pairs_order", "pairs_unique", "encryption_tags", "encrypt_ragged", "decrypt_ragged", "decrypt_ragged_checked", "encrypt_ragged_device",
           "decrypt_ragged_device"]
