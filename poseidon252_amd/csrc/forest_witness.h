// forest_witness.h — launch interface between forest_frontier.hip's append and forest_witness.hip: the openings of marked leaves kept
// current while a forest that is kept only as its frontiers grows (p252_merkle{4,2}_forest_frontier_append_witness_device_into).  The
// witnesses have the layout of p252_merkle{4,2}_forest_ragged_openings_device at the stride D = depth(max_leaves); the pass hashes
// nothing: every sibling it writes is in the append's scratch, in the frontier's old rows or zero.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "forest_frontier.h"

namespace p252 {

constexpr unsigned FOREST_WITNESS_BLOCK = 256;  // threads of a block: floor(256 / D) whole witnesses, one lane per (witness, row)

// The caller's k witnesses, all device arrays: witness i names leaf leaf_ids[i] of tree tree_ids[i] (read only); leaves[k],
// siblings[k][D][arity - 1], positions[k][D] and depths[k] are read and updated in place.  n_bad (uint32) may be null.
struct ForestWitnesses {
    const uint32_t* tree_ids = nullptr;
    const uint64_t* leaf_ids = nullptr;
    size_t k = 0;
    void* leaves = nullptr;
    void* siblings = nullptr;
    uint8_t* positions = nullptr;
    uint8_t* depths = nullptr;
    unsigned* n_bad = nullptr;
};

// blocks of one refresh of k witnesses at stride D (what the host checks against the grid's limit before anything is queued)
inline size_t forest_witness_blocks(size_t k, unsigned D) {
    const size_t per_block = D ? FOREST_WITNESS_BLOCK / D : FOREST_WITNESS_BLOCK;
    return (k + per_block - 1) / per_block;
}

// One launch on `st`, between the append's last digest launch and k_ff_finish: the view's frontier still holds the OLD rows, its values
// every level's computed nodes.  A view whose trees all have m_t == 0 (nothing to append, or n_trees == 0) is read for its counts alone:
// the pass then only marks and counts the bad witnesses.  witnesses.k == 0 launches nothing.
hipError_t launch_forest_witness_refresh(const ForestFrontierView& view, const ForestWitnesses& witnesses, hipStream_t st);

}  // namespace p252
