// pairs.h — launch interface between api_forest.cpp and pairs.hip: the stable sort and the de-duplication of k (tree id, leaf id) pairs
// on the device (p252_pairs_order_device_into, p252_pairs_unique_device_into), the order that the sequential updates and the shared
// proofs take.  A least-significant-digit radix sort over the 12 bytes of the 96-bit key: include/poseidon252_hip.h and DESIGN.md.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace p252 {

constexpr unsigned PAIRS_BLOCK = 256;       // lanes of a block of the tile kernels: four waves
constexpr unsigned PAIRS_ROUNDS = 8;        // records a lane takes, one per round; a round is PAIRS_BLOCK neighbours of the list
constexpr unsigned PAIRS_TILE = 2048;       // = PAIRS_BLOCK * PAIRS_ROUNDS: the records of one block
constexpr unsigned PAIRS_SCAN_BLOCK = 256;  // tiles one trip of a scan over the tiles covers (k_po_scan, k_po_scan_heads)
constexpr unsigned PAIRS_DIGITS = 256;      // values of one 8-bit digit
constexpr unsigned PAIRS_PASSES = 12;       // digits of a key: bytes 0 .. 7 of the leaf id, then bytes 0 .. 3 of the tree id
static_assert(PAIRS_TILE == PAIRS_BLOCK * PAIRS_ROUNDS, "a tile is one record per lane and round");
static_assert(PAIRS_BLOCK == PAIRS_DIGITS, "lane d of a block owns digit d");

// the work area of a call with k pairs, offsets into the first scratch buffer of the stream: the control words (what varies, the
// plan of the passes), the totals of the digits, two ping-pong arrays of 16-byte records {tree, index, leaf} and the per-tile digit
// counts, digit-major (the heads' per-tile counts of the de-duplication lie over them, after the sort).
// 32 + 1024 / PAIRS_TILE = 32.5 bytes a pair (rounded up to whole tiles), 1280 bytes.
struct PairsWork {
    size_t ctl, totals, recs[2], counts, bytes, n_tiles;
};
inline PairsWork pairs_work(size_t k) {
    PairsWork w{};
    w.n_tiles = (k + PAIRS_TILE - 1) / PAIRS_TILE;
    w.ctl = 0;
    w.totals = 256;
    w.recs[0] = w.totals + PAIRS_DIGITS * 4;
    w.recs[1] = w.recs[0] + k * 16;
    w.counts = w.recs[1] + k * 16;
    w.bytes = w.counts + w.n_tiles * PAIRS_DIGITS * 4;
    return w;
}

// 0 < k < 2^32; tree_ids may be null (every pair of tree 0); work = pairs_work(k).bytes of the stream's scratch.
// order: uint32[k], the indices sorted by (tree id, leaf id, index).
hipError_t launch_pairs_order(const void* tree_ids, const void* leaf_ids, size_t k, void* order, void* work, hipStream_t st);
// the distinct pairs ascending into the first *n_unique (uint64, required) entries of each non-null output
hipError_t launch_pairs_unique(const void* tree_ids, const void* leaf_ids, size_t k, void* tree_ids_out, void* leaf_ids_out, void* indices_out,
                               void* first, void* n_unique, void* work, hipStream_t st);

}  // namespace p252
