// crypt_ragged.h — launch interface between api.cpp and crypt_ragged.hip / kernels.hip: n encryptions or decryptions of messages of
// DIFFERENT lengths in one call (p252_{encrypt,decrypt}_ragged*).  Message i = messages[offsets[i] .. offsets[i+1]) scalars, its
// cipher the L_i + 1 scalars at ciphers[offsets[i] + i ..]; tags[L - 1] is the tag of a message of length L.
//
// The kernels (k_crypt<*, true>, k_crypt_coop<*, true>, kernels.hip) keep the control flow of the fixed-length call: every sponge
// position is wave-uniform.  That holds only if a wave never meets two lengths, so the schedule here is a condition of
// correctness, not a tuning (P252_RAGGED_SORT does not apply): the message indices are sorted by EXACT length, longest first, and
// every non-empty bucket starts at a multiple of G slots — G = 64 messages for the one-lane build, G = 8 for the lane-group build
// (8 lanes per message: a wave holds 8).  The slots between buckets hold an all-ones sentinel; a lane (group) that reads it exits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/poseidon252_hip.h"
#include "crypt_args.h"
#include "kernels.h"

namespace p252 {

// one bucket per length 1 .. P252_CRYPT_RAGGED_MAX_LEN; bucket 0 holds the bad messages, which sort last
constexpr unsigned CRYPT_RAGGED_BUCKETS = P252_CRYPT_RAGGED_MAX_LEN + 1;

// messages per length-uniform group of slots: a wave of the one-lane build, a wave of eight lane groups
inline size_t crypt_ragged_group(bool coop) { return coop ? 8 : 64; }
// slots of the order array.  The host cannot know how many lengths occur without a synchronisation; every non-empty bucket pads
// its end by at most G - 1 slots and there are at most max_len + 1 buckets in use
inline size_t crypt_ragged_slots(size_t n, size_t max_len, bool coop) {
    const size_t g = crypt_ragged_group(coop);
    return (n + (g - 1) * (max_len + 1) + g - 1) / g * g;
}
inline size_t crypt_ragged_order_bytes(size_t n, size_t max_len) { return crypt_ragged_slots(n, max_len, coop8(n)) * sizeof(uint64_t); }
inline size_t crypt_ragged_hist_bytes() { return (size_t)CRYPT_RAGGED_BUCKETS * sizeof(uint64_t); }

// the schedule: order (crypt_ragged_order_bytes) and hist (crypt_ragged_hist_bytes) are the call's scratch.  No hashing.
hipError_t launch_crypt_ragged_schedule(const void* offsets, size_t n, size_t max_len, uint64_t n_scalars, bool coop, void* order, void* hist,
                                        hipStream_t st);
// schedule + k_crypt<decrypt, true> (k_crypt_coop for batches coop8 takes) on `st`; in / out: the message and the cipher side
hipError_t launch_crypt_ragged(bool decrypt, int variant, const int32_t* tab, const void* tags, size_t max_len, const void* in, uint64_t n_scalars,
                               const void* offsets, const void* secrets, const void* nonces, void* out, void* flags, size_t n, void* n_bad,
                               void* order, void* hist, hipStream_t st);
}  // namespace p252
