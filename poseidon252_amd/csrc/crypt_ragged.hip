// crypt_ragged.hip — the launcher of p252_{encrypt,decrypt}_ragged*: n messages of DIFFERENT lengths encrypted or decrypted in one
// call.  Nothing here runs the permutation: the sponge is k_crypt<*, true> / k_crypt_coop<*, true> (kernels.hip).
//
// Those kernels keep every sponge position wave-uniform (scalar switches on the position, one inlined permutation inside scalar
// control flow, a lane index compared with a uniform position), so a wave must never hold two lengths.  Four small kernels sort
// the message indices by EXACT length, longest first — they stand in ragged.hip, beside the counting sort they are modelled on
// (the bucket primitives of blockops.hpp) — and the scan between the two passes rounds every bucket's size up to a multiple of
// G slots (G = 64 messages for the one-lane build, 8 for the lane-group build), so that every non-empty bucket starts at a
// multiple of G:
//   k_crypt_ragged_clear    counters to zero, sentinels into the order array
//   k_crypt_ragged_hist     per tile of 2,048 messages: bins in LDS, one global atomic per non-empty bin
//   k_crypt_ragged_scan     one block: padded bucket sizes -> bucket starts, descending bucket order
//   k_crypt_ragged_scatter  per tile: LDS rank within the bin, one global atomic per non-empty bin reserves the tile's range
// Bucket L holds the messages of length L (1 .. P252_CRYPT_RAGGED_MAX_LEN: 2,049 LDS counters); bucket 0 holds the bad messages
// (crypt_span_bad, crypt_args.h) and sorts last.  The order array is filled with an all-ones sentinel first; the slots the padding
// leaves stay sentinels and their lanes exit at once.  The order within a bucket depends on atomic timing; the outputs do not.
#include <hip/hip_runtime.h>

#include "crypt_ragged.h"
#include "kernels.h"

namespace p252 {

// ---------------------------------------------------------------------------------------------
// launcher (C++ linkage, called from api.cpp)
// ---------------------------------------------------------------------------------------------
hipError_t launch_crypt_ragged(bool decrypt, int variant, const int32_t* tab, const void* tags, size_t max_len, const void* in, uint64_t n_scalars,
                               const void* offsets, const void* secrets, const void* nonces, void* out, void* flags, size_t n, void* n_bad,
                               void* order, void* hist, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const bool coop = coop8(n);
    const hipError_t e = launch_crypt_ragged_schedule(offsets, n, max_len, n_scalars, coop, order, hist, st);
    if (e != hipSuccess) return e;
    CryptRaggedArgs rg;
    rg.tags = tags;
    rg.offsets = static_cast<const uint64_t*>(offsets);
    rg.order = static_cast<const unsigned long long*>(order);
    rg.n_scalars = n_scalars;
    rg.slots = crypt_ragged_slots(n, max_len, coop);
    rg.n_bad = static_cast<unsigned*>(n_bad);
    rg.variant = variant;
    return launch_crypt_mixed(decrypt, coop, tab, (unsigned)max_len, in, secrets, nonces, out, flags, n, rg, st);
}

}  // namespace p252
