// crypt_calls.hpp — the sponge-call sequence of dusk_safe::encrypt as a function of (variant, len, call index): what api.cpp's
// crypt_program() writes as a table (one word per call: kind << 29 | len; kinds as in kernels.hip k_crypt), computed one call at a
// time.  The ragged instantiations of k_crypt / k_crypt_coop call it in the kernel (a length per wave: no table to upload, no
// synchronisation); tests/cpp/crypt_calls_dump.cpp compiles it for the host and compares it with the table.  Plain C++: no HIP
// header, no state.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define P252_CALLS_FN __host__ __device__ __forceinline__
#else
#define P252_CALLS_FN inline
#endif

namespace p252 {

constexpr int CRYPT_STREAM = 0, CRYPT_DUPLEX = 1;  // P252_CRYPT_STREAM / P252_CRYPT_DUPLEX (include/poseidon252_hip.h)

// number of sponge calls for a message of len >= 1 scalars.  STREAM: [Absorb(2), Absorb(1), Squeeze(len), Absorb(len), Squeeze(1)];
// DUPLEX: [Absorb(2), Absorb(1), {Squeeze(c), Absorb(c)}*, Squeeze(1)], c = min(4, remaining)
P252_CALLS_FN uint32_t crypt_n_calls(int variant, uint32_t len) { return variant == CRYPT_STREAM ? 5u : 3u + 2u * ((len + 3u) / 4u); }

// call ci < crypt_n_calls(variant, len) as the word kind << 29 | count
P252_CALLS_FN uint32_t crypt_call(int variant, uint32_t len, uint32_t ci) {
    if (ci == 0) return (0u << 29) | 2u;  // Absorb(2): shared secret (u, v)
    if (ci == 1) return (1u << 29) | 1u;  // Absorb(1): nonce
    if (ci + 1 == crypt_n_calls(variant, len)) return (4u << 29) | 1u;  // Squeeze(1): MAC
    const uint32_t kind = 2u + ((ci - 2u) & 1u);  // 2 = squeeze masks, 3 = absorb the plaintext
    if (variant == CRYPT_STREAM) return (kind << 29) | len;
    const uint32_t done = ((ci - 2u) >> 1) * 4u, left = len - done;
    return (kind << 29) | (left < 4u ? left : 4u);
}

}  // namespace p252
