// crypt_args.h — what kernels.hip needs of the mixed-length encryption calls (crypt_ragged.h has the rest): the extra kernel argument
// of k_crypt<*, RAGGED> / k_crypt_coop<*, RAGGED>, the rule for a bad message, and the launcher of those instantiations.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace p252 {

constexpr unsigned long long CRYPT_RAGGED_SENTINEL = ~0ull;  // a padding slot of the order array

// message [a, b) of the offsets array is bad: empty, longer than max_len, decreasing (also where the unsigned difference wraps to
// something short), or ending past the array.  The schedule and the kernels ask this one function, and nothing is read or written
// through a bad message.
__host__ __device__ inline bool crypt_span_bad(uint64_t a, uint64_t b, uint64_t max_len, uint64_t n_scalars) {
    return b <= a || b - a > max_len || b > n_scalars;
}

// what the ragged instantiations of k_crypt / k_crypt_coop take beside the arguments of the fixed-length ones
struct CryptRaggedArgs {
    const void* tags;               // max_len scalars
    const uint64_t* offsets;        // n + 1 message offsets
    const unsigned long long* order;  // `slots` message indices or sentinels
    uint64_t n_scalars;             // scalars in the message-side array
    size_t slots;
    unsigned* n_bad;                // may be null
    int variant;
};
struct CryptFixedArgs {};  // (the fixed-length instantiations take nothing more)

// kernels.hip: the hashing launch alone, over an order array the schedule has filled
hipError_t launch_crypt_mixed(bool decrypt, bool coop, const int32_t* tab, unsigned max_len, const void* in, const void* secrets,
                                      const void* nonces, void* out, void* flags, size_t n, const CryptRaggedArgs& rg, hipStream_t st);

}  // namespace p252
