// primtest.hip — device build of primtest.hpp: one kernel per field primitive, one case per lane (tests/test_primitives_gpu.py).
// The kernels are straight-line arithmetic between plain global buffers of n * stride elements; lanes beyond n return before
// they touch memory.  Launchers run on the null stream and return hipGetLastError().  Test-only; libposeidon252_hip.so
// contains none of these.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "primtest.hpp"

using namespace p252;

#define P252_PT_DEV(name, NA, NB, NO)                                                                                      \
    __global__ void __launch_bounds__(P252_BLOCK)                                                                          \
        k_pt_##name(const int32_t* __restrict__ a, const int64_t* __restrict__ b, int32_t* __restrict__ out, size_t n) {   \
        const size_t idx = (size_t)blockIdx.x * P252_BLOCK + threadIdx.x;                                                  \
        if (idx >= n) return;                                                                                              \
        pt::name(a + idx * (NA), b + idx * (NB), out + idx * (NO));                                                        \
    }                                                                                                                      \
    extern "C" int ptd_##name(const int32_t* a, const int64_t* b, int32_t* out, size_t n) {                                \
        if (n == 0) return (int)hipSuccess;                                                                                \
        const unsigned blocks = (unsigned)((n + P252_BLOCK - 1) / P252_BLOCK);                                             \
        hipLaunchKernelGGL(k_pt_##name, dim3(blocks), dim3(P252_BLOCK), 0, 0, a, b, out, n);                               \
        return (int)hipGetLastError();                                                                                     \
    }
P252_PRIMTEST_LIST(P252_PT_DEV)
#undef P252_PT_DEV

// The device-only output stage: raw digits in, store_output<false> to out[idx][0] and store_output<true> to out[idx][1]
// (two 32-byte records per case; out must be 16-byte aligned, as every Scalar32 buffer of the kernels is).
__global__ void __launch_bounds__(P252_BLOCK) k_pt_store_output(const int32_t* __restrict__ a, Scalar32* __restrict__ out, size_t n) {
    const size_t idx = (size_t)blockIdx.x * P252_BLOCK + threadIdx.x;
    if (idx >= n) return;
    const E29 e = pt::ld(a + idx * NL);
    store_output<false>(out + 2 * idx, e);
    store_output<true>(out + 2 * idx + 1, e);
}
extern "C" int ptd_store_output(const int32_t* a, const int64_t*, int32_t* out, size_t n) {
    if (n == 0) return (int)hipSuccess;
    if ((uintptr_t)out & 15u) return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n + P252_BLOCK - 1) / P252_BLOCK);
    hipLaunchKernelGGL(k_pt_store_output, dim3(blocks), dim3(P252_BLOCK), 0, 0, a, reinterpret_cast<Scalar32*>(out), n);
    return (int)hipGetLastError();
}
