// crypt_calls_dump.cpp — csrc/crypt_calls.hpp compiled for the host: the sponge-call sequence the RAGGED instantiations of k_crypt
// compute in the kernel, printed one line per (variant, length) as
//   variant <TAB> length <TAB> kind:count kind:count ...
// for the lengths given on the command line.  tests/test_crypt_ragged_cpu.py compares the lines with the call table of api.cpp as
// tests/shapecases.py restates it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../poseidon252_amd/csrc/crypt_calls.hpp"

int main(int argc, char** argv) {
    for (int variant : {p252::CRYPT_STREAM, p252::CRYPT_DUPLEX})
        for (int i = 1; i < argc; ++i) {
            const uint32_t len = (uint32_t)std::strtoul(argv[i], nullptr, 10);
            std::printf("%d\t%u\t", variant, len);
            const uint32_t calls = p252::crypt_n_calls(variant, len);
            for (uint32_t ci = 0; ci < calls; ++ci) {
                const uint32_t w = p252::crypt_call(variant, len, ci);
                std::printf("%s%u:%u", ci ? " " : "", w >> 29, w & 0x1fffffffu);
            }
            std::printf("\n");
        }
    return 0;
}
