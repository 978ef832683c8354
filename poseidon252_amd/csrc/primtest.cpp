// primtest.cpp — CPU build of primtest.hpp: one loop over n cases per field primitive (tests/test_primitives_cpu.py).
// Its own translation unit, apart from hosttest.cpp, so that it compiles in seconds: the mutant control of that test module
// rebuilds it once per mutated header.  Test-only; not part of libposeidon252_hip.so.
#include <cstddef>
#include <cstdint>

#include "primtest.hpp"

using namespace p252;

extern "C" {

#define P252_PT_HOST(name, NA, NB, NO)                                                             \
    void pt_##name(const int32_t* a, const int64_t* b, int32_t* out, size_t n) {                   \
        for (size_t i = 0; i < n; ++i) pt::name(a + i * (NA), b + i * (NB), out + i * (NO));       \
    }                                                                                              \
    void pt_shape_##name(int32_t s[3]) {                                                           \
        s[0] = (NA);                                                                               \
        s[1] = (NB);                                                                               \
        s[2] = (NO);                                                                               \
    }
P252_PRIMTEST_LIST(P252_PT_HOST)
#undef P252_PT_HOST

// where the rows the tests feed to the integer-row primitives lie in the table ht_tables29 returns
void pt_layout(int32_t out[16]) {
    typedef Tab29Layout Lay;
    const int32_t v[16] = {Lay::C_FIRST, Lay::INT_N,     Lay::AI_AB,      Lay::AI_KAPPA,  Lay::AI_ENT_N, Lay::AI_ENT_FIX,
                           Lay::AI_ENT_ADD, Lay::AI_KG,  Lay::AI_EX_N,    Lay::AI_EX_FIX, Lay::AI_EX_ADD, Lay::AI_F,
                           Lay::INT_G,   Lay::INT_F,     ENTRY_W0_INT,    Lay::TOTAL};
    for (int k = 0; k < 16; ++k) out[k] = v[k];
}

}  // extern "C"
