// C++ host-side test of RaggedHashBatch (include/poseidon252.hpp): messages of the reference's test shapes (tests/hash.rs: 3, 5
// and 15 scalars) and a few more, of different lengths in ONE call, each equal to the oracle's digest of that message alone.
// The oracle (oracle/p252_oracle.h) is linked as the checker only.
#include <cstdio>
#include <vector>

#include "poseidon252.hpp"
#include "../../oracle/p252_oracle.h"

using namespace dusk_poseidon_hip;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    const std::vector<size_t> lens = {3, 5, 15, 1, 42, 4, 9, 16, 5, 3};
    std::vector<std::vector<BlsScalar>> msgs;
    for (size_t i = 0; i < lens.size(); ++i) {
        std::vector<BlsScalar> m(lens[i]);
        p252o_fill_random(100 + i, m[0].data(), m.size());
        msgs.push_back(m);
    }
    for (size_t out_len : {1, 3}) {
        RaggedHashBatch rb(Domain::Other, out_len);
        const std::vector<BlsScalar> got = rb.digest(msgs);
        const std::vector<JubJubRaw> trunc = rb.digest_truncated(msgs);
        EXPECT(got.size() == msgs.size() * out_len && trunc.size() == got.size());
        for (size_t i = 0; i < msgs.size(); ++i) {
            BlsScalar tag{};
            p252o_tag(P252_DOMAIN_OTHER, &lens[i], 1, out_len, tag.data());
            std::vector<BlsScalar> exp(out_len);
            p252o_hash_batch(tag.data(), msgs[i][0].data(), lens[i], out_len, exp[0].data(), 1);
            for (size_t o = 0; o < out_len; ++o) {
                EXPECT(got[i * out_len + o] == exp[o]);
                JubJubRaw t{};
                p252o_truncate250(exp[o].data(), t.data());
                EXPECT(trunc[i * out_len + o] == t);
            }
            EXPECT(rb.tags(lens[i])[lens[i] - 1] == tag);
        }
    }
    bool threw = false;
    try {
        RaggedHashBatch(Domain::Merkle4);
    } catch (const IoPatternError& e) {
        threw = e.kind == IoPatternError::IOPatternViolation;
    }
    EXPECT(threw);
    threw = false;
    try {
        RaggedHashBatch rb;
        rb.digest({{BlsScalar{}}, {}});
    } catch (const IoPatternError& e) {
        threw = e.kind == IoPatternError::InvalidIOPattern;
    }
    EXPECT(threw);
    if (failures) return 1;
    std::printf("ALL PASSED\n");
    return 0;
}
