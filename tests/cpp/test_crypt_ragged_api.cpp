// C++ host-side test of encrypt_ragged / decrypt_ragged (include/poseidon252.hpp): messages of the reference's test lengths
// (tests/encryption.rs: 42 and 21 scalars) and a few more, of different lengths in ONE call, each cipher equal to the oracle's
// encryption of that message alone, in both variants.  The oracle (oracle/p252_oracle.h) is linked as the checker only.
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
    const std::vector<size_t> lens = {42, 21, 1, 4, 5, 9, 21, 3, 43, 8};
    const size_t n = lens.size();
    std::vector<std::uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + lens[i];
    std::vector<BlsScalar> msgs(off[n]), secrets(2 * n), nonces(n);
    p252o_fill_random(7, msgs[0].data(), msgs.size());
    p252o_fill_random(8, secrets[0].data(), secrets.size());
    p252o_fill_random(9, nonces[0].data(), nonces.size());
    for (int variant : {P252_CRYPT_STREAM, P252_CRYPT_DUPLEX}) {
        const std::vector<BlsScalar> c = encrypt_ragged(msgs, off, secrets, nonces, variant);
        EXPECT(c.size() == off[n] + n);
        const std::vector<BlsScalar> tags = encryption_tags(43, variant);
        for (size_t i = 0; i < n; ++i) {
            BlsScalar tag{};
            EXPECT(p252o_encryption_tag_v(variant, lens[i], tag.data()) == 0);
            EXPECT(tags[lens[i] - 1] == tag && encryption_tag(lens[i], variant) == tag);
            std::vector<BlsScalar> exp(lens[i] + 1);
            EXPECT(p252o_encrypt_v(variant, tag.data(), msgs[off[i]].data(), lens[i], secrets[2 * i].data(), nonces[i].data(), exp[0].data()) == 0);
            for (size_t k = 0; k <= lens[i]; ++k) EXPECT(c[off[i] + i + k] == exp[k]);
        }
        std::vector<std::uint8_t> ok;
        EXPECT(decrypt_ragged(c, off, secrets, nonces, ok, variant) == msgs);
        for (std::uint8_t f : ok) EXPECT(f == 1);
        EXPECT(decrypt_ragged_checked(c, off, secrets, nonces, variant) == msgs);
        std::vector<BlsScalar> bad = c;
        bad[off[4] + 4][0] ^= 1;  // the first scalar of cipher 4
        decrypt_ragged(bad, off, secrets, nonces, ok, variant);
        for (size_t i = 0; i < n; ++i) EXPECT(ok[i] == (i == 4 ? 0 : 1));
        bool threw = false;
        try {
            decrypt_ragged_checked(bad, off, secrets, nonces, variant);
        } catch (const DecryptionFailed&) {
            threw = true;
        }
        EXPECT(threw);
    }
    bool threw = false;
    try {  // an empty message: Error::InvalidIOPattern, before anything is launched
        encrypt_ragged(msgs, {0, 3, 3}, {secrets[0], secrets[1], secrets[2], secrets[3]}, {nonces[0], nonces[1]});
    } catch (const IoPatternError& e) {
        threw = e.kind == IoPatternError::InvalidIOPattern;
    }
    EXPECT(threw);
    threw = false;
    try {
        encryption_tags(P252_CRYPT_RAGGED_MAX_LEN + 1);
    } catch (const std::exception&) {
        threw = true;
    }
    EXPECT(threw);
    EXPECT(encrypt_ragged({}, {0}, {}, {}).empty());
    if (failures) return 1;
    std::printf("ALL PASSED\n");
    return 0;
}
