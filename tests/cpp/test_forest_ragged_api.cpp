// C++ host-side test of merkle_forest_ragged (include/poseidon252.hpp): trees of different sizes in ONE call, each root and each
// tree's levels block equal to the oracle's builder of that tree alone, for both arities.  The oracle (oracle/p252_oracle.h) is
// linked as the checker only.
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
    const std::vector<size_t> sizes = {1, 5, 16, 17, 300, 2, 65};
    std::vector<std::vector<BlsScalar>> trees;
    for (size_t t = 0; t < sizes.size(); ++t) {
        std::vector<BlsScalar> leaves(sizes[t]);
        p252o_fill_random(300 + t, leaves[0].data(), leaves.size());
        trees.push_back(leaves);
    }
    for (unsigned arity : {4u, 2u}) {
        const RaggedForest f = merkle_forest_ragged(trees, arity, true);
        const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
        EXPECT(f.roots.size() == trees.size() && f.level_offsets.size() == trees.size() + 1);
        for (size_t t = 0; t < trees.size(); ++t) {
            const size_t ll = f.level_offsets[t + 1] - f.level_offsets[t];
            BlsScalar root{};
            std::vector<BlsScalar> levels(ll ? ll : 1);
            if (arity == 4)
                p252o_merkle4_tree(tag.data(), trees[t][0].data(), trees[t].size(), root.data(), levels[0].data());
            else
                p252o_merkle2_tree(tag.data(), trees[t][0].data(), trees[t].size(), root.data(), levels[0].data());
            EXPECT(f.roots[t] == root);
            for (size_t k = 0; k < ll; ++k) EXPECT(f.levels[f.level_offsets[t] + k] == levels[k]);
        }
        EXPECT(merkle_forest_ragged(trees, arity).roots == f.roots);
    }
    bool threw = false;
    try {
        merkle_forest_ragged({std::vector<BlsScalar>(3), std::vector<BlsScalar>()});
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
