// C++ host-side test of merkle_forest_frontier_append_device / _extract_device / _bound of include/poseidon252.hpp: a forest of trees
// of different sizes is built, its frontier state is taken out, leaves are appended to that state twice (an empty tree and a refused
// append among them), and the roots are compared with the oracle's single-tree builder over all leaves so far, the state with the
// extraction from a fresh build of the grown forest, for both arities.  All buffers are page-locked host memory (p252_host_alloc),
// which the device reads and writes in place: no HIP header is needed.  The oracle (oracle/p252_oracle.h) is linked as the checker only.
#include <cstdio>
#include <cstring>
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

template <class T>
struct Pinned {  // a zeroed page-locked array of n elements (at least one)
    T* p;
    explicit Pinned(std::size_t n) : p(static_cast<T*>(p252_host_alloc((n ? n : 1) * sizeof(T)))) {
        if (!p) throw DeviceError("p252_host_alloc failed");
        std::memset(p, 0, (n ? n : 1) * sizeof(T));
    }
    ~Pinned() { p252_host_free(p); }
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
};

int main() {
    const std::vector<std::size_t> sizes = {1, 5, 16, 17, 300, 2};
    // two rounds of appends; the fifth tree's first append is too long (refused)
    const std::vector<std::vector<std::size_t>> adds = {{3, 2, 1, 0, 50, 1}, {1, 9, 47, 4, 20, 0}};
    const std::size_t n_trees = sizes.size(), max_forest = 300, max_leaves = 320, refused = 4;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
        const std::size_t bound = merkle_forest_frontier_bound(max_leaves, arity);
        EXPECT(bound == (arity == 4 ? 6u * 3u : 10u * 1u) && merkle_forest_frontier_bound(0, arity) == 0);
        const std::size_t n_levels = n_leaves / (arity - 1) + n_trees * forest_openings_stride(max_forest, arity);
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees), frontier(n_trees * bound), state_roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1), counts(n_trees), hashed(1);
        Pinned<std::uint32_t> bad(1);
        p252o_fill_random(900 + arity, leaves.p[0].data(), n_leaves);
        std::vector<std::vector<BlsScalar>> all(n_trees);  // every tree's leaves so far
        for (std::size_t t = 0; t < n_trees; ++t) {
            offsets.p[t + 1] = offsets.p[t] + sizes[t];
            all[t].assign(leaves.p + offsets.p[t], leaves.p + offsets.p[t + 1]);
        }
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_forest, roots.p, arity, ctx, levels.p);
        const ForestView forest = {leaves.p, n_leaves, offsets.p, n_trees, max_forest, levels.p};
        const ForestFrontier state = {counts.p, frontier.p, state_roots.p, n_trees, max_leaves};
        merkle_forest_frontier_extract_device(forest, roots.p, state, arity, ctx, bad.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(bad.p[0] == 0);
        for (std::size_t t = 0; t < n_trees; ++t) EXPECT(counts.p[t] == sizes[t] && state_roots.p[t] == roots.p[t]);
        std::uint64_t want_hashed = 0;
        for (std::size_t round = 0; round < adds.size(); ++round) {
            std::size_t n_add = 0;
            for (std::size_t m : adds[round]) n_add += m;
            Pinned<BlsScalar> add(n_add);
            Pinned<std::uint64_t> add_offsets(n_trees + 1);
            p252o_fill_random(950 + 10 * round + arity, add.p[0].data(), n_add);
            for (std::size_t t = 0; t < n_trees; ++t) {
                add_offsets.p[t + 1] = add_offsets.p[t] + adds[round][t];
                const std::size_t n = all[t].size(), m = n + adds[round][t] > max_leaves ? 0 : adds[round][t];
                all[t].insert(all[t].end(), add.p + add_offsets.p[t], add.p + add_offsets.p[t] + m);
                std::size_t w = n + m, clean = n;
                while (m && w > 1) {
                    w = (w + arity - 1) / arity;
                    clean /= arity;
                    want_hashed += w - clean;
                }
            }
            merkle_forest_frontier_append_device(state, add.p, n_add, add_offsets.p, arity, ctx, bad.p, hashed.p);
            detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
            EXPECT(bad.p[0] == 1 && hashed.p[0] == want_hashed);  // (the one refusal of the first round; both counters add up)
            for (std::size_t t = 0; t < n_trees; ++t) {
                BlsScalar expected;
                std::vector<BlsScalar> lv(all[t].size() + 64);
                if (arity == 4)
                    p252o_merkle4_tree(tag.data(), all[t][0].data(), all[t].size(), expected.data(), lv[0].data());
                else
                    p252o_merkle2_tree(tag.data(), all[t][0].data(), all[t].size(), expected.data(), lv[0].data());
                EXPECT(state_roots.p[t] == expected && counts.p[t] == all[t].size());
                if (round == 0 && (t == 3 || t == refused)) EXPECT(state_roots.p[t] == roots.p[t]);  // untouched trees keep their roots
            }
        }
        // the state equals the extraction from a fresh build of the grown forest
        std::size_t total = 0;
        for (const auto& v : all) total += v.size();
        const std::size_t n_levels2 = total / (arity - 1) + n_trees * forest_openings_stride(max_leaves, arity);
        Pinned<BlsScalar> leaves2(total), levels2(n_levels2), roots2(n_trees), frontier2(n_trees * bound), state_roots2(n_trees);
        Pinned<std::uint64_t> offsets2(n_trees + 1), counts2(n_trees);
        for (std::size_t t = 0; t < n_trees; ++t) {
            std::memcpy(leaves2.p + offsets2.p[t], all[t].data(), all[t].size() * sizeof(BlsScalar));
            offsets2.p[t + 1] = offsets2.p[t] + all[t].size();
        }
        merkle_forest_ragged_device(leaves2.p, total, offsets2.p, n_trees, max_leaves, roots2.p, arity, ctx, levels2.p);
        const ForestView grown = {leaves2.p, total, offsets2.p, n_trees, max_leaves, levels2.p};
        merkle_forest_frontier_extract_device(grown, roots2.p, ForestFrontier{counts2.p, frontier2.p, state_roots2.p, n_trees, max_leaves}, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(std::memcmp(counts.p, counts2.p, n_trees * 8) == 0);
        EXPECT(std::memcmp(frontier.p, frontier2.p, n_trees * bound * sizeof(BlsScalar)) == 0);
        EXPECT(std::memcmp(state_roots.p, state_roots2.p, n_trees * sizeof(BlsScalar)) == 0);
    }
    bool threw = false;
    try {
        merkle_forest_frontier_append_device(ForestFrontier{}, nullptr, 0, nullptr, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
