// C++ host-side test of merkle_forest_frontier_append_witness_device of include/poseidon252.hpp: a forest of trees of different sizes
// is built, the openings of some of its leaves are taken and its frontier state is extracted; then leaves are appended to the state
// twice with those openings — and the openings of leaves that the appends bring — kept current by the same call.  After each round
// every witness of a leaf that is in its tree verifies against the state's roots and no other does; at the end all of them equal,
// byte for byte, the openings out of a fresh build of the grown forest, for both arities.  All buffers are page-locked host memory
// (p252_host_alloc), which the device reads and writes in place: no HIP header is needed.
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
    const std::size_t n_trees = sizes.size(), max_leaves = 320;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    // the watch list: every 3rd leaf that is there from the start, every 2nd that a round brings (a refused one among them), and one
    // pair that names no leaf at all
    std::vector<std::uint32_t> tid;
    std::vector<std::uint64_t> lid;
    std::vector<std::size_t> final_count = sizes;
    for (std::size_t t = 0; t < n_trees; ++t) {
        for (std::size_t p = 0; p < sizes[t]; p += 3) tid.push_back((std::uint32_t)t), lid.push_back(p);
        std::size_t n = sizes[t];
        for (const auto& round : adds) {
            const bool refused = n + round[t] > max_leaves;
            for (std::size_t p = n; p < n + round[t]; p += 2) tid.push_back((std::uint32_t)t), lid.push_back(p);
            if (!refused) n += round[t];
        }
        final_count[t] = n;
    }
    tid.push_back((std::uint32_t)n_trees), lid.push_back(0);
    const std::size_t k = tid.size();
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const std::size_t bound = merkle_forest_frontier_bound(max_leaves, arity), D = forest_openings_stride(max_leaves, arity), per = arity - 1;
        const std::size_t n_levels = n_leaves / per + n_trees * D;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees), frontier(n_trees * bound), state_roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1), counts(n_trees), hashed(1), d_lid(k);
        Pinned<std::uint32_t> bad(1), bad_witness(1), d_tid(k);
        Pinned<BlsScalar> w_leaves(k), w_sib(k * D * per);
        Pinned<std::uint8_t> w_pos(k * D), w_dep(k), ok(k);
        std::memcpy(d_tid.p, tid.data(), k * 4);
        std::memcpy(d_lid.p, lid.data(), k * 8);
        p252o_fill_random(700 + arity, leaves.p[0].data(), n_leaves);
        std::vector<std::vector<BlsScalar>> all(n_trees);  // every tree's leaves so far
        for (std::size_t t = 0; t < n_trees; ++t) {
            offsets.p[t + 1] = offsets.p[t] + sizes[t];
            all[t].assign(leaves.p + offsets.p[t], leaves.p + offsets.p[t + 1]);
        }
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        // the hand-over of a stored forest: the openings of the leaves to watch, then the extraction (the leaves to come are bad for now)
        merkle_forest_ragged_openings_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, d_tid.p, d_lid.p, k, w_leaves.p, w_sib.p,
                                             w_pos.p, w_dep.p, arity, ctx);
        const ForestView forest = {leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p};
        const ForestFrontier state = {counts.p, frontier.p, state_roots.p, n_trees, max_leaves};
        merkle_forest_frontier_extract_device(forest, roots.p, state, arity, ctx);
        const ForestWitnesses witnesses = {d_tid.p, d_lid.p, k, w_leaves.p, w_sib.p, w_pos.p, w_dep.p};
        for (std::size_t round = 0; round < adds.size(); ++round) {
            std::size_t n_add = 0;
            for (std::size_t m : adds[round]) n_add += m;
            Pinned<BlsScalar> add(n_add);
            Pinned<std::uint64_t> add_offsets(n_trees + 1);
            p252o_fill_random(750 + 10 * round + arity, add.p[0].data(), n_add);
            for (std::size_t t = 0; t < n_trees; ++t) {
                add_offsets.p[t + 1] = add_offsets.p[t] + adds[round][t];
                const std::size_t m = all[t].size() + adds[round][t] > max_leaves ? 0 : adds[round][t];
                all[t].insert(all[t].end(), add.p + add_offsets.p[t], add.p + add_offsets.p[t] + m);
            }
            bad_witness.p[0] = 0;
            merkle_forest_frontier_append_witness_device(state, add.p, n_add, add_offsets.p, witnesses, arity, ctx, bad.p, hashed.p, bad_witness.p);
            merkle_forest_ragged_verify_device(w_leaves.p, w_sib.p, w_pos.p, w_dep.p, D, d_tid.p, state_roots.p, n_trees, ok.p, k, arity, ctx);
            detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
            EXPECT(bad.p[0] == 1);  // (the one refusal of the first round)
            std::size_t want_bad = 0;
            for (std::size_t i = 0; i < k; ++i) {
                const bool in_tree = tid[i] < n_trees && lid[i] < all[tid[i]].size();
                want_bad += !in_tree;
                EXPECT(ok.p[i] == (in_tree ? 1 : 0) && (w_dep.p[i] == 0xFF) == !in_tree);
            }
            EXPECT(bad_witness.p[0] == want_bad);
            for (std::size_t t = 0; t < n_trees; ++t) EXPECT(counts.p[t] == all[t].size());
        }
        for (std::size_t t = 0; t < n_trees; ++t) EXPECT(all[t].size() == final_count[t]);
        // every witness equals the opening out of a fresh build of the grown forest
        std::size_t total = 0;
        for (const auto& v : all) total += v.size();
        Pinned<BlsScalar> leaves2(total), levels2(total / per + n_trees * D), roots2(n_trees), f_leaves(k), f_sib(k * D * per);
        Pinned<std::uint64_t> offsets2(n_trees + 1);
        Pinned<std::uint8_t> f_pos(k * D), f_dep(k);
        for (std::size_t t = 0; t < n_trees; ++t) {
            std::memcpy(leaves2.p + offsets2.p[t], all[t].data(), all[t].size() * sizeof(BlsScalar));
            offsets2.p[t + 1] = offsets2.p[t] + all[t].size();
        }
        merkle_forest_ragged_device(leaves2.p, total, offsets2.p, n_trees, max_leaves, roots2.p, arity, ctx, levels2.p);
        merkle_forest_ragged_openings_device(leaves2.p, total, offsets2.p, n_trees, max_leaves, levels2.p, d_tid.p, d_lid.p, k, f_leaves.p, f_sib.p,
                                             f_pos.p, f_dep.p, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(std::memcmp(w_leaves.p, f_leaves.p, k * sizeof(BlsScalar)) == 0);
        EXPECT(std::memcmp(w_sib.p, f_sib.p, k * D * per * sizeof(BlsScalar)) == 0);
        EXPECT(std::memcmp(w_pos.p, f_pos.p, k * D) == 0 && std::memcmp(w_dep.p, f_dep.p, k) == 0);
        EXPECT(std::memcmp(state_roots.p, roots2.p, n_trees * sizeof(BlsScalar)) == 0);
    }
    bool threw = false;
    try {
        merkle_forest_frontier_append_witness_device(ForestFrontier{}, nullptr, 0, nullptr, ForestWitnesses{}, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
