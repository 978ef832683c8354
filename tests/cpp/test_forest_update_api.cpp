// C++ host-side test of merkle_forest_ragged_update_device of include/poseidon252.hpp: a forest of trees of different sizes is built
// with its tree-major levels, leaves of several trees are changed in one call (a bad update among them), and the leaves, the levels
// and the roots are compared with a fresh build of the modified leaves and with the oracle's single-tree builder, for both arities.
// All buffers are page-locked host memory (p252_host_alloc), which the device reads and writes in place: no HIP header is needed.
// The oracle (oracle/p252_oracle.h) is linked as the checker only.
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
    const std::vector<std::size_t> sizes = {1, 5, 16, 17, 300, 2, 65};
    const std::size_t n_trees = sizes.size(), max_leaves = 300;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
        const std::size_t D = forest_openings_stride(max_leaves, arity), per = arity - 1, n_levels = n_leaves / per + n_trees * D;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees), fresh_levels(n_levels), fresh_roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1);
        p252o_fill_random(500 + arity, leaves.p[0].data(), n_leaves);
        std::size_t at = 0;
        for (std::size_t t = 0; t < n_trees; ++t) {
            offsets.p[t] = at;
            at += sizes[t];
        }
        offsets.p[n_trees] = at;
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        // updates: the single leaf of tree 0, all children of one node of tree 4, the last leaf of trees 3 and 6, a leaf of tree 5;
        // then a tree id past the forest and a leaf id past its tree (both bad)
        const std::vector<std::pair<std::uint32_t, std::uint64_t>> upd = {{0, 0}, {4, 8}, {4, 9}, {4, 10}, {4, 11}, {3, 16}, {6, 64}, {5, 1},
                                                                         {(std::uint32_t)n_trees, 0}, {1, 5}};
        const std::size_t k = upd.size(), n_good = k - 2;
        Pinned<std::uint32_t> tree_ids(k);
        Pinned<std::uint64_t> leaf_ids(k);
        Pinned<BlsScalar> fresh(k);
        p252o_fill_random(600 + arity, fresh.p[0].data(), k);
        std::vector<BlsScalar> before(roots.p, roots.p + n_trees), want(leaves.p, leaves.p + n_leaves);
        for (std::size_t i = 0; i < k; ++i) {
            tree_ids.p[i] = upd[i].first;
            leaf_ids.p[i] = upd[i].second;
            if (i < n_good) want[offsets.p[upd[i].first] + upd[i].second] = fresh.p[i];
        }
        merkle_forest_ragged_update_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, tree_ids.p, leaf_ids.p, fresh.p, k,
                                           arity, ctx, roots.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        for (std::size_t i = 0; i < n_leaves; ++i) EXPECT(leaves.p[i] == want[i]);
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, fresh_roots.p, arity, ctx, fresh_levels.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(std::memcmp(levels.p, fresh_levels.p, n_levels * sizeof(BlsScalar)) == 0);
        const bool touched[] = {true, false, false, true, true, true, true};
        for (std::size_t t = 0; t < n_trees; ++t) {
            BlsScalar expected;
            std::vector<BlsScalar> lv(sizes[t] + 64);
            if (arity == 4)
                p252o_merkle4_tree(tag.data(), want[offsets.p[t]].data(), sizes[t], expected.data(), lv[0].data());
            else
                p252o_merkle2_tree(tag.data(), want[offsets.p[t]].data(), sizes[t], expected.data(), lv[0].data());
            EXPECT(roots.p[t] == expected);
            EXPECT(fresh_roots.p[t] == expected);
            EXPECT((roots.p[t] == before[t]) == !touched[t]);
        }
    }
    bool threw = false;
    try {
        merkle_forest_ragged_update_device(nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 1, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
