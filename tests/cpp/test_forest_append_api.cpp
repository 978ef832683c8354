// C++ host-side test of merkle_forest_ragged_append_device of include/poseidon252.hpp: a forest of trees of different sizes is built
// with its tree-major levels, leaves are appended to several of its trees and a new tree is added in one call (a refused append
// among them), and the new forest's offsets, leaves, levels and roots are compared with a fresh build of the same new forest and with
// the oracle's single-tree builder, for both arities.  All buffers are page-locked host memory (p252_host_alloc), which the device
// reads and writes in place: no HIP header is needed.  The oracle (oracle/p252_oracle.h) is linked as the checker only.
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
    // a single leaf grows; a partial parent fills; a complete tree's root becomes a child; nothing; too long (refused); +1; a new tree
    const std::vector<std::size_t> adds = {3, 2, 1, 0, 50, 1, 9};
    const std::size_t n_trees = sizes.size(), n_trees_new = adds.size(), max_leaves = 300, max_new = 320, refused = 4;
    std::size_t n_leaves = 0, n_add = 0;
    for (std::size_t n : sizes) n_leaves += n;
    for (std::size_t m : adds) n_add += m;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
        const std::size_t n_levels = n_leaves / (arity - 1) + n_trees * forest_openings_stride(max_leaves, arity);
        const std::size_t cap = n_leaves + n_add, levels_cap = forest_append_levels_cap(cap, n_trees_new, max_new, arity);
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees), add(n_add);
        Pinned<BlsScalar> g_leaves(cap), g_levels(levels_cap), g_roots(n_trees_new), fresh_levels(levels_cap), fresh_roots(n_trees_new);
        Pinned<std::uint64_t> offsets(n_trees + 1), add_offsets(n_trees_new + 1), g_offsets(n_trees_new + 1), hashed(1);
        Pinned<std::uint32_t> bad(1);
        p252o_fill_random(700 + arity, leaves.p[0].data(), n_leaves);
        p252o_fill_random(800 + arity, add.p[0].data(), n_add);
        for (std::size_t t = 0; t < n_trees; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t];
        for (std::size_t t = 0; t < n_trees_new; ++t) add_offsets.p[t + 1] = add_offsets.p[t] + adds[t];
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        const ForestView old_forest = {leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p};
        const ForestOut grown = {g_leaves.p, cap, g_offsets.p, g_levels.p, levels_cap, g_roots.p};
        merkle_forest_ragged_append_device(old_forest, add.p, n_add, add_offsets.p, n_trees_new, max_new, grown, arity, ctx, bad.p, hashed.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        // what the new forest holds
        std::vector<BlsScalar> want;
        std::vector<std::uint64_t> want_off(1, 0);
        std::uint64_t want_hashed = 0;
        for (std::size_t t = 0; t < n_trees_new; ++t) {
            const std::size_t n = t < n_trees ? sizes[t] : 0, m = t == refused ? 0 : adds[t];
            for (std::size_t i = 0; i < n; ++i) want.push_back(leaves.p[offsets.p[t] + i]);
            for (std::size_t i = 0; i < m; ++i) want.push_back(add.p[add_offsets.p[t] + i]);
            want_off.push_back(want.size());
            std::size_t w = n + m, clean = n;
            while (m && w > 1) {
                w = (w + arity - 1) / arity;
                clean /= arity;
                want_hashed += w - clean;
            }
        }
        EXPECT(bad.p[0] == 1 && hashed.p[0] == want_hashed);
        EXPECT(std::memcmp(g_offsets.p, want_off.data(), (n_trees_new + 1) * 8) == 0);
        for (std::size_t i = 0; i < want.size(); ++i) EXPECT(g_leaves.p[i] == want[i]);
        merkle_forest_ragged_device(g_leaves.p, cap, g_offsets.p, n_trees_new, max_new, fresh_roots.p, arity, ctx, fresh_levels.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(std::memcmp(g_levels.p, fresh_levels.p, levels_cap * sizeof(BlsScalar)) == 0);  // (past the used part both are still zero)
        for (std::size_t t = 0; t < n_trees_new; ++t) {
            const std::size_t n = want_off[t + 1] - want_off[t];
            BlsScalar expected;
            std::vector<BlsScalar> lv(n + 64);
            if (arity == 4)
                p252o_merkle4_tree(tag.data(), want[want_off[t]].data(), n, expected.data(), lv[0].data());
            else
                p252o_merkle2_tree(tag.data(), want[want_off[t]].data(), n, expected.data(), lv[0].data());
            EXPECT(g_roots.p[t] == expected);
            EXPECT(fresh_roots.p[t] == expected);
            if (t == 3 || t == refused) EXPECT(g_roots.p[t] == roots.p[t]);  // unchanged trees keep their roots
        }
    }
    bool threw = false;
    try {
        merkle_forest_ragged_append_device(ForestView{}, nullptr, 0, nullptr, 1, 1, ForestOut{}, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
