// C++ host-side test of merkle_forest_ragged_resize_device of include/poseidon252.hpp: a forest of trees of different sizes is built
// with its tree-major levels; in one call its trees are cut (to nothing, to one leaf, to a whole power of the arity, past their size),
// some receive new leaves (a refused append among them: its tree is still cut), the trailing tree is dropped; then the new forest's
// offsets, leaves, levels and roots are compared with a fresh build of the same new forest and with the oracle's single-tree
// builder, for both arities.  A pure rollback (no d_add) follows.  All buffers are page-locked host memory (p252_host_alloc), which
// the device reads and writes in place: no HIP header is needed.  The oracle (oracle/p252_oracle.h) is linked as the checker only.
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
    const std::vector<std::size_t> sizes = {1, 5, 16, 17, 300, 2, 40};
    const std::size_t n_trees = sizes.size(), n_trees_new = 6, max_leaves = 300, max_new = 320, refused = 4;  // (the last tree is dropped)
    Context& ctx = Context::default_context();
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: cut and append; pass 1: a pure rollback (d_add == nullptr)
        const std::vector<std::uint64_t> keep = {~0ull, 1, 16, 16, 256, 0};
        const std::vector<std::size_t> adds = pass ? std::vector<std::size_t>(6, 0) : std::vector<std::size_t>{3, 2, 0, 4, 70, 5};
        std::size_t n_add = 0;
        for (std::size_t m : adds) n_add += m;
        for (unsigned arity : {4u, 2u}) {
            const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
            const std::size_t n_levels = n_leaves / (arity - 1) + n_trees * forest_openings_stride(max_leaves, arity);
            const std::size_t cap = n_leaves + n_add, levels_cap = forest_append_levels_cap(cap, n_trees_new, max_new, arity);
            Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees), add(n_add);
            Pinned<BlsScalar> g_leaves(cap), g_levels(levels_cap), g_roots(n_trees_new), fresh_levels(levels_cap), fresh_roots(n_trees_new);
            Pinned<std::uint64_t> offsets(n_trees + 1), add_offsets(n_trees_new + 1), g_offsets(n_trees_new + 1), hashed(1), d_keep(n_trees_new);
            Pinned<std::uint32_t> bad(1);
            p252o_fill_random(900 + arity, leaves.p[0].data(), n_leaves);
            if (n_add) p252o_fill_random(950 + arity, add.p[0].data(), n_add);
            for (std::size_t t = 0; t < n_trees; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t];
            for (std::size_t t = 0; t < n_trees_new; ++t) add_offsets.p[t + 1] = add_offsets.p[t] + adds[t], d_keep.p[t] = keep[t];
            merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
            const ForestView old_forest = {leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p};
            const ForestOut resized = {g_leaves.p, cap, g_offsets.p, g_levels.p, levels_cap, g_roots.p};
            merkle_forest_ragged_resize_device(old_forest, d_keep.p, n_add ? add.p : nullptr, n_add, add_offsets.p, n_trees_new, max_new, resized, arity,
                                               ctx, bad.p, hashed.p);
            detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
            // what the new forest holds
            std::vector<BlsScalar> want;
            std::vector<std::uint64_t> want_off(1, 0);
            std::uint64_t want_hashed = 0;
            std::uint32_t want_bad = 0;
            for (std::size_t t = 0; t < n_trees_new; ++t) {
                const std::size_t n = sizes[t], k = keep[t] < n ? (std::size_t)keep[t] : n;
                const bool refuse = k + adds[t] > max_new;  // (tree `refused`: 256 + 70)
                EXPECT(refuse == (pass == 0 && t == refused));
                const std::size_t m = refuse ? 0 : adds[t];
                for (std::size_t i = 0; i < k; ++i) want.push_back(leaves.p[offsets.p[t] + i]);
                for (std::size_t i = 0; i < m; ++i) want.push_back(add.p[add_offsets.p[t] + i]);
                want_off.push_back(want.size());
                want_bad += refuse || k + m == 0;
                std::size_t w = k + m, clean = k;
                while ((m || k < n) && w > 1) {
                    w = (w + arity - 1) / arity;
                    clean /= arity;
                    want_hashed += w - clean;
                }
            }
            EXPECT(bad.p[0] == want_bad && hashed.p[0] == want_hashed);
            EXPECT(std::memcmp(g_offsets.p, want_off.data(), (n_trees_new + 1) * 8) == 0);
            for (std::size_t i = 0; i < want.size(); ++i) EXPECT(g_leaves.p[i] == want[i]);
            merkle_forest_ragged_device(g_leaves.p, cap, g_offsets.p, n_trees_new, max_new, fresh_roots.p, arity, ctx, fresh_levels.p);
            detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
            EXPECT(std::memcmp(g_levels.p, fresh_levels.p, levels_cap * sizeof(BlsScalar)) == 0);  // (past the used part both are still zero)
            for (std::size_t t = 0; t < n_trees_new; ++t) {
                const std::size_t n = want_off[t + 1] - want_off[t];
                BlsScalar expected{};
                std::vector<BlsScalar> lv(n + 64);
                if (n == 0) {
                    EXPECT(g_roots.p[t] == expected);  // an empty tree: a zero root
                    continue;
                }
                if (arity == 4)
                    p252o_merkle4_tree(tag.data(), want[want_off[t]].data(), n, expected.data(), lv[0].data());
                else
                    p252o_merkle2_tree(tag.data(), want[want_off[t]].data(), n, expected.data(), lv[0].data());
                EXPECT(g_roots.p[t] == expected);
                EXPECT(fresh_roots.p[t] == expected);
                if (pass == 1 && t == 0) EXPECT(g_roots.p[t] == roots.p[t]);  // an unchanged tree keeps its root
            }
        }
    }
    bool threw = false;
    try {
        merkle_forest_ragged_resize_device(ForestView{}, nullptr, nullptr, 0, nullptr, 1, 1, ForestOut{}, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
