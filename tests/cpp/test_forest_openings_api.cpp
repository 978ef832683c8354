// C++ host-side test of the forest openings calls of include/poseidon252.hpp: a forest of trees of different sizes is built with
// its tree-major levels, EVERY leaf of every tree is opened in one call, the openings are re-hashed with a depth per opening and
// verified against the root of their own tree — roots checked against the oracle's single-tree builder, for both arities.  All
// buffers are page-locked host memory (p252_host_alloc), which the device reads and writes in place: no HIP header is needed.
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
        const std::size_t D = forest_openings_stride(max_leaves, arity), per = arity - 1;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_leaves / per + n_trees * D), roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1), leaf_ids(n_leaves);
        Pinned<std::uint32_t> tree_ids(n_leaves);
        p252o_fill_random(400 + arity, leaves.p[0].data(), n_leaves);
        std::vector<BlsScalar> expected(n_trees);
        std::vector<std::size_t> depth_of(n_trees);
        std::size_t at = 0;
        for (std::size_t t = 0; t < n_trees; ++t) {
            offsets.p[t] = at;
            std::vector<BlsScalar> lv(sizes[t] + 64);
            if (arity == 4)
                p252o_merkle4_tree(tag.data(), leaves.p[at].data(), sizes[t], expected[t].data(), lv[0].data());
            else
                p252o_merkle2_tree(tag.data(), leaves.p[at].data(), sizes[t], expected[t].data(), lv[0].data());
            depth_of[t] = arity == 4 ? p252_merkle4_depth(sizes[t]) : p252_merkle2_depth(sizes[t]);
            for (std::size_t i = 0; i < sizes[t]; ++i) {  // every leaf, trees interleaved from the back
                tree_ids.p[n_leaves - 1 - (at + i)] = (std::uint32_t)t;
                leaf_ids.p[n_leaves - 1 - (at + i)] = i;
            }
            at += sizes[t];
        }
        offsets.p[n_trees] = at;
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        const std::size_t k = n_leaves;
        Pinned<BlsScalar> out(k), sib(k * D * per), back(k);
        Pinned<std::uint8_t> pos(k * D), depths(k), ok(k);
        merkle_forest_ragged_openings_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, tree_ids.p, leaf_ids.p, k, out.p,
                                             sib.p, pos.p, depths.p, arity, ctx);
        merkle_path_ragged_device(out.p, sib.p, pos.p, depths.p, D, back.p, k, arity, ctx);
        merkle_forest_ragged_verify_device(out.p, sib.p, pos.p, depths.p, D, tree_ids.p, roots.p, n_trees, ok.p, k, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        for (std::size_t t = 0; t < n_trees; ++t) EXPECT(roots.p[t] == expected[t]);
        for (std::size_t i = 0; i < k; ++i) {
            const std::size_t t = tree_ids.p[i];
            EXPECT(out.p[i] == leaves.p[offsets.p[t] + leaf_ids.p[i]]);
            EXPECT(depths.p[i] == depth_of[t]);
            EXPECT(back.p[i] == expected[t]);
            EXPECT(ok.p[i] == 1);
        }
        // an opening pointed at another tree does not verify; a tree id past the forest is a bad opening
        const std::uint32_t own = tree_ids.p[0];
        tree_ids.p[0] = (own + 1) % (std::uint32_t)n_trees;
        merkle_forest_ragged_verify_device(out.p, sib.p, pos.p, depths.p, D, tree_ids.p, roots.p, n_trees, ok.p, k, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        tree_ids.p[0] = own;
        tree_ids.p[1] = (std::uint32_t)n_trees;
        merkle_forest_ragged_openings_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, tree_ids.p, leaf_ids.p, 2, out.p,
                                             sib.p, pos.p, depths.p, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(ok.p[0] == 0 && ok.p[1] == 1);
        EXPECT(depths.p[0] == depth_of[own] && depths.p[1] == 0xFF);
    }
    bool threw = false;
    try {
        merkle_path_ragged_device(nullptr, nullptr, nullptr, nullptr, 65, nullptr, 1);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
