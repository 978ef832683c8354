// C++ host-side test of merkle_forest_ragged_update_sequential_device of include/poseidon252.hpp: a forest of trees of different sizes
// is built, a sequence of updates that repeats pairs is applied in one call, for both arities; every witness re-hashes
// (merkle_path_ragged_device) to the root before with the old leaf and to the root after with the new one, the roots of a tree chain,
// the forest afterwards is a fresh build of the final leaves, a leaf past its tree is skipped alone, and an order that is no stable
// sort refuses the whole batch.  All buffers are page-locked host memory (p252_host_alloc), which the device reads and writes in
// place: no HIP header is needed.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
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
    const std::size_t n_trees = sizes.size(), max_leaves = 300;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const std::size_t D = forest_openings_stride(max_leaves, arity), per = arity - 1;
        const std::size_t n_levels = n_leaves / per + n_trees * D;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees), built(n_trees), fresh_levels(n_levels), fresh_roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1);
        p252o_fill_random(2400 + arity, leaves.p[0].data(), n_leaves);
        for (std::size_t t = 0; t < n_trees; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t];
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        std::memcpy(built.p, roots.p, n_trees * sizeof(BlsScalar));
        // (tree, leaf): leaf 7 of tree 4 three times, two leaves of one parent in turn, the one-leaf tree twice; update 6 is past its tree
        const std::uint32_t tid[] = {4, 2, 4, 3, 2, 0, 1, 4, 0, 3, 5};
        const std::uint64_t lid[] = {7, 4, 7, 16, 5, 0, 5, 7, 0, 0, 1};
        const std::size_t k = 11, bad_update = 6;
        Pinned<std::uint32_t> u_tree(k), order(k), bad(2);
        Pinned<std::uint64_t> u_leaf(k), hashed(1);
        Pinned<BlsScalar> fresh(k), old(k), sib(k * D * per), before(k), after(k), back_old(k), back_new(k);
        Pinned<std::uint8_t> pos(k * D), dep(k), dep2(k);
        p252o_fill_random(77 + arity, fresh.p[0].data(), k);
        std::vector<std::uint32_t> idx(k);
        std::iota(idx.begin(), idx.end(), 0u);
        std::stable_sort(idx.begin(), idx.end(), [&](std::uint32_t a, std::uint32_t b) { return tid[a] != tid[b] ? tid[a] < tid[b] : lid[a] < lid[b]; });
        for (std::size_t i = 0; i < k; ++i) u_tree.p[i] = tid[i], u_leaf.p[i] = lid[i], order.p[i] = idx[i];
        const SequentialUpdates updates = {u_tree.p, u_leaf.p, fresh.p, order.p, k};
        const SequentialWitnesses out = {old.p, sib.p, pos.p, dep.p, before.p, after.p};
        // an order that is no stable sort (two entries swapped) refuses the whole batch and touches nothing
        std::swap(order.p[0], order.p[1]);
        merkle_forest_ragged_update_sequential_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, updates, out, arity, ctx, roots.p,
                                                      bad.p + 1);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(bad.p[1] == k);
        for (std::size_t i = 0; i < k; ++i) EXPECT(dep.p[i] == 0xFF);
        for (std::size_t t = 0; t < n_trees; ++t) EXPECT(roots.p[t] == built.p[t]);
        std::swap(order.p[0], order.p[1]);
        merkle_forest_ragged_update_sequential_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, updates, out, arity, ctx, roots.p,
                                                      bad.p, hashed.p);
        merkle_path_ragged_device(old.p, sib.p, pos.p, dep.p, D, back_old.p, k, arity, ctx);
        merkle_path_ragged_device(fresh.p, sib.p, pos.p, dep.p, D, back_new.p, k, arity, ctx);
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, fresh_roots.p, arity, ctx, fresh_levels.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(bad.p[0] == 1);
        std::size_t want_hashed = 0;
        std::vector<int> last(n_trees, -1);
        for (std::size_t i = 0; i < k; ++i) {
            if (i == bad_update) {
                EXPECT(dep.p[i] == 0xFF && old.p[i] == BlsScalar{} && before.p[i] == BlsScalar{} && after.p[i] == BlsScalar{});
                continue;
            }
            const std::size_t d = forest_openings_stride(sizes[tid[i]], arity);
            want_hashed += d;
            EXPECT(dep.p[i] == d);
            if (d) {  // (a one-leaf tree's root is its leaf mod p; the re-hash of a depth-0 opening returns the leaf)
                EXPECT(back_old.p[i] == before.p[i]);
                EXPECT(back_new.p[i] == after.p[i]);
            }
            EXPECT(before.p[i] == (last[tid[i]] < 0 ? built.p[tid[i]] : after.p[last[tid[i]]]));
            last[tid[i]] = (int)i;
        }
        EXPECT(hashed.p[0] == want_hashed);
        EXPECT(old.p[2] == fresh.p[0] && old.p[7] == fresh.p[2] && old.p[8] == fresh.p[5]);  // a repeated pair sees the update before it
        EXPECT(leaves.p[offsets.p[4] + 7] == fresh.p[7] && leaves.p[offsets.p[0]] == fresh.p[8]);
        for (std::size_t t = 0; t < n_trees; ++t) EXPECT(roots.p[t] == fresh_roots.p[t]);
        EXPECT(std::memcmp(levels.p, fresh_levels.p, n_levels * sizeof(BlsScalar)) == 0);
    }
    bool threw = false;
    try {
        merkle_forest_ragged_update_sequential_device(nullptr, 1, nullptr, 1, 1, nullptr, SequentialUpdates{}, SequentialWitnesses{}, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
