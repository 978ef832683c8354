// C++ host-side test of pairs_order_device and pairs_unique_device of include/poseidon252.hpp: a program with nothing but the library
// goes from (tree, leaf) pairs in any order, with repeats, to a verified sequential update and to a verified shared proof of the
// forest.  d_order comes from the library and is compared with std::stable_sort; the sequential call accepts it (no bad update) and
// every witness re-hashes; the distinct pairs come from the library, are compared with a sorted std::vector, and the shared proof
// extracted for them verifies for every tree that has a pair.  All buffers are page-locked host memory (p252_host_alloc), which the
// device reads and writes in place: no HIP header is needed.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <utility>
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

static void sync(Context& ctx) { detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync"); }

int main() {
    const std::vector<std::size_t> sizes = {1, 5, 16, 17, 300, 2};
    const std::size_t n_trees = sizes.size(), max_leaves = 300;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    Context& ctx = Context::default_context();
    // 300 pairs inside the forest, about half of them repeats of an earlier one
    const std::size_t k = 300;
    std::vector<std::uint32_t> tid(k);
    std::vector<std::uint64_t> lid(k);
    std::uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&x]() {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return x;
    };
    for (std::size_t i = 0; i < k; ++i) {
        if (i && next() % 2) {
            const std::size_t j = next() % i;
            tid[i] = tid[j], lid[i] = lid[j];
        } else {
            tid[i] = (std::uint32_t)(next() % n_trees), lid[i] = next() % sizes[tid[i]];
        }
    }
    std::vector<std::uint32_t> want_order(k);
    std::iota(want_order.begin(), want_order.end(), 0u);
    std::stable_sort(want_order.begin(), want_order.end(),
                     [&](std::uint32_t a, std::uint32_t b) { return tid[a] != tid[b] ? tid[a] < tid[b] : lid[a] < lid[b]; });
    std::vector<std::pair<std::uint32_t, std::uint64_t>> distinct;
    std::vector<std::uint32_t> want_first;
    for (std::uint32_t i : want_order)
        if (distinct.empty() || distinct.back() != std::make_pair(tid[i], lid[i])) distinct.push_back({tid[i], lid[i]}), want_first.push_back(i);

    for (unsigned arity : {4u, 2u}) {
        const std::size_t D = forest_openings_stride(max_leaves, arity), per = arity - 1;
        const std::size_t n_levels = n_leaves / per + n_trees * D;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1);
        p252o_fill_random(3100 + arity, leaves.p[0].data(), n_leaves);
        for (std::size_t t = 0; t < n_trees; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t];
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        Pinned<std::uint32_t> u_tree(k), order(k), bad(3);
        Pinned<std::uint64_t> u_leaf(k);
        for (std::size_t i = 0; i < k; ++i) u_tree.p[i] = tid[i], u_leaf.p[i] = lid[i];

        // ---- the order, then the sequential update with it ----
        pairs_order_device(u_tree.p, u_leaf.p, k, order.p, ctx);
        sync(ctx);
        EXPECT(std::equal(want_order.begin(), want_order.end(), order.p));
        Pinned<BlsScalar> fresh(k), old(k), sib(k * D * per), before(k), after(k), back_old(k), back_new(k);
        Pinned<std::uint8_t> pos(k * D), dep(k);
        p252o_fill_random(91 + arity, fresh.p[0].data(), k);
        const SequentialUpdates updates = {u_tree.p, u_leaf.p, fresh.p, order.p, k};
        const SequentialWitnesses out = {old.p, sib.p, pos.p, dep.p, before.p, after.p};
        merkle_forest_ragged_update_sequential_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, updates, out, arity, ctx, roots.p,
                                                      bad.p);
        merkle_path_ragged_device(old.p, sib.p, pos.p, dep.p, D, back_old.p, k, arity, ctx);
        merkle_path_ragged_device(fresh.p, sib.p, pos.p, dep.p, D, back_new.p, k, arity, ctx);
        sync(ctx);
        EXPECT(bad.p[0] == 0);
        for (std::size_t i = 0; i < k; ++i) {
            EXPECT(dep.p[i] == forest_openings_stride(sizes[tid[i]], arity));
            if (dep.p[i] && dep.p[i] != 0xFF) EXPECT(back_old.p[i] == before.p[i] && back_new.p[i] == after.p[i]);
        }

        // ---- the distinct pairs, then the forest's shared proof for them ----
        Pinned<std::uint32_t> q_tree(k), q_index(k), first(k);
        Pinned<std::uint64_t> q_leaf(k), n_unique(1);
        std::memset(q_tree.p, 0xEE, k * 4), std::memset(q_leaf.p, 0xEE, k * 8), std::memset(first.p, 0xEE, k * 4), std::memset(q_index.p, 0xEE, k * 4);
        pairs_unique_device(u_tree.p, u_leaf.p, k, UniquePairs{q_tree.p, q_leaf.p, q_index.p, first.p, n_unique.p}, ctx);
        sync(ctx);
        const std::size_t m = distinct.size();
        EXPECT(n_unique.p[0] == m);
        for (std::size_t i = 0; i < m && n_unique.p[0] == m; ++i) {
            EXPECT(q_tree.p[i] == distinct[i].first && q_leaf.p[i] == distinct[i].second && first.p[i] == want_first[i]);
            EXPECT(q_index.p[i] == (std::uint32_t)distinct[i].second);
        }
        for (std::size_t i = m; i < k; ++i) EXPECT(q_tree.p[i] == 0xEEEEEEEEu && first.p[i] == 0xEEEEEEEEu && q_leaf.p[i] == 0xEEEEEEEEEEEEEEEEull);
        const ForestView forest = {leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p};
        const std::size_t cap = merkle_forest_ragged_multiproof_bound(n_leaves, n_trees, max_leaves, m, arity);
        Pinned<BlsScalar> opened(m), proof(cap);
        Pinned<std::uint64_t> proof_offsets(n_trees + 1);
        Pinned<std::uint8_t> ok(n_trees);
        merkle_forest_ragged_multiproof_device(forest, q_tree.p, q_leaf.p, m, opened.p, proof.p, cap, proof_offsets.p, arity, ctx, bad.p + 1);
        sync(ctx);
        EXPECT(bad.p[1] == 0);
        merkle_forest_ragged_multiproof_verify_device(forest, q_tree.p, q_leaf.p, opened.p, m, proof.p, proof_offsets.p[n_trees], proof_offsets.p,
                                                      roots.p, ok.p, arity, ctx, nullptr, nullptr, bad.p + 2);
        sync(ctx);
        EXPECT(bad.p[2] == 0);
        std::vector<bool> has(n_trees, false);
        for (const auto& pr : distinct) has[pr.first] = true;
        for (std::size_t t = 0; t < n_trees; ++t) EXPECT(ok.p[t] == (has[t] ? 1 : 0));
        for (std::size_t i = 0; i < m; ++i) EXPECT(opened.p[i] == leaves.p[offsets.p[distinct[i].first] + distinct[i].second]);

        // ---- one tree: positions with repeats -> d_indices of the single tree's shared proof ----
        if (arity == 4) {
            const std::size_t kk = 40;
            Pinned<std::uint64_t> where(kk), count(1);
            Pinned<std::uint32_t> indices(kk);
            for (std::size_t i = 0; i < kk; ++i) where.p[i] = (i * 37) % 25 * 11;
            pairs_unique_device(nullptr, where.p, kk, UniquePairs{nullptr, nullptr, indices.p, nullptr, count.p}, ctx);
            sync(ctx);
            std::vector<std::uint64_t> sorted(where.p, where.p + kk);
            std::sort(sorted.begin(), sorted.end());
            sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
            EXPECT(count.p[0] == sorted.size());
            for (std::size_t i = 0; i < sorted.size() && count.p[0] == sorted.size(); ++i) EXPECT(indices.p[i] == sorted[i]);
        }
    }
    bool threw = false;
    try {
        pairs_order_device(nullptr, nullptr, 0, nullptr);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
