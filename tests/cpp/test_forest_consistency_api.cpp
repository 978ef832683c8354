// C++ host-side test of merkle_forest_ragged_consistency_device / merkle_forest_consistency_verify_device of include/poseidon252.hpp: a
// forest of trees of different sizes is built, and for every tree and a set of old counts n the proof that the tree extends its first n
// leaves is extracted and verified against the oracle's single-tree roots of the first n leaves and of all leaves, for both arities —
// with the claims one per proof, and with the claims one per tree named by tree id.  A bad proof, an unchanged tree and a wrong old root
// are among them.  All buffers are page-locked host memory (p252_host_alloc), which the device reads and writes in place: no HIP header
// is needed.  The oracle (oracle/p252_oracle.h) is linked as the checker only.
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

static BlsScalar oracle_root(unsigned arity, const BlsScalar& tag, const BlsScalar* leaves, std::size_t n) {
    BlsScalar root;
    std::vector<BlsScalar> lv(n + 64);
    if (arity == 4)
        p252o_merkle4_tree(tag.data(), leaves[0].data(), n, root.data(), lv[0].data());
    else
        p252o_merkle2_tree(tag.data(), leaves[0].data(), n, root.data(), lv[0].data());
    return root;
}

int main() {
    const std::vector<std::size_t> sizes = {1, 5, 16, 17, 300, 2};
    const std::size_t n_trees = sizes.size(), max_leaves = 300;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
        const std::size_t D = forest_openings_stride(max_leaves, arity), per = arity - 1;
        const std::size_t n_levels = n_leaves / per + n_trees * D;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1), sizes64(n_trees);
        p252o_fill_random(1900 + arity, leaves.p[0].data(), n_leaves);
        for (std::size_t t = 0; t < n_trees; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t], sizes64.p[t] = sizes[t];
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        // the proofs: per tree the old counts 1, n_t / 2, n_t - 1 and n_t (those that are >= 1), then three bad ones
        std::vector<std::uint32_t> tid;
        std::vector<std::uint64_t> old;
        for (std::size_t t = 0; t < n_trees; ++t)
            for (std::size_t n : {std::size_t(1), sizes[t] / 2, sizes[t] - 1, sizes[t]})
                if (n >= 1) tid.push_back((std::uint32_t)t), old.push_back(n);
        const std::size_t n_good = tid.size();
        tid.push_back(4), old.push_back(0);
        tid.push_back(4), old.push_back(301);
        tid.push_back((std::uint32_t)n_trees), old.push_back(1);
        const std::size_t k = tid.size();
        Pinned<std::uint32_t> tree_ids(k), bad(1);
        Pinned<std::uint64_t> old_counts(k), new_counts(k), hashed(1);
        Pinned<BlsScalar> p_leaves(k), p_sib(k * D * per), old_roots(k), new_roots(k), old_out(k), new_out(k);
        Pinned<std::uint8_t> p_pos(k * D), p_dep(k), ok(k);
        std::memcpy(tree_ids.p, tid.data(), k * 4);
        std::memcpy(old_counts.p, old.data(), k * 8);
        const ForestView forest = {leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p};
        const ConsistencyProofs proof = {p_leaves.p, p_sib.p, p_pos.p, p_dep.p, D};
        merkle_forest_ragged_consistency_device(forest, tree_ids.p, old_counts.p, k, new_counts.p, proof, arity, ctx, bad.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(bad.p[0] == 3);
        for (std::size_t i = 0; i < k; ++i) {
            const bool good = i < n_good;
            EXPECT(new_counts.p[i] == (good ? sizes[tid[i]] : 0));
            EXPECT(good ? p_dep.p[i] == forest_openings_stride(sizes[tid[i]], arity) : p_dep.p[i] == 0xFF);
            if (good) {
                old_roots.p[i] = oracle_root(arity, tag, leaves.p + offsets.p[tid[i]], old[i]);
                new_roots.p[i] = roots.p[tid[i]];
                EXPECT(roots.p[tid[i]] == oracle_root(arity, tag, leaves.p + offsets.p[tid[i]], sizes[tid[i]]));
            }
        }
        // one claim per proof
        const ConsistencyClaims claims = {old_counts.p, old_roots.p, new_counts.p, new_roots.p};
        merkle_forest_consistency_verify_device(claims, proof, k, ok.p, arity, ctx, old_out.p, new_out.p, hashed.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        std::uint64_t grown = 0;
        for (std::size_t i = 0; i < k; ++i) {
            EXPECT(ok.p[i] == (i < n_good ? 1 : 0));
            if (i < n_good) EXPECT(old_out.p[i] == old_roots.p[i] && new_out.p[i] == new_roots.p[i]);
            if (i < n_good && old[i] < sizes[tid[i]]) grown += forest_openings_stride(sizes[tid[i]], arity);
        }
        EXPECT(hashed.p[0] >= grown && hashed.p[0] <= 2 * grown);
        // a wrong old root is refused, and only that proof
        const std::size_t victim = 9 < n_good ? 9 : 0;
        old_roots.p[victim][0] ^= 1;
        merkle_forest_consistency_verify_device(claims, proof, k, ok.p, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        for (std::size_t i = 0; i < n_good; ++i) EXPECT(ok.p[i] == (i == victim ? 0 : 1));
        // one claim per tree, named by tree id: every tree against its own size and root (n == m), so the bad ids alone are refused
        const ConsistencyClaims same = {sizes64.p, roots.p, sizes64.p, roots.p, tree_ids.p, n_trees};
        Pinned<std::uint8_t> dep_same(k);
        for (std::size_t i = 0; i < k; ++i) dep_same.p[i] = (std::uint8_t)forest_openings_stride(sizes[tid[i] < n_trees ? tid[i] : 0], arity);
        const ConsistencyProofs zero = {p_leaves.p, p_sib.p, p_pos.p, dep_same.p, D};
        merkle_forest_consistency_verify_device(same, zero, k, ok.p, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        for (std::size_t i = 0; i < k; ++i) EXPECT(ok.p[i] == (tid[i] < n_trees ? 1 : 0));
    }
    bool threw = false;
    try {
        merkle_forest_consistency_verify_device(ConsistencyClaims{}, ConsistencyProofs{}, 0, nullptr, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
