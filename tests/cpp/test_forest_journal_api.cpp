// C++ host-side test of merkle_forest_ragged_update_journaled_device / merkle_forest_ragged_journal_swap_device /
// merkle_forest_ragged_journal_bound of include/poseidon252.hpp: a forest of trees of different sizes is built with its tree-major
// levels, leaves of several trees are changed in one journaled call (a repeated pair and a bad update among them) and compared with a
// fresh build of the modified leaves; one swap gives back the forest from before the update byte for byte, a second one the forest
// after it; both arities.  All buffers are page-locked host memory (p252_host_alloc), which the device reads and writes in place: no
// HIP header is needed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "poseidon252.hpp"

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
    const std::vector<std::size_t> sizes = {1, 5, 16, 17, 300, 2, 65};
    const std::size_t n_trees = sizes.size(), max_leaves = 300;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const std::size_t D = forest_openings_stride(max_leaves, arity), per = arity - 1, n_levels = n_leaves / per + n_trees * D;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees), fresh_levels(n_levels), fresh_roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1);
        for (std::size_t i = 0; i < n_leaves; ++i) leaves.p[i] = BlsScalar{i + 1, 7 * i + arity, i * i, i & 0xff};
        std::size_t at = 0;
        for (std::size_t t = 0; t < n_trees; ++t) {
            offsets.p[t] = at;
            at += sizes[t];
        }
        offsets.p[n_trees] = at;
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        sync(ctx);
        const std::vector<BlsScalar> leaves0(leaves.p, leaves.p + n_leaves), levels0(levels.p, levels.p + n_levels), roots0(roots.p, roots.p + n_trees);
        // the single leaf of tree 0, all children of one node of tree 4, the last leaf of trees 3 and 6, a leaf of tree 5 given twice
        // (one value); then a tree id past the forest and a leaf id past its tree (both bad)
        const std::vector<std::pair<std::uint32_t, std::uint64_t>> upd = {{0, 0}, {4, 8}, {4, 9}, {4, 10}, {4, 11}, {3, 16}, {6, 64}, {5, 1},
                                                                         {5, 1}, {(std::uint32_t)n_trees, 0}, {1, 5}};
        const std::size_t k = upd.size(), n_good = k - 2, n_distinct = n_good - 1;
        Pinned<std::uint32_t> tree_ids(k), n_bad(2);
        Pinned<std::uint64_t> leaf_ids(k), n_hashed(1), journal_len(1);
        Pinned<BlsScalar> fresh(k);
        std::vector<BlsScalar> want(leaves0);
        for (std::size_t i = 0; i < k; ++i) {
            tree_ids.p[i] = upd[i].first;
            leaf_ids.p[i] = upd[i].second;
            fresh.p[i] = BlsScalar{100 + upd[i].second, arity, upd[i].first, 3};
            if (i < n_good) want[offsets.p[upd[i].first] + upd[i].second] = fresh.p[i];
        }
        const std::size_t cap = merkle_forest_ragged_journal_bound(n_leaves, n_trees, max_leaves, k, arity);
        EXPECT(cap >= k && cap <= k * (D + 1));
        Pinned<std::uint32_t> ids(4 * (cap + 1));
        Pinned<BlsScalar> values(cap + 1);
        journal_len.p[0] = ~0ull;  // (the call sets it)
        const ForestJournal journal{ids.p, values.p, cap, journal_len.p};
        merkle_forest_ragged_update_journaled_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, tree_ids.p, leaf_ids.p, fresh.p,
                                                     k, journal, arity, ctx, roots.p, n_bad.p, n_hashed.p);
        sync(ctx);
        EXPECT(n_bad.p[0] == 2 && n_hashed.p[0] > 0 && journal_len.p[0] == n_distinct + n_hashed.p[0] && journal_len.p[0] <= cap);
        for (std::size_t i = 0; i < n_leaves; ++i) EXPECT(leaves.p[i] == want[i]);
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, fresh_roots.p, arity, ctx, fresh_levels.p);
        sync(ctx);
        EXPECT(std::memcmp(levels.p, fresh_levels.p, n_levels * sizeof(BlsScalar)) == 0);
        const bool touched[] = {true, false, false, true, true, true, true};
        for (std::size_t t = 0; t < n_trees; ++t) EXPECT(touched[t] ? roots.p[t] == fresh_roots.p[t] : roots.p[t] == roots0[t]);
        const std::vector<BlsScalar> levels1(levels.p, levels.p + n_levels), roots1(roots.p, roots.p + n_trees);
        // undo
        merkle_forest_ragged_journal_swap_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, journal, arity, ctx, roots.p,
                                                 n_bad.p + 1);
        sync(ctx);
        EXPECT(n_bad.p[1] == 0);
        EXPECT(std::memcmp(leaves.p, leaves0.data(), n_leaves * sizeof(BlsScalar)) == 0);
        EXPECT(std::memcmp(levels.p, levels0.data(), n_levels * sizeof(BlsScalar)) == 0);
        EXPECT(std::memcmp(roots.p, roots0.data(), n_trees * sizeof(BlsScalar)) == 0);
        // redo
        merkle_forest_ragged_journal_swap_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, journal, arity, ctx, roots.p,
                                                 n_bad.p + 1);
        sync(ctx);
        EXPECT(n_bad.p[1] == 0);
        EXPECT(std::memcmp(leaves.p, want.data(), n_leaves * sizeof(BlsScalar)) == 0);
        EXPECT(std::memcmp(levels.p, levels1.data(), n_levels * sizeof(BlsScalar)) == 0);
        EXPECT(std::memcmp(roots.p, roots1.data(), n_trees * sizeof(BlsScalar)) == 0);
        // a journal one entry short is refused, and nothing is written
        bool refused = false;
        try {
            const ForestJournal tight{ids.p, values.p, cap - 1, journal_len.p};
            merkle_forest_ragged_update_journaled_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p, tree_ids.p, leaf_ids.p,
                                                         fresh.p, k, tight, arity, ctx, roots.p);
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        EXPECT(refused);
    }
    bool threw = false;
    try {
        merkle_forest_ragged_journal_bound(1, 1, 1, 1, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
