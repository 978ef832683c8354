// C++ host-side test of merkle_forest_ragged_anchor_openings_device of include/poseidon252.hpp: a forest of trees of different sizes is
// built, and for every tree and a set of earlier counts c the root the tree had at c leaves is taken out and compared with the oracle's
// single-tree root of the first c leaves; leaves are opened under those anchors and verified with merkle_forest_ragged_verify_device
// against the anchor roots, for both arities.  Bad anchors and bad openings are among them, and the roots-alone call (k == 0).  All
// buffers are page-locked host memory (p252_host_alloc), which the device reads and writes in place: no HIP header is needed.  The
// oracle (oracle/p252_oracle.h) is linked as the checker only.
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
        Pinned<std::uint64_t> offsets(n_trees + 1);
        p252o_fill_random(2100 + arity, leaves.p[0].data(), n_leaves);
        for (std::size_t t = 0; t < n_trees; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t];
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        // the anchors: per tree the counts 1, n_t / 2, n_t - 1 and n_t (those that are >= 1), then three bad ones
        std::vector<std::uint32_t> tid;
        std::vector<std::uint64_t> cnt;
        for (std::size_t t = 0; t < n_trees; ++t)
            for (std::size_t c : {std::size_t(1), sizes[t] / 2, sizes[t] - 1, sizes[t]})
                if (c >= 1) tid.push_back((std::uint32_t)t), cnt.push_back(c);
        const std::size_t n_good = tid.size();
        tid.push_back(4), cnt.push_back(0);
        tid.push_back(4), cnt.push_back(301);
        tid.push_back((std::uint32_t)n_trees), cnt.push_back(1);
        const std::size_t m = tid.size();
        // the openings: under every anchor its first and its last leaf, and leaf c (a bad one); one under an anchor that does not exist
        std::vector<std::uint32_t> aid;
        std::vector<std::uint64_t> lid;
        for (std::size_t a = 0; a < m; ++a)
            for (std::uint64_t leaf : {std::uint64_t(0), cnt[a] ? cnt[a] - 1 : 0, cnt[a]}) aid.push_back((std::uint32_t)a), lid.push_back(leaf);
        aid.push_back((std::uint32_t)m), lid.push_back(0);
        const std::size_t k = aid.size();
        Pinned<std::uint32_t> a_tree(m), o_anchor(k), bad_anchors(1), bad(1);
        Pinned<std::uint64_t> a_count(m), o_leaf(k), hashed(1);
        Pinned<BlsScalar> a_roots(m), a_roots_alone(m), o_leaves(k), o_sib(k * D * per);
        Pinned<std::uint8_t> a_depths(m), a_depths_alone(m), o_pos(k * D), o_dep(k), ok(k);
        std::memcpy(a_tree.p, tid.data(), m * 4);
        std::memcpy(a_count.p, cnt.data(), m * 8);
        std::memcpy(o_anchor.p, aid.data(), k * 4);
        std::memcpy(o_leaf.p, lid.data(), k * 8);
        const ForestView forest = {leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p};
        const ForestAnchors anchors = {a_tree.p, a_count.p, m, a_roots.p, a_depths.p};
        const AnchorOpenings openings = {o_leaves.p, o_sib.p, o_pos.p, o_dep.p};
        merkle_forest_ragged_anchor_openings_device(forest, anchors, o_anchor.p, o_leaf.p, k, openings, arity, ctx, bad_anchors.p, bad.p, hashed.p);
        merkle_forest_ragged_verify_device(o_leaves.p, o_sib.p, o_pos.p, o_dep.p, D, o_anchor.p, a_roots.p, m, ok.p, k, arity, ctx);
        // the roots alone
        const ForestAnchors alone = {a_tree.p, a_count.p, m, a_roots_alone.p, a_depths_alone.p};
        merkle_forest_ragged_anchor_openings_device(forest, alone, nullptr, nullptr, 0, AnchorOpenings{}, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(bad_anchors.p[0] == 3);
        std::uint64_t most = 0;
        for (std::size_t a = 0; a < m; ++a) {
            const bool good = a < n_good;
            EXPECT(a_roots.p[a] == a_roots_alone.p[a] && a_depths.p[a] == a_depths_alone.p[a]);
            if (good) {
                EXPECT(a_roots.p[a] == oracle_root(arity, tag, leaves.p + offsets.p[tid[a]], cnt[a]));
                EXPECT(a_depths.p[a] == forest_openings_stride(cnt[a], arity));
                if (cnt[a] == sizes[tid[a]]) EXPECT(a_roots.p[a] == roots.p[tid[a]]);
                most += a_depths.p[a];
            } else {
                EXPECT(a_roots.p[a] == BlsScalar{} && a_depths.p[a] == 0xFF);
            }
        }
        EXPECT(hashed.p[0] > 0 && hashed.p[0] <= most);
        std::size_t n_bad = 0;
        for (std::size_t i = 0; i < k; ++i) {
            const bool good = aid[i] < n_good && lid[i] < cnt[aid[i]];
            n_bad += !good;
            EXPECT(ok.p[i] == (good ? 1 : 0));
            EXPECT(o_dep.p[i] == (good ? a_depths.p[aid[i]] : 0xFF));
            if (good) EXPECT(o_leaves.p[i] == leaves.p[offsets.p[tid[aid[i]]] + lid[i]]);
        }
        EXPECT(bad.p[0] == n_bad);
    }
    bool threw = false;
    try {
        merkle_forest_ragged_anchor_openings_device(ForestView{}, ForestAnchors{}, nullptr, nullptr, 0, AnchorOpenings{}, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
