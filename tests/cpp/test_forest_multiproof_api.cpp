// C++ host-side test of merkle_forest_ragged_multiproof_device / _verify_device / _bound of include/poseidon252.hpp: a forest of three
// trees of different sizes is built with its levels, a shared proof of leaves of two of them is extracted and verified, the recomputed
// roots are compared with the oracle's single-tree builder, one tree's part is cut out and checked with the single-tree verify, and a
// changed proof, a short proof and unsorted pairs are refused, for both arities.
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
    Context& ctx = Context::default_context();
    auto sync = [&] { detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync"); };
    for (unsigned arity : {4u, 2u}) {
        const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
        const std::size_t sizes[3] = {37, 1, 301}, T = 3, n = 339, top = 301;
        const std::size_t depth = arity == 4 ? p252_merkle4_depth(top) : p252_merkle2_depth(top);
        Pinned<BlsScalar> leaves(n), levels(n / (arity - 1) + T * depth), roots(T), expected(T), scratch(2 * top);
        Pinned<std::uint64_t> offsets(T + 1);
        p252o_fill_random(900 + arity, leaves.p[0].data(), n);
        for (std::size_t t = 0; t < T; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t];
        auto build = arity == 4 ? p252_merkle4_forest_ragged_device : p252_merkle2_forest_ragged_device;
        detail::check(build(ctx.get(), tag.data(), leaves.p, n, offsets.p, T, top, roots.p, levels.p, nullptr, nullptr), ctx.get(), "forest_ragged_device");
        sync();
        for (std::size_t t = 0; t < T; ++t) {
            if (sizes[t] == 1) continue;  // (a one-leaf tree's root is its leaf, reduced: random leaves are canonical or not)
            if (arity == 4)
                p252o_merkle4_tree(tag.data(), leaves.p[offsets.p[t]].data(), sizes[t], expected.p[t].data(), scratch.p[0].data());
            else
                p252o_merkle2_tree(tag.data(), leaves.p[offsets.p[t]].data(), sizes[t], expected.p[t].data(), scratch.p[0].data());
            EXPECT(roots.p[t] == expected.p[t]);
        }
        const ForestView forest = {leaves.p, n, offsets.p, T, top, levels.p};
        // tree 0: two leaves of one parent and the last leaf; tree 2: a lone leaf, a run, the last leaf; tree 1: nobody asks
        const std::vector<std::uint32_t> tid = {0, 0, 0, 2, 2, 2, 2, 2, 2};
        const std::vector<std::uint64_t> lid = {4, 5, 36, 77, 150, 151, 152, 153, 300};
        const std::size_t k = tid.size(), bound = merkle_forest_ragged_multiproof_bound(n, T, top, k, arity);
        Pinned<std::uint32_t> tree_ids(k), n_bad(1);
        Pinned<std::uint64_t> leaf_ids(k), po(T + 1), n_hashed(1);
        Pinned<BlsScalar> out(k), proof(bound + 1), roots_out(T);
        Pinned<std::uint8_t> ok(T);
        for (std::size_t i = 0; i < k; ++i) tree_ids.p[i] = tid[i], leaf_ids.p[i] = lid[i];
        merkle_forest_ragged_multiproof_device(forest, tree_ids.p, leaf_ids.p, k, out.p, proof.p, bound, po.p, arity, ctx, n_bad.p);
        sync();
        const std::size_t len = po.p[T];
        EXPECT(n_bad.p[0] == 0 && len > 0 && len <= bound && po.p[0] == 0 && po.p[1] > 0 && po.p[2] == po.p[1] && po.p[3] > po.p[2]);
        for (std::size_t i = 0; i < k; ++i) EXPECT(out.p[i] == leaves.p[offsets.p[tid[i]] + lid[i]]);
        if (arity == 4) EXPECT(proof.p[0] == leaves.p[6]);  // the first missing sibling of tree 0: leaf 6 of parent 1 (leaves 4 and 5 are known)
        merkle_forest_ragged_multiproof_verify_device(forest, tree_ids.p, leaf_ids.p, out.p, k, proof.p, len, po.p, roots.p, ok.p, arity, ctx,
                                                      roots_out.p, n_hashed.p, n_bad.p);
        sync();
        EXPECT(ok.p[0] == 1 && ok.p[1] == 0 && ok.p[2] == 1 && roots_out.p[0] == expected.p[0] && roots_out.p[2] == expected.p[2]);
        EXPECT(n_hashed.p[0] > 0 && n_bad.p[0] == 0);
        // tree 2's part alone, with the single-tree verify
        Pinned<std::uint32_t> pos2(6);
        Pinned<std::uint8_t> ok1(1);
        for (std::size_t i = 0; i < 6; ++i) pos2.p[i] = (std::uint32_t)lid[3 + i];
        merkle_multiproof_verify_device(sizes[2], pos2.p, out.p + 3, 6, proof.p + po.p[2], po.p[3] - po.p[2], roots.p + 2, ok1.p, arity, ctx);
        sync();
        EXPECT(ok1.p[0] == 1);
        merkle_forest_ragged_multiproof_verify_device(forest, tree_ids.p, leaf_ids.p, out.p, k, proof.p, len - 1, po.p, roots.p, ok.p, arity, ctx);
        sync();
        EXPECT(ok.p[0] == 1 && ok.p[2] == 0);  // one scalar short: the last tree only
        proof.p[0][0] ^= 1;  // one scalar of tree 0's part changed
        merkle_forest_ragged_multiproof_verify_device(forest, tree_ids.p, leaf_ids.p, out.p, k, proof.p, len, po.p, roots.p, ok.p, arity, ctx);
        sync();
        EXPECT(ok.p[0] == 0 && ok.p[2] == 1);
        proof.p[0][0] ^= 1;
        tree_ids.p[3] = 0;  // (0, 77) behind (0, 36): leaf 77 is outside tree 0
        merkle_forest_ragged_multiproof_device(forest, tree_ids.p, leaf_ids.p, k, out.p, proof.p, bound, po.p, arity, ctx, n_bad.p);
        sync();
        EXPECT(n_bad.p[0] == 1 && po.p[T] == 0 && po.p[1] == 0);
    }
    bool threw = false;
    try {
        merkle_forest_ragged_multiproof_device(ForestView{nullptr, 0, nullptr, 0, 0, nullptr}, nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    EXPECT(merkle_forest_ragged_multiproof_bound(3 * 64, 3, 64, 3) == 27 && merkle_forest_ragged_multiproof_bound(0, 3, 64, 3) == 0);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
