// C++ host-side test of merkle_multiproof_device / merkle_multiproof_verify_device / merkle_multiproof_bound of
// include/poseidon252.hpp: a tree is built with its levels, a shared proof of several of its leaves is extracted and verified, the
// recomputed root is compared with the oracle's single-tree builder, and a changed proof, a short proof and unsorted positions are
// refused, for both arities.
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
        const std::size_t n = 301;
        const std::size_t n_levels = arity == 4 ? p252_merkle4_levels_len(n) : p252_merkle2_levels_len(n);
        Pinned<BlsScalar> leaves(n), levels(n_levels), root(1), expected(1), oracle_levels(n_levels);
        p252o_fill_random(700 + arity, leaves.p[0].data(), n);
        auto build = arity == 4 ? p252_merkle4_tree_device : p252_merkle2_tree_device;
        detail::check(build(ctx.get(), tag.data(), leaves.p, n, root.p, levels.p, nullptr), ctx.get(), "tree_device");
        sync();
        if (arity == 4)
            p252o_merkle4_tree(tag.data(), leaves.p[0].data(), n, expected.p[0].data(), oracle_levels.p[0].data());
        else
            p252o_merkle2_tree(tag.data(), leaves.p[0].data(), n, expected.p[0].data(), oracle_levels.p[0].data());
        EXPECT(root.p[0] == expected.p[0]);
        // two leaves of one parent, a lone leaf, the last leaf (its parent has one child)
        const std::vector<std::uint32_t> pos = {4, 5, 77, 150, 151, 152, 153, 300};
        const std::size_t k = pos.size(), bound = merkle_multiproof_bound(n, k, arity);
        Pinned<std::uint32_t> indices(k), n_bad(1);
        Pinned<BlsScalar> out(k), proof(bound + 1), root_out(1);
        Pinned<std::uint64_t> proof_len(1), n_hashed(1);
        Pinned<std::uint8_t> ok(1);
        for (std::size_t i = 0; i < k; ++i) indices.p[i] = pos[i];
        merkle_multiproof_device(leaves.p, n, levels.p, indices.p, k, out.p, proof.p, bound, proof_len.p, arity, ctx, n_bad.p);
        sync();
        const std::size_t len = proof_len.p[0];
        EXPECT(n_bad.p[0] == 0 && len > 0 && len <= bound);
        for (std::size_t i = 0; i < k; ++i) EXPECT(out.p[i] == leaves.p[pos[i]]);
        EXPECT(proof.p[0] == leaves.p[arity == 4 ? 6 : 76]);  // the first missing sibling: leaf 6 of parent 1 (arity 4), leaf 76 (arity 2)
        merkle_multiproof_verify_device(n, indices.p, out.p, k, proof.p, len, root.p, ok.p, arity, ctx, root_out.p, n_hashed.p, n_bad.p);
        sync();
        EXPECT(ok.p[0] == 1 && root_out.p[0] == expected.p[0] && n_hashed.p[0] > 0 && n_bad.p[0] == 0);
        merkle_multiproof_verify_device(n, indices.p, out.p, k, proof.p, len - 1, root.p, ok.p, arity, ctx);  // one scalar short
        sync();
        EXPECT(ok.p[0] == 0);
        proof.p[len / 2][0] ^= 1;  // one scalar changed
        merkle_multiproof_verify_device(n, indices.p, out.p, k, proof.p, len, root.p, ok.p, arity, ctx);
        sync();
        EXPECT(ok.p[0] == 0);
        proof.p[len / 2][0] ^= 1;
        indices.p[2] = 3;  // not above its predecessor
        merkle_multiproof_device(leaves.p, n, levels.p, indices.p, k, out.p, proof.p, bound, proof_len.p, arity, ctx, n_bad.p);
        sync();
        EXPECT(n_bad.p[0] == 1 && proof_len.p[0] == 0);
    }
    bool threw = false;
    try {
        merkle_multiproof_device(nullptr, 0, nullptr, nullptr, 1, nullptr, nullptr, 0, nullptr, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    EXPECT(merkle_multiproof_bound(64, 1) == 9 && merkle_multiproof_bound(64, 64) == 0 && merkle_multiproof_bound(1, 1) == 0);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
