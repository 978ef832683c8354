// C++ host-side test of merkle_forest_range_stride, merkle_forest_ragged_range_proofs_device and merkle_forest_range_verify_device of
// include/poseidon252.hpp: a forest of trees of different sizes is built, runs of leaves of its trees are proved in one call and
// checked in one call against the build's roots, for both arities; a whole tree has an empty proof, a run past its tree is refused
// alone, and a changed leaf fails its run alone.  All buffers are page-locked host memory (p252_host_alloc), which the device reads and
// writes in place: no HIP header is needed.
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
    const std::size_t n_trees = sizes.size(), max_leaves = 300;
    std::size_t n_leaves = 0;
    for (std::size_t n : sizes) n_leaves += n;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const std::size_t D = forest_openings_stride(max_leaves, arity), per = arity - 1;
        const std::size_t stride = merkle_forest_range_stride(max_leaves, arity);
        EXPECT(stride == 2 * per * D);
        const std::size_t n_levels = n_leaves / per + n_trees * D;
        Pinned<BlsScalar> leaves(n_leaves), levels(n_levels), roots(n_trees);
        Pinned<std::uint64_t> offsets(n_trees + 1);
        p252o_fill_random(2300 + arity, leaves.p[0].data(), n_leaves);
        for (std::size_t t = 0; t < n_trees; ++t) offsets.p[t + 1] = offsets.p[t] + sizes[t];
        merkle_forest_ragged_device(leaves.p, n_leaves, offsets.p, n_trees, max_leaves, roots.p, arity, ctx, levels.p);
        // (tree, first, length): a middle run, a whole tree, one leaf, a run to the end, the one-leaf tree; run 5 is one leaf too long
        const std::uint32_t tid[] = {4, 2, 3, 4, 0, 1};
        const std::uint64_t first[] = {101, 0, 16, 250, 0, 3}, len[] = {77, 16, 1, 50, 1, 3};
        const std::size_t m = 6, bad_run = 5;
        Pinned<std::uint32_t> r_tree(m), lens(m), bad(2);
        Pinned<std::uint64_t> r_first(m), r_off(m + 1), counts(m), hashed(1);
        for (std::size_t r = 0; r < m; ++r) r_tree.p[r] = tid[r], r_first.p[r] = first[r], r_off.p[r + 1] = r_off.p[r] + len[r];
        const std::size_t k = r_off.p[m];
        Pinned<BlsScalar> out(k), proof(m * stride), roots_out(m);
        Pinned<std::uint8_t> ok(m), ok2(m);
        const ForestView forest = {leaves.p, n_leaves, offsets.p, n_trees, max_leaves, levels.p};
        const ForestRuns runs = {r_tree.p, r_first.p, r_off.p, m, k};
        const RangeProofs proofs = {out.p, proof.p, stride, lens.p, counts.p};
        merkle_forest_ragged_range_proofs_device(forest, runs, proofs, arity, ctx, bad.p);
        merkle_forest_range_verify_device(runs, proofs, max_leaves, roots.p, n_trees, ok.p, arity, ctx, roots_out.p, hashed.p, bad.p + 1);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(bad.p[0] == 1 && bad.p[1] == 1 && hashed.p[0] > 0);
        for (std::size_t r = 0; r < m; ++r) {
            const bool good = r != bad_run;
            EXPECT(ok.p[r] == (good ? 1 : 0));
            EXPECT(counts.p[r] == (good ? sizes[tid[r]] : 0));
            EXPECT(good ? lens.p[r] <= stride : lens.p[r] == 0xFFFFFFFFu);
            if (!good) continue;
            EXPECT(roots_out.p[r] == roots.p[tid[r]]);
            for (std::size_t j = 0; j < len[r]; ++j) EXPECT(out.p[r_off.p[r] + j] == leaves.p[offsets.p[tid[r]] + first[r] + j]);
            for (std::size_t q = lens.p[r]; q < stride; ++q) EXPECT(proof.p[r * stride + q] == BlsScalar{});
        }
        EXPECT(lens.p[1] == 0 && lens.p[4] == 0 && lens.p[0] > 0);
        // a changed leaf fails its run alone
        out.p[r_off.p[3] + 7][0] ^= 1;
        merkle_forest_range_verify_device(runs, proofs, max_leaves, roots.p, n_trees, ok2.p, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        for (std::size_t r = 0; r < m; ++r) EXPECT(ok2.p[r] == (r == 3 || r == bad_run ? 0 : 1));
    }
    bool threw = false;
    try {
        merkle_forest_range_stride(100, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
