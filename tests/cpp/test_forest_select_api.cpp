// C++ host-side test of merkle_forest_ragged_select_device of include/poseidon252.hpp: two forests of trees of different sizes are
// built with their tree-major levels, trees of both are gathered into a new forest in one call (out of order, one twice, one id out of
// range), and the new forest's offsets, leaves, levels and roots are compared with a fresh build of the same new forest and with the
// oracle's single-tree builder, for both arities; then the host refusals of the C entry points.  All buffers are page-locked host
// memory (p252_host_alloc), which the device reads and writes in place: no HIP header is needed.  The oracle (oracle/p252_oracle.h)
// is linked as the checker only.
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

static std::size_t sum(const std::vector<std::size_t>& v) {
    std::size_t s = 0;
    for (std::size_t n : v) s += n;
    return s;
}

int main() {
    const std::vector<std::size_t> sizes_a = {1, 5, 16, 17, 300, 2}, sizes_b = {64, 1, 700};
    const std::size_t n_a = sizes_a.size(), n_b = sizes_b.size(), max_a = 300, max_b = 700, leaves_a = sum(sizes_a), leaves_b = sum(sizes_b);
    // B's large tree first, a tree of A twice, an id past both forests (refused: an empty tree), single leaves of both
    const std::vector<std::uint64_t> pick = {8, 4, 0, 6, 4, 9, 7, 2, 1};
    const std::size_t n_pick = pick.size(), max_new = max_b;
    Context& ctx = Context::default_context();
    for (unsigned arity : {4u, 2u}) {
        const BlsScalar tag = arity == 4 ? compute_tag(Domain::Merkle4, {4}, 1) : compute_tag(Domain::Merkle2, {2}, 1);
        const std::size_t lv_a = forest_append_levels_cap(leaves_a, n_a, max_a, arity), lv_b = forest_append_levels_cap(leaves_b, n_b, max_b, arity);
        std::vector<std::size_t> want_sizes;
        for (std::uint64_t id : pick) want_sizes.push_back(id < n_a ? sizes_a[id] : id - n_a < n_b ? sizes_b[id - n_a] : 0);
        const std::size_t cap = sum(want_sizes) + 5, levels_cap = forest_append_levels_cap(cap, n_pick, max_new, arity);
        Pinned<BlsScalar> a_leaves(leaves_a), a_levels(lv_a), a_roots(n_a), b_leaves(leaves_b), b_levels(lv_b), b_roots(n_b);
        Pinned<BlsScalar> s_leaves(cap), s_levels(levels_cap), s_roots(n_pick), fresh_levels(levels_cap), fresh_roots(n_pick);
        Pinned<std::uint64_t> a_off(n_a + 1), b_off(n_b + 1), d_pick(n_pick), s_off(n_pick + 1);
        Pinned<std::uint32_t> bad(1);
        p252o_fill_random(900 + arity, a_leaves.p[0].data(), leaves_a);
        p252o_fill_random(950 + arity, b_leaves.p[0].data(), leaves_b);
        for (std::size_t t = 0; t < n_a; ++t) a_off.p[t + 1] = a_off.p[t] + sizes_a[t];
        for (std::size_t t = 0; t < n_b; ++t) b_off.p[t + 1] = b_off.p[t] + sizes_b[t];
        for (std::size_t j = 0; j < n_pick; ++j) d_pick.p[j] = pick[j];
        merkle_forest_ragged_device(a_leaves.p, leaves_a, a_off.p, n_a, max_a, a_roots.p, arity, ctx, a_levels.p);
        merkle_forest_ragged_device(b_leaves.p, leaves_b, b_off.p, n_b, max_b, b_roots.p, arity, ctx, b_levels.p);
        const ForestSource A = {{a_leaves.p, leaves_a, a_off.p, n_a, max_a, a_levels.p}, a_roots.p};
        const ForestSource B = {{b_leaves.p, leaves_b, b_off.p, n_b, max_b, b_levels.p}, b_roots.p};
        const ForestOut picked = {s_leaves.p, cap, s_off.p, s_levels.p, levels_cap, s_roots.p};
        merkle_forest_ragged_select_device(A, &B, d_pick.p, n_pick, picked, arity, ctx, bad.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        // what the new forest holds
        std::vector<BlsScalar> want;
        std::vector<std::uint64_t> want_off(1, 0);
        for (std::size_t j = 0; j < n_pick; ++j) {
            const bool from_b = pick[j] >= n_a;
            const std::size_t t = from_b ? pick[j] - n_a : pick[j];
            const BlsScalar* src = from_b ? b_leaves.p + b_off.p[t < n_b ? t : 0] : a_leaves.p + a_off.p[t];
            for (std::size_t i = 0; i < want_sizes[j]; ++i) want.push_back(src[i]);
            want_off.push_back(want.size());
        }
        EXPECT(bad.p[0] == 1);
        EXPECT(std::memcmp(s_off.p, want_off.data(), (n_pick + 1) * 8) == 0);
        for (std::size_t i = 0; i < want.size(); ++i) EXPECT(s_leaves.p[i] == want[i]);
        for (std::size_t i = want.size(); i < cap; ++i) EXPECT(s_leaves.p[i] == BlsScalar{});  // nothing past the used length
        bad.p[0] = 0;
        merkle_forest_ragged_device(s_leaves.p, cap, s_off.p, n_pick, max_new, fresh_roots.p, arity, ctx, fresh_levels.p, bad.p);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(bad.p[0] == 1);
        EXPECT(std::memcmp(s_levels.p, fresh_levels.p, levels_cap * sizeof(BlsScalar)) == 0);  // (past the used part both are still zero)
        for (std::size_t j = 0; j < n_pick; ++j) {
            const std::size_t n = want_sizes[j];
            EXPECT(s_roots.p[j] == fresh_roots.p[j]);
            if (n == 0) {
                EXPECT(s_roots.p[j] == BlsScalar{});
                continue;
            }
            BlsScalar expected;
            std::vector<BlsScalar> lv(n + 64);
            if (arity == 4)
                p252o_merkle4_tree(tag.data(), want[want_off[j]].data(), n, expected.data(), lv[0].data());
            else
                p252o_merkle2_tree(tag.data(), want[want_off[j]].data(), n, expected.data(), lv[0].data());
            EXPECT(s_roots.p[j] == expected);
        }
        // A alone, every tree in place: the forest itself
        Pinned<std::uint64_t> ident(n_a), i_off(n_a + 1);
        Pinned<BlsScalar> i_leaves(leaves_a), i_levels(lv_a), i_roots(n_a);
        for (std::size_t t = 0; t < n_a; ++t) ident.p[t] = t;
        merkle_forest_ragged_select_device(A, nullptr, ident.p, n_a, ForestOut{i_leaves.p, leaves_a, i_off.p, i_levels.p, lv_a, i_roots.p}, arity, ctx);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
        EXPECT(std::memcmp(i_off.p, a_off.p, (n_a + 1) * 8) == 0 && std::memcmp(i_leaves.p, a_leaves.p, leaves_a * 32) == 0);
        EXPECT(std::memcmp(i_levels.p, a_levels.p, lv_a * 32) == 0 && std::memcmp(i_roots.p, a_roots.p, n_a * 32) == 0);

        // the host refusals of the C entry point: nothing is enqueued, the outputs stay as they are
        auto* fn = arity == 4 ? p252_merkle4_forest_ragged_select_device_into : p252_merkle2_forest_ragged_select_device_into;
        auto call = [&](const void* la, std::size_t nta, const void* pk, std::size_t np, void* out_leaves, std::size_t lcap, std::size_t vcap) {
            return fn(ctx.get(), la, leaves_a, a_off.p, nta, max_a, a_levels.p, a_roots.p, b_leaves.p, leaves_b, b_off.p, n_b, max_b, b_levels.p,
                      b_roots.p, pk, np, out_leaves, lcap, s_off.p, s_levels.p, vcap, s_roots.p, bad.p, nullptr);
        };
        EXPECT(call(a_leaves.p, n_a, d_pick.p, n_pick, s_leaves.p, cap, levels_cap) == P252_OK);  // the control
        EXPECT(call(a_leaves.p, 0, d_pick.p, n_pick, s_leaves.p, cap, levels_cap) == P252_ERR_INVALID_ARGUMENT);
        EXPECT(call(a_leaves.p, n_a, d_pick.p, 0, s_leaves.p, cap, levels_cap) == P252_OK);
        EXPECT(call(nullptr, n_a, d_pick.p, n_pick, s_leaves.p, cap, levels_cap) == P252_ERR_INVALID_ARGUMENT);
        EXPECT(call(a_leaves.p, n_a, nullptr, n_pick, s_leaves.p, cap, levels_cap) == P252_ERR_INVALID_ARGUMENT);
        EXPECT(call(a_leaves.p, n_a, reinterpret_cast<const char*>(d_pick.p) + 4, n_pick - 1, s_leaves.p, cap, levels_cap) == P252_ERR_INVALID_ARGUMENT);
        EXPECT(call(a_leaves.p, n_a, d_pick.p, n_pick, reinterpret_cast<char*>(s_leaves.p) + 8, cap - 1, levels_cap) == P252_ERR_INVALID_ARGUMENT);
        EXPECT(call(a_leaves.p, n_a, d_pick.p, n_pick, s_leaves.p, 0, levels_cap) == P252_ERR_INVALID_ARGUMENT);
        EXPECT(call(a_leaves.p, n_a, d_pick.p, n_pick, s_leaves.p, cap, levels_cap - 1) == P252_ERR_INVALID_ARGUMENT);
        EXPECT(call(a_leaves.p, n_a, d_pick.p, n_pick, a_leaves.p + leaves_a - 1, cap, levels_cap) == P252_ERR_INVALID_ARGUMENT);  // overlaps d_leaves_a
        EXPECT(std::string(p252_last_error(ctx.get())).find("d_leaves_new overlaps d_leaves_a") != std::string::npos);
        detail::check(p252_sync(ctx.get(), nullptr), ctx.get(), "p252_sync");
    }
    bool threw = false;
    try {
        merkle_forest_ragged_select_device(ForestSource{}, nullptr, nullptr, 1, ForestOut{}, 3);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s\n", failures ? "FAILED" : "ALL PASSED");
    return failures ? 1 : 0;
}
