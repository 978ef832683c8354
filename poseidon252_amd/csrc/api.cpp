// api.cpp — C ABI of libposeidon252_hip.so (include/poseidon252_hip.h).
// Host side only: context / device-memory management, io-pattern rules mirroring src/hash.rs,
// launch sequencing.  All hashing runs in kernels.hip; there is no CPU path.  (The ragged-forest family is in api_forest.cpp, the
// host-buffer entry points in host_io.cpp.)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/poseidon252_hip.h"
#include "api_util.hpp"
#include "blake2b.hpp"
#include "crypt_ragged.h"
#include "ctx.hpp"
#include "hades29.hpp"
#include "kernels.h"
#include "multiproof.h"
#include "openings.h"
#include "ragged.h"
#include "tables.hpp"
#include "_gen/assets.inc"

using namespace p252;
using namespace p252host;

static std::string g_create_err;
static std::mutex g_mu;

int p252host::fail(p252_ctx* ctx, int code, const std::string& msg) {
    if (ctx)
        ctx->err = msg;
    else {
        std::lock_guard<std::mutex> lk(g_mu);
        g_create_err = msg;
    }
    return code;
}

int p252host::ensure(p252_ctx* ctx, void** buf, size_t* cap, size_t need) {
    if (need <= *cap) return P252_OK;
    if (*buf) HIP_TRY(ctx, hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    HIP_TRY(ctx, hipMalloc(buf, need));
    *cap = need;
    return P252_OK;
}

// the scratch pair of a call on `st` (at least need0 / need1 bytes) and, below, the record of its event behind the call's last launch:
// with_stream_scratch (api_util.hpp) is their only caller
int p252host::level_set(p252_ctx* ctx, hipStream_t st, size_t need0, size_t need1, p252_ctx::LevelSet** out) {
    p252_ctx::LevelSet* set = nullptr;
    for (auto& s : ctx->lvl)
        if (s.st == st) set = &s;
    if (!set && ctx->lvl.size() < p252_ctx::MAX_LEVEL_SETS) {
        if (ctx->lvl.capacity() < p252_ctx::MAX_LEVEL_SETS) ctx->lvl.reserve(p252_ctx::MAX_LEVEL_SETS);  // (pointers into it stay valid)
        ctx->lvl.emplace_back();
        set = &ctx->lvl.back();
        set->st = st;
        const hipError_t e = hipEventCreateWithFlags(&set->done, hipEventDisableTiming);
        if (e != hipSuccess) {  // never leave a half-made pair (done == nullptr) in the list
            ctx->lvl.pop_back();
            return fail(ctx, P252_ERR_HIP, std::string("hipEventCreateWithFlags: ") + hipGetErrorString(e));
        }
    }
    if (!set) {  // more streams than pairs: take over the least recently used pair, behind its last build
        set = &ctx->lvl[0];
        for (auto& s : ctx->lvl)
            if (s.stamp < set->stamp) set = &s;
        if (set->stamp) HIP_TRY(ctx, hipStreamWaitEvent(st, set->done, 0));
        set->st = st;
    }
    // (growing frees the old buffer: hipFree waits for the device, so no queued launch still reads it)
    int rc = ensure(ctx, &set->buf[0], &set->cap[0], need0);
    if (rc == P252_OK) rc = ensure(ctx, &set->buf[1], &set->cap[1], need1);
    if (rc) return rc;
    *out = set;
    return P252_OK;
}

int p252host::level_set_done(p252_ctx* ctx, p252_ctx::LevelSet* set) {
    set->stamp = ++ctx->lvl_clock;
    HIP_TRY(ctx, hipEventRecord(set->done, set->st));
    return P252_OK;
}

const std::vector<int32_t>& p252host::host_tables() {
    static const std::vector<int32_t> tab = [] {
        HadesTables T;
        derive_tables(ARC_BIN, MDS_BIN, T);
        // the kernels' schedule rests on mds.bin being R/(i+j+5) (tables.hpp): never run it on anything else
        return T.int_ok ? encode_tables29(T) : std::vector<int32_t>();
    }();
    return tab;
}

TagArg p252host::tag_arg(const uint64_t tag[4]) {
    TagArg t;
    std::memcpy(t.w, tag, 32);
    const E29 x0 = hades_pre0(from_mont4(t.w), host_tables().data());
    for (int k = 0; k < NL; ++k) t.x0[k] = x0.d[k];
    return t;
}

// runs f(t) for every context index on its own host thread (t = 0 on the calling thread); first failure wins
template <class F>
static int for_each_ctx(p252_ctx* const* ctxs, size_t n_ctx, F&& f) {
    std::vector<int> rcs(n_ctx, P252_OK);
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_ctx; ++t) pool.emplace_back([&, t] { rcs[t] = f(t); });
    rcs[0] = f(0);
    for (auto& th : pool) th.join();
    for (size_t t = 0; t < n_ctx; ++t)
        if (rcs[t] != P252_OK) {
            if (t != 0 && ctxs[0]) ctxs[0]->err = "context " + std::to_string(t) + ": " + ctxs[t]->err;  // p252_last_error(ctxs[0])
            return rcs[t];
        }
    return P252_OK;
}

// ---- secret hygiene (the reference builds its scalars with `zeroize`, Cargo.toml:14, and dusk-safe zeroizes the sponge state
// when a sponge finishes; src/encryption.rs:62-95 hands shared secrets, nonces and plaintexts through it).  The kernels keep
// every sponge state in registers; what outlives a HOST-buffer encrypt / decrypt call is the library's own copy of the
// caller's arrays: the context's device scratch and the page-locked staging lanes.  wipe_span / wipe_lanes clear exactly
// those at the end of such a call; wipe_all clears every buffer the context owns (p252_wipe, p252_destroy). ----
hipError_t p252host::wipe_span(void* d, size_t bytes) { return (d && bytes) ? hipMemsetAsync(d, 0, bytes, nullptr) : hipSuccess; }

// dirty_only: just the bytes calls may have written since the last wipe (staged_run keeps the extent per slot) — what the per-call
// wipe of a host-buffer encrypt / decrypt needs; the full capacity otherwise (p252_wipe, p252_trim, p252_destroy)
hipError_t p252host::wipe_lanes(p252_ctx* ctx, bool dirty_only) {
    hipError_t first = hipSuccess;
    for (auto& l : ctx->lanes)
        for (auto& sl : l.slot) {
            const size_t in_b = dirty_only ? sl.in_dirty : sl.in_cap, out_b = dirty_only ? sl.out_dirty : sl.out_cap;
            if (sl.h_in && in_b) std::memset(sl.h_in, 0, in_b);
            if (sl.h_out && out_b) std::memset(sl.h_out, 0, out_b);
            hipError_t e = wipe_span(sl.d_in, in_b);
            if (e == hipSuccess) e = wipe_span(sl.d_out, out_b);
            if (e != hipSuccess && first == hipSuccess) first = e;
            sl.in_dirty = sl.out_dirty = 0;
        }
    return first;
}

static hipError_t wipe_all(p252_ctx* ctx) {
    hipError_t e = hipDeviceSynchronize();  // nothing queued may still read or write what is cleared below
    auto keep = [&](hipError_t r) {
        if (r != hipSuccess && e == hipSuccess) e = r;
    };
    keep(wipe_span(ctx->d_in, ctx->d_in_cap));
    keep(wipe_span(ctx->d_out, ctx->d_out_cap));
    for (auto& set : ctx->lvl)
        for (int i = 0; i < 2; ++i) keep(wipe_span(set.buf[i], set.cap[i]));
    keep(wipe_span(ctx->d_prog, ctx->d_prog_cap));
    ctx->prog_variant = -1;  // (the call table is gone: the next encrypt / decrypt uploads it again)
    ctx->prog_len = 0;
    keep(wipe_lanes(ctx));
    keep(hipStreamSynchronize(nullptr));
    return e;
}

// non-zero bytes of a device buffer, read back 16 MiB at a time (diagnostics only)
static hipError_t count_nonzero_device(const void* d, size_t bytes, uint64_t* total) {
    if (!d || !bytes) return hipSuccess;
    std::vector<uint64_t> host((size_t)2 << 20);
    for (size_t off = 0; off < bytes; off += host.size() * 8) {
        const size_t cnt = bytes - off < host.size() * 8 ? bytes - off : host.size() * 8;
        host[(cnt - 1) / 8] = 0;
        const hipError_t e = hipMemcpy(host.data(), static_cast<const char*>(d) + off, cnt, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        const unsigned char* b = reinterpret_cast<const unsigned char*>(host.data());
        for (size_t i = 0; i < cnt; ++i) *total += b[i] != 0;
    }
    return hipSuccess;
}

size_t p252host::levels_len(size_t n_leaves, size_t arity) {
    size_t total = 0, c = n_leaves;
    while (c > 1) {
        c = (c + arity - 1) / arity;
        total += c;
    }
    return total;
}

int p252host::merkle_tree_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                              void* d_root, void* d_levels, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle_tree"};
    if (n_leaves == 0) return refuse("n_leaves must be > 0");
    if (!tag || !d_leaves || !d_root) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels})) return rc;  // d_root: plain copy
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const TagArg t = tag_arg(tag);
    // A build with wide levels (more nodes than the chip has lanes at one wave per SIMD: 65,536) keeps every SIMD
    // loaded through its narrow levels by computing them redundantly (kernels.hip k_merkle4_pad: the next wide launch
    // would otherwise start at a dipped clock).  P252_TREE_PAD_LANES overrides the lane count; 0 = off.
    static const long pad_env = [] {
        const char* e = std::getenv("P252_TREE_PAD_LANES");
        return e ? std::atol(e) : -1L;
    }();
    const size_t chip_lanes = 65536;
    const size_t l1 = (n_leaves + arity - 1) / arity, l2 = (l1 + arity - 1) / arity;
    const size_t pad = pad_env >= 0 ? (size_t)pad_env : (l1 > chip_lanes ? chip_lanes : 0);
    auto build = [&](void* const* ping) {  // the levels go to d_levels, or ping-pong between ping[0] and ping[1]
        const char* cur = static_cast<const char*>(d_leaves);
        size_t cur_n = n_leaves;
        char* lv = static_cast<char*>(d_levels);
        int parity = 0;
        while (cur_n > 1) {  // a single leaf is its own root: an arity^k-leaf tree costs exactly k levels
            const size_t next_n = (cur_n + arity - 1) / arity;
            char* next = d_levels ? lv : static_cast<char*>(ping[parity]);
            const hipError_t e = launch_merkle4(ctx->d_tab, t, cur, cur_n, next, next_n, st, arity, pad);
            if (e != hipSuccess) return e;
            cur = next;
            cur_n = next_n;
            if (d_levels) lv += next_n * 32;
            parity ^= 1;
        }
        return hipMemcpyAsync(d_root, cur, 32, hipMemcpyDeviceToDevice, st);
    };
    if (d_levels || n_leaves == 1) return launched(ctx, "merkle_tree", build(nullptr));  // no context scratch
    // ping-pong in context-owned scratch: the pair of THIS stream (ctx.hpp)
    return with_stream_scratch(ctx, "merkle_tree", st, l1 * 32, l2 * 32, [&](p252_ctx::LevelSet& set) { return build(set.buf); });
}

// The sponge-call sequence dusk_safe::encrypt makes, as a table (one word per call: kind << 29 | len; kinds as in
// kernels.hip k_crypt).  Two candidates (include/poseidon252_hip.h): P252_CRYPT_STREAM — squeeze all `len` masks, then
// absorb the whole message — and P252_CRYPT_DUPLEX — squeeze / absorb per chunk of <= 4.  Adding a third is one more
// branch here: the kernel, the tag and the oracle all derive from the table.
static std::vector<uint32_t> crypt_program(int variant, size_t len) {
    std::vector<uint32_t> prog;
    auto call = [&](uint32_t kind, size_t n) { prog.push_back((kind << 29) | (uint32_t)n); };
    call(0, 2);  // Absorb(2): shared secret (u, v)
    call(1, 1);  // Absorb(1): nonce
    if (variant == P252_CRYPT_STREAM) {
        call(2, len);  // Squeeze(len): masks
        call(3, len);  // Absorb(len): message
    } else {
        for (size_t left = len; left;) {
            const size_t c = left < 4 ? left : 4;
            call(2, c);
            call(3, c);
            left -= c;
        }
    }
    call(4, 1);  // Squeeze(1): MAC
    return prog;
}

bool p252host::crypt_variant_ok(int variant) { return variant == P252_CRYPT_STREAM || variant == P252_CRYPT_DUPLEX; }

// the sponge-call table of (variant, len) on the device (kept until another one is asked for)
int p252host::prepare_prog(p252_ctx* ctx, int variant, size_t len) {
    if (ctx->prog_variant == variant && ctx->prog_len == len) return P252_OK;
    const std::vector<uint32_t> prog = crypt_program(variant, len);
    // the previous program may still be read by a kernel in flight on another stream: drain before replacing it
    HIP_TRY(ctx, hipDeviceSynchronize());
    int rc = ensure(ctx, (void**)&ctx->d_prog, &ctx->d_prog_cap, prog.size() * sizeof(uint32_t));
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->d_prog, prog.data(), prog.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->prog_variant = variant;
    ctx->prog_len = len;
    ctx->prog_calls = (unsigned)prog.size();
    return P252_OK;
}

bool p252host::power_of_4(size_t v) {
    if (v == 0 || (v & (v - 1))) return false;
    int tz = 0;
    while (!((v >> tz) & 1)) ++tz;
    return (tz & 1) == 0;
}

int p252host::check_ctxs(p252_ctx* const* ctxs, size_t n_ctx) {
    if (!ctxs || n_ctx == 0) return P252_ERR_INVALID_ARGUMENT;
    for (size_t t = 0; t < n_ctx; ++t)
        if (!ctxs[t]) return P252_ERR_INVALID_ARGUMENT;
    for (size_t a = 0; a < n_ctx; ++a)  // a context is used by one thread at a time: no duplicates
        for (size_t b = a + 1; b < n_ctx; ++b)
            if (ctxs[a] == ctxs[b]) return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT, "multi: the same context appears twice");
    // one context per GPU is the point of these entry points: when the node has at least n_ctx devices, two contexts on the
    // same device are a caller's mistake (every shard would land on one GPU).  Fewer devices than contexts — the
    // single-GPU test configuration — is allowed.  P252_MULTI_ALLOW_SHARED_DEVICE=1 lifts the check.
    static const bool allow_shared = [] {
        const char* e = std::getenv("P252_MULTI_ALLOW_SHARED_DEVICE");
        return e && e[0] == '1';
    }();
    if (!allow_shared && (size_t)p252_device_count() >= n_ctx)
        for (size_t a = 0; a < n_ctx; ++a)
            for (size_t b = a + 1; b < n_ctx; ++b)
                if (ctxs[a]->device == ctxs[b]->device)
                    return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT,
                                "multi: contexts " + std::to_string(a) + " and " + std::to_string(b) + " are bound to the same device although the node has one per context");
    return P252_OK;
}

extern "C" {

int p252_abi_version(void) { return P252_ABI_VERSION; }

const char* p252_version(void) { return "poseidon252_hip 0.8 (gfx950; 9x29-bit limbs; integer MDS + integer ARMA recurrence; 32-bit Montgomery quotient digits; lane-group kernels for small batches)"; }

int p252_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int p252_create(int device_id, p252_ctx** out) {
    if (!out) return fail(nullptr, P252_ERR_INVALID_ARGUMENT, "p252_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, P252_ERR_NO_DEVICE,
                    std::string("no HIP device available (") + hipGetErrorString(e) +
                        "); this library has no CPU fallback");
    if (device_id < 0 || device_id >= n) return fail(nullptr, P252_ERR_INVALID_ARGUMENT, "p252_create: bad device id");
    p252_ctx* ctx = new p252_ctx();
    ctx->device = device_id;
    ctx->h_tab = host_tables();
    if (ctx->h_tab.empty()) {
        delete ctx;
        return fail(nullptr, P252_ERR_INVALID_ARGUMENT, "p252_create: the built-in mds.bin is not the Cauchy matrix R/(i+j+5) the kernels' schedule requires");
    }
    hipError_t e2 = hipSetDevice(device_id);
    if (e2 == hipSuccess) e2 = hipMalloc((void**)&ctx->d_tab, ctx->h_tab.size() * sizeof(int32_t));
    if (e2 == hipSuccess)
        e2 = hipMemcpy(ctx->d_tab, ctx->h_tab.data(), ctx->h_tab.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e2 != hipSuccess) {
        std::string msg = std::string("p252_create: ") + hipGetErrorString(e2);
        delete ctx;
        return fail(nullptr, P252_ERR_HIP, msg);
    }
    *out = ctx;
    return P252_OK;
}

// gives back what the grow-only scratch has grown to (after a 2^32-leaf root-only build the context kept 40 GiB
// until p252_destroy).  Wiped first, like p252_wipe; the constant table, the communicator and its 100 bytes stay.
static void free_scratch(p252_ctx* ctx) {
    if (ctx->d_in) (void)hipFree(ctx->d_in);
    if (ctx->d_out) (void)hipFree(ctx->d_out);
    ctx->d_in = ctx->d_out = nullptr;
    ctx->d_in_cap = ctx->d_out_cap = 0;
    for (auto& s : ctx->lvl) {
        for (int i = 0; i < 2; ++i)
            if (s.buf[i]) (void)hipFree(s.buf[i]);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    ctx->lvl.clear();
    if (ctx->d_prog) (void)hipFree(ctx->d_prog);
    ctx->d_prog = nullptr;
    ctx->d_prog_cap = 0;
    ctx->prog_variant = -1;
    ctx->prog_len = 0;
    for (auto& l : ctx->lanes) {
        if (l.st) (void)hipStreamDestroy(l.st);
        for (auto& sl : l.slot) {
            if (sl.h_in) (void)hipHostFree(sl.h_in);
            if (sl.h_out) (void)hipHostFree(sl.h_out);
            if (sl.d_in) (void)hipFree(sl.d_in);
            if (sl.d_out) (void)hipFree(sl.d_out);
            if (sl.done) (void)hipEventDestroy(sl.done);
        }
    }
    ctx->lanes.clear();
}

void p252_destroy(p252_ctx* ctx) {
    if (!ctx) return;
    release_ctx_comm(ctx);
    (void)hipSetDevice(ctx->device);
    (void)wipe_all(ctx);  // nothing a call left in the context's scratch or staging survives it (zeroize, Cargo.toml:14)
    if (ctx->d_tab) (void)hipFree(ctx->d_tab);
    free_scratch(ctx);
    for (int i = 0; i < 3; ++i)
        if (ctx->streams[i]) (void)hipStreamDestroy(ctx->streams[i]);
    delete ctx;
}

const char* p252_last_error(const p252_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    std::lock_guard<std::mutex> lk(g_mu);
    return g_create_err.c_str();
}

int p252_sync(p252_ctx* ctx, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)hip_stream));
    return comm_take_failure(ctx);  // a peer's failed local build in a sharded tree on this stream surfaces here (comm.cpp)
}

int p252_trim(p252_ctx* ctx) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, wipe_all(ctx));  // (starts with a device synchronisation: nothing queued still uses what is freed below)
    free_scratch(ctx);
    return P252_OK;
}

int p252_wipe(p252_ctx* ctx) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, wipe_all(ctx));
    return P252_OK;
}

int p252_scratch_residue(p252_ctx* ctx, uint64_t* nonzero_bytes) {
    if (!ctx || !nonzero_bytes) return Refusal{ctx, "scratch_residue"}("NULL argument");
    *nonzero_bytes = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, count_nonzero_device(ctx->d_in, ctx->d_in_cap, nonzero_bytes));
    HIP_TRY(ctx, count_nonzero_device(ctx->d_out, ctx->d_out_cap, nonzero_bytes));
    for (auto& set : ctx->lvl)
        for (int i = 0; i < 2; ++i) HIP_TRY(ctx, count_nonzero_device(set.buf[i], set.cap[i], nonzero_bytes));
    // (d_prog, the sponge-call table of the last (variant, length), holds nothing of the caller's: not counted)
    for (auto& l : ctx->lanes)
        for (auto& sl : l.slot) {
            HIP_TRY(ctx, count_nonzero_device(sl.d_in, sl.in_cap, nonzero_bytes));
            HIP_TRY(ctx, count_nonzero_device(sl.d_out, sl.out_cap, nonzero_bytes));
            for (size_t i = 0; sl.h_in && i < sl.in_cap; ++i) *nonzero_bytes += static_cast<const unsigned char*>(sl.h_in)[i] != 0;
            for (size_t i = 0; sl.h_out && i < sl.out_cap; ++i) *nonzero_bytes += static_cast<const unsigned char*>(sl.h_out)[i] != 0;
        }
    return P252_OK;
}

// ------------------------------------------------------------------------------------------
// device-buffer entry points
// ------------------------------------------------------------------------------------------
int p252_permute_batch_device(p252_ctx* ctx, const void* d_states, void* d_out, size_t n, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "permute"};
    if (n == 0) return P252_OK;
    if (!d_states || !d_out) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_states, d_out})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_permute(ctx->d_tab, d_states, d_out, n, (hipStream_t)hip_stream));
    return P252_OK;
}

// trunc250: Hash::finalize_truncated (hash.rs:164-183) — the digest kernels' output stage canonicalises, masks to 250 bits and
// stores the raw limbs JubJubScalar::from_raw receives: one launch, no BlsScalar round trip through HBM
static int hash_batch_device_impl(p252_ctx* ctx, const uint64_t tag[4], const void* d_in, size_t in_len,
                                  size_t out_len, void* d_out, size_t n, void* hip_stream, bool trunc250) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "hash"};
    // dusk-safe rejects io-patterns with an empty absorb or squeeze -> Hash::finalize panics (hash.rs:134-137)
    if (in_len == 0 || out_len == 0)
        return fail(ctx, P252_ERR_INVALID_IO_PATTERN, "hash: in_len and out_len must be > 0");
    if (in_len > 0x7fffffffu || out_len > 0x7fffffffu) return refuse("length too large");
    if (n == 0) return P252_OK;
    if (!tag || !d_in || !d_out) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_in, d_out})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (in_len == 4 && out_len == 1)
        HIP_TRY(ctx, launch_merkle4(ctx->d_tab, tag_arg(tag), d_in, 4 * n, d_out, n, st, 4, 0, trunc250));
    else if (in_len == 2 && out_len == 1)  // Merkle2-shaped digests take the single-permutation kernel too
        HIP_TRY(ctx, launch_merkle4(ctx->d_tab, tag_arg(tag), d_in, 2 * n, d_out, n, st, 2, 0, trunc250));
    else
        HIP_TRY(ctx, launch_sponge(ctx->d_tab, tag_arg(tag), d_in, (unsigned)in_len, (unsigned)out_len, d_out, n, st, trunc250));
    return P252_OK;
}

int p252_hash_batch_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_in, size_t in_len,
                           size_t out_len, void* d_out, size_t n, void* hip_stream) {
    return hash_batch_device_impl(ctx, tag, d_in, in_len, out_len, d_out, n, hip_stream, false);
}

int p252_hash_batch_truncated_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_in, size_t in_len,
                                     size_t out_len, void* d_out_raw, size_t n, void* hip_stream) {
    return hash_batch_device_impl(ctx, tag, d_in, in_len, out_len, d_out_raw, n, hip_stream, true);
}

P252_MERKLE_PAIR(size_t, levels_len, (size_t n_leaves), levels_len(n_leaves, arity))

P252_MERKLE_PAIR(int, tree_device,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves, void* d_root, void* d_levels, void* hip_stream),
                 merkle_tree_device(ctx, arity, tag, d_leaves, n_leaves, d_root, d_levels, hip_stream))

// A forest of n_trees independent complete arity-4 trees of leaves_per_tree = 4^k leaves each, tree-major in d_leaves
// (the shape of the downstream poseidon-merkle consumers, AGENTS.md:62-66: many small trees).  Level l of ALL trees is one
// array of n_trees * 4^(k-l) nodes, tree-major — so the forest is the first k levels of the level-by-level reduction of
// the concatenated leaves, and each level is ONE launch across all trees: the narrow upper levels of many small trees
// fill the chip together instead of each paying one wave's latency per tree.
static int forest_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves, size_t n_trees, size_t leaves_per_tree,
                         void* d_roots, void* d_levels, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle_forest"};
    if (n_trees == 0) return P252_OK;
    const bool pow_ok = arity == 4 ? power_of_4(leaves_per_tree) : (leaves_per_tree != 0 && (leaves_per_tree & (leaves_per_tree - 1)) == 0);
    if (!pow_ok) return refuse("leaves_per_tree must be arity^k");
    if (n_trees > (SIZE_MAX / 32) / leaves_per_tree) return refuse("size overflow");
    if (!tag || !d_leaves || !d_roots) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_roots, d_levels})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t cur_n = n_trees * leaves_per_tree;
    if (leaves_per_tree == 1) {  // a single leaf is its own root (as in p252_merkle4_tree_device)
        HIP_TRY(ctx, hipMemcpyAsync(d_roots, d_leaves, cur_n * 32, hipMemcpyDeviceToDevice, st));
        return P252_OK;
    }
    const TagArg t = tag_arg(tag);
    // narrow levels after wide ones are computed redundantly on every SIMD, as in the tree builder (clock dip)
    const size_t pad = cur_n / arity > 65536 ? 65536 : 0;
    auto build = [&](void* const* ping) {  // the levels go to d_levels, or ping-pong between ping[0] and ping[1]
        const char* cur = static_cast<const char*>(d_leaves);
        char* lv = static_cast<char*>(d_levels);
        size_t level_n = cur_n;
        int parity = 0;
        while (level_n > n_trees) {
            const size_t next_n = level_n / arity;
            char* next = next_n == n_trees ? static_cast<char*>(d_roots) : (d_levels ? lv : static_cast<char*>(ping[parity]));
            hipError_t e = launch_merkle4(ctx->d_tab, t, cur, level_n, next, next_n, st, arity, pad);
            if (e == hipSuccess && d_levels && next_n == n_trees) e = hipMemcpyAsync(lv, d_roots, next_n * 32, hipMemcpyDeviceToDevice, st);  // levels hold the roots too
            if (e != hipSuccess) return e;
            if (d_levels) lv += next_n * 32;
            cur = next;
            level_n = next_n;
            parity ^= 1;
        }
        return hipSuccess;
    };
    if (d_levels) return launched(ctx, "merkle_forest", build(nullptr));  // no context scratch
    // ping-pong in context-owned scratch, this stream's pair (the last level goes straight to d_roots)
    return with_stream_scratch(ctx, "merkle_forest", st, cur_n / arity * 32, cur_n / arity / arity * 32 + 32,
                               [&](p252_ctx::LevelSet& set) { return build(set.buf); });
}

P252_MERKLE_PAIR(int, forest_device,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_trees, size_t leaves_per_tree, void* d_roots, void* d_levels,
                  void* hip_stream),
                 forest_device(ctx, arity, tag, d_leaves, n_trees, leaves_per_tree, d_roots, d_levels, hip_stream))

// ---- messages of different lengths in one call (ragged.hip): the sort's order array and bucket counters live in the scratch
// pair of the calling stream (as the verify path's re-hashed roots), so calls on different streams of one context never share them
static int hash_ragged_device_impl(p252_ctx* ctx, const void* d_tags, size_t max_len, const void* d_in, const void* d_offsets,
                                   size_t out_len, void* d_out, size_t n, void* d_n_bad, void* hip_stream, bool trunc250) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "hash_ragged"};
    if (out_len == 0) return fail(ctx, P252_ERR_INVALID_IO_PATTERN, "hash_ragged: out_len must be > 0");
    if (out_len > 0x7fffffffu) return refuse("out_len too large");
    if (n == 0) return P252_OK;
    if (max_len == 0) return refuse("max_len must be > 0");
    if (!d_tags || !d_in || !d_offsets || !d_out) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_tags, d_in, d_out})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    if (n >= SIZE_MAX / 8 / (out_len > 8 ? out_len : 8)) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (!ragged_sort_enabled()) {  // P252_RAGGED_SORT=0: identity order, no scratch
        HIP_TRY(ctx, launch_hash_ragged(ctx->d_tab, d_tags, max_len, d_in, d_offsets, (unsigned)out_len, d_out, n, d_n_bad, nullptr,
                                        nullptr, st, trunc250));
        return P252_OK;
    }
    return with_stream_scratch(ctx, "hash_ragged", st, ragged_order_bytes(n), ragged_hist_bytes(), [&](p252_ctx::LevelSet& set) {
        return launch_hash_ragged(ctx->d_tab, d_tags, max_len, d_in, d_offsets, (unsigned)out_len, d_out, n, d_n_bad, set.buf[0], set.buf[1], st,
                                  trunc250);
    });
}

int p252_hash_ragged_device(p252_ctx* ctx, const void* d_tags, size_t max_len, const void* d_in, const void* d_offsets, size_t out_len,
                            void* d_out, size_t n, void* d_n_bad, void* hip_stream) {
    return hash_ragged_device_impl(ctx, d_tags, max_len, d_in, d_offsets, out_len, d_out, n, d_n_bad, hip_stream, false);
}

int p252_hash_ragged_truncated_device(p252_ctx* ctx, const void* d_tags, size_t max_len, const void* d_in, const void* d_offsets,
                                      size_t out_len, void* d_out_raw, size_t n, void* d_n_bad, void* hip_stream) {
    return hash_ragged_device_impl(ctx, d_tags, max_len, d_in, d_offsets, out_len, d_out_raw, n, d_n_bad, hip_stream, true);
}

// (the ragged-forest family — every entry point named _forest_ragged_, _path_ragged_, _forest_frontier_ or _forest_consistency_ —
// is in api_forest.cpp)

// (the host-buffer entry points — caller memory in, results back, synchronous — are in host_io.cpp)

// page-locked host memory for callers that want the host-buffer entry points at PCIe speed
void* p252_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void p252_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int p252_host_register(void* p, size_t bytes) {
    if (!p || bytes == 0) return P252_ERR_INVALID_ARGUMENT;
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return P252_ERR_HIP;
    }
    return P252_OK;
}

int p252_host_unregister(void* p) {
    if (!p) return P252_ERR_INVALID_ARGUMENT;
    if (hipHostUnregister(p) != hipSuccess) {
        (void)hipGetLastError();
        return P252_ERR_HIP;
    }
    return P252_OK;
}

// ------------------------------------------------------------------------------------------
// SURVEY §8(f) "next" rows: truncated outputs and batched Merkle openings
// ------------------------------------------------------------------------------------------
int p252_truncate250_device(p252_ctx* ctx, const void* d_scalars, void* d_out_raw, size_t n, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "truncate250"};
    if (n == 0) return P252_OK;
    if (!d_scalars || !d_out_raw) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_scalars, d_out_raw})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_truncate250(d_scalars, d_out_raw, n, (hipStream_t)hip_stream));
    return P252_OK;
}

// ---- incremental update of a stored arity-4 tree (the poseidon-merkle consumer changes leaves of a tree it
// keeps): the k leaves are written into d_leaves, then every level re-hashes the (at most k) nodes above them, in place in
// d_levels (layout of p252_merkle4_tree_device: the levels above the leaves, bottom-up); d_root (optional) gets the new root.
static int merkle4_update_device(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, void* d_levels,
                                 const void* d_indices, const void* d_new_leaves, size_t k, void* d_root, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle4_update"};
    if (n_leaves == 0 || n_leaves > 0xffffffffULL) return refuse("n_leaves must be in 1 .. 2^32 - 1");
    if (!tag || !d_leaves || (n_leaves > 1 && !d_levels)) return refuse("NULL buffer");
    if (k && (!d_indices || !d_new_leaves)) return refuse("NULL update list");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_new_leaves})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const TagArg t = tag_arg(tag);
    HIP_TRY(ctx, launch_scatter_scalars(d_indices, d_new_leaves, d_leaves, k, n_leaves, d_n_bad, st));
    const char* cur = static_cast<const char*>(d_leaves);
    size_t cur_n = n_leaves;
    char* lv = static_cast<char*>(d_levels);
    unsigned shift = 2;
    while (cur_n > 1) {
        const size_t next_n = (cur_n + 3) / 4;
        HIP_TRY(ctx, launch_merkle4_update(ctx->d_tab, t, d_indices, shift, cur, cur_n, lv, k, st));
        cur = lv;
        cur_n = next_n;
        lv += next_n * 32;
        shift += 2;
    }
    if (d_root) HIP_TRY(ctx, hipMemcpyAsync(d_root, cur, 32, hipMemcpyDeviceToDevice, st));
    return P252_OK;
}

int p252_merkle4_update_device(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, void* d_levels,
                               const void* d_indices, const void* d_new_leaves, size_t k, void* d_root, void* hip_stream) {
    return merkle4_update_device(ctx, tag, d_leaves, n_leaves, d_levels, d_indices, d_new_leaves, k, d_root, nullptr, hip_stream);
}

int p252_merkle4_update_checked_device(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, void* d_levels,
                                       const void* d_indices, const void* d_new_leaves, size_t k, void* d_root, void* d_n_bad,
                                       void* hip_stream) {
    const Refusal refuse{ctx, "merkle4_update_checked"};  // (before `!ctx`, as ever: without a context the message goes to p252_last_error(NULL))
    if (!d_n_bad) return refuse("d_n_bad is NULL");
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    return merkle4_update_device(ctx, tag, d_leaves, n_leaves, d_levels, d_indices, d_new_leaves, k, d_root, d_n_bad, hip_stream);
}

// ---- the canonical byte format of a scalar (BlsScalar::to_bytes / from_bytes; the reference round-trips its round
// constants through the pair, src/hades/round_constants.rs:66-67, and reads its KAT inputs with from_hex_str, src/hades.rs:131)
int p252_to_bytes_device(p252_ctx* ctx, const void* d_scalars, void* d_bytes, size_t n, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "to_bytes"};
    if (n == 0) return P252_OK;
    if (!d_scalars || !d_bytes) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_scalars, d_bytes})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_to_canonical(d_scalars, d_bytes, n, (hipStream_t)hip_stream));
    return P252_OK;
}

int p252_from_bytes_device(p252_ctx* ctx, const void* d_bytes, void* d_scalars, void* d_ok, size_t n, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "from_bytes"};
    if (n == 0) return P252_OK;
    if (!d_scalars || !d_bytes) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_scalars, d_bytes})) return rc;
    static const Digits9 r2 = [] {
        Digits9 d;
        encode_balanced29(FrHost::pow2(517), d.d);  // v * 2^517 / 2^261 = v * 2^256: the Montgomery form
        return d;
    }();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_from_canonical(d_bytes, d_scalars, d_ok, n, r2, (hipStream_t)hip_stream));
    return P252_OK;
}

// the argument checks of the fixed-depth re-hash (shared with the verify call)
static int path_batch_check(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves, const void* d_siblings,
                            const void* d_positions, size_t depth, const void* d_roots) {
    const Refusal refuse{ctx, arity == 4 ? "merkle4_path" : "merkle2_path"};
    if (!tag || !d_leaves || !d_roots || (depth && (!d_siblings || !d_positions))) return refuse("NULL buffer");
    if (depth > 0xffffu) return refuse("depth too large");
    if (int rc = refuse.unless_aligned({d_leaves, d_roots, depth ? d_siblings : nullptr})) return rc;
    return P252_OK;
}

static hipError_t launch_path(unsigned arity, const int32_t* tab, const TagArg& tag, const void* d_leaves, const void* d_siblings,
                              const void* d_positions, size_t depth, void* d_roots, size_t n, hipStream_t st) {
    return (arity == 4 ? launch_merkle4_path : launch_merkle2_path)(tab, tag, d_leaves, d_siblings, d_positions, (unsigned)depth, d_roots, n, st);
}

// both arities (arity 2: Domain::Merkle2 nodes, pass the Merkle2 tag; siblings[n][depth], positions 0..1)
static int path_batch_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves, const void* d_siblings,
                             const void* d_positions, size_t depth, void* d_roots, size_t n, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (n == 0) return P252_OK;
    if (int rc = path_batch_check(ctx, arity, tag, d_leaves, d_siblings, d_positions, depth, d_roots)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_path(arity, ctx->d_tab, tag_arg(tag), d_leaves, d_siblings, d_positions, depth, d_roots, n, (hipStream_t)hip_stream));
    return P252_OK;
}

P252_MERKLE_PAIR(int, path_batch_device,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, const void* d_siblings, const void* d_positions, size_t depth,
                  void* d_roots, size_t n, void* hip_stream),
                 path_batch_device(ctx, arity, tag, d_leaves, d_siblings, d_positions, depth, d_roots, n, hip_stream))

// Opening::verify in bulk: re-hash (either arity) into this stream's scratch, then one byte per opening
static int verify_batch_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const void* d_leaves, const void* d_siblings,
                               const void* d_positions, size_t depth, const void* d_root, void* d_ok, size_t n, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (n == 0) return P252_OK;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_verify" : "merkle2_verify"};
    if (!d_root || !d_ok) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_root})) return rc;
    if (n > (SIZE_MAX / 32)) return refuse("size overflow");
    // the re-hash's own refusals, before any scratch is taken (its output is the scratch: d_root, checked above, stands in for it)
    if (int rc = path_batch_check(ctx, arity, tag, d_leaves, d_siblings, d_positions, depth, d_root)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    // the recomputed roots live in the scratch pair of THIS stream (ctx.hpp): n x 32 bytes
    return with_stream_scratch(ctx, refuse.who, st, n * 32, 0, [&](p252_ctx::LevelSet& set) {
        const hipError_t e = launch_path(arity, ctx->d_tab, tag_arg(tag), d_leaves, d_siblings, d_positions, depth, set.buf[0], n, st);
        if (e != hipSuccess) return e;
        return launch_compare_roots(set.buf[0], d_root, d_ok, n, st);
    });
}

P252_MERKLE_PAIR(int, verify_batch_device,
                 (p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, const void* d_siblings, const void* d_positions, size_t depth,
                  const void* d_root, void* d_ok, size_t n, void* hip_stream),
                 verify_batch_device(ctx, arity, tag, d_leaves, d_siblings, d_positions, depth, d_root, d_ok, n, hip_stream))

// depth of the tree over n_leaves = number of levels above the leaves (an arity^k-leaf tree: k; a single leaf: 0).  The sum wraps
// at the top of size_t, which callers see (ABI): the depth of SIZE_MAX leaves is 1.
static size_t tree_depth(size_t n_leaves, size_t arity) {
    size_t d = 0;
    for (size_t c = n_leaves; c > 1; c = (c + arity - 1) / arity) ++d;
    return d;
}
P252_MERKLE_PAIR(size_t, depth, (size_t n_leaves), tree_depth(n_leaves, arity))

// Openings of a STORED tree, extracted on the device (openings.hip: pure data movement): for each of the k leaf positions the
// leaf, the three siblings per level and the position bytes, in exactly the layout p252_merkle4_path_batch_device takes — build
// (all levels) -> extract -> verify never leaves the GPU.
static int openings_device(p252_ctx* ctx, unsigned arity, const void* d_leaves, size_t n_leaves, const void* d_levels, const void* d_indices, size_t k,
                           void* d_leaves_out, void* d_siblings, void* d_positions, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    if (k == 0) return P252_OK;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_openings" : "merkle2_openings"};
    if (n_leaves == 0 || n_leaves > 0xffffffffu) return refuse("n_leaves must be in 1 .. 2^32 - 1 (positions are uint32)");
    const size_t depth = tree_depth(n_leaves, arity);
    if (!d_leaves || !d_indices || !d_leaves_out || (depth && (!d_levels || !d_siblings || !d_positions))) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_leaves_out, d_siblings})) return rc;
    if (misaligned_to(d_indices, 4) || misaligned_to(d_n_bad, 4)) return refuse("indices / counter must be 4-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    if (d_n_bad) HIP_TRY(ctx, hipMemsetAsync(d_n_bad, 0, 4, st));
    HIP_TRY(ctx, (arity == 4 ? launch_merkle4_openings : launch_merkle2_openings)(d_leaves, n_leaves, d_levels, d_indices, k, (unsigned)depth, d_leaves_out, d_siblings,
                                                                                       d_positions, d_n_bad, st));
    return P252_OK;
}

P252_MERKLE_PAIR(int, openings_device,
                 (p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_levels, const void* d_indices, size_t k, void* d_leaves_out,
                  void* d_siblings, void* d_positions, void* d_n_bad, void* hip_stream),
                 openings_device(ctx, arity, d_leaves, n_leaves, d_levels, d_indices, k, d_leaves_out, d_siblings, d_positions, d_n_bad, hip_stream))

// ---- many leaves of ONE stored tree behind one shared proof (multiproof.hip): a sibling that another leaf of the batch determines
// is not stored, and verification hashes every ancestor once.  The scratch — the counters, the scan tiles and two work lists in the
// first buffer; the verify's two lists of node values in the second — is the pair of the calling stream ----
P252_MERKLE_PAIR(size_t, multiproof_bound, (size_t n_leaves, size_t k), n_leaves && k ? multiproof_plan(arity, n_leaves, k).bound : 0)

static int multiproof_shape_check(const Refusal& refuse, size_t n_leaves, size_t k) {
    if (k == 0 || n_leaves == 0) return refuse("n_leaves and k must be > 0");
    if (n_leaves > 0xffffffffu || k > 0xffffffffu) return refuse("n_leaves and k must be below 2^32 (positions are uint32)");
    return P252_OK;
}

static int multiproof_device(p252_ctx* ctx, unsigned arity, const void* d_leaves, size_t n_leaves, const void* d_levels,
                             const void* d_indices, size_t k, void* d_leaves_out, void* d_proof, size_t proof_cap, void* d_proof_len,
                             void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_multiproof" : "merkle2_multiproof"};
    if (int rc = multiproof_shape_check(refuse, n_leaves, k)) return rc;
    const MultiproofPlan plan = multiproof_plan(arity, n_leaves, k);
    if (!d_leaves || !d_indices || !d_leaves_out || !d_proof_len || (plan.depth && !d_levels) || (proof_cap && !d_proof))
        return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves, d_levels, d_leaves_out, d_proof})) return rc;
    if (misaligned_to(d_indices, 4) || misaligned_to(d_n_bad, 4) || misaligned_to(d_proof_len, 8))
        return refuse("indices / d_n_bad must be 4-byte, d_proof_len 8-byte aligned");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_stream_scratch(ctx, refuse.who, st, plan.work_bytes(), 0, [&](p252_ctx::LevelSet& set) {
        return launch_multiproof(plan, d_leaves, d_levels, d_indices, d_leaves_out, d_proof, proof_cap, d_proof_len, d_n_bad, set.buf[0], st);
    });
}

static int multiproof_verify_device(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], size_t n_leaves, const void* d_indices,
                                    const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_len, const void* d_root,
                                    void* d_ok, void* d_root_out, void* d_n_hashed, void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, arity == 4 ? "merkle4_multiproof_verify" : "merkle2_multiproof_verify"};
    if (int rc = multiproof_shape_check(refuse, n_leaves, k)) return rc;
    if (!tag || !d_indices || !d_leaves_in || !d_root || !d_ok || (proof_len && !d_proof)) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_leaves_in, d_proof, d_root, d_root_out})) return rc;
    if (misaligned_to(d_indices, 4) || misaligned_to(d_n_bad, 4) || misaligned_to(d_n_hashed, 8))
        return refuse("indices / d_n_bad must be 4-byte, d_n_hashed 8-byte aligned");
    if (proof_len > SIZE_MAX / 32) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const MultiproofPlan plan = multiproof_plan(arity, n_leaves, k);
    return with_stream_scratch(ctx, refuse.who, st, plan.work_bytes(), plan.values_bytes(), [&](p252_ctx::LevelSet& set) {
        return launch_multiproof_verify(ctx->d_tab, tag_arg(tag), plan, d_indices, d_leaves_in, d_proof, proof_len, d_root, d_ok, d_root_out,
                                        d_n_hashed, d_n_bad, set.buf[0], set.buf[1], st);
    });
}

P252_MERKLE_PAIR(int, multiproof_device,
                 (p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_levels, const void* d_indices, size_t k, void* d_leaves_out,
                  void* d_proof, size_t proof_cap, void* d_proof_len, void* d_n_bad, void* hip_stream),
                 multiproof_device(ctx, arity, d_leaves, n_leaves, d_levels, d_indices, k, d_leaves_out, d_proof, proof_cap, d_proof_len, d_n_bad,
                                   hip_stream))

P252_MERKLE_PAIR(int, multiproof_verify_device,
                 (p252_ctx* ctx, const uint64_t tag[4], size_t n_leaves, const void* d_indices, const void* d_leaves_in, size_t k,
                  const void* d_proof, size_t proof_len, const void* d_root, void* d_ok, void* d_root_out, void* d_n_hashed, void* d_n_bad,
                  void* hip_stream),
                 multiproof_verify_device(ctx, arity, tag, n_leaves, d_indices, d_leaves_in, k, d_proof, proof_len, d_root, d_ok, d_root_out,
                                          d_n_hashed, d_n_bad, hip_stream))

// ---- encryption row (src/encryption.rs:62-95 -> dusk_safe::encrypt / decrypt) ----
static int crypt_device(p252_ctx* ctx, int variant, bool decrypt, const uint64_t tag[4], const void* d_in, const void* d_secrets,
                        const void* d_nonces, size_t len, void* d_out, void* d_ok, size_t n, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "encrypt/decrypt"};
    if (!crypt_variant_ok(variant)) return refuse("unknown variant");
    if (len == 0) return fail(ctx, P252_ERR_INVALID_IO_PATTERN, "encrypt/decrypt: empty message");
    if (len >= 0x1ffffff0u) return refuse("message too long");
    if (n == 0) return P252_OK;
    if (!tag || !d_in || !d_secrets || !d_nonces || !d_out || (decrypt && !d_ok)) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_in, d_secrets, d_nonces, d_out})) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = prepare_prog(ctx, variant, len);
    if (rc) return rc;
    HIP_TRY(ctx, launch_crypt(decrypt, ctx->d_tab, tag_arg(tag), d_in, d_secrets, d_nonces, (unsigned)len, d_out, d_ok, n, ctx->d_prog,
                              ctx->prog_calls, st));
    return P252_OK;
}

int p252_encrypt_batch_device(p252_ctx* ctx, int variant, const uint64_t tag[4], const void* d_messages, const void* d_secrets,
                              const void* d_nonces, size_t len, void* d_ciphers, size_t n, void* hip_stream) {
    return crypt_device(ctx, variant, false, tag, d_messages, d_secrets, d_nonces, len, d_ciphers, nullptr, n, hip_stream);
}

int p252_decrypt_batch_device(p252_ctx* ctx, int variant, const uint64_t tag[4], const void* d_ciphers, const void* d_secrets,
                              const void* d_nonces, size_t len, void* d_messages, void* d_ok, size_t n, void* hip_stream) {
    return crypt_device(ctx, variant, true, tag, d_ciphers, d_secrets, d_nonces, len, d_messages, d_ok, n, hip_stream);
}

// ---- messages of different lengths in one call (crypt_ragged.hip: the schedule; kernels.hip: k_crypt<*, true>).  The order array
// and the bucket counters live in the scratch pair of the calling stream.  No call table, hence no prepare_prog and none of its
// synchronisation: the kernels compute the calls from (variant, length).  in / out: the message and the cipher side. ----
static int crypt_ragged_device(p252_ctx* ctx, int variant, bool decrypt, const void* d_tags, size_t max_len, const void* d_in, size_t n_scalars,
                               const void* d_offsets, const void* d_secrets, const void* d_nonces, void* d_out, void* d_ok, size_t n,
                               void* d_n_bad, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, decrypt ? "decrypt_ragged" : "encrypt_ragged"};
    if (!crypt_variant_ok(variant)) return refuse("unknown variant");
    if (max_len == 0 || max_len > P252_CRYPT_RAGGED_MAX_LEN)
        return refuse("max_len must be 1 .. P252_CRYPT_RAGGED_MAX_LEN = " + std::to_string(P252_CRYPT_RAGGED_MAX_LEN));
    if (n == 0) return P252_OK;
    if (!d_tags || !d_in || !d_offsets || !d_secrets || !d_nonces || !d_out || (decrypt && !d_ok)) return refuse("NULL buffer");
    if (int rc = refuse.unless_aligned({d_tags, d_in, d_secrets, d_nonces, d_out})) return rc;
    if (int rc = refuse.unless_aligned(8, {P252_NAMED(d_offsets)})) return rc;
    if (int rc = refuse.unless_aligned(4, {P252_NAMED(d_n_bad)})) return rc;
    if (n >= SIZE_MAX / 128 || n_scalars >= SIZE_MAX / 64 || n_scalars + n >= SIZE_MAX / 64) return refuse("size overflow");
    const size_t msg_bytes = n_scalars * 32, cph_bytes = (n_scalars + n) * 32;
    const ByteRange in[] = {{d_tags, max_len * 32, "d_tags"},
                            {d_in, decrypt ? cph_bytes : msg_bytes, decrypt ? "d_ciphers" : "d_messages"},
                            {d_offsets, (n + 1) * 8, "d_offsets"},
                            {d_secrets, n * 64, "d_secrets"},
                            {d_nonces, n * 32, "d_nonces"}};
    const ByteRange out[] = {{d_out, decrypt ? msg_bytes : cph_bytes, decrypt ? "d_messages" : "d_ciphers"}, {d_ok, decrypt ? n : 0, "d_ok"}, {d_n_bad, 4, "d_n_bad"}};
    if (int rc = refuse_overlaps(refuse, in, std::size(in), out, std::size(out), true)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)hip_stream;
    return with_stream_scratch(ctx, refuse.who, st, crypt_ragged_order_bytes(n, max_len), crypt_ragged_hist_bytes(), [&](p252_ctx::LevelSet& set) {
        return launch_crypt_ragged(decrypt, variant, ctx->d_tab, d_tags, max_len, d_in, (uint64_t)n_scalars, d_offsets, d_secrets, d_nonces, d_out, d_ok, n,
                                   d_n_bad, set.buf[0], set.buf[1], st);
    });
}

int p252_encrypt_ragged_device_into(p252_ctx* ctx, int variant, const void* d_tags, size_t max_len, const void* d_messages, size_t n_scalars,
                               const void* d_offsets, const void* d_secrets, const void* d_nonces, void* d_ciphers, size_t n, void* d_n_bad,
                               void* hip_stream) {
    return crypt_ragged_device(ctx, variant, false, d_tags, max_len, d_messages, n_scalars, d_offsets, d_secrets, d_nonces, d_ciphers, nullptr, n,
                               d_n_bad, hip_stream);
}

int p252_decrypt_ragged_device_into(p252_ctx* ctx, int variant, const void* d_tags, size_t max_len, const void* d_ciphers, size_t n_scalars,
                               const void* d_offsets, const void* d_secrets, const void* d_nonces, void* d_messages, void* d_ok, size_t n,
                               void* d_n_bad, void* hip_stream) {
    return crypt_ragged_device(ctx, variant, true, d_tags, max_len, d_ciphers, n_scalars, d_offsets, d_secrets, d_nonces, d_messages, d_ok, n, d_n_bad,
                               hip_stream);
}

// shared by p252_tag and p252_encryption_tag: tag = hash_to_scalar(io-words (BE u32) || domain separator (BE u64)),
// hash_to_scalar = BLAKE2b-512 read as a 512-bit little-endian integer mod p.  UNPINNED recipe (header).
static void tag_from_words(const std::vector<uint32_t>& words, uint64_t sep, uint64_t tag_out[4]) {
    std::vector<uint8_t> buf;
    for (uint32_t w : words)
        for (int b = 0; b < 4; ++b) buf.push_back((uint8_t)(w >> (24 - 8 * b)));
    for (int b = 0; b < 8; ++b) buf.push_back((uint8_t)(sep >> (56 - 8 * b)));
    uint8_t h[64];
    blake2b_512(buf.data(), buf.size(), h);
    uint64_t lo[4], hi[4];
    for (int k = 0; k < 4; ++k) {
        lo[k] = u64_from_buffer(h, 8 * k);
        hi[k] = u64_from_buffer(h, 32 + 8 * k);
    }
    FrHost r = FrHost::from_raw(lo) + FrHost::from_raw(hi) * FrHost::pow2(256);
    std::memcpy(tag_out, r.l, 32);
}

// UNPINNED: tag of the encryption io-pattern of `variant` (adjacent calls of one kind aggregated, as dusk-safe does)
int p252_encryption_tag(int variant, size_t message_len, uint64_t tag_out[4]) {
    if (!tag_out || !crypt_variant_ok(variant)) return P252_ERR_INVALID_ARGUMENT;
    if (message_len == 0) return P252_ERR_INVALID_IO_PATTERN;
    if (message_len >= 0x1ffffff0ULL) return P252_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> words;
    int prev_absorb = -1;
    for (uint32_t c : crypt_program(variant, message_len)) {
        const uint32_t kind = c >> 29, n = c & 0x1fffffffu;
        const int is_absorb = kind == 0 || kind == 1 || kind == 3;
        if (!words.empty() && is_absorb == prev_absorb)
            words.back() += n;
        else
            words.push_back((is_absorb ? 0x80000000u : 0u) | n);
        prev_absorb = is_absorb;
    }
    uint64_t sep = 0;
    p252_domain_separator(P252_DOMAIN_ENCRYPTION, &sep);
    tag_from_words(words, sep, tag_out);
    return P252_OK;
}

// the tag table of the ragged calls: row L - 1 = p252_encryption_tag(variant, L), L = 1 .. max_len
int p252_encryption_tags(int variant, size_t max_len, uint64_t* tags_out) {
    if (!tags_out || !crypt_variant_ok(variant) || max_len == 0 || max_len > P252_CRYPT_RAGGED_MAX_LEN) return P252_ERR_INVALID_ARGUMENT;
    for (size_t len = 1; len <= max_len; ++len)
        if (int rc = p252_encryption_tag(variant, len, tags_out + 4 * (len - 1))) return rc;
    return P252_OK;
}

// ------------------------------------------------------------------------------------------
// multi-device entry points (SURVEY §8(b) sketch, §8(e)): an array of contexts, one per GPU.  Shards are contiguous and
// independent — no inter-GPU dependence, no collective on the data path; the only exchange of the sharded tree is the
// 32-byte subtree root of every device, gathered by the host.  One host thread per context for the duration of the call.
// ------------------------------------------------------------------------------------------
// for the duration of one multi call every context works within its share of the CPU budget
struct LaneBudgetScope {
    p252_ctx* const* ctxs;
    size_t n;
    LaneBudgetScope(p252_ctx* const* c, size_t n_ctx) : ctxs(c), n(n_ctx) {
        const int per = staging_lanes_per_ctx(n_ctx);
        for (size_t t = 0; t < n; ++t) ctxs[t]->lane_budget = per;
    }
    ~LaneBudgetScope() {
        for (size_t t = 0; t < n; ++t) ctxs[t]->lane_budget = 0;
    }
};

int p252_hash_batch_multi(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const uint64_t* in, size_t in_len,
                          size_t out_len, uint64_t* out, size_t n) {
    int rc = check_ctxs(ctxs, n_ctx);
    if (rc) return rc;
    if (in_len == 0 || out_len == 0) return fail(ctxs[0], P252_ERR_INVALID_IO_PATTERN, "hash: in_len and out_len must be > 0");
    if (n == 0) return P252_OK;
    if (!tag || !in || !out) return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT, "hash: NULL buffer");
    // contiguous shards, sizes differing by at most one item
    const size_t base = n / n_ctx, rem = n % n_ctx;
    LaneBudgetScope budget(ctxs, n_ctx);
    return for_each_ctx(ctxs, n_ctx, [&](size_t t) {
        const size_t lo = t * base + (t < rem ? t : rem), cnt = base + (t < rem ? 1 : 0);
        return p252_hash_batch(ctxs[t], tag, in + lo * in_len * 4, in_len, out_len, out + lo * out_len * 4, cnt);
    });
}

int p252_hash_batch_multi_device(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const void* const* d_in, size_t in_len,
                                 size_t out_len, void* const* d_out, const size_t* n_per_ctx, void* const* hip_streams) {
    int rc = check_ctxs(ctxs, n_ctx);
    if (rc) return rc;
    if (!d_in || !d_out || !n_per_ctx) return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT, "hash_multi_device: NULL array");
    for (size_t t = 0; t < n_ctx; ++t) {  // launches are asynchronous: a plain loop, no threads needed
        rc = p252_hash_batch_device(ctxs[t], tag, d_in[t], in_len, out_len, d_out[t], n_per_ctx[t], hip_streams ? hip_streams[t] : nullptr);
        if (rc) {
            if (t) ctxs[0]->err = "context " + std::to_string(t) + ": " + ctxs[t]->err;
            return rc;
        }
    }
    return P252_OK;
}

static int tree_top(p252_ctx* ctx0, const uint64_t tag[4], const std::vector<uint64_t>& roots, size_t n_ctx, uint64_t root[4]) {
    if (n_ctx == 1) {
        std::memcpy(root, roots.data(), 32);
        return P252_OK;
    }
    return p252_merkle4_tree(ctx0, tag, roots.data(), n_ctx, root, nullptr);  // <= log4(n_ctx) + 1 tiny levels, zero-padded
}

int p252_merkle4_tree_multi(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const uint64_t* leaves, size_t n_leaves,
                            uint64_t root[4]) {
    int rc = check_ctxs(ctxs, n_ctx);
    if (rc) return rc;
    if (!tag || !leaves || !root) return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT, "merkle_tree_multi: NULL buffer");
    if (n_leaves == 0 || n_leaves % n_ctx || !power_of_4(n_leaves / n_ctx))
        return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT,
                    "merkle_tree_multi: every device must own a complete subtree (n_leaves = n_ctx * 4^k)");
    const size_t m = n_leaves / n_ctx;
    std::vector<uint64_t> roots(4 * n_ctx);
    LaneBudgetScope budget(ctxs, n_ctx);
    rc = for_each_ctx(ctxs, n_ctx, [&](size_t t) { return p252_merkle4_tree(ctxs[t], tag, leaves + t * m * 4, m, &roots[4 * t], nullptr); });
    if (rc) return rc;
    return tree_top(ctxs[0], tag, roots, n_ctx, root);
}

int p252_merkle4_tree_multi_device(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const void* const* d_leaves,
                                   size_t leaves_per_ctx, uint64_t root[4]) {
    int rc = check_ctxs(ctxs, n_ctx);
    if (rc) return rc;
    if (!tag || !d_leaves || !root) return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT, "merkle_tree_multi_device: NULL buffer");
    if (!power_of_4(leaves_per_ctx))
        return fail(ctxs[0], P252_ERR_INVALID_ARGUMENT, "merkle_tree_multi_device: every device must own a complete subtree (4^k leaves)");
    // RCCL path (contexts on distinct devices; the communicator is created on first use and kept): subtrees, ONE grouped
    // ncclAllGather of the 32-byte roots on the devices' streams, top levels on every device — the root is device-resident
    // everywhere and only its 32 bytes come back to the host, from ctxs[0]
    bool used_rccl = false;
    std::vector<void*> d_top(n_ctx, nullptr);
    for (size_t t = 0; t < n_ctx && rc == P252_OK; ++t) {
        p252_ctx* c = ctxs[t];
        if (hipSetDevice(c->device) != hipSuccess) { rc = fail(c, P252_ERR_HIP, "hipSetDevice"); break; }
        rc = ensure(c, &c->d_out, &c->d_out_cap, 32);
        d_top[t] = c->d_out;
    }
    if (rc == P252_OK) rc = tree_multi_device_rccl(ctxs, n_ctx, tag, d_leaves, leaves_per_ctx, d_top.data(), nullptr, &used_rccl);
    if (rc) {
        if (ctxs[0]->err.empty()) ctxs[0]->err = "merkle_tree_multi_device failed on another context";
        return rc;
    }
    if (used_rccl) {
        for (size_t t = 1; t < n_ctx; ++t) {  // the call is synchronous: every device has its copy of the root when it returns
            HIP_TRY(ctxs[t], hipSetDevice(ctxs[t]->device));
            HIP_TRY(ctxs[t], hipStreamSynchronize(nullptr));
        }
        HIP_TRY(ctxs[0], hipSetDevice(ctxs[0]->device));
        HIP_TRY(ctxs[0], hipMemcpy(root, d_top[0], 32, hipMemcpyDeviceToHost));
        return P252_OK;
    }
    // HOST-GATHER path — only when the contexts share a device (RCCL wants one device per rank: the single-GPU test
    // configuration) or P252_MULTI_HOST_GATHER=1: every device reduces its resident subtree (asynchronous launches on its
    // own default stream) ...
    std::vector<void*> d_roots(n_ctx, nullptr);
    for (size_t t = 0; t < n_ctx && rc == P252_OK; ++t) {
        p252_ctx* c = ctxs[t];
        if (hipSetDevice(c->device) != hipSuccess) { rc = fail(c, P252_ERR_HIP, "hipSetDevice"); break; }
        rc = ensure(c, &c->d_out, &c->d_out_cap, 32);
        if (rc == P252_OK) rc = merkle_tree_device(c, 4, tag, d_leaves[t], leaves_per_ctx, c->d_out, nullptr, nullptr);
        d_roots[t] = c->d_out;
    }
    // ... then the only exchange step of the path: 32 bytes per device to the host
    std::vector<uint64_t> roots(4 * n_ctx);
    for (size_t t = 0; t < n_ctx && rc == P252_OK; ++t) {
        p252_ctx* c = ctxs[t];
        if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(&roots[4 * t], d_roots[t], 32, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(c, P252_ERR_HIP, "merkle_tree_multi_device: root copy failed");
    }
    if (rc) {
        if (ctxs[0]->err.empty()) ctxs[0]->err = "merkle_tree_multi_device failed on another context";
        return rc;
    }
    return tree_top(ctxs[0], tag, roots, n_ctx, root);
}

// ------------------------------------------------------------------------------------------
// measurement aids
// ------------------------------------------------------------------------------------------
int p252_clock_probe_device(p252_ctx* ctx, void* d_out6, unsigned spin_us, void* hip_stream) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "clock_probe"};
    if (!d_out6 || misaligned_to(d_out6, 8)) return refuse("d_out6 must be an 8-byte aligned device buffer of 6 x uint64");
    if (spin_us > 1000000u) return refuse("spin_us > 1 s");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch_clock_probe(d_out6, spin_us * 100u, (hipStream_t)hip_stream));  // real-time counter: 100 MHz
    return P252_OK;
}

int p252_staging_lanes(size_t n_ctx) { return staging_lanes_per_ctx(n_ctx ? n_ctx : 1); }

// ------------------------------------------------------------------------------------------
// constant-table exchange
// ------------------------------------------------------------------------------------------
size_t p252_tables_size(void) { return (size_t)Tab29Layout::TOTAL * sizeof(int32_t); }

int p252_tables_export(p252_ctx* ctx, void* host_buf, size_t len) {
    if (!ctx || !host_buf || len != p252_tables_size()) return Refusal{ctx, "tables_export"}("bad args");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(host_buf, ctx->d_tab, len, hipMemcpyDeviceToHost));
    return P252_OK;
}

int p252_tables_import(p252_ctx* ctx, const void* host_buf, size_t len) {
    const Refusal refuse{ctx, "tables_import"};
    if (!ctx || !host_buf || len != p252_tables_size()) return refuse("bad args");
    // The table is a pure function of arc.bin / mds.bin, which are compiled in: anything else than what this library
    // derives itself (with its Cauchy-structure and column-bound checks) is a corrupted or mismatched broadcast and
    // would give silently wrong digests — refuse it.
    if (std::memcmp(host_buf, host_tables().data(), len) != 0)
        return refuse("the table differs from the one this library derives from its arc.bin / mds.bin");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(ctx->d_tab, host_buf, len, hipMemcpyHostToDevice));
    std::memcpy(ctx->h_tab.data(), host_buf, len);
    return P252_OK;
}

// ------------------------------------------------------------------------------------------
// host helpers mirroring src/hash.rs
// ------------------------------------------------------------------------------------------
int p252_domain_separator(int domain, uint64_t* sep_out) {  // hash.rs:38-56
    if (!sep_out) return P252_ERR_INVALID_ARGUMENT;
    switch (domain) {
        case P252_DOMAIN_MERKLE4: *sep_out = 0x000000000000000fULL; return P252_OK;
        case P252_DOMAIN_MERKLE2: *sep_out = 0x0000000000000003ULL; return P252_OK;
        case P252_DOMAIN_ENCRYPTION: *sep_out = 0x0000000100000000ULL; return P252_OK;
        case P252_DOMAIN_OTHER: *sep_out = 0; return P252_OK;
        default: return P252_ERR_INVALID_ARGUMENT;
    }
}

int p252_check_io_pattern(int domain, const size_t* absorb_lens, size_t n_absorbs, size_t out_len) {
    if (domain < 0 || domain > 3) return P252_ERR_INVALID_ARGUMENT;
    if (n_absorbs && !absorb_lens) return P252_ERR_INVALID_ARGUMENT;
    size_t total = 0;
    for (size_t i = 0; i < n_absorbs; ++i) total += absorb_lens[i];
    // hash.rs:70-78
    if (domain == P252_DOMAIN_MERKLE2 && (total != 2 || out_len != 1)) return P252_ERR_IO_PATTERN_VIOLATION;
    if (domain == P252_DOMAIN_MERKLE4 && (total != 4 || out_len != 1)) return P252_ERR_IO_PATTERN_VIOLATION;
    // dusk-safe: a pattern must start with an absorb, end with a squeeze, and hold no zero-length call
    if (n_absorbs == 0 || out_len == 0) return P252_ERR_INVALID_IO_PATTERN;
    for (size_t i = 0; i < n_absorbs; ++i)
        if (absorb_lens[i] == 0) return P252_ERR_INVALID_IO_PATTERN;
    return P252_OK;
}

int p252_tag(int domain, const size_t* absorb_lens, size_t n_absorbs, size_t out_len, uint64_t tag_out[4]) {
    if (!tag_out) return P252_ERR_INVALID_ARGUMENT;
    int rc = p252_check_io_pattern(domain, absorb_lens, n_absorbs, out_len);
    if (rc) return rc;
    uint64_t absorbed = 0;
    for (size_t i = 0; i < n_absorbs; ++i) absorbed += absorb_lens[i];
    if (absorbed >= 0x80000000ULL || out_len >= 0x80000000ULL) return P252_ERR_INVALID_ARGUMENT;
    // tag input: aggregated io-pattern words (big-endian u32, absorb flagged by the top bit), then
    // the domain separator as a big-endian u64
    uint64_t sep = 0;
    p252_domain_separator(domain, &sep);
    tag_from_words({0x80000000u | (uint32_t)absorbed, (uint32_t)out_len}, sep, tag_out);
    return P252_OK;
}

int p252_truncate250(const uint64_t* scalars, uint64_t* out_raw, size_t n) {  // hash.rs:164-183
    if (n && (!scalars || !out_raw)) return P252_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; ++i) {
        FrHost::from_limbs(scalars + 4 * i).to_canonical(out_raw + 4 * i);
        out_raw[4 * i + 3] &= 0x03ffffffffffffffULL;
    }
    return P252_OK;
}

// host-side twins of the two conversions (one Montgomery multiplication per scalar: not worth a transfer)
int p252_to_bytes(const uint64_t* scalars, uint8_t* bytes, size_t n) {
    if (n && (!scalars || !bytes)) return P252_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; ++i) {
        uint64_t c[4];
        FrHost::from_limbs(scalars + 4 * i).to_canonical(c);
        for (int k = 0; k < 32; ++k) bytes[32 * i + k] = (uint8_t)(c[k / 8] >> (8 * (k % 8)));
    }
    return P252_OK;
}

int p252_from_bytes(const uint8_t* bytes, uint64_t* scalars, uint8_t* ok, size_t n) {
    if (n && (!bytes || !scalars)) return P252_ERR_INVALID_ARGUMENT;
    for (size_t i = 0; i < n; ++i) {
        uint64_t v[4] = {0, 0, 0, 0};
        for (int k = 0; k < 32; ++k) v[k / 8] |= (uint64_t)bytes[32 * i + k] << (8 * (k % 8));
        if (ok) ok[i] = FrHost::geq_p(v) ? 0 : 1;
        while (FrHost::geq_p(v)) FrHost::sub_p(v);  // (a 256-bit value is below 3p)
        std::memcpy(scalars + 4 * i, FrHost::from_raw(v).l, 32);
    }
    return P252_OK;
}

}  // (the C ABI)
