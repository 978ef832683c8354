// api_util.hpp — what the files of the C ABI share (api.cpp; api_forest.cpp, the ragged-forest family; host_io.cpp, the host-buffer entry
// points): one definition for a merkle4 / merkle2 pair of entry points, the one spelling of a refused argument, the alignment rules of
// device buffers, what a call's launches came to, and the one way to the scratch pair of the calling stream.
// Internal: nothing here is part of the ABI.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <string>

#include "ctx.hpp"

namespace p252host {

// device-resident scalar arrays are read and written with 16-byte accesses (a BlsScalar array from hipMalloc, or any
// 32-byte-multiple offset into one, qualifies); anything else would fault on the GPU, so it is refused here
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
// the id, offset and counter arrays beside them: `bytes` = the size of one element (a power of two); null is aligned
inline bool misaligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }
inline const char* const ALIGN_MSG = "device scalar arrays must be 16-byte aligned";

// One definition for the p252_merkle4_<stem> / p252_merkle2_<stem> pair of the C ABI: `params` is the parenthesised parameter list of
// both, `call` the one expression both return, with `arity` (4 or 2) in scope.  The header keeps both prototypes written out, so a
// parameter list that disagrees with it does not compile (conflicting types under C linkage).
#define P252_MERKLE_PAIR(ret, stem, params, call)                                 \
    ret p252_merkle4_##stem params { constexpr unsigned arity = 4; return call; } \
    ret p252_merkle2_##stem params { constexpr unsigned arity = 2; return call; }

// The one spelling of "this call refuses its arguments": P252_ERR_INVALID_ARGUMENT with "<who>: <what>" as the context's message.
// A value (ctx and a literal): making one costs nothing, and no std::string exists until a check has failed.
struct Refusal {
    p252_ctx* ctx;
    const char* who;
    struct Named {
        const char* name;
        const void* p;
    };
    int operator()(const char* what) const { return fail(ctx, P252_ERR_INVALID_ARGUMENT, text().append(what)); }
    int operator()(const std::string& what) const { return (*this)(what.c_str()); }
    // the 16-byte rule of the scalar arrays (its text names neither the call nor an array), P252_OK when every one is aligned ...
    int unless_aligned(std::initializer_list<const void*> scalars) const {
        for (const void* p : scalars)
            if (misaligned(p)) return fail(ctx, P252_ERR_INVALID_ARGUMENT, ALIGN_MSG);
        return P252_OK;
    }
    // ... and the `bytes`-byte rule of the arrays beside them: the text lists every name given, "a, b and c must be 8-byte aligned"
    int unless_aligned(size_t bytes, std::initializer_list<Named> arrays) const {
        bool ok = true;
        for (const Named& a : arrays) ok = ok && !misaligned_to(a.p, bytes);
        if (ok) return P252_OK;
        std::string msg = text();
        size_t i = 0;
        for (const Named& a : arrays) {
            if (i++) msg += i < arrays.size() ? ", " : " and ";
            msg += a.name;
        }
        return fail(ctx, P252_ERR_INVALID_ARGUMENT, msg.append(" must be ").append(std::to_string(bytes)).append("-byte aligned"));
    }
    // what every call on a built forest asks of its three sizes
    int unless_built_forest(size_t n_leaves, size_t n_trees, size_t max_leaves) const {
        return n_leaves && n_trees && max_leaves ? P252_OK : (*this)("n_leaves, n_trees and max_leaves must be > 0");
    }

private:
    // "<who>: ", with room for the longest message behind it: one allocation a refusal
    std::string text() const {
        std::string t;
        t.reserve(192);
        t.append(who).append(": ");
        return t;
    }
};
// {"d_x", d_x}: an array under the name the message gives it, where that is the argument's own
#define P252_NAMED(ptr) {#ptr, ptr}

// the buffers of a call as byte ranges, for the calls that refuse overlapping ones (a null or empty range overlaps nothing)
struct ByteRange {
    const void* p;
    size_t bytes;
    const char* name;
};
inline bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
// each written range, in listed order, against the read ranges in listed order and then — `among` — against the written ranges before
// it; the first hit is the refusal
inline int refuse_overlaps(const Refusal& refuse, const ByteRange* read, size_t n_read, const ByteRange* written, size_t n_written,
                           bool among) {
    for (size_t a = 0; a < n_written; ++a)
        for (size_t i = 0; i < n_read + (among ? a : 0); ++i) {
            const ByteRange& other = i < n_read ? read[i] : written[i - n_read];
            if (ranges_overlap(written[a], other)) return refuse(std::string(written[a].name) + " overlaps " + other.name);
        }
    return P252_OK;
}

// what a call's launches on the device came to, as the entry point's return value
inline int launched(p252_ctx* ctx, const char* who, hipError_t e) {
    return e == hipSuccess ? P252_OK : fail(ctx, P252_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

// the scratch pair of a call on `st` (at least need0 / need1 bytes) and the record of its event behind the call's last launch
// (api.cpp): with_stream_scratch, below, is their only caller
int level_set(p252_ctx* ctx, hipStream_t st, size_t need0, size_t need1, p252_ctx::LevelSet** out);
int level_set_done(p252_ctx* ctx, p252_ctx::LevelSet* set);

// The ONE way to the scratch pair of the calling stream (ctx.hpp): body(set) enqueues the call's launches on `st` and returns their
// hipError_t.  Once the pair is acquired its event is recorded on EVERY way out — also when a launch failed half way: the launches
// before it are queued and touch the pair, and a later takeover by another stream waits on this event (early
// returns used to skip it and left the event of an OLDER build for the next takeover).  A failure of the body keeps its code and
// message over the record's; on success the record's own status is returned.
template <class Body>
int with_stream_scratch(p252_ctx* ctx, const char* who, hipStream_t st, size_t need0, size_t need1, Body&& body) {
    p252_ctx::LevelSet* set = nullptr;
    if (int rc = level_set(ctx, st, need0, need1, &set)) return rc;
    const int rc = launched(ctx, who, body(*set));
    const std::string msg = ctx->err;
    const int rc_done = level_set_done(ctx, set);
    if (rc) ctx->err = msg;
    return rc ? rc : rc_done;
}

}  // namespace p252host
