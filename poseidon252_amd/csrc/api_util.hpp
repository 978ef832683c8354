// api_util.hpp — what the two files of the C ABI's device entry points share (api.cpp; api_forest.cpp, the ragged-forest family):
// the alignment rules of device buffers, what a call's launches came to, and the one way to the scratch pair of the calling stream.
// Internal: nothing here is part of the ABI.
#pragma once
#include <cstdint>
#include <string>

#include "ctx.hpp"

namespace p252host {

// device-resident scalar arrays are read and written with 16-byte accesses (a BlsScalar array from hipMalloc, or any
// 32-byte-multiple offset into one, qualifies); anything else would fault on the GPU, so it is refused here
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }
// the id, offset and counter arrays beside them: `bytes` = the size of one element (a power of two); null is aligned
inline bool misaligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }
inline const char* const ALIGN_MSG = "device scalar arrays must be 16-byte aligned";

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
inline int refuse_overlaps(p252_ctx* ctx, const std::string& who, const ByteRange* read, size_t n_read, const ByteRange* written,
                           size_t n_written, bool among) {
    for (size_t a = 0; a < n_written; ++a)
        for (size_t i = 0; i < n_read + (among ? a : 0); ++i) {
            const ByteRange& other = i < n_read ? read[i] : written[i - n_read];
            if (ranges_overlap(written[a], other)) return fail(ctx, P252_ERR_INVALID_ARGUMENT, who + ": " + written[a].name + " overlaps " + other.name);
        }
    return P252_OK;
}

// what a call's launches on the device came to, as the entry point's return value
inline int launched(p252_ctx* ctx, const std::string& who, hipError_t e) {
    return e == hipSuccess ? P252_OK : fail(ctx, P252_ERR_HIP, who + ": " + hipGetErrorString(e));
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
int with_stream_scratch(p252_ctx* ctx, const std::string& who, hipStream_t st, size_t need0, size_t need1, Body&& body) {
    p252_ctx::LevelSet* set = nullptr;
    if (int rc = level_set(ctx, st, need0, need1, &set)) return rc;
    const int rc = launched(ctx, who, body(*set));
    const std::string msg = ctx->err;
    const int rc_done = level_set_done(ctx, set);
    if (rc) ctx->err = msg;
    return rc ? rc : rc_done;
}

}  // namespace p252host
