// host_io.cpp — the host-buffer entry points of the C ABI: synchronous calls that take caller memory, copy it to the GPU, launch
// and copy the results back.  Each one validates its arguments, describes its arrays as spans and hands them to host_batch(),
// the one transfer path, with a launch that calls the kernels directly.  host_batch moves the spans one of three ways:
//   ONE_SHOT    every array in one copy each way through the context's grow-only scratch (ctx->d_in / ctx->d_out)
//   STAGED      chunks through the library's page-locked staging lanes (pageable caller memory, see staged_run)
//   PINNED_DMA  chunks DMA'd straight from / to caller memory that is page-locked on both sides, over three streams
// Each entry point picks its route in one expression at its call site; P252_HOST_PIPELINE=0 makes every one of them ONE_SHOT.
#include <hip/hip_runtime.h>

#include <sched.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/poseidon252_hip.h"
#include "api_util.hpp"
#include "ctx.hpp"
#include "kernels.h"

using namespace p252;
using namespace p252host;

static bool is_pinned(const void* p) {
    hipPointerAttribute_t a;
    const bool is = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    return is;
}

// Pageable caller memory (a Rust Vec<BlsScalar>, a numpy array): page-locking it per call costs as much as the transfer
// (round 1: 1.9e8 digests/s against 4.0e8 from pinned memory).  So a large host-buffer call is split into chunks of items
// handled by a few LANES: a worker thread with its own stream and TWO slots (page-locked staging pair + device pair +
// event).  Per chunk: memcpy in -> H2D -> kernel -> D2H (all asynchronous on the lane's stream) and, one chunk later,
// memcpy out — the host copies of chunk c+1 overlap the DMA and kernel of chunk c, the lanes overlap each other, and
// nothing the caller owns is ever registered.  Events are blocking-sync: a waiting worker sleeps instead of spinning (the
// benchmark box grants 16 CPUs; spinning workers get the whole process throttled).  The host copies themselves are not
// the limit (EPYC 9575F: memcpy 30 GB/s per thread, bench_tools/ntcopy.cpp; non-temporal stores changed nothing end to
// end) — in-flight depth is: round 2's first version (one slot per lane, spinning waits, 8-12 lanes) reached 2.0-3.1e8.
struct HostSpan {  // one per-item array of a batched call: item i occupies bytes [i * stride, (i + 1) * stride)
    const char* src;  // input arrays: caller memory to read
    char* dst;        // output arrays: caller memory to write
    size_t stride;
};

// launch(d_in[], d_out[], first_item, count, stream): the kernels of items [first_item, first_item + count) on `stream`; d_in[a] /
// d_out[a] hold those items of ins[a] / outs[a]
using Launch = std::function<hipError_t(const void* const*, void* const*, size_t, size_t, hipStream_t)>;

// CPUs this process may actually use: min(affinity mask, cgroup quota — v2 cpu.max, else v1 cfs_quota_us / cfs_period_us,
// as bench.py's usable_cpus() reads them).  The benchmark box shows 256 logical CPUs and grants 16.
static double cpu_budget() {
    static const double cpus = [] {
        double c = (double)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) c = (double)CPU_COUNT(&set);
        if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
            char q[32];
            double period = 0;
            if (std::fscanf(f, "%31s %lf", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) {
                const double quota = std::atof(q) / period;
                if (quota > 0 && quota < c) c = quota;
            }
            std::fclose(f);
        } else {  // cgroup v1: quota in microseconds per period, -1 = unlimited
            double quota = -1, period = 0;
            if (FILE* fq = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
                if (std::fscanf(fq, "%lf", &quota) != 1) quota = -1;
                std::fclose(fq);
            }
            if (FILE* fp = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (std::fscanf(fp, "%lf", &period) != 1) period = 0;
                std::fclose(fp);
            }
            if (quota > 0 && period > 0 && quota / period < c) c = quota / period;
        }
        return c < 1 ? 1.0 : c;
    }();
    return cpus;
}

static int staging_lanes_env() {  // P252_HOST_LANES: 0 = not set
    static const int lanes = [] {
        if (const char* e = std::getenv("P252_HOST_LANES")) {
            const int v = std::atoi(e);
            return v < 1 ? 1 : (v > 32 ? 32 : v);
        }
        return 0;
    }();
    return lanes;
}

// staging lanes of ONE context driven on its own
static int staging_lanes_wanted() {
    if (staging_lanes_env()) return staging_lanes_env();
    // Three lanes x two slots keep the PCIe link busy; MORE lanes are slower on the benchmark box (16 CPUs of cgroup
    // budget, 256 visible): 3 lanes 3.6-3.8e8 digests/s, 6 lanes 3.1-3.3e8, 12 lanes 2.0-2.2e8
    // (profiles/r02_host_path.txt).  Two when the process may use fewer than four CPUs.
    return cpu_budget() < 4 ? 2 : 3;
}

// staging lanes per context when n_ctx contexts are driven at once (p252_*_multi: one driver thread per context, which
// is that context's first lane, plus its extra lanes): the contexts SHARE the CPU budget — 8 contexts x 3 lanes under a
// 16-CPU quota is the 24-worker configuration the single-context sweep measured at half speed.
// A lane is host-memcpy work: ONE worker moves 1.66e8 digests/s (26.5 GB/s, profiles/r03_host_path_multi.txt: one context,
// one lane), a GPU takes 4.1e8, so a GPU wants 2.5 workers and the whole budget is worth using: lanes = floor(CPUs / n_ctx),
// at most the single-context optimum of 3, at least 1 — never more workers than CPUs (they sleep on blocking-sync events
// while their chunks are in flight; only the copies cost CPU time).
int p252host::staging_lanes_per_ctx(size_t n_ctx) {
    if (staging_lanes_env()) return staging_lanes_env();
    if (n_ctx <= 1) return staging_lanes_wanted();
    int per = (int)(cpu_budget() / (double)n_ctx);
    return per < 1 ? 1 : (per > 3 ? 3 : per);
}

// offsets of the spans' arrays of `items` items each in one buffer, 256-byte aligned; returns the total bytes
static size_t lay_out(const std::vector<HostSpan>& spans, size_t items, std::vector<size_t>& offs) {
    size_t total = 0;
    for (const HostSpan& sp : spans) {
        offs.push_back(total);
        total += (items * sp.stride + 255) & ~(size_t)255;
    }
    return total;
}

// Runs `launch(d_in[], d_out[], first_item, count, stream)` over n items in chunks of `chunk`, streaming the input arrays
// in and the output arrays out through the staging lanes.  d_in[a] / d_out[a] are the device copies of chunk-local slices
// of ins[a] / outs[a] (256-byte aligned).  `outs` may be empty (results stay on the device: the launch writes them itself).
static int staged_run(p252_ctx* ctx, size_t n, size_t chunk, const std::vector<HostSpan>& ins, const std::vector<HostSpan>& outs,
                      const Launch& launch) {
    const size_t n_chunks = (n + chunk - 1) / chunk;
    const int lanes_wanted = ctx->lane_budget > 0 ? ctx->lane_budget : staging_lanes_wanted();
    const int n_lanes = (int)(n_chunks < (size_t)lanes_wanted ? n_chunks : (size_t)lanes_wanted);
    if ((int)ctx->lanes.size() < n_lanes) ctx->lanes.resize(n_lanes);
    std::vector<size_t> in_off, out_off;
    size_t in_chunk_b = lay_out(ins, chunk, in_off), out_chunk_b = lay_out(outs, chunk, out_off);
    if (!in_chunk_b) in_chunk_b = 256;
    if (!out_chunk_b) out_chunk_b = 256;
    for (int l = 0; l < n_lanes; ++l) {
        p252_ctx::Lane& L = ctx->lanes[l];
        if (!L.st) HIP_TRY(ctx, hipStreamCreateWithFlags(&L.st, hipStreamNonBlocking));
        for (auto& S : L.slot) {
            if (!S.done) HIP_TRY(ctx, hipEventCreateWithFlags(&S.done, hipEventBlockingSync | hipEventDisableTiming));
            if (S.in_cap < in_chunk_b) {
                if (S.h_in) (void)hipHostFree(S.h_in);
                if (S.d_in) (void)hipFree(S.d_in);
                S.h_in = S.d_in = nullptr;
                S.in_cap = 0;
                HIP_TRY(ctx, hipHostMalloc(&S.h_in, in_chunk_b, hipHostMallocDefault));
                HIP_TRY(ctx, hipMalloc(&S.d_in, in_chunk_b));
                S.in_cap = in_chunk_b;
            }
            if (S.out_cap < out_chunk_b) {
                if (S.h_out) (void)hipHostFree(S.h_out);
                if (S.d_out) (void)hipFree(S.d_out);
                S.h_out = S.d_out = nullptr;
                S.out_cap = 0;
                HIP_TRY(ctx, hipHostMalloc(&S.h_out, out_chunk_b, hipHostMallocDefault));
                HIP_TRY(ctx, hipMalloc(&S.d_out, out_chunk_b));
                S.out_cap = out_chunk_b;
            }
            if (S.in_dirty < in_chunk_b) S.in_dirty = in_chunk_b;
            if (S.out_dirty < out_chunk_b) S.out_dirty = out_chunk_b;
        }
    }
    std::atomic<size_t> next{0};
    std::atomic<int> status{P252_OK};
    std::mutex err_mu;
    std::string err;
    auto work = [&](int l) {
        p252_ctx::Lane& L = ctx->lanes[l];
        auto bad = [&](const char* what, hipError_t e) {
            std::lock_guard<std::mutex> lk(err_mu);
            if (status.load() == P252_OK) {
                status.store(P252_ERR_HIP);
                err = std::string(what) + ": " + hipGetErrorString(e);
            }
        };
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return bad("hipSetDevice", e);
        long pending[2] = {-1, -1};  // chunk whose results sit (or will sit) in the slot's h_out
        auto retire = [&](int k) {    // wait for slot k's chunk and hand its outputs to the caller
            if (pending[k] < 0) return true;
            const hipError_t w = hipEventSynchronize(L.slot[k].done);
            if (w != hipSuccess) { bad("event sync", w); return false; }
            const size_t off = (size_t)pending[k] * chunk, cnt = n - off < chunk ? n - off : chunk;
            for (size_t a = 0; a < outs.size(); ++a)
                std::memcpy(outs[a].dst + off * outs[a].stride, static_cast<char*>(L.slot[k].h_out) + out_off[a], cnt * outs[a].stride);
            pending[k] = -1;
            return true;
        };
        std::vector<const void*> d_in(ins.size());
        std::vector<void*> d_out(outs.size());
        int k = 0;
        for (;;) {
            const size_t c = next.fetch_add(1);
            if (c >= n_chunks || status.load() != P252_OK) break;
            if (!retire(k)) return;
            p252_ctx::Slot& S = L.slot[k];
            const size_t off = c * chunk, cnt = n - off < chunk ? n - off : chunk;
            for (size_t a = 0; a < ins.size(); ++a) {
                char* h = static_cast<char*>(S.h_in) + in_off[a];
                char* d = static_cast<char*>(S.d_in) + in_off[a];
                std::memcpy(h, ins[a].src + off * ins[a].stride, cnt * ins[a].stride);
                e = hipMemcpyAsync(d, h, cnt * ins[a].stride, hipMemcpyHostToDevice, L.st);
                if (e != hipSuccess) return bad("H2D", e);
                d_in[a] = d;
            }
            for (size_t a = 0; a < outs.size(); ++a) d_out[a] = static_cast<char*>(S.d_out) + out_off[a];
            e = launch(d_in.data(), d_out.data(), off, cnt, L.st);
            if (e != hipSuccess) return bad("kernel launch", e);
            for (size_t a = 0; a < outs.size(); ++a) {
                e = hipMemcpyAsync(static_cast<char*>(S.h_out) + out_off[a], d_out[a], cnt * outs[a].stride, hipMemcpyDeviceToHost, L.st);
                if (e != hipSuccess) return bad("D2H", e);
            }
            e = hipEventRecord(S.done, L.st);
            if (e != hipSuccess) return bad("event record", e);
            pending[k] = (long)c;
            k ^= 1;
        }
        // drain, older chunk first (slot k holds the older one)
        if (!retire(k)) return;
        retire(k ^ 1);
    };
    std::vector<std::thread> pool;
    for (int l = 1; l < n_lanes; ++l) pool.emplace_back(work, l);
    work(0);
    for (auto& t : pool) t.join();
    if (status.load() != P252_OK) {
        for (int l = 0; l < n_lanes; ++l) (void)hipStreamSynchronize(ctx->lanes[l].st);  // never leave work in flight on the staging buffers
        return fail(ctx, status.load(), err);
    }
    return P252_OK;
}

// items per chunk so that a chunk moves about P252_HOST_CHUNK_MB (default 8) MiB, a multiple of the block size
static size_t staging_chunk_items(size_t bytes_per_item) {
    static const size_t chunk_bytes_target = [] {
        const char* e = std::getenv("P252_HOST_CHUNK_MB");
        const int mb = e ? std::atoi(e) : 8;
        return (size_t)(mb < 1 ? 1 : (mb > 256 ? 256 : mb)) << 20;
    }();
    size_t chunk = chunk_bytes_target / (bytes_per_item ? bytes_per_item : 1);
    if (chunk < 4096) chunk = 4096;
    return chunk & ~(size_t)255;
}

// P252_HOST_PIPELINE (developer switch): 0 = every host-buffer entry point takes its ONE_SHOT route (one copy each way)
static bool host_pipeline() {
    static const bool on = [] {
        const char* e = std::getenv("P252_HOST_PIPELINE");
        return !e || std::atoi(e) != 0;
    }();
    return on;
}

enum class Route { ONE_SHOT, STAGED, PINNED_DMA };

// the context's grow-only device scratch, at least in_b / out_b bytes; the extents handed out are recorded for crypt_host's wipe
static int scratch(p252_ctx* ctx, size_t in_b, size_t out_b) {
    int rc = ensure(ctx, &ctx->d_in, &ctx->d_in_cap, in_b);
    if (rc == P252_OK) rc = ensure(ctx, &ctx->d_out, &ctx->d_out_cap, out_b);
    if (rc) return rc;
    if (ctx->io_used.in < in_b) ctx->io_used.in = in_b;
    if (ctx->io_used.out < out_b) ctx->io_used.out = out_b;
    return P252_OK;
}

// The one transfer path of the host-buffer entry points: n items of the arrays `ins` to the device, `launch` over them, the
// arrays `outs` back (see the top of this file for the routes; `chunk` = items per chunk of STAGED and PINNED_DMA).  `outs` may
// be empty: the launch then leaves its results on the device itself.
static int host_batch(p252_ctx* ctx, Route route, size_t n, size_t chunk, const std::vector<HostSpan>& ins,
                      const std::vector<HostSpan>& outs, const Launch& launch) {
    if (route == Route::STAGED) {
        ctx->io_used.lanes = true;
        return staged_run(ctx, n, chunk, ins, outs, launch);
    }
    std::vector<size_t> in_off, out_off;
    const size_t in_b = lay_out(ins, n, in_off), out_b = lay_out(outs, n, out_off);
    int rc = scratch(ctx, in_b, out_b);
    if (rc) return rc;
    // ONE_SHOT: one chunk of n items, synchronous copies, the null stream.  PINNED_DMA: no staging copy; chunks round-robin over 3
    // streams so that the H2D copy of chunk c+1, the kernel of chunk c and the D2H copy of chunk c-1 overlap
    const bool dma = route == Route::PINNED_DMA;
    if (!dma) chunk = n;
    for (int i = 0; dma && i < 3; ++i)
        if (!ctx->streams[i]) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->streams[i], hipStreamNonBlocking));
    char* const d_in = static_cast<char*>(ctx->d_in);
    char* const d_out = static_cast<char*>(ctx->d_out);
    std::vector<void*> di(ins.size()), dout(outs.size());
    std::string err;
    auto check = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && err.empty()) err = std::string(what) + ": " + hipGetErrorString(e);
    };
    auto copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st, const char* what) {
        if (bytes && err.empty()) check(dma ? hipMemcpyAsync(dst, src, bytes, kind, st) : hipMemcpy(dst, src, bytes, kind), what);
    };
    size_t c = 0;
    for (size_t off = 0; off < n && err.empty(); off += chunk, ++c) {
        const size_t cnt = n - off < chunk ? n - off : chunk;
        hipStream_t st = dma ? ctx->streams[c % 3] : nullptr;
        for (size_t a = 0; a < ins.size(); ++a)
            copy(di[a] = d_in + in_off[a] + off * ins[a].stride, ins[a].src + off * ins[a].stride, cnt * ins[a].stride, hipMemcpyHostToDevice, st, "H2D");
        for (size_t a = 0; a < outs.size(); ++a) dout[a] = d_out + out_off[a] + off * outs[a].stride;
        if (err.empty()) check(launch(di.data(), dout.data(), off, cnt, st), "kernel launch");
        for (size_t a = 0; a < outs.size(); ++a)
            copy(outs[a].dst + off * outs[a].stride, dout[a], cnt * outs[a].stride, hipMemcpyDeviceToHost, st, "D2H");
    }
    for (int i = 0; dma && i < 3; ++i) check(hipStreamSynchronize(ctx->streams[i]), "stream sync");
    return err.empty() ? P252_OK : fail(ctx, P252_ERR_HIP, err);
}

// results a build left on the device (a root, tree levels, forest roots) into caller memory: ONE_SHOT = one hipMemcpy, STAGED =
// 32-byte items chunk by chunk through the staging lanes
static int download(p252_ctx* ctx, Route route, void* dst, const char* d_src, size_t bytes) {
    if (route == Route::STAGED)
        return host_batch(ctx, Route::STAGED, bytes / 32, staging_chunk_items(32), {}, {{nullptr, static_cast<char*>(dst), 32}},
                          [&](const void* const*, void* const* d_out, size_t off, size_t cnt, hipStream_t st) {
                              return hipMemcpyAsync(d_out[0], d_src + off * 32, cnt * 32, hipMemcpyDeviceToDevice, st);
                          });
    HIP_TRY(ctx, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
    return P252_OK;
}

// first-level nodes per chunk when a tree or forest streams its leaves: 8 MiB of leaves
static size_t level1_chunk(unsigned arity) { return (((size_t)8 << 20) / (arity * 32)) & ~(size_t)255; }

// The leaves of a tree or forest build on the device; *cur / *cur_n: the array the build continues from.  ONE_SHOT: the leaves,
// uploaded whole.  STAGED — big pageable leaf arrays (512 MiB at 2^24 leaves): the upload would take longer than the whole build —
// the FIRST level, hashed chunk by chunk while the leaves stream in through the staging lanes, into d_l1 (NULL: the context's
// scratch); the leaves are never resident as a whole.
static int leaves_to_device(p252_ctx* ctx, Route route, unsigned arity, const uint64_t tag[4], const uint64_t* leaves, size_t n_leaves,
                            char* d_l1, const void** cur, size_t* cur_n) {
    const char* h_leaves = reinterpret_cast<const char*>(leaves);
    if (route == Route::ONE_SHOT) {
        *cur_n = n_leaves;
        return host_batch(ctx, Route::ONE_SHOT, 1, 1, {{h_leaves, nullptr, n_leaves * 32}}, {},
                          [&](const void* const* d_in, void* const*, size_t, size_t, hipStream_t) {
                              *cur = d_in[0];  // (an upload only: the build follows on the same stream)
                              return hipSuccess;
                          });
    }
    const size_t n_l1 = n_leaves / arity;
    if (!d_l1) {
        int rc = scratch(ctx, n_l1 * 32, 0);
        if (rc) return rc;
        d_l1 = static_cast<char*>(ctx->d_in);
    }
    *cur = d_l1;
    *cur_n = n_l1;
    const TagArg targ = tag_arg(tag);
    return host_batch(ctx, Route::STAGED, n_l1, level1_chunk(arity), {{h_leaves, nullptr, arity * 32}}, {},
                      [&](const void* const* d_in, void* const*, size_t off, size_t cnt, hipStream_t st) {
                          return launch_merkle4(ctx->d_tab, targ, d_in[0], arity * cnt, d_l1 + off * 32, cnt, st, arity);
                      });
}

static int hash_batch_host_impl(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* in, size_t in_len, size_t out_len,
                                uint64_t* out, size_t n, bool trunc250) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "hash"};
    // dusk-safe rejects io-patterns with an empty absorb or squeeze -> Hash::finalize panics (hash.rs:134-137)
    if (in_len == 0 || out_len == 0)
        return fail(ctx, P252_ERR_INVALID_IO_PATTERN, "hash: in_len and out_len must be > 0");
    if (in_len > 0x7fffffffu || out_len > 0x7fffffffu) return refuse("length too large");
    if (n == 0) return P252_OK;
    if (!tag || !in || !out) return refuse("NULL buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const TagArg targ = tag_arg(tag);
    const bool single = in_len == 4 && out_len == 1, pair = in_len == 2 && out_len == 1;
    const size_t chunk = staging_chunk_items((in_len > out_len ? in_len : out_len) * 32);
    const Route route = !host_pipeline() || n < 2 * chunk ? Route::ONE_SHOT
                        : !is_pinned(in) || !is_pinned(out) ? Route::STAGED : Route::PINNED_DMA;
    return host_batch(ctx, route, n, chunk, {{reinterpret_cast<const char*>(in), nullptr, in_len * 32}},
                      {{nullptr, reinterpret_cast<char*>(out), out_len * 32}},
                      [&](const void* const* d_in, void* const* d_out, size_t, size_t cnt, hipStream_t st) {
                          // Merkle4- and Merkle2-shaped digests take the single-permutation kernel
                          if (single) return launch_merkle4(ctx->d_tab, targ, d_in[0], 4 * cnt, d_out[0], cnt, st, 4, 0, trunc250);
                          if (pair) return launch_merkle4(ctx->d_tab, targ, d_in[0], 2 * cnt, d_out[0], cnt, st, 2, 0, trunc250);
                          return launch_sponge(ctx->d_tab, targ, d_in[0], (unsigned)in_len, (unsigned)out_len, d_out[0], cnt, st, trunc250);
                      });
}

// messages of different lengths: every message is checked here first, then [messages | tags | offsets rebased to 0] go to the
// device in one copy each and the outputs come back — synchronous, no chunked pipeline
static int hash_ragged_host_impl(p252_ctx* ctx, const uint64_t* tags, size_t max_len, const uint64_t* in, const uint64_t* offsets,
                                 size_t out_len, uint64_t* out, size_t n, bool trunc250) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "hash_ragged"};
    if (out_len == 0) return fail(ctx, P252_ERR_INVALID_IO_PATTERN, "hash_ragged: out_len must be > 0");
    if (out_len > 0x7fffffffu) return refuse("out_len too large");
    if (n == 0) return P252_OK;
    if (max_len == 0) return refuse("max_len must be > 0");
    if (!tags || !offsets || !out) return refuse("NULL buffer");
    for (size_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return refuse("offsets decrease at message " + std::to_string(i));
        const uint64_t len = offsets[i + 1] - offsets[i];
        if (len == 0)  // a zero-length absorb is an invalid io-pattern (dusk-safe; Hash::finalize panics, hash.rs:134-137)
            return fail(ctx, P252_ERR_INVALID_IO_PATTERN, "hash_ragged: message " + std::to_string(i) + " is empty");
        if (len > max_len) return refuse("message " + std::to_string(i) + " is longer than max_len");
    }
    if (!in) return refuse("NULL buffer");
    const uint64_t total = offsets[n] - offsets[0];
    if (total > SIZE_MAX / 64 || max_len > SIZE_MAX / 64 || n > SIZE_MAX / 64 / out_len) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> rebased(offsets, offsets + n + 1);
    for (auto& o : rebased) o -= offsets[0];
    // the arrays are not per message: each is one item of its whole size
    const std::vector<HostSpan> ins = {{reinterpret_cast<const char*>(in + offsets[0] * 4), nullptr, (size_t)total * 32},
                                       {reinterpret_cast<const char*>(tags), nullptr, max_len * 32},
                                       {reinterpret_cast<const char*>(rebased.data()), nullptr, (n + 1) * 8}};
    int dev_rc = P252_OK;  // (the `_device` call takes the sort's scratch pair of the stream; its status is an entry-point code)
    const int rc = host_batch(ctx, Route::ONE_SHOT, 1, 1, ins, {{nullptr, reinterpret_cast<char*>(out), n * out_len * 32}},
                              [&](const void* const* d_in, void* const* d_out, size_t, size_t, hipStream_t st) {
                                  dev_rc = (trunc250 ? p252_hash_ragged_truncated_device : p252_hash_ragged_device)(
                                      ctx, d_in[1], max_len, d_in[0], d_in[2], out_len, d_out[0], n, nullptr, st);
                                  return hipSuccess;
                              });
    return dev_rc ? dev_rc : rc;
}

// trees of different sizes: every tree is checked here first, then [leaves | offsets rebased to 0] go to the device in one copy
// each and the roots (and the tree-major levels) come back — synchronous, no chunked pipeline
static int forest_ragged_host(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const uint64_t* leaves, const uint64_t* offsets,
                              size_t n_trees, uint64_t* roots, uint64_t* levels) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle_forest_ragged"};
    if (n_trees == 0) return P252_OK;
    if (!tag || !leaves || !offsets || !roots) return refuse("NULL buffer");
    size_t max_leaves = 0, lvl_n = 0;
    for (size_t t = 0; t < n_trees; ++t) {
        if (offsets[t + 1] < offsets[t]) return refuse("offsets decrease at tree " + std::to_string(t));
        const uint64_t n = offsets[t + 1] - offsets[t];
        if (n == 0) return refuse("tree " + std::to_string(t) + " is empty");
        if (n > max_leaves) max_leaves = n;
    }
    const uint64_t total = offsets[n_trees] - offsets[0];
    if (total > SIZE_MAX / 64 || n_trees > SIZE_MAX / 64) return refuse("size overflow");
    if (levels)
        for (size_t t = 0; t < n_trees; ++t) lvl_n += levels_len(offsets[t + 1] - offsets[t], arity);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> rebased(offsets, offsets + n_trees + 1);
    for (auto& o : rebased) o -= offsets[0];
    // the arrays are not per tree: each is one item of its whole size
    const std::vector<HostSpan> ins = {{reinterpret_cast<const char*>(leaves + offsets[0] * 4), nullptr, (size_t)total * 32},
                                       {reinterpret_cast<const char*>(rebased.data()), nullptr, (n_trees + 1) * 8}};
    std::vector<HostSpan> outs = {{nullptr, reinterpret_cast<char*>(roots), n_trees * 32}};
    if (lvl_n) outs.push_back({nullptr, reinterpret_cast<char*>(levels), lvl_n * 32});
    int dev_rc = P252_OK;  // (the `_device` call takes the scratch pair of the stream; its status is an entry-point code)
    const int rc = host_batch(ctx, Route::ONE_SHOT, 1, 1, ins, outs,
                              [&](const void* const* d_in, void* const* d_out, size_t, size_t, hipStream_t st) {
                                  dev_rc = (arity == 4 ? p252_merkle4_forest_ragged_device : p252_merkle2_forest_ragged_device)(
                                      ctx, tag, d_in[0], (size_t)total, d_in[1], n_trees, max_leaves, d_out[0], lvl_n ? d_out[1] : nullptr,
                                      nullptr, st);
                                  return hipSuccess;
                              });
    return dev_rc ? dev_rc : rc;
}

static int merkle_tree_host(p252_ctx* ctx, unsigned arity, const uint64_t tag[4], const uint64_t* leaves, size_t n_leaves,
                            uint64_t root[4], uint64_t* levels) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle_tree"};
    if (n_leaves == 0) return refuse("n_leaves must be > 0");
    if (!tag || !leaves || !root) return refuse("NULL buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t lvl_bytes = levels_len(n_leaves, arity) * 32, n_l1 = n_leaves / arity;
    int rc = scratch(ctx, 0, (levels ? lvl_bytes : 0) + 32);
    if (rc) return rc;
    char* d_root = static_cast<char*>(ctx->d_out);
    char* d_levels = levels ? d_root + 32 : nullptr;
    const Route first = host_pipeline() && n_leaves % arity == 0 && n_l1 >= 4 * level1_chunk(arity) && !is_pinned(leaves) ? Route::STAGED
                                                                                                                         : Route::ONE_SHOT;
    const void* cur = nullptr;
    size_t cur_n = 0;
    rc = leaves_to_device(ctx, first, arity, tag, leaves, n_leaves, d_levels, &cur, &cur_n);  // (a streamed level 1 is the first of the levels)
    if (rc) return rc;
    rc = merkle_tree_device(ctx, arity, tag, cur, cur_n, d_root, d_levels && first == Route::STAGED ? d_levels + n_l1 * 32 : d_levels, nullptr);
    if (rc) return rc;
    rc = download(ctx, Route::ONE_SHOT, root, d_root, 32);  // (also orders the download below behind the build)
    if (rc || !levels || !lvl_bytes) return rc;
    // all levels of a big tree (171 MiB at 2^24 leaves) into pageable memory: chunk by chunk through the staging lanes
    const Route down = host_pipeline() && lvl_bytes / 32 >= 2 * staging_chunk_items(32) && !is_pinned(levels) ? Route::STAGED : Route::ONE_SHOT;
    return download(ctx, down, levels, d_levels, lvl_bytes);
}

extern "C" {

int p252_permute_batch(p252_ctx* ctx, const uint64_t* states, uint64_t* out, size_t n) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "permute"};
    if (n == 0) return P252_OK;
    if (!states || !out) return refuse("NULL buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t chunk = staging_chunk_items(P252_HADES_WIDTH * 32);
    const Route route = host_pipeline() && n >= 2 * chunk && !(is_pinned(states) && is_pinned(out)) ? Route::STAGED : Route::ONE_SHOT;
    return host_batch(ctx, route, n, chunk, {{reinterpret_cast<const char*>(states), nullptr, P252_HADES_WIDTH * 32}},
                      {{nullptr, reinterpret_cast<char*>(out), P252_HADES_WIDTH * 32}},
                      [&](const void* const* d_in, void* const* d_out, size_t, size_t cnt, hipStream_t st) {
                          return launch_permute(ctx->d_tab, d_in[0], d_out[0], cnt, st);
                      });
}

int p252_hash_batch(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* in, size_t in_len, size_t out_len,
                    uint64_t* out, size_t n) {
    return hash_batch_host_impl(ctx, tag, in, in_len, out_len, out, n, false);
}

int p252_hash_batch_truncated(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* in, size_t in_len, size_t out_len,
                              uint64_t* out_raw, size_t n) {
    return hash_batch_host_impl(ctx, tag, in, in_len, out_len, out_raw, n, true);
}

int p252_hash_ragged(p252_ctx* ctx, const uint64_t* tags, size_t max_len, const uint64_t* in, const uint64_t* offsets, size_t out_len,
                     uint64_t* out, size_t n) {
    return hash_ragged_host_impl(ctx, tags, max_len, in, offsets, out_len, out, n, false);
}

int p252_hash_ragged_truncated(p252_ctx* ctx, const uint64_t* tags, size_t max_len, const uint64_t* in, const uint64_t* offsets,
                               size_t out_len, uint64_t* out_raw, size_t n) {
    return hash_ragged_host_impl(ctx, tags, max_len, in, offsets, out_len, out_raw, n, true);
}

P252_MERKLE_PAIR(int, tree,
                 (p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, size_t n_leaves, uint64_t root[4], uint64_t* levels),
                 merkle_tree_host(ctx, arity, tag, leaves, n_leaves, root, levels))

P252_MERKLE_PAIR(int, forest_ragged,
                 (p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, const uint64_t* offsets, size_t n_trees, uint64_t* roots,
                  uint64_t* levels),
                 forest_ragged_host(ctx, arity, tag, leaves, offsets, n_trees, roots, levels))

// Forest from HOST leaves (pageable memory is fine).  Large forests stream the FIRST level — three quarters of all permutations —
// through the staging lanes (leaves_to_device), then the upper levels run ONCE, one launch per level across all trees, so their
// latency-bound launches are paid once per forest and not once per chunk (a first version that built a whole forest per
// 32-MiB chunk ran at 2.5e8 perm/s: every chunk paid the five narrow levels).  Trees are independent: no exchange.
int p252_merkle4_forest(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, size_t n_trees, size_t leaves_per_tree, uint64_t* roots) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle_forest"};
    if (n_trees == 0) return P252_OK;
    if (!power_of_4(leaves_per_tree)) return refuse("leaves_per_tree must be arity^k");
    if (n_trees > (SIZE_MAX / 32) / leaves_per_tree) return refuse("size overflow");
    if (!tag || !leaves || !roots) return refuse("NULL buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n_leaves = n_trees * leaves_per_tree;
    int rc = scratch(ctx, 0, n_trees * 32);
    if (rc) return rc;
    // (small forests, or page-locked leaves — the DMA runs at PCIe speed anyway: one upload, one build)
    const Route first = host_pipeline() && leaves_per_tree >= 4 && n_leaves / 4 >= 4 * level1_chunk(4) && !is_pinned(leaves) ? Route::STAGED
                                                                                                                           : Route::ONE_SHOT;
    const void* cur = nullptr;
    size_t cur_n = 0;
    rc = leaves_to_device(ctx, first, 4, tag, leaves, n_leaves, nullptr, &cur, &cur_n);
    if (rc) return rc;
    rc = p252_merkle4_forest_device(ctx, tag, cur, n_trees, cur_n / n_trees, ctx->d_out, nullptr, nullptr);
    if (rc) return rc;
    return download(ctx, Route::ONE_SHOT, roots, static_cast<const char*>(ctx->d_out), n_trees * 32);
}

int p252_merkle4_path_batch(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, const uint64_t* siblings,
                            const uint8_t* positions, size_t depth, uint64_t* roots, size_t n) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "merkle4_path"};
    if (n == 0) return P252_OK;
    if (!tag || !leaves || !roots || (depth && (!siblings || !positions))) return refuse("NULL buffer");
    for (size_t i = 0; i < n * depth; ++i)
        if (positions[i] > 3) return refuse("position outside 0..3");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (depth > 0xffffu) return refuse("depth too large");
    const TagArg targ = tag_arg(tag);
    const size_t chunk = staging_chunk_items(64 + depth * 97);
    // (a large batch: leaves, sibling blocks and positions stream through the staging lanes, whether page-locked or not)
    const Route route = host_pipeline() && depth && n >= 2 * chunk ? Route::STAGED : Route::ONE_SHOT;
    return host_batch(ctx, route, n, chunk,
                      {{reinterpret_cast<const char*>(leaves), nullptr, 32},
                       {reinterpret_cast<const char*>(siblings), nullptr, depth * 96},
                       {reinterpret_cast<const char*>(positions), nullptr, depth}},
                      {{nullptr, reinterpret_cast<char*>(roots), 32}},
                      [&](const void* const* d_in, void* const* d_out, size_t, size_t cnt, hipStream_t st) {
                          return launch_merkle4_path(ctx->d_tab, targ, d_in[0], d_in[1], d_in[2], (unsigned)depth, d_out[0], cnt, st);
                      });
}

}  // extern "C"

// ---- encryption row (src/encryption.rs:62-95 -> dusk_safe::encrypt / decrypt) ----
static int crypt_host_run(p252_ctx* ctx, int variant, bool decrypt, const uint64_t tag[4], const uint64_t* in, const uint64_t* secrets,
                          const uint64_t* nonces, size_t len, uint64_t* out, uint8_t* ok, size_t n) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, "encrypt/decrypt"};
    if (!crypt_variant_ok(variant)) return refuse("unknown variant");
    if (len == 0) return fail(ctx, P252_ERR_INVALID_IO_PATTERN, "encrypt/decrypt: empty message");
    if (n == 0) return P252_OK;
    if (!tag || !in || !secrets || !nonces || !out || (decrypt && !ok)) return refuse("NULL buffer");
    if (len >= 0x1ffffff0u) return refuse("message too long");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the call table is uploaded once, here; the launches only read it (no shared state between the lanes, no lock)
    int rc = prepare_prog(ctx, variant, len);
    if (rc) return rc;
    const TagArg targ = tag_arg(tag);
    const uint32_t* d_prog = ctx->d_prog;
    const unsigned n_calls = ctx->prog_calls;
    const size_t in_stride = (decrypt ? len + 1 : len) * 32, out_stride = (decrypt ? len : len + 1) * 32;
    std::vector<HostSpan> ins = {{reinterpret_cast<const char*>(in), nullptr, in_stride},
                                 {reinterpret_cast<const char*>(secrets), nullptr, 64},
                                 {reinterpret_cast<const char*>(nonces), nullptr, 32}};
    std::vector<HostSpan> outs = {{nullptr, reinterpret_cast<char*>(out), out_stride}};
    if (decrypt) outs.push_back({nullptr, reinterpret_cast<char*>(ok), 1});
    const size_t chunk = staging_chunk_items(in_stride + out_stride + 96);
    return host_batch(ctx, host_pipeline() && n >= 2 * chunk ? Route::STAGED : Route::ONE_SHOT, n, chunk, ins, outs,
                      [&](const void* const* d_in, void* const* d_out, size_t, size_t cnt, hipStream_t st) {
                          return launch_crypt(decrypt, ctx->d_tab, targ, d_in[0], d_in[1], d_in[2], (unsigned)len, d_out[0],
                                              decrypt ? d_out[1] : nullptr, cnt, d_prog, n_calls, st);
                      });
}

// the host-buffer encrypt / decrypt: whatever the call copied into library-owned memory — shared secrets, nonces, plaintexts
// and ciphertexts in the context's device scratch or in the staging lanes (page-locked host + device chunks) — is cleared
// before it returns, on success and on failure (the reference: zeroize, Cargo.toml:14; dusk-safe zeroizes a finished sponge)
// (`run` is the call proper; stream_scratch: it also worked in the null stream's scratch pair — the ragged calls' order array and
// counters, which hold no secret but are cleared with the rest)
template <class Run>
static int crypt_host_wiped(p252_ctx* ctx, bool stream_scratch, Run&& run) {
    if (ctx) ctx->io_used = {};
    const int rc = run();
    if (!ctx) return rc;
    const p252_ctx::IoUse used = ctx->io_used;
    if (!used.in && !used.out && !used.lanes) return rc;
    const std::string msg = ctx->err;
    // Nothing of THIS call may still be in flight on what is cleared: the call ran on the staging lanes' streams (non-blocking) or
    // on the null stream — those are synchronised, not the device (other contexts and streams keep running).  Every
    // step runs whatever an earlier one reported (the first error is kept): the page-locked host halves need no device at all.
    hipError_t e = hipSuccess;
    auto keep = [&](hipError_t r) {
        if (r != hipSuccess && e == hipSuccess) e = r;
    };
    if (used.lanes)
        for (auto& l : ctx->lanes)
            if (l.st) keep(hipStreamSynchronize(l.st));
    keep(hipStreamSynchronize(nullptr));
    // only the bytes the lanes may have written are cleared, not their whole capacity (host halves first, then the device ones)
    if (used.lanes) keep(wipe_lanes(ctx, /*dirty_only=*/true));
    keep(wipe_span(ctx->d_in, used.in < ctx->d_in_cap ? used.in : ctx->d_in_cap));
    keep(wipe_span(ctx->d_out, used.out < ctx->d_out_cap ? used.out : ctx->d_out_cap));
    if (stream_scratch)
        for (auto& set : ctx->lvl)
            if (set.st == nullptr)
                for (int i = 0; i < 2; ++i) keep(wipe_span(set.buf[i], set.cap[i]));
    keep(hipStreamSynchronize(nullptr));
    if (e != hipSuccess && rc == P252_OK) return fail(ctx, P252_ERR_HIP, std::string("encrypt/decrypt: wiping the scratch failed: ") + hipGetErrorString(e));
    ctx->err = msg;
    return rc;
}

static int crypt_host(p252_ctx* ctx, int variant, bool decrypt, const uint64_t tag[4], const uint64_t* in, const uint64_t* secrets,
                      const uint64_t* nonces, size_t len, uint64_t* out, uint8_t* ok, size_t n) {
    return crypt_host_wiped(ctx, false, [&] { return crypt_host_run(ctx, variant, decrypt, tag, in, secrets, nonces, len, out, ok, n); });
}

// messages of different lengths: every message is checked here first (the codes of hash_ragged), then [message or cipher side |
// tags | offsets rebased to 0 | secrets | nonces] go to the device in one copy each and the other side (and the flags) come back —
// synchronous, no chunked pipeline.  The cipher of message i lies at offsets[i] + i, so the cipher side of a call whose offsets do
// not start at 0 starts offsets[0] scalars into the caller's array, as the message side does.
static int crypt_ragged_host_run(p252_ctx* ctx, int variant, bool decrypt, const uint64_t* tags, size_t max_len, const uint64_t* in,
                                 const uint64_t* offsets, const uint64_t* secrets, const uint64_t* nonces, uint64_t* out, uint8_t* ok, size_t n) {
    if (!ctx) return P252_ERR_INVALID_ARGUMENT;
    const Refusal refuse{ctx, decrypt ? "decrypt_ragged" : "encrypt_ragged"};
    if (!crypt_variant_ok(variant)) return refuse("unknown variant");
    if (max_len == 0 || max_len > P252_CRYPT_RAGGED_MAX_LEN)
        return refuse("max_len must be 1 .. P252_CRYPT_RAGGED_MAX_LEN = " + std::to_string(P252_CRYPT_RAGGED_MAX_LEN));
    if (n == 0) return P252_OK;
    if (!tags || !offsets || !secrets || !nonces || !out || (decrypt && !ok)) return refuse("NULL buffer");
    for (size_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return refuse("offsets decrease at message " + std::to_string(i));
        const uint64_t len = offsets[i + 1] - offsets[i];
        if (len == 0) return fail(ctx, P252_ERR_INVALID_IO_PATTERN, std::string(refuse.who) + ": message " + std::to_string(i) + " is empty");
        if (len > max_len) return refuse("message " + std::to_string(i) + " is longer than max_len");
    }
    if (!in) return refuse("NULL buffer");
    const uint64_t total = offsets[n] - offsets[0];
    if (total > SIZE_MAX / 128 || n > SIZE_MAX / 128) return refuse("size overflow");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> rebased(offsets, offsets + n + 1);
    for (auto& o : rebased) o -= offsets[0];
    const size_t msg_bytes = (size_t)total * 32, cph_bytes = ((size_t)total + n) * 32;
    // the arrays are not per message: each is one item of its whole size
    const std::vector<HostSpan> ins = {{reinterpret_cast<const char*>(in + offsets[0] * 4), nullptr, decrypt ? cph_bytes : msg_bytes},
                                       {reinterpret_cast<const char*>(tags), nullptr, max_len * 32},
                                       {reinterpret_cast<const char*>(rebased.data()), nullptr, (n + 1) * 8},
                                       {reinterpret_cast<const char*>(secrets), nullptr, n * 64},
                                       {reinterpret_cast<const char*>(nonces), nullptr, n * 32}};
    std::vector<HostSpan> outs = {{nullptr, reinterpret_cast<char*>(out + offsets[0] * 4), decrypt ? msg_bytes : cph_bytes}};
    if (decrypt) outs.push_back({nullptr, reinterpret_cast<char*>(ok), n});
    int dev_rc = P252_OK;  // (the `_device` call takes the schedule's scratch pair of the stream; its status is an entry-point code)
    const int rc = host_batch(ctx, Route::ONE_SHOT, 1, 1, ins, outs, [&](const void* const* d_in, void* const* d_out, size_t, size_t, hipStream_t st) {
        dev_rc = decrypt ? p252_decrypt_ragged_device_into(ctx, variant, d_in[1], max_len, d_in[0], (size_t)total, d_in[2], d_in[3], d_in[4], d_out[0], d_out[1],
                                                      n, nullptr, st)
                         : p252_encrypt_ragged_device_into(ctx, variant, d_in[1], max_len, d_in[0], (size_t)total, d_in[2], d_in[3], d_in[4], d_out[0], n, nullptr,
                                                      st);
        return hipSuccess;
    });
    return dev_rc ? dev_rc : rc;
}

extern "C" {

int p252_encrypt_batch(p252_ctx* ctx, int variant, const uint64_t tag[4], const uint64_t* messages, const uint64_t* secrets,
                       const uint64_t* nonces, size_t len, uint64_t* ciphers, size_t n) {
    return crypt_host(ctx, variant, false, tag, messages, secrets, nonces, len, ciphers, nullptr, n);
}

int p252_decrypt_batch(p252_ctx* ctx, int variant, const uint64_t tag[4], const uint64_t* ciphers, const uint64_t* secrets,
                       const uint64_t* nonces, size_t len, uint64_t* messages, uint8_t* ok, size_t n) {
    return crypt_host(ctx, variant, true, tag, ciphers, secrets, nonces, len, messages, ok, n);
}

int p252_encrypt_ragged(p252_ctx* ctx, int variant, const uint64_t* tags, size_t max_len, const uint64_t* messages, const uint64_t* offsets,
                        const uint64_t* secrets, const uint64_t* nonces, uint64_t* ciphers, size_t n) {
    return crypt_host_wiped(ctx, true, [&] {
        return crypt_ragged_host_run(ctx, variant, false, tags, max_len, messages, offsets, secrets, nonces, ciphers, nullptr, n);
    });
}

int p252_decrypt_ragged(p252_ctx* ctx, int variant, const uint64_t* tags, size_t max_len, const uint64_t* ciphers, const uint64_t* offsets,
                        const uint64_t* secrets, const uint64_t* nonces, uint64_t* messages, uint8_t* ok, size_t n) {
    return crypt_host_wiped(ctx, true, [&] {
        return crypt_ragged_host_run(ctx, variant, true, tags, max_len, ciphers, offsets, secrets, nonces, messages, ok, n);
    });
}

}  // extern "C"
