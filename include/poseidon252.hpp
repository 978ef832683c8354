// poseidon252.hpp — C++17 host-side mirror of dusk_poseidon::{Domain, Hash} over the C ABI
// (include/poseidon252_hip.h).  Header-only; link with -lposeidon252_hip.
//
// The reference (dusk-poseidon 0.42, Rust) is compiled code and no Rust toolchain exists in the build
// image, so the host side above the C ABI is provided in C++ (and in Python, poseidon252_amd/hash.py)
// with the reference's names, argument meaning and error behaviour:
//
//   reference (src/hash.rs)                       here
//   ------------------------------------------    -----------------------------------------------
//   enum Domain {Merkle4,Merkle2,Encryption,Other}  enum class Domain            (hash.rs:21-36)
//   impl From<Domain> for u64                       domain_separator(Domain)     (hash.rs:38-56)
//   Hash::new / output_len / update / finalize      Hash(...) / same names       (hash.rs:98-155)
//   Hash::finalize_truncated / digest[_truncated]   same names                   (hash.rs:164-210)
//   panic!("io-pattern should be valid")            throws IoPatternError        (hash.rs:124-137)
//   —                                               HashBatch: n messages, one kernel launch
//   Hash::digest over messages of any lengths       RaggedHashBatch: n messages of different lengths, one call
//   —                                               merkle_forest_ragged: trees of different sizes, one call
//   —                                               merkle_forest_ragged_openings_device / merkle_path_ragged_device /
//                                                   merkle_forest_ragged_verify_device: openings out of such a forest
//   —                                               merkle_forest_ragged_update_device: leaf updates anywhere in such a forest
//   —                                               merkle_forest_ragged_update_journaled_device / merkle_forest_ragged_journal_swap_device /
//                                                   merkle_forest_ragged_journal_bound: such updates undone and redone, no hashing
//   —                                               merkle_forest_ragged_append_device: leaves appended to its trees, into a new forest
//   —                                               merkle_forest_ragged_resize_device: its trees cut, then appended to; trailing trees dropped
//   —                                               merkle_forest_ragged_select_device: any of its trees (and another forest's) gathered into a new forest
//   —                                               merkle_multiproof_device / merkle_multiproof_verify_device /
//                                                   merkle_multiproof_bound: many leaves of one tree, one shared proof
//   —                                               merkle_forest_ragged_multiproof_device / _verify_device / _bound: leaves of many
//                                                   trees of a ragged forest, one tree-major shared proof
//   —                                               merkle_forest_frontier_append_device / _extract_device / _bound: a forest of
//                                                   append-only trees kept only as their frontiers;
//                                                   merkle_forest_frontier_append_witness_device: the same with the openings of
//                                                   marked leaves kept current
//
// A BlsScalar is 4 little-endian u64 Montgomery limbs (a * 2^256 mod p), exactly the reference's
// memory layout, so buffers are interchangeable with a Rust &[BlsScalar].
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "poseidon252_hip.h"

namespace dusk_poseidon_hip {

using BlsScalar = std::array<uint64_t, 4>;     // Montgomery limbs, as dusk_bls12_381::BlsScalar
using JubJubRaw = std::array<uint64_t, 4>;     // argument of JubJubScalar::from_raw (hash.rs:180)
constexpr std::size_t HADES_WIDTH = P252_HADES_WIDTH;  // src/lib.rs:17

enum class Domain : int {  // declaration order of src/hash.rs:21-36
    Merkle4 = P252_DOMAIN_MERKLE4,
    Merkle2 = P252_DOMAIN_MERKLE2,
    Encryption = P252_DOMAIN_ENCRYPTION,
    Other = P252_DOMAIN_OTHER,
};

// dusk_poseidon::Error (src/error.rs:9-29) — the variants the hash path can produce.  Where the
// reference panics (`.expect`, hash.rs:131-154) this mirror throws.
struct IoPatternError : std::logic_error {
    enum Kind { IOPatternViolation, InvalidIOPattern } kind;
    IoPatternError(Kind k, const std::string& what) : std::logic_error(what), kind(k) {}
};
struct DeviceError : std::runtime_error {  // no HIP device / HIP failure: there is no CPU fallback
    using std::runtime_error::runtime_error;
};

inline uint64_t domain_separator(Domain d) {  // From<Domain> for u64
    uint64_t sep = 0;
    p252_domain_separator(static_cast<int>(d), &sep);
    return sep;
}

namespace detail {
inline void check(int rc, p252_ctx* ctx, const char* what) {
    if (rc == P252_OK) return;
    const std::string msg = std::string(what) + ": " + (ctx ? p252_last_error(ctx) : "");
    if (rc == P252_ERR_IO_PATTERN_VIOLATION)
        throw IoPatternError(IoPatternError::IOPatternViolation, "io-pattern should be valid: IOPatternViolation " + msg);
    if (rc == P252_ERR_INVALID_IO_PATTERN)
        throw IoPatternError(IoPatternError::InvalidIOPattern, "at this point the io-pattern is valid: InvalidIOPattern " + msg);
    if (rc == P252_ERR_INVALID_ARGUMENT) throw std::invalid_argument(msg);
    throw DeviceError(msg + " (rc " + std::to_string(rc) + ")");
}
}  // namespace detail

// One p252_ctx, bound to one HIP device (one process/thread per GPU).
class Context {
  public:
    explicit Context(int device = 0) {
        // argument lists have changed between library versions under unchanged names: never call into another interface
        if (p252_abi_version() != P252_ABI_VERSION)
            throw DeviceError("libposeidon252_hip.so implements ABI version " + std::to_string(p252_abi_version()) +
                              ", this header is version " + std::to_string(P252_ABI_VERSION));
        p252_ctx* c = nullptr;
        const int rc = p252_create(device, &c);
        if (rc != P252_OK) throw DeviceError(std::string("p252_create: ") + p252_last_error(nullptr));
        ctx_.reset(c, p252_destroy);
    }
    p252_ctx* get() const { return ctx_.get(); }
    // clears every scratch buffer the context owns (zeroize, Cargo.toml:14); the host-buffer encrypt / decrypt calls and the
    // destructor do so themselves
    void wipe() { detail::check(p252_wipe(ctx_.get()), ctx_.get(), "Context::wipe"); }
    // gives the grow-only scratch back (waits for the device, wipes, frees); the next call allocates what it needs again
    void trim() { detail::check(p252_trim(ctx_.get()), ctx_.get(), "Context::trim"); }
    static Context& default_context() {
        static Context c(0);
        return c;
    }

  private:
    std::shared_ptr<p252_ctx> ctx_;
};

// Page-locks a caller-owned buffer for its lifetime (p252_host_register / p252_host_unregister): host-buffer calls on it
// copy at PCIe speed instead of page-locking it on every call.  The buffer must outlive this object.
class HostRegistration {
  public:
    HostRegistration(void* p, std::size_t bytes) : p_(p) {
        if (p252_host_register(p, bytes) != P252_OK) throw DeviceError("p252_host_register failed");
    }
    ~HostRegistration() { (void)p252_host_unregister(p_); }
    HostRegistration(const HostRegistration&) = delete;
    HostRegistration& operator=(const HostRegistration&) = delete;

  private:
    void* p_;
};

// io_pattern() of src/hash.rs:62-85 plus dusk-safe's validation; throws like Hash::finalize panics
inline void check_io_pattern(Domain d, const std::vector<std::size_t>& absorb_lens, std::size_t output_len) {
    detail::check(p252_check_io_pattern(static_cast<int>(d), absorb_lens.data(), absorb_lens.size(), output_len), nullptr,
                  "io_pattern");
}

// Safe::tag for this io-pattern (scalar.rs:29-31).  UNPINNED recipe: pass the value
// from the real crates through the `tag` parameters instead when it is available.
inline BlsScalar compute_tag(Domain d, const std::vector<std::size_t>& absorb_lens, std::size_t output_len) {
    BlsScalar t{};
    detail::check(p252_tag(static_cast<int>(d), absorb_lens.data(), absorb_lens.size(), output_len, t.data()), nullptr, "tag");
    return t;
}

// ---- Hash: one message, absorbed in chunks, squeezed once (src/hash.rs:87-211) ----
class Hash {
  public:
    explicit Hash(Domain domain, Context& ctx = Context::default_context()) : domain_(domain), ctx_(ctx) {}  // Hash::new
    static Hash new_(Domain domain) { return Hash(domain); }

    // hash.rs:111-115: honoured only for Domain::Other and output_len > 0
    void output_len(std::size_t n) {
        if (domain_ == Domain::Other && n > 0) output_len_ = n;
    }
    // hash.rs:118-120: the slice is borrowed, never copied or modified; it must outlive finalize()
    void update(const BlsScalar* input, std::size_t len) { input_.emplace_back(input, len); }
    void update(const std::vector<BlsScalar>& input) { update(input.data(), input.size()); }

    // hash.rs:128-155.  Throws IoPatternError where the reference panics.
    std::vector<BlsScalar> finalize() const { return run(false); }
    // hash.rs:164-183: the digest kernel's output stage canonicalises, masks to 250 bits and stores the raw limbs
    // JubJubScalar::from_raw receives — one launch (p252_hash_batch_truncated)
    std::vector<JubJubRaw> finalize_truncated() const { return run(true); }

  private:
    std::vector<BlsScalar> run(bool truncated) const {
        std::vector<std::size_t> lens;
        std::size_t total = 0;
        for (auto& c : input_) {
            lens.push_back(c.second);
            total += c.second;
        }
        check_io_pattern(domain_, lens, output_len_);
        const BlsScalar tag = has_tag_ ? tag_ : compute_tag(domain_, lens, output_len_);
        std::vector<BlsScalar> msg;
        msg.reserve(total);
        for (auto& c : input_) msg.insert(msg.end(), c.first, c.first + c.second);
        std::vector<BlsScalar> out(output_len_);
        detail::check((truncated ? p252_hash_batch_truncated : p252_hash_batch)(ctx_.get(), tag.data(), msg[0].data(), total, output_len_,
                                                                                out[0].data(), 1),
                      ctx_.get(), truncated ? "Hash::finalize_truncated" : "Hash::finalize");
        return out;
    }

  public:
    // hash.rs:191-195, 203-210
    static std::vector<BlsScalar> digest(Domain domain, const std::vector<BlsScalar>& input) {
        Hash h(domain);
        h.update(input);
        return h.finalize();
    }
    static std::vector<JubJubRaw> digest_truncated(Domain domain, const std::vector<BlsScalar>& input) {
        Hash h(domain);
        h.update(input);
        return h.finalize_truncated();
    }
    // inject the capacity element computed by the real crates (BlsScalar::hash_to_scalar)
    void set_tag(const BlsScalar& tag) {
        tag_ = tag;
        has_tag_ = true;
    }

  private:
    Domain domain_;
    Context& ctx_;
    std::vector<std::pair<const BlsScalar*, std::size_t>> input_;
    std::size_t output_len_ = 1;
    BlsScalar tag_{};
    bool has_tag_ = false;
};

// ---- HashBatch: n independent messages with one io-pattern in one kernel launch.  Per item the
// result equals Hash::digest(domain, item): same validation, same tag, same output order. ----
class HashBatch {
  public:
    HashBatch(Domain domain, std::size_t item_len, std::size_t output_len = 1, Context& ctx = Context::default_context())
        : domain_(domain), item_len_(item_len), output_len_((domain == Domain::Other && output_len > 0) ? output_len : 1), ctx_(ctx) {
        check_io_pattern(domain_, {item_len_}, output_len_);
        tag_ = compute_tag(domain_, {item_len_}, output_len_);
    }
    void set_tag(const BlsScalar& tag) { tag_ = tag; }
    const BlsScalar& tag() const { return tag_; }
    std::size_t output_len() const { return output_len_; }

    // host buffers: input.size() must be a multiple of item_len
    std::vector<BlsScalar> digest(const std::vector<BlsScalar>& input) const {
        if (item_len_ == 0 || input.size() % item_len_) throw std::invalid_argument("HashBatch::digest: ragged input");
        const std::size_t n = input.size() / item_len_;
        std::vector<BlsScalar> out(n * output_len_);
        if (n)
            detail::check(p252_hash_batch(ctx_.get(), tag_.data(), input[0].data(), item_len_, output_len_, out[0].data(), n),
                          ctx_.get(), "HashBatch::digest");
        return out;
    }
    // Hash::digest_truncated per item (hash.rs:203-210), truncated inside the digest kernel: one launch
    std::vector<JubJubRaw> digest_truncated(const std::vector<BlsScalar>& input) const {
        if (item_len_ == 0 || input.size() % item_len_) throw std::invalid_argument("HashBatch::digest_truncated: ragged input");
        const std::size_t n = input.size() / item_len_;
        std::vector<JubJubRaw> out(n * output_len_);
        if (n)
            detail::check(p252_hash_batch_truncated(ctx_.get(), tag_.data(), input[0].data(), item_len_, output_len_, out[0].data(), n),
                          ctx_.get(), "HashBatch::digest_truncated");
        return out;
    }
    // device buffers, asynchronous on `stream` (a hipStream_t)
    void digest_device(const void* d_in, void* d_out, std::size_t n, void* stream = nullptr) const {
        detail::check(p252_hash_batch_device(ctx_.get(), tag_.data(), d_in, item_len_, output_len_, d_out, n, stream), ctx_.get(),
                      "HashBatch::digest_device");
    }
    void digest_truncated_device(const void* d_in, void* d_out_raw, std::size_t n, void* stream = nullptr) const {
        detail::check(p252_hash_batch_truncated_device(ctx_.get(), tag_.data(), d_in, item_len_, output_len_, d_out_raw, n, stream),
                      ctx_.get(), "HashBatch::digest_truncated_device");
    }

  private:
    Domain domain_;
    std::size_t item_len_, output_len_;
    Context& ctx_;
    BlsScalar tag_{};
};

// n messages of DIFFERENT lengths in one call (p252_hash_ragged*): per message Hash::digest(domain, message), hash.rs:191-195.
// The tag table (row L - 1 = the tag of [Absorb(L), Squeeze(output_len)]) grows to the longest message seen; the Merkle domains
// have one fixed length and are refused (HashBatch).
class RaggedHashBatch {
  public:
    explicit RaggedHashBatch(Domain domain = Domain::Other, std::size_t output_len = 1, Context& ctx = Context::default_context())
        : domain_(domain), output_len_((domain == Domain::Other && output_len > 0) ? output_len : 1), ctx_(ctx) {
        if (domain == Domain::Merkle4 || domain == Domain::Merkle2)
            throw IoPatternError(IoPatternError::IOPatternViolation,
                                 "io-pattern should be valid: IOPatternViolation — Merkle messages have one fixed length; use HashBatch");
    }
    std::size_t output_len() const { return output_len_; }
    // the tag table of lengths 1 .. max_len (computed on first use, kept)
    const std::vector<BlsScalar>& tags(std::size_t max_len) {
        while (tags_.size() < max_len) tags_.push_back(compute_tag(domain_, {tags_.size() + 1}, output_len_));
        return tags_;
    }

    // host buffers: out[i * output_len ..] = the digest of messages[i]
    std::vector<BlsScalar> digest(const std::vector<std::vector<BlsScalar>>& messages) { return run<BlsScalar>(messages, false); }
    std::vector<JubJubRaw> digest_truncated(const std::vector<std::vector<BlsScalar>>& messages) { return run<JubJubRaw>(messages, true); }
    // device buffers, asynchronous on `stream`: d_offsets = n + 1 uint64 scalar indices into d_in; d_tags = tags(max_len) uploaded by
    // the caller (this header links no HIP runtime, and a tag is an input of every entry point).  Bad messages (empty, longer than
    // max_len, decreasing offsets) get zero rows and increment *d_n_bad (device uint32, zeroed by the caller; may be null).
    void digest_device(const void* d_tags, std::size_t max_len, const void* d_in, const void* d_offsets, std::size_t n, void* d_out,
                       void* d_n_bad = nullptr, void* stream = nullptr) const {
        detail::check(p252_hash_ragged_device(ctx_.get(), d_tags, max_len, d_in, d_offsets, output_len_, d_out, n, d_n_bad, stream),
                      ctx_.get(), "RaggedHashBatch::digest_device");
    }

  private:
    template <class Out>
    std::vector<Out> run(const std::vector<std::vector<BlsScalar>>& messages, bool truncated) {
        std::vector<uint64_t> offsets(1, 0);
        std::size_t longest = 0;
        for (const auto& m : messages) {
            offsets.push_back(offsets.back() + m.size());
            longest = m.size() > longest ? m.size() : longest;
        }
        std::vector<BlsScalar> flat;
        flat.reserve(offsets.back());
        for (const auto& m : messages) flat.insert(flat.end(), m.begin(), m.end());
        std::vector<Out> out(messages.size() * output_len_);
        if (messages.empty()) return out;
        const std::size_t max_len = longest ? longest : 1;
        const auto& t = tags(max_len);
        const uint64_t* in = flat.empty() ? t[0].data() : flat[0].data();  // (all-empty input: refused before it is read)
        const int rc = truncated ? p252_hash_ragged_truncated(ctx_.get(), t[0].data(), max_len, in, offsets.data(), output_len_, out[0].data(), messages.size())
                                 : p252_hash_ragged(ctx_.get(), t[0].data(), max_len, in, offsets.data(), output_len_, out[0].data(), messages.size());
        detail::check(rc, ctx_.get(), truncated ? "RaggedHashBatch::digest_truncated" : "RaggedHashBatch::digest");
        return out;
    }
    Domain domain_;
    std::size_t output_len_;
    Context& ctx_;
    std::vector<BlsScalar> tags_;
};

// Arity-4 Merkle root over Hash::digest(Domain::Merkle4, ..) nodes (empty slots = zero, hash.rs:22-26)
inline BlsScalar merkle4_root(const std::vector<BlsScalar>& leaves, Context& ctx = Context::default_context()) {
    const BlsScalar tag = compute_tag(Domain::Merkle4, {4}, 1);
    BlsScalar root{};
    if (leaves.empty()) throw std::invalid_argument("merkle4_root: no leaves");
    detail::check(p252_merkle4_tree(ctx.get(), tag.data(), leaves[0].data(), leaves.size(), root.data(), nullptr), ctx.get(),
                  "merkle4_root");
    return root;
}

// ---- several GPUs from one process: one Context per device, sharded inside the library (p252_*_multi) ----
// digests[i*output_len..] == Hash::digest(domain, item i); contiguous shards, no inter-GPU dependence
inline std::vector<BlsScalar> digest_multi(const std::vector<Context*>& ctxs, const HashBatch& hb, std::size_t item_len,
                                           const std::vector<BlsScalar>& input) {
    if (ctxs.empty() || item_len == 0 || input.size() % item_len) throw std::invalid_argument("digest_multi: bad arguments");
    std::vector<p252_ctx*> raw;
    for (Context* c : ctxs) raw.push_back(c->get());
    const std::size_t n = input.size() / item_len;
    std::vector<BlsScalar> out(n * hb.output_len());
    if (n)
        detail::check(p252_hash_batch_multi(raw.data(), raw.size(), hb.tag().data(), input[0].data(), item_len, hb.output_len(),
                                            out[0].data(), n),
                      raw[0], "digest_multi");
    return out;
}
// root of the arity-4 tree over ctxs.size() * 4^k leaves: one complete subtree per device, 32-byte roots gathered on the host
// (host leaves: they stream in through each context's staging lanes; device-resident shards: p252_merkle4_tree_multi_device, RCCL)
inline BlsScalar merkle4_root_multi(const std::vector<Context*>& ctxs, const std::vector<BlsScalar>& leaves) {
    if (ctxs.empty() || leaves.empty()) throw std::invalid_argument("merkle4_root_multi: bad arguments");
    std::vector<p252_ctx*> raw;
    for (Context* c : ctxs) raw.push_back(c->get());
    const BlsScalar tag = compute_tag(Domain::Merkle4, {4}, 1);
    BlsScalar root{};
    detail::check(p252_merkle4_tree_multi(raw.data(), raw.size(), tag.data(), leaves[0].data(), leaves.size(), root.data()), raw[0],
                  "merkle4_root_multi");
    return root;
}

// ---- RCCL communicator of the library (p252_comm_*): the constants are broadcast and validated when it is created, the
// sharded tree build all-gathers its 32-byte subtree roots on the stream.  One Comm per Context.  One process per GPU:
// rank 0 calls Comm::unique_id() and hands the bytes to the other ranks, every rank constructs Comm(ctx, id, rank, world).
// One process, several GPUs: Comm::create_all(contexts on distinct devices). ----
class Comm {
  public:
    using Id = std::array<unsigned char, P252_COMM_ID_BYTES>;
    static Id unique_id() {
        Id id{};
        detail::check(p252_comm_unique_id(id.data(), id.size()), nullptr, "p252_comm_unique_id");
        return id;
    }
    Comm(Context& ctx, const Id& id, int rank, int world) : ctx_(ctx) {
        p252_comm* c = nullptr;
        detail::check(p252_comm_create_rank(ctx.get(), id.data(), id.size(), rank, world, &c), ctx.get(), "p252_comm_create_rank");
        comm_.reset(c, p252_comm_destroy);
    }
    static std::vector<Comm> create_all(const std::vector<Context*>& ctxs) {
        if (ctxs.empty()) throw std::invalid_argument("Comm::create_all: no contexts");
        std::vector<p252_ctx*> raw;
        for (Context* c : ctxs) raw.push_back(c->get());
        std::vector<p252_comm*> out(raw.size(), nullptr);
        detail::check(p252_comm_create_all(raw.data(), raw.size(), out.data()), raw[0], "p252_comm_create_all");
        std::vector<Comm> v;
        for (std::size_t t = 0; t < raw.size(); ++t) v.push_back(Comm(*ctxs[t], out[t]));
        return v;
    }
    int rank() const { return p252_comm_rank(comm_.get()); }
    int size() const { return p252_comm_size(comm_.get()); }
    // this rank's 4^k device-resident leaves -> root over ALL ranks' leaves in d_root (32 B, device), asynchronously on
    // `stream`; collective (every rank calls it)
    void merkle4_root_sharded_device(const void* d_leaves, std::size_t n_leaves_local, void* d_root, void* stream = nullptr) {
        const BlsScalar tag = compute_tag(Domain::Merkle4, {4}, 1);
        detail::check(p252_merkle4_tree_sharded_device(comm_.get(), tag.data(), d_leaves, n_leaves_local, d_root, stream), ctx_.get(),
                      "merkle4_root_sharded_device");
    }
    // waits for `stream`, then throws if a sharded build of this communicator met a failed peer since the last check (that build's
    // root is all-ones on every healthy rank): p252_comm_check
    void check(void* stream = nullptr) { detail::check(p252_comm_check(comm_.get(), stream), ctx_.get(), "Comm::check"); }
    // the RCCL shared object the library resolved for this process at run time (p252_comm_backend)
    static std::string backend() {
        char path[4096] = {0};
        detail::check(p252_comm_backend(path, sizeof path), nullptr, "p252_comm_backend");
        return path;
    }
    p252_comm* get() const { return comm_.get(); }

  private:
    Comm(Context& ctx, p252_comm* c) : ctx_(ctx) { comm_.reset(c, p252_comm_destroy); }
    Context ctx_;  // (shared ownership: the context outlives its communicator)
    std::shared_ptr<p252_comm> comm_;
};

// Roots of the leaves.size() / leaves_per_tree independent complete trees stored tree-major in HOST memory
// (p252_merkle4_forest: the first level is hashed while the leaves stream in through the staging lanes, the upper levels once)
inline std::vector<BlsScalar> merkle4_forest(const std::vector<BlsScalar>& leaves, std::size_t leaves_per_tree,
                                             Context& ctx = Context::default_context()) {
    if (leaves_per_tree == 0 || leaves.size() % leaves_per_tree) throw std::invalid_argument("merkle4_forest: not whole trees");
    const BlsScalar tag = compute_tag(Domain::Merkle4, {4}, 1);
    std::vector<BlsScalar> roots(leaves.size() / leaves_per_tree);
    if (!roots.empty())
        detail::check(p252_merkle4_forest(ctx.get(), tag.data(), leaves[0].data(), roots.size(), leaves_per_tree, roots[0].data()), ctx.get(),
                      "merkle4_forest");
    return roots;
}

// A forest of roots.size() independent complete trees of leaves_per_tree = 4^k device-resident leaves each (tree-major):
// one launch per level across all trees (p252_merkle4_forest_device); d_roots receives n_trees scalars.
inline void merkle4_forest_device(const void* d_leaves, std::size_t n_trees, std::size_t leaves_per_tree, void* d_roots,
                                  Context& ctx = Context::default_context(), void* d_levels = nullptr, void* stream = nullptr) {
    const BlsScalar tag = compute_tag(Domain::Merkle4, {4}, 1);
    detail::check(p252_merkle4_forest_device(ctx.get(), tag.data(), d_leaves, n_trees, leaves_per_tree, d_roots, d_levels, stream), ctx.get(),
                  "merkle4_forest_device");
}

namespace detail {
// The p252_merkle{4,2}_* entry points of ONE arity that the functions below call — a member per name of the list, so that no merkle2
// slot can hold a merkle4 function — and the io-pattern of that arity's node hash (tag(): computed per call, as compute_tag is).
#define P252_MERKLE_FNS(X, N)                                                                                                                \
    X(N, levels_len) X(N, depth) X(N, forest_ragged) X(N, forest_ragged_device) X(N, forest_ragged_openings_device) X(N, path_ragged_device) \
    X(N, forest_ragged_verify_device) X(N, forest_ragged_update_device) X(N, forest_ragged_append_device_into) X(N, multiproof_bound)        \
    X(N, forest_ragged_resize_device_into) X(N, forest_ragged_journal_bound) X(N, forest_ragged_update_journaled_device_into)                    \
    X(N, forest_ragged_journal_swap_device_into) X(N, forest_ragged_select_device_into)                                                      \
    X(N, multiproof_device) X(N, multiproof_verify_device) X(N, forest_ragged_multiproof_bound) X(N, forest_ragged_multiproof_device_into)        \
    X(N, forest_ragged_multiproof_verify_device_into) X(N, forest_frontier_bound) X(N, forest_frontier_append_device_into)                \
    X(N, forest_frontier_extract_device_into) X(N, forest_frontier_append_witness_device_into)                                            \
    X(N, forest_ragged_consistency_device_into) X(N, forest_consistency_verify_device_into)                                              \
    X(N, forest_ragged_anchor_openings_device_into) X(N, forest_range_stride) X(N, forest_ragged_range_proofs_device_into)               \
    X(N, forest_range_verify_device_into) X(N, forest_ragged_update_sequential_device_into)
#define P252_MEMBER(N, f) decltype(&p252_merkle##N##_##f) f;
#define P252_SYMBOL(N, f) p252_merkle##N##_##f,
struct MerkleAbi {
    Domain domain;
    std::size_t width;
    P252_MERKLE_FNS(P252_MEMBER, 4)
    BlsScalar tag() const { return compute_tag(domain, {width}, 1); }
};
inline const MerkleAbi& merkle_abi(const char* who, unsigned arity) {
    static const MerkleAbi merkle4{Domain::Merkle4, 4, P252_MERKLE_FNS(P252_SYMBOL, 4)}, merkle2{Domain::Merkle2, 2, P252_MERKLE_FNS(P252_SYMBOL, 2)};
    if (arity != 4 && arity != 2) throw std::invalid_argument(std::string(who) + ": arity must be 4 or 2");
    return arity == 4 ? merkle4 : merkle2;
}
#undef P252_MERKLE_FNS
#undef P252_MEMBER
#undef P252_SYMBOL
}  // namespace detail

// Trees of DIFFERENT sizes in one call (p252_merkle{4,2}_forest_ragged): roots[t] = the root of trees[t] alone (what
// p252_merkle{4,2}_tree returns), one launch per level across all trees.  With want_levels, `levels` is TREE-MAJOR — tree t's
// block, at level_offsets[t], is byte for byte what the single-tree call writes (not the level-major layout of
// merkle4_forest_device) — and level_offsets holds the n_trees + 1 prefix sums of p252_merkle{4,2}_levels_len(n_t).
struct RaggedForest {
    std::vector<BlsScalar> roots;
    std::vector<BlsScalar> levels;
    std::vector<std::uint64_t> level_offsets;
};
inline RaggedForest merkle_forest_ragged(const std::vector<std::vector<BlsScalar>>& trees, unsigned arity = 4, bool want_levels = false,
                                         Context& ctx = Context::default_context()) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged", arity);
    RaggedForest f;
    std::vector<BlsScalar> flat;
    std::vector<std::uint64_t> offsets(1, 0);
    f.level_offsets.assign(1, 0);
    for (std::size_t t = 0; t < trees.size(); ++t) {
        if (trees[t].empty()) throw std::invalid_argument("merkle_forest_ragged: tree " + std::to_string(t) + " is empty");
        flat.insert(flat.end(), trees[t].begin(), trees[t].end());
        offsets.push_back(flat.size());
        f.level_offsets.push_back(f.level_offsets.back() + m.levels_len(trees[t].size()));
    }
    f.roots.resize(trees.size());
    if (want_levels) f.levels.resize(f.level_offsets.back());
    if (trees.empty()) return f;
    std::uint64_t* lv = f.levels.empty() ? nullptr : f.levels[0].data();
    detail::check(m.forest_ragged(ctx.get(), m.tag().data(), flat[0].data(), offsets.data(), trees.size(), f.roots[0].data(), lv), ctx.get(),
                  "merkle_forest_ragged");
    if (!want_levels) f.level_offsets.clear();
    return f;
}

// The device form (p252_merkle{4,2}_forest_ragged_device), asynchronous on `stream`: tree t = d_leaves[d_offsets[t] .. d_offsets[t+1])
// (n_trees + 1 device uint64 offsets), n_leaves = the scalars d_leaves holds.  Bad trees get zero roots and increment *d_n_bad.
// d_levels (tree-major) must hold n_leaves / (arity - 1) + n_trees * p252_merkle{4,2}_depth(max_leaves) scalars.
inline void merkle_forest_ragged_device(const void* d_leaves, std::size_t n_leaves, const void* d_offsets, std::size_t n_trees,
                                        std::size_t max_leaves, void* d_roots, unsigned arity = 4, Context& ctx = Context::default_context(),
                                        void* d_levels = nullptr, void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_device", arity);
    detail::check(m.forest_ragged_device(ctx.get(), m.tag().data(), d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_roots, d_levels,
                                         d_n_bad, stream), ctx.get(), "merkle_forest_ragged_device");
}

// Openings out of such a forest in one call (p252_merkle{4,2}_forest_ragged_openings_device): opening i = leaf d_leaf_ids[i] (uint64)
// of tree d_tree_ids[i] (uint32); the forest arguments exactly as the build took them (d_levels required unless every tree is a
// single leaf).  Outputs at the stride D = forest_openings_stride(max_leaves, arity): d_leaves_out[k], d_siblings[k][D][arity - 1],
// d_positions[k][D], d_depths[k] (uint8; 0xFF = a bad opening, all zero, counted in *d_n_bad).
inline std::size_t forest_openings_stride(std::size_t max_leaves, unsigned arity = 4) {
    return detail::merkle_abi("forest_openings_stride", arity).depth(max_leaves);
}
inline void merkle_forest_ragged_openings_device(const void* d_leaves, std::size_t n_leaves, const void* d_offsets, std::size_t n_trees,
                                                 std::size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                                 const void* d_leaf_ids, std::size_t k, void* d_leaves_out, void* d_siblings,
                                                 void* d_positions, void* d_depths, unsigned arity = 4,
                                                 Context& ctx = Context::default_context(), void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_openings_device", arity);
    detail::check(m.forest_ragged_openings_device(ctx.get(), d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids, d_leaf_ids,
                                                  k, d_leaves_out, d_siblings, d_positions, d_depths, d_n_bad, stream),
                  ctx.get(), "merkle_forest_ragged_openings_device");
}

// The re-hash with a depth per opening (p252_merkle{4,2}_path_ragged_device): d_roots_out[i] from the first d_depths[i] levels of
// opening i in the layout above; a depth above stride_depth (0xFF included) gives a zero root and is counted in *d_n_bad.
inline void merkle_path_ragged_device(const void* d_leaves, const void* d_siblings, const void* d_positions, const void* d_depths,
                                      std::size_t stride_depth, void* d_roots_out, std::size_t k, unsigned arity = 4,
                                      Context& ctx = Context::default_context(), void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_path_ragged_device", arity);
    detail::check(m.path_ragged_device(ctx.get(), m.tag().data(), d_leaves, d_siblings, d_positions, d_depths, stride_depth, d_roots_out, k,
                                       d_n_bad, stream), ctx.get(), "merkle_path_ragged_device");
}

// `Opening::verify` across a forest (p252_merkle{4,2}_forest_ragged_verify_device): d_ok[i] = 1 iff opening i is well-formed and
// re-hashes to d_roots[d_tree_ids[i]], the root of ITS tree.
inline void merkle_forest_ragged_verify_device(const void* d_leaves, const void* d_siblings, const void* d_positions, const void* d_depths,
                                               std::size_t stride_depth, const void* d_tree_ids, const void* d_roots, std::size_t n_trees,
                                               void* d_ok, std::size_t k, unsigned arity = 4, Context& ctx = Context::default_context(),
                                               void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_verify_device", arity);
    detail::check(m.forest_ragged_verify_device(ctx.get(), m.tag().data(), d_leaves, d_siblings, d_positions, d_depths, stride_depth, d_tree_ids,
                                                d_roots, n_trees, d_ok, k, stream), ctx.get(), "merkle_forest_ragged_verify_device");
}

// Leaf updates anywhere in such a forest in one call (p252_merkle{4,2}_forest_ragged_update_device): update i writes d_new_leaves[i]
// to leaf d_leaf_ids[i] (uint64) of tree d_tree_ids[i] (uint32) and every dirty ancestor is re-hashed once, in place; the forest
// arguments exactly as the build took them.  d_roots[t] is rewritten for the trees that were touched; a bad update writes nothing
// and is counted in *d_n_bad; *d_n_hashed (device uint64, zeroed by the caller) grows by the number of digests computed.
inline void merkle_forest_ragged_update_device(void* d_leaves, std::size_t n_leaves, const void* d_offsets, std::size_t n_trees,
                                               std::size_t max_leaves, void* d_levels, const void* d_tree_ids, const void* d_leaf_ids,
                                               const void* d_new_leaves, std::size_t k, unsigned arity = 4,
                                               Context& ctx = Context::default_context(), void* d_roots = nullptr, void* d_n_bad = nullptr,
                                               void* d_n_hashed = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_update_device", arity);
    detail::check(m.forest_ragged_update_device(ctx.get(), m.tag().data(), d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_tree_ids,
                                                d_leaf_ids, d_new_leaves, k, d_roots, d_n_bad, d_n_hashed, stream),
                  ctx.get(), "merkle_forest_ragged_update_device");
}

// The same update keeping a journal of every leaf and node it overwrites (p252_merkle{4,2}_forest_ragged_update_journaled_device_into), and the
// swap that plays the journal back (p252_merkle{4,2}_forest_ragged_journal_swap_device_into): one swap undoes the update byte for byte, a
// second one redoes it, and nothing is hashed.  The journal is the caller's: ids (16 bytes per entry) and values (32 bytes per entry)
// for `cap` entries, cap >= merkle_forest_ragged_journal_bound(..), and a device uint64 length that the update sets.  Of a (tree, leaf)
// pair given several times one update is applied, whole.  A journal is only meaningful for the forest shape it was taken on.
struct ForestJournal {
    void* d_ids;
    void* d_values;
    std::size_t cap;
    void* d_len;
};
inline std::size_t merkle_forest_ragged_journal_bound(std::size_t n_leaves, std::size_t n_trees, std::size_t max_leaves, std::size_t k,
                                                      unsigned arity = 4) {
    return detail::merkle_abi("merkle_forest_ragged_journal_bound", arity).forest_ragged_journal_bound(n_leaves, n_trees, max_leaves, k);
}
inline void merkle_forest_ragged_update_journaled_device(void* d_leaves, std::size_t n_leaves, const void* d_offsets, std::size_t n_trees,
                                                         std::size_t max_leaves, void* d_levels, const void* d_tree_ids, const void* d_leaf_ids,
                                                         const void* d_new_leaves, std::size_t k, const ForestJournal& journal, unsigned arity = 4,
                                                         Context& ctx = Context::default_context(), void* d_roots = nullptr,
                                                         void* d_n_bad = nullptr, void* d_n_hashed = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_update_journaled_device", arity);
    detail::check(m.forest_ragged_update_journaled_device_into(ctx.get(), m.tag().data(), d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels,
                                                          d_tree_ids, d_leaf_ids, d_new_leaves, k, d_roots, d_n_bad, d_n_hashed, journal.d_ids,
                                                          journal.d_values, journal.cap, journal.d_len, stream),
                  ctx.get(), "merkle_forest_ragged_update_journaled_device");
}
// An entry that names no node of this forest writes nothing and is counted in *d_n_bad (device uint32, zeroed by the caller).
inline void merkle_forest_ragged_journal_swap_device(void* d_leaves, std::size_t n_leaves, const void* d_offsets, std::size_t n_trees,
                                                     std::size_t max_leaves, void* d_levels, const ForestJournal& journal, unsigned arity = 4,
                                                     Context& ctx = Context::default_context(), void* d_roots = nullptr, void* d_n_bad = nullptr,
                                                     void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_journal_swap_device", arity);
    detail::check(m.forest_ragged_journal_swap_device_into(ctx.get(), d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, journal.d_ids,
                                                      journal.d_values, journal.cap, journal.d_len, d_roots, d_n_bad, stream),
                  ctx.get(), "merkle_forest_ragged_journal_swap_device");
}

// Leaves appended to the trees of such a forest, written INTO a new compact forest (p252_merkle{4,2}_forest_ragged_append_device_into):
// `old_forest` exactly as the build took and filled it (read-only); tree t of the n_trees_new >= old.n_trees new trees receives
// d_add[d_add_offsets[t] .. d_add_offsets[t + 1]) (n_trees_new + 1 device uint64).  `grown` names the caller's output buffers and their
// capacities in scalars (leaves_cap >= old.n_leaves + n_add; levels_cap >= forest_append_levels_cap(..)): afterwards they hold byte for
// byte a fresh build of the new forest — the unchanged nodes moved, only the nodes above a new leaf hashed.  A refused append or an
// empty new tree is counted in *d_n_bad; *d_n_hashed (device uint64, zeroed by the caller) receives the digests computed.
struct ForestView {  // the old forest
    const void* d_leaves;
    std::size_t n_leaves;
    const void* d_offsets;
    std::size_t n_trees, max_leaves;
    const void* d_levels;
};
struct ForestOut {  // where the new one goes
    void* d_leaves;
    std::size_t leaves_cap;
    void* d_offsets;
    void* d_levels;
    std::size_t levels_cap;
    void* d_roots;
};
inline std::size_t forest_append_levels_cap(std::size_t n_leaves_total, std::size_t n_trees_new, std::size_t max_leaves_new, unsigned arity = 4) {
    return n_leaves_total / (arity - 1) + n_trees_new * detail::merkle_abi("forest_append_levels_cap", arity).depth(max_leaves_new);
}
inline void merkle_forest_ragged_append_device(const ForestView& old_forest, const void* d_add, std::size_t n_add, const void* d_add_offsets,
                                               std::size_t n_trees_new, std::size_t max_leaves_new, const ForestOut& grown, unsigned arity = 4,
                                               Context& ctx = Context::default_context(), void* d_n_bad = nullptr, void* d_n_hashed = nullptr,
                                               void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_append_device", arity);
    detail::check(m.forest_ragged_append_device_into(ctx.get(), m.tag().data(), old_forest.d_leaves, old_forest.n_leaves, old_forest.d_offsets,
                                                     old_forest.n_trees, old_forest.max_leaves, old_forest.d_levels, d_add, n_add, d_add_offsets,
                                                     n_trees_new, max_leaves_new, grown.d_leaves, grown.leaves_cap, grown.d_offsets, grown.d_levels,
                                                     grown.levels_cap, grown.d_roots, d_n_bad, d_n_hashed, stream),
                  ctx.get(), "merkle_forest_ragged_append_device");
}

// Such a forest rolled back and forward in one call (p252_merkle{4,2}_forest_ragged_resize_device_into): the append above after tree t
// was cut to its first min(d_keep[t], n_t) leaves (d_keep: n_trees_new device uint64, nullptr = every tree whole; a value >= n_t keeps
// the tree whole).  n_trees_new may be smaller than old.n_trees: the trailing trees are dropped.  d_add may be nullptr with n_add == 0
// (a pure rollback: at most one node per tree and level is hashed); a refused append still leaves its tree cut.  `resized` is sized as
// `grown` above; afterwards it holds byte for byte a fresh build of the new forest.
inline void merkle_forest_ragged_resize_device(const ForestView& old_forest, const void* d_keep, const void* d_add, std::size_t n_add,
                                               const void* d_add_offsets, std::size_t n_trees_new, std::size_t max_leaves_new,
                                               const ForestOut& resized, unsigned arity = 4, Context& ctx = Context::default_context(),
                                               void* d_n_bad = nullptr, void* d_n_hashed = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_resize_device", arity);
    detail::check(m.forest_ragged_resize_device_into(ctx.get(), m.tag().data(), old_forest.d_leaves, old_forest.n_leaves, old_forest.d_offsets,
                                                     old_forest.n_trees, old_forest.max_leaves, old_forest.d_levels, d_keep, d_add, n_add,
                                                     d_add_offsets, n_trees_new, max_leaves_new, resized.d_leaves, resized.leaves_cap,
                                                     resized.d_offsets, resized.d_levels, resized.levels_cap, resized.d_roots, d_n_bad, d_n_hashed,
                                                     stream),
                  ctx.get(), "merkle_forest_ragged_resize_device");
}

// Any trees of one or two such forests gathered INTO a new compact forest, with no digest (p252_merkle{4,2}_forest_ragged_select_device_into):
// `a` and `b` exactly as their builds took and filled them, with their n_trees roots (read-only; b may be nullptr).  d_pick = n_pick
// device uint64: below a.n_trees a tree of a, then a tree of b; any order, repeats allowed.  `picked` names the caller's output buffers
// and their capacities in scalars (levels_cap >= forest_append_levels_cap(leaves_cap, n_pick, max of the two max_leaves)): afterwards
// they hold byte for byte a fresh build of the new forest.  A pick out of range, of a bad tree, or past leaves_cap (and every non-empty
// one behind it) becomes an empty tree — a zero root, no storage — and is counted in *d_n_bad (device uint32, zeroed by the caller).
struct ForestSource {
    ForestView forest;
    const void* d_roots;
};
inline void merkle_forest_ragged_select_device(const ForestSource& a, const ForestSource* b, const void* d_pick, std::size_t n_pick,
                                               const ForestOut& picked, unsigned arity = 4, Context& ctx = Context::default_context(),
                                               void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_select_device", arity);
    const ForestSource none{{nullptr, 0, nullptr, 0, 0, nullptr}, nullptr};
    const ForestSource& s = b ? *b : none;
    detail::check(m.forest_ragged_select_device_into(ctx.get(), a.forest.d_leaves, a.forest.n_leaves, a.forest.d_offsets, a.forest.n_trees,
                                                     a.forest.max_leaves, a.forest.d_levels, a.d_roots, s.forest.d_leaves, s.forest.n_leaves,
                                                     s.forest.d_offsets, s.forest.n_trees, s.forest.max_leaves, s.forest.d_levels, s.d_roots, d_pick,
                                                     n_pick, picked.d_leaves, picked.leaves_cap, picked.d_offsets, picked.d_levels,
                                                     picked.levels_cap, picked.d_roots, d_n_bad, stream),
                  ctx.get(), "merkle_forest_ragged_select_device");
}

// Many leaves of ONE stored tree behind one shared proof (p252_merkle{4,2}_multiproof_*; the format is in poseidon252_hip.h).
// merkle_multiproof_bound: the most scalars such a proof holds.
inline std::size_t merkle_multiproof_bound(std::size_t n_leaves, std::size_t k, unsigned arity = 4) {
    return detail::merkle_abi("merkle_multiproof_bound", arity).multiproof_bound(n_leaves, k);
}
// Extraction: d_indices = k strictly ascending uint32 positions; d_leaves_out[k], d_proof (nothing written at or past proof_cap
// scalars) and *d_proof_len (device uint64: the scalars the proof needs; 0 after a bad position, which *d_n_bad counts).
inline void merkle_multiproof_device(const void* d_leaves, std::size_t n_leaves, const void* d_levels, const void* d_indices, std::size_t k,
                                     void* d_leaves_out, void* d_proof, std::size_t proof_cap, void* d_proof_len, unsigned arity = 4,
                                     Context& ctx = Context::default_context(), void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_multiproof_device", arity);
    detail::check(m.multiproof_device(ctx.get(), d_leaves, n_leaves, d_levels, d_indices, k, d_leaves_out, d_proof, proof_cap, d_proof_len, d_n_bad,
                                      stream), ctx.get(), "merkle_multiproof_device");
}
// Verification, every ancestor hashed once: *d_ok (1 byte) = 1 iff no position is bad, the structure of (n_leaves, d_indices)
// consumes exactly proof_len scalars and the recomputed root equals *d_root.
inline void merkle_multiproof_verify_device(std::size_t n_leaves, const void* d_indices, const void* d_leaves_in, std::size_t k,
                                            const void* d_proof, std::size_t proof_len, const void* d_root, void* d_ok, unsigned arity = 4,
                                            Context& ctx = Context::default_context(), void* d_root_out = nullptr,
                                            void* d_n_hashed = nullptr, void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_multiproof_verify_device", arity);
    detail::check(m.multiproof_verify_device(ctx.get(), m.tag().data(), n_leaves, d_indices, d_leaves_in, k, d_proof, proof_len, d_root, d_ok,
                                             d_root_out, d_n_hashed, d_n_bad, stream), ctx.get(), "merkle_multiproof_verify_device");
}

// The shared proof across a forest of trees of DIFFERENT sizes (p252_merkle{4,2}_forest_ragged_multiproof_*; the format is in
// poseidon252_hip.h): k (tree id: uint32, leaf id: uint64) pairs, strictly ascending in (tree, leaf), anywhere in `forest` — exactly
// as the build took and filled it.  merkle_forest_ragged_multiproof_bound: the most scalars such a proof holds.
inline std::size_t merkle_forest_ragged_multiproof_bound(std::size_t n_leaves, std::size_t n_trees, std::size_t max_leaves, std::size_t k,
                                                         unsigned arity = 4) {
    return detail::merkle_abi("merkle_forest_ragged_multiproof_bound", arity).forest_ragged_multiproof_bound(n_leaves, n_trees, max_leaves, k);
}
// Extraction: d_leaves_out[k], d_proof (tree-major; nothing written at or past proof_cap scalars) and d_proof_offsets (n_trees + 1 device
// uint64: where each tree's single-tree proof starts, the last entry the scalars the proof needs; all zero after a bad pair, which
// *d_n_bad counts).
inline void merkle_forest_ragged_multiproof_device(const ForestView& forest, const void* d_tree_ids, const void* d_leaf_ids, std::size_t k,
                                                   void* d_leaves_out, void* d_proof, std::size_t proof_cap, void* d_proof_offsets,
                                                   unsigned arity = 4, Context& ctx = Context::default_context(), void* d_n_bad = nullptr,
                                                   void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_multiproof_device", arity);
    detail::check(m.forest_ragged_multiproof_device_into(ctx.get(), forest.d_leaves, forest.n_leaves, forest.d_offsets, forest.n_trees,
                                                    forest.max_leaves, forest.d_levels, d_tree_ids, d_leaf_ids, k, d_leaves_out, d_proof,
                                                    proof_cap, d_proof_offsets, d_n_bad, stream),
                  ctx.get(), "merkle_forest_ragged_multiproof_device");
}
// Verification, every ancestor hashed once, from the forest's shape alone (forest.d_leaves and forest.d_levels are not read): d_ok[t]
// (n_trees bytes) = 1 iff tree t has a pair, no pair is bad, its offsets are in order and inside proof_len, its structure consumes
// exactly its part of the proof and the recomputed root equals d_roots[t].
inline void merkle_forest_ragged_multiproof_verify_device(const ForestView& forest, const void* d_tree_ids, const void* d_leaf_ids,
                                                          const void* d_leaves_in, std::size_t k, const void* d_proof, std::size_t proof_len,
                                                          const void* d_proof_offsets, const void* d_roots, void* d_ok, unsigned arity = 4,
                                                          Context& ctx = Context::default_context(), void* d_roots_out = nullptr,
                                                          void* d_n_hashed = nullptr, void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_multiproof_verify_device", arity);
    detail::check(m.forest_ragged_multiproof_verify_device_into(ctx.get(), m.tag().data(), forest.d_offsets, forest.n_leaves, forest.n_trees,
                                                           forest.max_leaves, d_tree_ids, d_leaf_ids, d_leaves_in, k, d_proof, proof_len,
                                                           d_proof_offsets, d_roots, d_ok, d_roots_out, d_n_hashed, d_n_bad, stream),
                  ctx.get(), "merkle_forest_ragged_multiproof_verify_device");
}

// A forest of append-only trees kept ONLY as their frontiers (p252_merkle{4,2}_forest_frontier_*): per tree a leaf count, a root and
// merkle_forest_frontier_bound(max_leaves) = (depth(max_leaves) + 1) * (arity - 1) scalars, all device-resident and owned by the caller;
// all zero is a forest of empty trees.
struct ForestFrontier {
    void* d_counts;    // n_trees uint64
    void* d_frontier;  // n_trees x merkle_forest_frontier_bound(max_leaves) scalars
    void* d_roots;     // n_trees scalars
    std::size_t n_trees, max_leaves;
};
inline std::size_t merkle_forest_frontier_bound(std::size_t max_leaves, unsigned arity = 4) {
    return detail::merkle_abi("merkle_forest_frontier_bound", arity).forest_frontier_bound(max_leaves);
}
// Tree t receives d_add[d_add_offsets[t] .. d_add_offsets[t + 1]) (n_trees + 1 device uint64), in place: afterwards d_roots[t] is the
// root of every leaf the tree was given so far.  A refused append leaves its tree untouched and is counted in *d_n_bad; *d_n_hashed
// (device uint64, zeroed by the caller) receives the digests computed.
inline void merkle_forest_frontier_append_device(const ForestFrontier& state, const void* d_add, std::size_t n_add, const void* d_add_offsets,
                                                 unsigned arity = 4, Context& ctx = Context::default_context(), void* d_n_bad = nullptr,
                                                 void* d_n_hashed = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_frontier_append_device", arity);
    detail::check(m.forest_frontier_append_device_into(ctx.get(), m.tag().data(), state.d_counts, state.d_frontier, state.d_roots, state.n_trees,
                                                       state.max_leaves, d_add, n_add, d_add_offsets, d_n_bad, d_n_hashed, stream),
                  ctx.get(), "merkle_forest_frontier_append_device");
}
// The same append keeping the openings of k marked leaves current (p252_merkle{4,2}_forest_frontier_append_witness_device_into):
// witness i names leaf d_leaf_ids[i] (uint64) of tree d_tree_ids[i] (uint32); d_leaves[k], d_siblings[k][D][arity - 1],
// d_positions[k][D] and d_depths[k] at the stride D = forest_openings_stride(state.max_leaves, arity) are the layout of
// merkle_forest_ragged_openings_device, read and updated in place.  A witness of a leaf below its tree's old count must be its opening
// at that count; one of a leaf this call appends is written whole; one that names no leaf becomes all zero with depth 0xFF and is
// counted in *d_n_bad_witness.  Every good witness then verifies against state.d_roots (merkle_forest_ragged_verify_device).
struct ForestWitnesses {
    const void* d_tree_ids;
    const void* d_leaf_ids;
    std::size_t k;
    void* d_leaves;
    void* d_siblings;
    void* d_positions;
    void* d_depths;
};
inline void merkle_forest_frontier_append_witness_device(const ForestFrontier& state, const void* d_add, std::size_t n_add,
                                                         const void* d_add_offsets, const ForestWitnesses& witnesses, unsigned arity = 4,
                                                         Context& ctx = Context::default_context(), void* d_n_bad = nullptr,
                                                         void* d_n_hashed = nullptr, void* d_n_bad_witness = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_frontier_append_witness_device", arity);
    detail::check(m.forest_frontier_append_witness_device_into(ctx.get(), m.tag().data(), state.d_counts, state.d_frontier, state.d_roots,
                                                               state.n_trees, state.max_leaves, d_add, n_add, d_add_offsets, witnesses.d_tree_ids,
                                                               witnesses.d_leaf_ids, witnesses.k, witnesses.d_leaves, witnesses.d_siblings,
                                                               witnesses.d_positions, witnesses.d_depths, d_n_bad, d_n_hashed, d_n_bad_witness,
                                                               stream),
                  ctx.get(), "merkle_forest_frontier_append_witness_device");
}
// The state of a BUILT forest (`forest` and d_roots_forest exactly as the build took and filled them), with no digest:
// state.max_leaves >= forest.max_leaves.  A bad tree becomes an empty one and is counted in *d_n_bad.
inline void merkle_forest_frontier_extract_device(const ForestView& forest, const void* d_roots_forest, const ForestFrontier& state,
                                                  unsigned arity = 4, Context& ctx = Context::default_context(), void* d_n_bad = nullptr,
                                                  void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_frontier_extract_device", arity);
    detail::check(m.forest_frontier_extract_device_into(ctx.get(), forest.d_leaves, forest.n_leaves, forest.d_offsets, forest.n_trees,
                                                        forest.max_leaves, forest.d_levels, d_roots_forest, state.max_leaves, state.d_counts,
                                                        state.d_frontier, state.d_roots, d_n_bad, stream),
                  ctx.get(), "merkle_forest_frontier_extract_device");
}

// Consistency proofs (p252_merkle{4,2}_forest_ragged_consistency_device_into / _forest_consistency_verify_device_into): that a tree of a
// built forest, now of n_t leaves, is the tree it was at d_old_counts[i] (uint64) leaves with leaves appended and nothing before them
// changed.  Proof i, for tree d_tree_ids[i] (uint32), is the opening of leaf index n of the tree — `proof` in the layout of
// merkle_forest_ragged_openings_device at the stride forest_openings_stride(forest.max_leaves, arity) — and d_new_counts_out[i] = n_t.
// n == n_t: zeros with the depth of n_t; a tree id out of range, a bad tree, n == 0 or n > n_t: zeros, depth 0xFF, new count 0, counted
// in *d_n_bad.  No digest.
struct ConsistencyProofs {
    void* d_leaves;     // k scalars
    void* d_siblings;   // k x stride x (arity - 1) scalars
    void* d_positions;  // k x stride bytes
    void* d_depths;     // k bytes
    std::size_t stride_depth;
};
inline void merkle_forest_ragged_consistency_device(const ForestView& forest, const void* d_tree_ids, const void* d_old_counts, std::size_t k,
                                                    void* d_new_counts_out, const ConsistencyProofs& proof, unsigned arity = 4,
                                                    Context& ctx = Context::default_context(), void* d_n_bad = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_consistency_device", arity);
    detail::check(m.forest_ragged_consistency_device_into(ctx.get(), forest.d_leaves, forest.n_leaves, forest.d_offsets, forest.n_trees,
                                                          forest.max_leaves, forest.d_levels, d_tree_ids, d_old_counts, k, d_new_counts_out,
                                                          proof.d_leaves, proof.d_siblings, proof.d_positions, proof.d_depths, d_n_bad, stream),
                  ctx.get(), "merkle_forest_ragged_consistency_device");
}
// The check: d_ok[i] = 1 iff proof i re-hashes to the new root and its left siblings alone to the old root, with its slots the digits of
// the old count (the rules: poseidon252_hip.h).  The claims — old count, old root, new count, new root — are element i of the four
// arrays, or element d_tree_ids[i] of arrays of n_trees entries when d_tree_ids is given: the d_counts / d_roots of a ForestFrontier serve
// as the old claims as they stand.  d_old_roots_out / d_new_roots_out receive the recomputed roots, *d_n_hashed the digests computed.
struct ConsistencyClaims {
    const void* d_old_counts;
    const void* d_old_roots;
    const void* d_new_counts;
    const void* d_new_roots;
    const void* d_tree_ids = nullptr;
    std::size_t n_trees = 0;
};
inline void merkle_forest_consistency_verify_device(const ConsistencyClaims& claims, const ConsistencyProofs& proof, std::size_t k, void* d_ok,
                                                    unsigned arity = 4, Context& ctx = Context::default_context(),
                                                    void* d_old_roots_out = nullptr, void* d_new_roots_out = nullptr,
                                                    void* d_n_hashed = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_consistency_verify_device", arity);
    detail::check(m.forest_consistency_verify_device_into(ctx.get(), m.tag().data(), claims.d_old_counts, claims.d_old_roots, claims.d_new_counts,
                                                          claims.d_new_roots, proof.d_leaves, proof.d_siblings, proof.d_positions, proof.d_depths,
                                                          proof.stride_depth, k, claims.d_tree_ids, claims.n_trees, d_ok, d_old_roots_out,
                                                          d_new_roots_out, d_n_hashed, stream),
                  ctx.get(), "merkle_forest_consistency_verify_device");
}

// Anchors (p252_merkle{4,2}_forest_ragged_anchor_openings_device_into): the roots the trees of a built forest had at earlier leaf counts,
// and openings of their leaves against those roots, with no second copy of the forest.  Anchor a is tree d_tree_ids[a] (uint32) at count
// d_counts[a] (uint64): d_roots[a] receives the root of the tree's first c leaves, d_depths[a] (uint8) its depth; a bad anchor (unknown or
// bad tree, c == 0, c > n_t) a zero root, depth 0xFF and one count in *d_n_bad_anchors.  Opening i is leaf d_leaf_ids[i] (uint64) under
// anchor d_anchor_ids[i] (uint32), written into `openings` in the layout of merkle_forest_ragged_openings_device at the stride
// forest_openings_stride(forest.max_leaves, arity), byte for byte what that call writes on a fresh build of the tree's first c leaves;
// a bad opening (anchor id >= m, a bad anchor, leaf id >= c) is zeros with depth 0xFF, counted in *d_n_bad.  *d_n_hashed (device
// uint64, zeroed by the caller) gains the digests the anchors need.  Verification needs nothing new: merkle_forest_ragged_verify_device
// takes the openings with d_tree_ids = d_anchor_ids, d_roots = anchors.d_roots and n_trees = anchors.m.  k == 0: the roots alone.
struct ForestAnchors {
    const void* d_tree_ids;  // m uint32
    const void* d_counts;    // m uint64
    std::size_t m;
    void* d_roots;   // m scalars
    void* d_depths;  // m bytes
};
struct AnchorOpenings {
    void* d_leaves;     // k scalars
    void* d_siblings;   // k x stride x (arity - 1) scalars
    void* d_positions;  // k x stride bytes
    void* d_depths;     // k bytes
};
inline void merkle_forest_ragged_anchor_openings_device(const ForestView& forest, const ForestAnchors& anchors, const void* d_anchor_ids,
                                                        const void* d_leaf_ids, std::size_t k, const AnchorOpenings& openings,
                                                        unsigned arity = 4, Context& ctx = Context::default_context(),
                                                        void* d_n_bad_anchors = nullptr, void* d_n_bad = nullptr, void* d_n_hashed = nullptr,
                                                        void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_anchor_openings_device", arity);
    detail::check(m.forest_ragged_anchor_openings_device_into(ctx.get(), m.tag().data(), forest.d_leaves, forest.n_leaves, forest.d_offsets,
                                                              forest.n_trees, forest.max_leaves, forest.d_levels, anchors.d_tree_ids,
                                                              anchors.d_counts, anchors.m, d_anchor_ids, d_leaf_ids, k, anchors.d_roots,
                                                              anchors.d_depths, openings.d_leaves, openings.d_siblings, openings.d_positions,
                                                              openings.d_depths, d_n_bad_anchors, d_n_bad, d_n_hashed, stream),
                  ctx.get(), "merkle_forest_ragged_anchor_openings_device");
}

// Runs (p252_merkle{4,2}_forest_range_stride, _forest_ragged_range_proofs_device_into, _forest_range_verify_device_into): whole runs of
// leaves [first, first + len) of the trees of a built forest proved by closed-form proofs and checked, many runs of many trees in one
// call.  Run r is tree d_tree_ids[r] (uint32), leaves d_first[r] (uint64) .. with len = d_leaf_offsets[r + 1] - d_leaf_offsets[r]
// (m + 1 uint64, k leaves in all, flat at those offsets).  Row r of the proofs (m rows of merkle_forest_range_stride(max_leaves, arity)
// scalars) is byte for byte the shared proof of merkle_multiproof_device for the run's positions, zeros behind it; a bad run: a zero
// row, length 0xFFFFFFFF, count 0, one count in *d_n_bad.  The verification needs no forest, only the claimed leaf counts.
inline std::size_t merkle_forest_range_stride(std::size_t max_leaves, unsigned arity = 4) {
    return detail::merkle_abi("merkle_forest_range_stride", arity).forest_range_stride(max_leaves);
}
struct ForestRuns {
    const void* d_tree_ids;      // m uint32
    const void* d_first;         // m uint64
    const void* d_leaf_offsets;  // m + 1 uint64
    std::size_t m, k;
};
struct RangeProofs {
    void* d_leaves;      // k scalars (extraction: may be null)
    void* d_proof;       // m x stride scalars
    std::size_t stride;  // scalars a row (extraction writes at merkle_forest_range_stride(forest.max_leaves, arity))
    void* d_proof_lens;  // m uint32
    void* d_counts;      // m uint64: the leaf count of every run's tree
};
inline void merkle_forest_ragged_range_proofs_device(const ForestView& forest, const ForestRuns& runs, const RangeProofs& out, unsigned arity = 4,
                                                     Context& ctx = Context::default_context(), void* d_n_bad = nullptr,
                                                     void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_range_proofs_device", arity);
    detail::check(m.forest_ragged_range_proofs_device_into(ctx.get(), forest.d_leaves, forest.n_leaves, forest.d_offsets, forest.n_trees,
                                                           forest.max_leaves, forest.d_levels, runs.d_tree_ids, runs.d_first,
                                                           runs.d_leaf_offsets, runs.m, runs.k, out.d_leaves, out.d_proof, out.d_proof_lens,
                                                           out.d_counts, d_n_bad, stream),
                  ctx.get(), "merkle_forest_ragged_range_proofs_device");
}
// d_ok[r] (uint8) = 1 iff run r, with its leaves and row r of the proofs, re-hashes to d_roots[d_tree_ids[r]] (n_trees roots)
inline void merkle_forest_range_verify_device(const ForestRuns& runs, const RangeProofs& proofs, std::size_t max_leaves, const void* d_roots,
                                              std::size_t n_trees, void* d_ok, unsigned arity = 4, Context& ctx = Context::default_context(),
                                              void* d_roots_out = nullptr, void* d_n_hashed = nullptr, void* d_n_bad = nullptr,
                                              void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_range_verify_device", arity);
    detail::check(m.forest_range_verify_device_into(ctx.get(), m.tag().data(), runs.d_tree_ids, proofs.d_counts, runs.d_first, runs.d_leaf_offsets,
                                                    runs.m, max_leaves, proofs.d_leaves, runs.k, proofs.d_proof, proofs.stride,
                                                    proofs.d_proof_lens, d_roots, n_trees, d_ok, d_roots_out, d_n_hashed, d_n_bad, stream),
                  ctx.get(), "merkle_forest_range_verify_device");
}

// Sequential updates (p252_merkle{4,2}_forest_ragged_update_sequential_device_into): k leaf updates of a built forest applied IN ORDER in
// one call, the same (tree, leaf) pair any number of times, the forest updated in place as merkle_forest_ragged_update_device does.
// d_order (k uint32) is the indices sorted by (tree id, leaf id, index) — a stable sort by pair (pairs_order_device makes it); this call
// checks it and sorts nothing.  Witness i, in the layout of merkle_forest_ragged_openings_device at stride depth(max_leaves): the leaf as stored just before
// update i, its opening in that state, the tree's root just before and just after.  A bad update: zero rows, depth 0xFF, zero roots,
// one count in *d_n_bad; an invalid order: every depth 0xFF, *d_n_bad += k, nothing else written.
struct SequentialUpdates {
    const void* d_tree_ids;    // k uint32
    const void* d_leaf_ids;    // k uint64
    const void* d_new_leaves;  // k scalars
    const void* d_order;       // k uint32
    std::size_t k;
};
struct SequentialWitnesses {
    void* d_old_leaves;    // k scalars (may be null)
    void* d_siblings;      // k x stride x (arity - 1) scalars
    void* d_positions;     // k x stride bytes
    void* d_depths;        // k bytes
    void* d_roots_before;  // k scalars (may be null)
    void* d_roots_after;   // k scalars
};
inline void merkle_forest_ragged_update_sequential_device(void* d_leaves, std::size_t n_leaves, const void* d_offsets, std::size_t n_trees,
                                                          std::size_t max_leaves, void* d_levels, const SequentialUpdates& updates,
                                                          const SequentialWitnesses& out, unsigned arity = 4,
                                                          Context& ctx = Context::default_context(), void* d_roots = nullptr,
                                                          void* d_n_bad = nullptr, void* d_n_hashed = nullptr, void* stream = nullptr) {
    const detail::MerkleAbi& m = detail::merkle_abi("merkle_forest_ragged_update_sequential_device", arity);
    detail::check(m.forest_ragged_update_sequential_device_into(ctx.get(), m.tag().data(), d_leaves, n_leaves, d_offsets, n_trees, max_leaves,
                                                                d_levels, updates.d_tree_ids, updates.d_leaf_ids, updates.d_new_leaves,
                                                                updates.d_order, updates.k, out.d_old_leaves, out.d_siblings, out.d_positions,
                                                                out.d_depths, out.d_roots_before, out.d_roots_after, d_roots, d_n_bad,
                                                                d_n_hashed, stream),
                  ctx.get(), "merkle_forest_ragged_update_sequential_device");
}

// The order of (tree id, leaf id) pairs, made on the device (p252_pairs_order_device_into, p252_pairs_unique_device_into; no arity):
// pairs_order_device fills d_order (k uint32) — SequentialUpdates::d_order — with the indices sorted by (tree id, leaf id, index);
// pairs_unique_device writes the distinct pairs, ascending, into the first *d_n_unique (a device uint64) entries of every output that
// is not null: what merkle_forest_ragged_multiproof_device takes as its pairs and, with d_indices, merkle_multiproof_device as its
// positions.  d_tree_ids (k uint32) may be null: every pair is of tree 0.  d_leaf_ids: k uint64.  Both parts compare as unsigned.
struct UniquePairs {
    void* d_tree_ids;  // k uint32 (may be null)
    void* d_leaf_ids;  // k uint64 (may be null)
    void* d_indices;   // k uint32, the low word of the leaf id (may be null)
    void* d_first;     // k uint32, the lowest input index that holds the pair (may be null)
    void* d_n_unique;  // one uint64
};
inline void pairs_order_device(const void* d_tree_ids, const void* d_leaf_ids, std::size_t k, void* d_order,
                               Context& ctx = Context::default_context(), void* stream = nullptr) {
    detail::check(p252_pairs_order_device_into(ctx.get(), d_tree_ids, d_leaf_ids, k, d_order, stream), ctx.get(), "pairs_order_device");
}
inline void pairs_unique_device(const void* d_tree_ids, const void* d_leaf_ids, std::size_t k, const UniquePairs& out,
                                Context& ctx = Context::default_context(), void* stream = nullptr) {
    detail::check(p252_pairs_unique_device_into(ctx.get(), d_tree_ids, d_leaf_ids, k, out.d_tree_ids, out.d_leaf_ids, out.d_indices, out.d_first,
                                                out.d_n_unique, stream),
                  ctx.get(), "pairs_unique_device");
}

// `Opening::verify` of the downstream poseidon-merkle consumer (AGENTS.md:62-66) for n device-resident arity-4 openings against ONE
// root: d_ok[i] = 1 iff opening i re-hashes to *d_root (p252_merkle4_verify_batch_device); layouts as p252_merkle4_path_batch_device.
inline void merkle4_verify_batch_device(const void* d_leaves, const void* d_siblings, const void* d_positions, std::size_t depth,
                                        const void* d_root, void* d_ok, std::size_t n, Context& ctx = Context::default_context(),
                                        void* stream = nullptr) {
    const BlsScalar tag = compute_tag(Domain::Merkle4, {4}, 1);
    detail::check(p252_merkle4_verify_batch_device(ctx.get(), tag.data(), d_leaves, d_siblings, d_positions, depth, d_root, d_ok, n, stream),
                  ctx.get(), "merkle4_verify_batch_device");
}

// ---- dusk_poseidon::encrypt / decrypt (src/encryption.rs:62-95), batched; `variant` = P252_CRYPT_STREAM (default) or
// P252_CRYPT_DUPLEX — the construction is UNPINNED.  secrets[i] = {shared.get_u(), shared.get_v()}. ----
struct DecryptionFailed : std::runtime_error {  // dusk_poseidon::Error::DecryptionFailed (src/error.rs:27-29)
    DecryptionFailed() : std::runtime_error("DecryptionFailed") {}
};
inline BlsScalar encryption_tag(std::size_t message_len, int variant = P252_CRYPT_STREAM) {
    BlsScalar t{};
    detail::check(p252_encryption_tag(variant, message_len, t.data()), nullptr, "encryption_tag");
    return t;
}
inline std::vector<BlsScalar> encrypt_batch(const std::vector<BlsScalar>& messages, std::size_t message_len,
                                            const std::vector<BlsScalar>& secrets, const std::vector<BlsScalar>& nonces,
                                            int variant = P252_CRYPT_STREAM, Context& ctx = Context::default_context()) {
    const std::size_t n = nonces.size();
    if (messages.size() != n * message_len || secrets.size() != 2 * n) throw std::invalid_argument("encrypt_batch: sizes");
    const BlsScalar tag = encryption_tag(message_len, variant);
    std::vector<BlsScalar> out(n * (message_len + 1));
    if (n)
        detail::check(p252_encrypt_batch(ctx.get(), variant, tag.data(), messages[0].data(), secrets[0].data(), nonces[0].data(), message_len,
                                         out[0].data(), n),
                      ctx.get(), "encrypt_batch");
    return out;
}
// returns the messages; ok[i] == 0 marks an item whose MAC did not verify (its message is unspecified)
inline std::vector<BlsScalar> decrypt_batch(const std::vector<BlsScalar>& ciphers, std::size_t message_len,
                                            const std::vector<BlsScalar>& secrets, const std::vector<BlsScalar>& nonces,
                                            std::vector<std::uint8_t>& ok, int variant = P252_CRYPT_STREAM,
                                            Context& ctx = Context::default_context()) {
    const std::size_t n = nonces.size();
    if (ciphers.size() != n * (message_len + 1) || secrets.size() != 2 * n) throw std::invalid_argument("decrypt_batch: sizes");
    const BlsScalar tag = encryption_tag(message_len, variant);
    std::vector<BlsScalar> out(n * message_len);
    ok.assign(n, 0);
    if (n)
        detail::check(p252_decrypt_batch(ctx.get(), variant, tag.data(), ciphers[0].data(), secrets[0].data(), nonces[0].data(), message_len,
                                         out[0].data(), ok.data(), n),
                      ctx.get(), "decrypt_batch");
    return out;
}
// single message, the reference's call shape: throws DecryptionFailed like decrypt() returns Err
inline std::vector<BlsScalar> decrypt(const std::vector<BlsScalar>& cipher, const BlsScalar& secret_u, const BlsScalar& secret_v,
                                      const BlsScalar& nonce, int variant = P252_CRYPT_STREAM, Context& ctx = Context::default_context()) {
    if (cipher.size() < 2) throw IoPatternError(IoPatternError::InvalidIOPattern, "decrypt: empty message");
    std::vector<std::uint8_t> ok;
    auto m = decrypt_batch(cipher, cipher.size() - 1, {secret_u, secret_v}, {nonce}, ok, variant, ctx);
    if (!ok[0]) throw DecryptionFailed();
    return m;
}

// ---- messages of DIFFERENT lengths in one call (p252_{encrypt,decrypt}_ragged*): each cipher equals encrypt_batch's at its length.
// One array of n + 1 MESSAGE offsets serves both sides: message i = messages[offsets[i] .. offsets[i+1]), its cipher the L_i + 1
// scalars at ciphers[offsets[i] + i ..].  Lengths 1 .. P252_CRYPT_RAGGED_MAX_LEN. ----
inline std::vector<BlsScalar> encryption_tags(std::size_t max_len, int variant = P252_CRYPT_STREAM) {
    std::vector<BlsScalar> t(max_len ? max_len : 1);
    detail::check(p252_encryption_tags(variant, max_len, t[0].data()), nullptr, "encryption_tags");
    return t;
}
namespace detail {
inline std::size_t ragged_max_len(const std::vector<std::uint64_t>& offsets) {
    std::size_t longest = 1;
    for (std::size_t i = 0; i + 1 < offsets.size(); ++i)
        if (offsets[i + 1] > offsets[i] && offsets[i + 1] - offsets[i] > longest) longest = offsets[i + 1] - offsets[i];
    return longest;
}
}  // namespace detail
// flat messages + offsets -> the flat ciphers (offsets.back() + n scalars); the library checks every length before it launches
inline std::vector<BlsScalar> encrypt_ragged(const std::vector<BlsScalar>& messages, const std::vector<std::uint64_t>& offsets,
                                             const std::vector<BlsScalar>& secrets, const std::vector<BlsScalar>& nonces,
                                             int variant = P252_CRYPT_STREAM, Context& ctx = Context::default_context()) {
    const std::size_t n = nonces.size();
    if (offsets.size() != n + 1 || secrets.size() != 2 * n || (n && offsets.back() > messages.size())) throw std::invalid_argument("encrypt_ragged: sizes");
    if (!n) return {};
    const std::size_t max_len = detail::ragged_max_len(offsets);
    const std::vector<BlsScalar> tags = encryption_tags(max_len, variant);
    std::vector<BlsScalar> out(offsets.back() + n);
    detail::check(p252_encrypt_ragged(ctx.get(), variant, tags[0].data(), max_len, messages.empty() ? nullptr : messages[0].data(), offsets.data(),
                                      secrets[0].data(), nonces[0].data(), out[0].data(), n),
                  ctx.get(), "encrypt_ragged");
    return out;
}
// flat ciphers + the MESSAGE offsets -> the flat messages; ok[i] == 0 marks a message whose MAC did not verify (content unspecified)
inline std::vector<BlsScalar> decrypt_ragged(const std::vector<BlsScalar>& ciphers, const std::vector<std::uint64_t>& offsets,
                                             const std::vector<BlsScalar>& secrets, const std::vector<BlsScalar>& nonces,
                                             std::vector<std::uint8_t>& ok, int variant = P252_CRYPT_STREAM,
                                             Context& ctx = Context::default_context()) {
    const std::size_t n = nonces.size();
    if (offsets.size() != n + 1 || secrets.size() != 2 * n || (n && offsets.back() + n > ciphers.size())) throw std::invalid_argument("decrypt_ragged: sizes");
    ok.assign(n, 0);
    if (!n) return {};
    const std::size_t max_len = detail::ragged_max_len(offsets);
    const std::vector<BlsScalar> tags = encryption_tags(max_len, variant);
    std::vector<BlsScalar> out(offsets.back() ? offsets.back() : 1);
    detail::check(p252_decrypt_ragged(ctx.get(), variant, tags[0].data(), max_len, ciphers[0].data(), offsets.data(), secrets[0].data(),
                                      nonces[0].data(), out[0].data(), ok.data(), n),
                  ctx.get(), "decrypt_ragged");
    out.resize(offsets.back());
    return out;
}
// the same, throwing DecryptionFailed if any MAC failed — what decrypt is to decrypt_batch
inline std::vector<BlsScalar> decrypt_ragged_checked(const std::vector<BlsScalar>& ciphers, const std::vector<std::uint64_t>& offsets,
                                                     const std::vector<BlsScalar>& secrets, const std::vector<BlsScalar>& nonces,
                                                     int variant = P252_CRYPT_STREAM, Context& ctx = Context::default_context()) {
    std::vector<std::uint8_t> ok;
    auto m = decrypt_ragged(ciphers, offsets, secrets, nonces, ok, variant, ctx);
    for (std::uint8_t f : ok)
        if (!f) throw DecryptionFailed();
    return m;
}
// device buffers, asynchronous on `stream`: thin checked wrappers of p252_{encrypt,decrypt}_ragged_device (see poseidon252_hip.h)
inline void encrypt_ragged_device(Context& ctx, int variant, const void* d_tags, std::size_t max_len, const void* d_messages, std::size_t n_scalars,
                                  const void* d_offsets, const void* d_secrets, const void* d_nonces, void* d_ciphers, std::size_t n,
                                  void* d_n_bad = nullptr, void* stream = nullptr) {
    detail::check(p252_encrypt_ragged_device_into(ctx.get(), variant, d_tags, max_len, d_messages, n_scalars, d_offsets, d_secrets, d_nonces, d_ciphers, n,
                                             d_n_bad, stream),
                  ctx.get(), "encrypt_ragged_device");
}
inline void decrypt_ragged_device(Context& ctx, int variant, const void* d_tags, std::size_t max_len, const void* d_ciphers, std::size_t n_scalars,
                                  const void* d_offsets, const void* d_secrets, const void* d_nonces, void* d_messages, void* d_ok, std::size_t n,
                                  void* d_n_bad = nullptr, void* stream = nullptr) {
    detail::check(p252_decrypt_ragged_device_into(ctx.get(), variant, d_tags, max_len, d_ciphers, n_scalars, d_offsets, d_secrets, d_nonces, d_messages, d_ok,
                                             n, d_n_bad, stream),
                  ctx.get(), "decrypt_ragged_device");
}

// ---- the canonical byte format: BlsScalar::to_bytes / from_bytes (src/hades/round_constants.rs:66-67) ----
using ScalarBytes = std::array<std::uint8_t, 32>;  // little-endian bytes of the canonical value
inline std::vector<ScalarBytes> to_bytes(const std::vector<BlsScalar>& scalars) {
    std::vector<ScalarBytes> out(scalars.size());
    if (!scalars.empty()) detail::check(p252_to_bytes(scalars[0].data(), out[0].data(), scalars.size()), nullptr, "to_bytes");
    return out;
}
// ok[i] == 0 where the value is not below the modulus (BlsScalar::from_bytes returns an error there)
inline std::vector<BlsScalar> from_bytes(const std::vector<ScalarBytes>& bytes, std::vector<std::uint8_t>& ok) {
    std::vector<BlsScalar> out(bytes.size());
    ok.assign(bytes.size(), 0);
    if (!bytes.empty()) detail::check(p252_from_bytes(bytes[0].data(), out[0].data(), ok.data(), bytes.size()), nullptr, "from_bytes");
    return out;
}

}  // namespace dusk_poseidon_hip
