/*
 * poseidon252_hip.h — C ABI of libposeidon252_hip.so: batched Poseidon252 (Hades width-5 + SAFE
 * sponge over the BLS12-381 scalar field) on AMD MI355X (gfx950).
 *
 * This is the drop-in boundary for the reference's native hash path.  The reference
 * (dusk-poseidon 0.42) has no FFI of its own; the seam this library replaces is
 *     dusk_poseidon::Hash::{new, update, output_len, finalize, digest}   src/hash.rs:98-195
 *     dusk_poseidon::Domain + From<Domain> for u64                        src/hash.rs:21-56
 *     dusk_safe::Safe<BlsScalar, 5>::permute for ScalarPermutation        src/hades/permutation/scalar.rs:24-27
 * A per-call replacement of Safe::permute would be one permutation per kernel launch, so the
 * boundary is the BATCHED sibling of Hash with identical per-item semantics.  INTEGRATION.md shows
 * the Rust `extern "C"` block and the `HashBatch` wrapper a maintainer would add.
 *
 * Scalars: every `uint64_t*` scalar buffer is an array of BlsScalar in the reference's memory
 * layout — 4 little-endian u64 limbs of the Montgomery residue a*2^256 mod p — so a Rust
 * `&[BlsScalar]` is passed as a pointer with zero conversion.  Callers should pass fully reduced
 * scalars, as the reference holds them.  A scalar whose limbs are >= p (any 256-bit pattern V, up to
 * 2^256 - 1) is hashed / absorbed / encrypted / decrypted as V mod p by every entry point: tags,
 * messages, leaves, siblings, proof nodes, secrets, nonces, cipher elements.  Values that are
 * COMPARED rather than hashed are compared as the 32 bytes they are: the stored MAC of a cipher
 * (p252_decrypt_batch*), the expected root of a verification (p252_merkle{4,2}_verify_batch_device,
 * _forest_ragged_verify_device, _multiproof_verify_device) — MAC + p or root + p is refused, as by the
 * reference, whose scalar equality is limb equality.  Calls that only move scalars (openings and
 * multiproof extraction, the leaves an update stores) copy their bytes.  Outputs that are computed
 * are always fully reduced (bit-exact equality with the reference is limb equality); that includes
 * the root of a one-leaf tree of a ragged forest (the leaf mod p: what re-hashing its opening of
 * depth 0 gives), while the single-tree builds hand a lone leaf back as the 32 bytes it is.
 * tests/test_edge_values_gpu.py holds every hashing kernel to this.
 *
 * Tag: the sponge capacity element state[0] = Safe::tag(...) = BlsScalar::hash_to_scalar(tag_input)
 * (scalar.rs:29-31) is an explicit INPUT of every hashing call.  A Rust caller passes the value
 * computed by the real dusk crates; p252_tag() is a host convenience whose byte-level recipe is
 * not covered by any reference test ("parity unpinned").
 *
 * Device-resident (`*_device`) scalar arrays must be 16-byte aligned (any hipMalloc'ed BlsScalar array, or a
 * whole-scalar offset into one, is); a misaligned pointer returns P252_ERR_INVALID_ARGUMENT.  Input and output
 * arrays of one call must not overlap unless a function says otherwise (inputs are only read, hash.rs:94,118-120).
 * Errors: functions return 0 on success or a negative P252_ERR_*; nothing unwinds across the
 * boundary.  Where the reference panics (Hash::finalize on an invalid io-pattern, hash.rs:124-137)
 * this library returns P252_ERR_IO_PATTERN_VIOLATION / P252_ERR_INVALID_IO_PATTERN and the host
 * wrapper raises.  There is NO CPU fallback: without a usable HIP device every compute entry point
 * fails with P252_ERR_NO_DEVICE / P252_ERR_HIP.
 *
 * Batch size: any n >= 0.  A batch of at most 8,192 items (16,384 Merkle digests) cannot fill the chip and is bound by
 * one wave's latency; such batches run kernels that spread each state over a group of lanes (0.12 ms per permutation
 * instead of 0.17).  Results are the same bytes whichever kernel runs.
 *
 * Threading and streams: a context is bound to one device and its functions are CALLED by one thread at a time; distinct
 * contexts are independent.  The `*_device` entry points only enqueue on the stream they are given, and calls on DIFFERENT
 * streams of one context may overlap on the device: every root-only tree / forest build (d_levels == NULL) ping-pongs its
 * levels in scratch owned by the context PER STREAM (up to four streams at once; a fifth takes over the least recently used
 * scratch behind an event — never concurrently), and a communicator's buffers are handed from one stream to the next behind
 * an event as well.  Memory: that scratch is grow-only and sized by the largest build of its stream — 5/16 of the leaves' bytes
 * (160 MiB for 2^24 leaves, 40 GiB for 2^32) PER stream in use; pass d_levels to keep a build's memory entirely the caller's.  The one context-wide piece of state is the encryption call table: p252_{encrypt,decrypt}_batch_device
 * with another (variant, len) than the previous call drains the device before replacing it.
 * HIP graphs: the `*_device` hashing and tree entry points do nothing but enqueue kernels (and one 32-byte copy) on `hip_stream`, so
 * they can be stream-captured into a hipGraph and replayed on new data in the same buffers; call once outside the capture first
 * (context-owned scratch and the encryption call table are allocated / uploaded on first use, which a capture cannot do).
 * A tree / forest / verify build that is CAPTURED should pass caller-owned scratch (d_levels; for verify: re-hash into a buffer of
 * the caller's with p252_merkle{4,2}_path_batch_device): with d_levels = NULL the graph holds the addresses of the context's
 * per-stream pair and the pair's hand-over event becomes a graph node, so a replay is ordered against nothing the context does
 * later — a fifth stream taking the pair over, p252_trim, a growing build — and would race with it.  The hashing
 * entry points (digests, sponges, permutations, truncated forms) use no context scratch and capture without conditions; the
 * ragged ones (p252_hash_ragged*_device) sort in the per-stream pair as a tree build does.
 * Multi-GPU = one context per GPU: either one process (or thread) per GPU driving its own context,
 * or the p252_*_multi entry points below, which take the array of contexts and shard inside the library; batches
 * shard with no inter-GPU dependence.
 */
#ifndef POSEIDON252_HIP_H
#define POSEIDON252_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this interface.  Bindings compare it with p252_abi_version() of the library they loaded: a function that
 * changes its argument list keeps its name only together with a new number here.
 *   4  p252_encryption_tag / p252_{encrypt,decrypt}_batch[_device] take a leading `int variant`; the default construction
 *      of every wrapper is P252_CRYPT_STREAM (version 0.2 of the library had no selector and computed P252_CRYPT_DUPLEX:
 *      ciphertexts of messages longer than 4 scalars made then decrypt only with variant = P252_CRYPT_DUPLEX)
 *   5  + p252_abi_version, p252_merkle4_update_checked_device, p252_clock_probe_device, p252_staging_lanes; out-of-range
 *      indices of p252_merkle4_update_device are skipped (were undefined behaviour)
 *   6  + the RCCL communicator (p252_comm_*), p252_merkle4_tree_sharded_device, p252_merkle4_tree_multi_device_resident,
 *      p252_merkle4_forest[_device], p252_merkle2_forest_device, p252_merkle{4,2}_openings_device, p252_merkle{4,2}_depth,
 *      p252_merkle2_path_batch_device, P252_ERR_COMM; p252_merkle4_tree_multi_device exchanges the subtree roots with one
 *      ncclAllGather whenever its contexts sit on distinct devices (versions 6 and 7 linked librccl; version 8 resolves it at run time)
 *   7  + p252_hash_batch_truncated[_device] (finalize_truncated fused into the digest kernels' output stage: one launch),
 *      p252_wipe, p252_scratch_residue, p252_merkle{4,2}_verify_batch_device; the host-buffer p252_{encrypt,decrypt}_batch and p252_destroy clear the library-owned
 *      copies of what they were handed; root-only tree / forest builds on DIFFERENT streams of one context no longer share
 *      scratch; p252_merkle4_tree_multi_device accepts any array of contexts again (as ABI 5 did) and makes no communicator for
 *      a single context
 *   8  RCCL is no longer a load-time dependency: the library resolves it on the first p252_comm_* / RCCL-path call (search
 *      order: $P252_RCCL_PATH, a copy the process already holds, the loader's path, $ROCM_PATH/lib), so a single-GPU hashing
 *      deployment needs no RCCL and a process gets ONE copy; + p252_comm_backend (which copy), p252_comm_check (a peer's failed
 *      local build in a sharded tree: the healthy ranks' root becomes all-ones and p252_comm_check / p252_sync return
 *      P252_ERR_COMM — they used to return a garbage root as P252_OK), p252_trim (gives the grow-only scratch back);
 *      p252_scratch_residue no longer counts the encryption call table (it holds nothing of the caller's)
 *   9  + p252_hash_ragged[_truncated][_device]: n messages of different lengths in one call;
 *      + p252_merkle{4,2}_forest_ragged[_device] (additive, same version): trees of different sizes in one call;
 *      + p252_merkle{4,2}_forest_ragged_openings_device, p252_merkle{4,2}_path_ragged_device,
 *      p252_merkle{4,2}_forest_ragged_verify_device (additive, same version): openings out of such a forest in one call;
 *      + p252_merkle{4,2}_forest_ragged_update_device (additive, same version): leaf updates anywhere in such a forest in one
 *      call, each dirty node hashed once;
 *      + p252_merkle{4,2}_forest_ragged_journal_bound, _update_journaled_device_into, _journal_swap_device_into (additive, same
 *      version; `_into`: the journal is the caller's buffer): the same update keeping a journal of what it overwrites, and the swap
 *      that undoes and redoes it with no digest;
 *      + p252_merkle{4,2}_multiproof_bound, p252_merkle{4,2}_multiproof_device, p252_merkle{4,2}_multiproof_verify_device
 *      (additive, same version): many leaves of one tree behind one shared proof, each ancestor hashed once;
 *      + p252_merkle{4,2}_forest_ragged_append_device_into (additive, same version): leaves appended to the trees of such a
 *      forest, written as a new compact forest; unchanged nodes are moved, not hashed again;
 *      + p252_merkle{4,2}_forest_ragged_resize_device_into (additive, same version): the same after each tree was cut to its
 *      first k_t leaves, trailing trees dropped: a rollback, a reorg or a prune without a rebuild;
 *      + p252_merkle{4,2}_forest_ragged_select_device_into (additive, same version): any trees of one or two such forests
 *      gathered into a new compact forest, in any order, with no digest: a prune in the middle, a merge, a split, a reorder;
 *      + p252_merkle{4,2}_forest_ragged_multiproof_bound, _multiproof_device_into, _multiproof_verify_device_into (additive, same
 *      version; `_into` as the append: every result goes into buffers the caller owns):
 *      leaves of many trees of such a forest behind one tree-major shared proof, each ancestor hashed once;
 *      + p252_merkle{4,2}_forest_frontier_bound, _forest_frontier_append_device_into, _forest_frontier_extract_device_into
 *      (additive, same version; `_into`: the state is the caller's three buffers): leaves appended to a forest that is kept only
 *      as its frontiers — a count, a root and depth + 1 short rows per tree — and that state taken out of a built forest;
 *      + p252_merkle{4,2}_forest_frontier_append_witness_device_into (additive, same version): the same append keeping the
 *      openings of marked leaves current, so that such a forest can prove membership without being stored;
 *      + p252_merkle{4,2}_forest_ragged_consistency_device_into, _forest_consistency_verify_device_into (additive, same version;
 *      `_into`: every result goes into buffers the caller owns): the proof that a tree of such a forest is the tree it was at an
 *      older leaf count with leaves appended and nothing before them changed, and its check against the two roots;
 *      + p252_encryption_tags, p252_{encrypt,decrypt}_ragged[_device_into] (additive, same version): encryption and decryption of
 *      messages of different lengths in one call;
 *      + p252_merkle{4,2}_forest_ragged_anchor_openings_device_into (additive, same version; `_into`: every result goes into buffers
 *      the caller owns): the roots the trees of such a forest had at earlier leaf counts, and openings of their leaves against
 *      those roots, with no second copy of the forest;
 *      + p252_merkle{4,2}_forest_range_stride, p252_merkle{4,2}_forest_ragged_range_proofs_device_into,
 *      p252_merkle{4,2}_forest_range_verify_device_into (additive, same version; `_into`: every result goes into buffers the caller
 *      owns): whole runs of leaves [a, b) of the trees of such a forest proved by closed-form proofs and checked, many runs of many
 *      trees in one call;
 *      + p252_merkle{4,2}_forest_ragged_update_sequential_device_into (additive, same version; `_into`: every witness goes into buffers
 *      the caller owns): leaf updates of such a forest applied in order, the same leaf any number of times, each with the leaf it
 *      replaces, that leaf's opening in the state just before it and the root just after it;
 *      + p252_pairs_order_device_into, p252_pairs_unique_device_into (additive, same version; `_into`: every result goes into buffers
 *      the caller owns): the stable sort of (tree id, leaf id) pairs that the sequential updates take as d_order, and the ascending
 *      distinct pairs that the shared proofs take, made on the device by the library itself */
#define P252_ABI_VERSION 9

#define P252_OK 0
#define P252_ERR_IO_PATTERN_VIOLATION (-1) /* dusk_poseidon::Error::IOPatternViolation, src/error.rs:12-14 */
#define P252_ERR_INVALID_IO_PATTERN (-2)   /* dusk_poseidon::Error::InvalidIOPattern,   src/error.rs:16-17 */
#define P252_ERR_INVALID_ARGUMENT (-3)
#define P252_ERR_HIP (-4)
#define P252_ERR_NO_DEVICE (-5)
#define P252_ERR_COMM (-6) /* an RCCL call failed (communicator creation, broadcast of the constants, all-gather of the roots) */

/* Domain discriminants, in the declaration order of `enum Domain` (src/hash.rs:21-36) */
#define P252_DOMAIN_MERKLE4 0
#define P252_DOMAIN_MERKLE2 1
#define P252_DOMAIN_ENCRYPTION 2
#define P252_DOMAIN_OTHER 3

#define P252_HADES_WIDTH 5 /* dusk_poseidon::HADES_WIDTH, src/lib.rs:17 */

typedef struct p252_ctx p252_ctx;
typedef struct p252_comm p252_comm; /* one rank of an RCCL communicator, bound to one context (multi-GPU section below) */
#define P252_COMM_ID_BYTES 128      /* size of the opaque id p252_comm_unique_id produces (= RCCL's ncclUniqueId) */

/* ---- lifecycle ---- */
int p252_device_count(void);
/* Binds to HIP device `device_id`, derives the constant tables from the embedded arc.bin / mds.bin
 * (round_constants.rs:26-54, mds_matrix.rs:17-39) and uploads them. */
int p252_create(int device_id, p252_ctx** out);
void p252_destroy(p252_ctx* ctx);
/* message for the last error on this context (ctx == NULL: last p252_create failure) */
const char* p252_last_error(const p252_ctx* ctx);

/* ---- batched compute, HOST buffers (synchronous; H2D + kernel + D2H) ---- */
/* n independent Hades permutations: replaces Safe::permute / Hades::perm
 * (scalar.rs:25-27, permutation.rs:105-123).  states/out: n x 5 scalars. */
int p252_permute_batch(p252_ctx* ctx, const uint64_t* states, uint64_t* out, size_t n);
/* n independent sponge hashes with the same io-pattern: replaces Hash::finalize (hash.rs:128-155)
 * for n messages of in_len scalars each (contiguous, message-major), out_len outputs each in
 * squeeze order.  Merkle4 digest = (in_len 4, out_len 1).  in_len == 0 or out_len == 0 ->
 * P252_ERR_INVALID_IO_PATTERN. */
int p252_hash_batch(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* in, size_t in_len,
                    size_t out_len, uint64_t* out, size_t n);
/* the same with Hash::finalize_truncated's outputs (hash.rs:164-183): out_raw = n x out_len x 4 raw limbs, canonical value
 * & (2^250 - 1), truncated inside the digest kernel (see p252_hash_batch_truncated_device) */
int p252_hash_batch_truncated(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* in, size_t in_len,
                              size_t out_len, uint64_t* out_raw, size_t n);
/* Arity-4 Merkle tree over Hash::digest(Domain::Merkle4, [c0,c1,c2,c3]) nodes; empty child slots
 * are the zero scalar (hash.rs:22-26).  Levels are built while more than one node remains (a single
 * leaf is its own root; a 4^k-leaf tree costs exactly k levels).  `levels`
 * (optional) receives every level above the leaves, bottom-up, p252_merkle4_levels_len(n_leaves)
 * scalars.  n_leaves == 0 -> P252_ERR_INVALID_ARGUMENT. */
int p252_merkle4_tree(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, size_t n_leaves,
                      uint64_t root[4], uint64_t* levels);
size_t p252_merkle4_levels_len(size_t n_leaves);
/* The same for arity 2: nodes are Hash::digest(Domain::Merkle2, [c0, c1]) (hash.rs:27-31), an odd level is
 * padded with the zero scalar; `tag` must be the Merkle2 tag ([Absorb(2), Squeeze(1)], separator 0x3). */
int p252_merkle2_tree(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, size_t n_leaves,
                      uint64_t root[4], uint64_t* levels);
size_t p252_merkle2_levels_len(size_t n_leaves);

/* Page-locked host memory (hipHostMalloc).  p252_hash_batch pipelines H2D / kernel / D2H for large batches.  With
 * ordinary (pageable) caller memory — a Rust Vec<BlsScalar> — nothing the caller owns is touched: chunks go through
 * library-owned page-locked staging lanes (a worker thread and stream per lane, two chunks in flight per lane;
 * P252_HOST_LANES, default 3; P252_HOST_CHUNK_MB, default 8) so that the host copy of one chunk overlaps the DMA and kernel
 * of the others: 3.5-3.8e8 Merkle4 digests/s host-to-host.  With buffers from p252_host_alloc / p252_host_register on BOTH
 * sides the copies are zero-copy DMA over 3 streams: 4.0e8.  NULL on failure. */
void* p252_host_alloc(size_t bytes);
void p252_host_free(void* p);
/* Page-lock / release a buffer the caller already owns (hipHostRegister / hipHostUnregister) — e.g. a Rust
 * Vec<BlsScalar> that is hashed repeatedly: registered once, every later host-buffer call on it runs at the
 * p252_host_alloc rate instead of paying the per-call page-locking.  The buffer must stay allocated until it is
 * unregistered.  0 or P252_ERR_HIP / P252_ERR_INVALID_ARGUMENT. */
int p252_host_register(void* p, size_t bytes);
int p252_host_unregister(void* p);

/* ---- batched compute, DEVICE buffers (asynchronous on `hip_stream`, a hipStream_t; NULL = the
 * default stream).  Pointers are device addresses with the same layouts as above.  This is the
 * path bench.py times: inputs already resident in HBM. ---- */
int p252_permute_batch_device(p252_ctx* ctx, const void* d_states, void* d_out, size_t n, void* hip_stream);
int p252_hash_batch_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_in, size_t in_len,
                           size_t out_len, void* d_out, size_t n, void* hip_stream);
/* Hash::finalize_truncated / digest_truncated (hash.rs:164-183, 203-210) for the whole batch in ONE launch: the same kernels
 * with a truncating output stage — every squeezed scalar is canonicalised (Montgomery form dropped), masked to its low 250 bits
 * and stored as the raw limbs JubJubScalar::from_raw receives; identical to p252_hash_batch_device followed by
 * p252_truncate250_device without the second launch and the 64 B / scalar round trip through HBM. */
int p252_hash_batch_truncated_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_in, size_t in_len,
                                     size_t out_len, void* d_out_raw, size_t n, void* hip_stream);
/* n independent sponge hashes of DIFFERENT lengths in one call: Hash::digest per message (hash.rs:191-195).
 * Message i = d_in[offsets[i] .. offsets[i+1]) scalars; d_offsets = n + 1 uint64 scalar indices (64-bit, so one array may hold
 * more than 2^32 scalars; 8-byte aligned).  d_tags = max_len scalars (Montgomery limbs like every BlsScalar): a message of
 * length L uses d_tags[L - 1], the tag of [Absorb(L), Squeeze(out_len)] for the caller's domain (p252_tag; since a chunked
 * Hash::update aggregates to the same tag, one table indexed by total length covers every Domain::Other / Domain::Encryption
 * message).  d_out = n x out_len scalars in INPUT order.
 * A message is bad when its length is 0, exceeds max_len, or its offsets decrease (the unsigned difference then wraps above
 * max_len): its out_len output scalars are written as zero, and *d_n_bad (a device uint32 the caller has zeroed; may be NULL) is
 * incremented once per bad message.  Valid neighbours are unaffected.  out_len == 0 -> P252_ERR_INVALID_IO_PATTERN; max_len == 0
 * -> P252_ERR_INVALID_ARGUMENT.
 * Schedule: the messages are sorted by absorb-block count, longest first, on the device (three small kernels) so that the lanes
 * of a wave run the same number of permutations; the order and the bucket counters live in the context's scratch of THIS stream
 * (as the tree builds' levels), so calls on different streams of one context never share it.  P252_RAGGED_SORT=0 (read once per
 * process) hashes in input order instead.  n <= 8,192: eight lanes per message, as every entry point (P252_COOP_MAX_NODES). */
int p252_hash_ragged_device(p252_ctx* ctx, const void* d_tags, size_t max_len, const void* d_in, const void* d_offsets,
                            size_t out_len, void* d_out, size_t n, void* d_n_bad, void* hip_stream);
/* the same with Hash::finalize_truncated's outputs (raw limbs, canonical value & (2^250 - 1)) from the same launch */
int p252_hash_ragged_truncated_device(p252_ctx* ctx, const void* d_tags, size_t max_len, const void* d_in, const void* d_offsets,
                                      size_t out_len, void* d_out_raw, size_t n, void* d_n_bad, void* hip_stream);
/* host-buffer twins (synchronous): offsets and lengths are checked on the host before anything is launched — a zero-length
 * message -> P252_ERR_INVALID_IO_PATTERN, decreasing offsets or a length above max_len -> P252_ERR_INVALID_ARGUMENT (nothing
 * is hashed; p252_last_error names the message).  The messages, tags and offsets are copied through the context's grow-only
 * device scratch in one piece: there is no chunked pipeline over pageable memory as p252_hash_batch has. */
int p252_hash_ragged(p252_ctx* ctx, const uint64_t* tags, size_t max_len, const uint64_t* in, const uint64_t* offsets,
                     size_t out_len, uint64_t* out, size_t n);
int p252_hash_ragged_truncated(p252_ctx* ctx, const uint64_t* tags, size_t max_len, const uint64_t* in, const uint64_t* offsets,
                               size_t out_len, uint64_t* out_raw, size_t n);
/* d_levels may be NULL: the levels then ping-pong in context-owned scratch — one pair per caller stream, so builds queued on
 * different streams of one context never share it (see "Threading and streams"); d_root receives 1 scalar. */
int p252_merkle4_tree_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                             void* d_root, void* d_levels, void* hip_stream);
int p252_merkle2_tree_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                             void* d_root, void* d_levels, void* hip_stream);
/* waits for hip_stream.  P252_ERR_COMM when a sharded tree build of this context's communicator found a failed peer since the
 * last call (see p252_comm_check). */
int p252_sync(p252_ctx* ctx, void* hip_stream);
/* Secret hygiene (the reference builds with `zeroize`, Cargo.toml:14; dusk-safe zeroizes a finished sponge).  The kernels keep
 * sponge states in registers only.  What a HOST-buffer call leaves behind is the library's copy of the caller's arrays — the
 * context's device scratch and the page-locked staging lanes: p252_encrypt_batch / p252_decrypt_batch clear what they used
 * before returning, p252_destroy clears everything before freeing it, and p252_wipe clears every buffer the context owns on
 * demand (it waits for the device first; hashing calls do not wipe — their inputs are public).  `_device` callers own their
 * buffers; the only thing such a call leaves in the context is the (variant, len) call table, which holds no secret. */
int p252_wipe(p252_ctx* ctx);
/* diagnostics: the number of non-zero bytes in every buffer of the context that receives caller data (device scratch, level
 * scratch, staging lanes on both sides; not the encryption call table) — 0 right after p252_wipe, p252_trim or a host-buffer
 * encrypt / decrypt call on a context that has done nothing else since its last wipe */
int p252_scratch_residue(p252_ctx* ctx, uint64_t* nonzero_bytes);
/* The context's scratch is grow-only (device scratch of the host-buffer entry points, up to four per-stream level pairs of
 * 5/16 of a root-only build's leaves each, staging lanes, the call table): p252_trim waits for the device, clears it as p252_wipe
 * does and FREES it — the reference holds no state at all (hash.rs:92-96).  The next call allocates what it needs again.  The
 * constant table and a communicator stay.  Not to be called while a hipGraph captured from this context's root-only builds is
 * still to be replayed: captured builds that pass d_levels = NULL bake the scratch addresses in (pass caller-owned d_levels to
 * builds that are captured, which is also what keeps a replay from racing with another stream's build on the same pair). */
int p252_trim(p252_ctx* ctx);

/* ---- SURVEY §8(f) "next" rows ---- */
/* finalize_truncated's post-processing (hash.rs:164-183) on n device-resident BlsScalars: canonical
 * value & (2^250 - 1), written as the raw limbs JubJubScalar::from_raw receives.  d_out_raw may alias
 * d_scalars. */
int p252_truncate250_device(p252_ctx* ctx, const void* d_scalars, void* d_out_raw, size_t n, void* hip_stream);
/* Incremental update of a stored arity-4 tree (the poseidon-merkle consumer keeps its tree and changes leaves): writes
 * d_new_leaves[i] to d_leaves[d_indices[i]] (k distinct uint32 positions < n_leaves) and re-hashes every ancestor, level by
 * level, in place in d_levels (the layout p252_merkle4_tree_device fills: all levels above the leaves, bottom-up,
 * p252_merkle4_levels_len(n_leaves) scalars).  Cost: log4(n_leaves) launches of k digests; afterwards leaves and levels equal
 * those of a fresh build.  d_root (optional) receives the new root.  An index >= n_leaves is skipped (nothing is written for
 * it).  The positions must be distinct: the same position twice with different values leaves one of them — or, the two
 * 16-byte halves of a scalar being stored separately, a mix — in the leaf, and the levels above consistent with whatever
 * was stored.  The _checked variant additionally counts the skipped indices: *d_n_bad (a device uint32 the caller has
 * zeroed) is incremented once per out-of-range index. */
int p252_merkle4_update_device(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, void* d_levels,
                               const void* d_indices, const void* d_new_leaves, size_t k, void* d_root, void* hip_stream);
int p252_merkle4_update_checked_device(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, void* d_levels,
                                       const void* d_indices, const void* d_new_leaves, size_t k, void* d_root, void* d_n_bad,
                                       void* hip_stream);
/* The canonical byte format on either side of the path: BlsScalar::to_bytes / from_bytes (dusk-bls12_381; the reference
 * round-trips its round constants through the pair, src/hades/round_constants.rs:66-67, and reads its KAT inputs with
 * from_hex_str, src/hades.rs:131).  bytes = n records of 32 little-endian bytes of the canonical value (16-byte aligned
 * on the device).  from_bytes: ok[i] = 1 iff the value is < p — BlsScalar::from_bytes fails otherwise; the limbs written
 * are then those of the value mod p; ok may be NULL.  Buffers may alias (in place). */
int p252_to_bytes_device(p252_ctx* ctx, const void* d_scalars, void* d_bytes, size_t n, void* hip_stream);
int p252_from_bytes_device(p252_ctx* ctx, const void* d_bytes, void* d_scalars, void* d_ok, size_t n, void* hip_stream);
/* Batched Merkle openings (arity 4): recompute the root from a leaf and its sibling path — the branch
 * re-hash a `poseidon-merkle` verifier performs (AGENTS.md:62-66 names the downstream crate).  Per
 * level l, node = Hash::digest(Domain::Merkle4, children) where children[positions[l]] is the value
 * coming from below and the 3 siblings fill the other slots in order.  Layouts: leaves[n],
 * siblings[n][depth][3] scalars, positions[n][depth] bytes in 0..3, roots[n].  depth == 0 copies the
 * leaves.  positions outside 0..3 -> P252_ERR_INVALID_ARGUMENT (host variant; the device variant masks).
 * THE POSITION BYTE (every device call that re-hashes an opening: p252_merkle{4,2}_path_batch_device, _path_ragged_device,
 * _verify_batch_device, _forest_ragged_verify_device): only the low two bits of a position byte are read (arity 2: the low bit), so
 * a byte of 5 re-hashes — and verifies — as 1; the extraction calls write values below the arity only.  A caller for whom the
 * byte itself is a claim must check its high bits.  p252_merkle{4,2}_forest_consistency_verify_device_into alone compares whole
 * bytes: a position byte with a high bit set is refused there. */
int p252_merkle4_path_batch(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, const uint64_t* siblings,
                            const uint8_t* positions, size_t depth, uint64_t* roots, size_t n);
int p252_merkle4_path_batch_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, const void* d_siblings,
                                   const void* d_positions, size_t depth, void* d_roots, size_t n, void* hip_stream);

/* Batched encryption / decryption: replaces dusk_poseidon::encrypt / decrypt (src/encryption.rs:62-95),
 * thin wrappers over dusk_safe::encrypt / decrypt with ScalarPermutation and Domain::Encryption.  Per
 * item: message of `len` scalars, shared secret = the 2 coordinates (u, v) of the JubJub shared point as
 * BlsScalars (encryption.rs:66-69), nonce = 1 scalar; cipher = len + 1 scalars (masked message + MAC).
 * Layouts: messages[n][len], secrets[n][2], nonces[n], ciphers[n][len+1], ok[n] bytes (1 = MAC verified;
 * 0 = dusk_poseidon::Error::DecryptionFailed, src/error.rs:27-29, and that item's message output is
 * unspecified).
 *
 * `variant` selects the sponge-call sequence.  dusk-safe 0.3 is not vendored in the reference and the reference's
 * tests (tests/encryption.rs:30-115, message lengths 42 and 21) are round trips and failures only, so NO reference
 * value pins the construction; both candidates run on the KAT-pinned sponge state machine, and the library, its
 * p252_encryption_tag() and the test oracle all derive from one call table per variant:
 *   P252_CRYPT_STREAM (0, the default of every wrapper — dusk-safe's encrypt as published, to the best of three
 *       independent recollections): io-pattern [Absorb(2), Absorb(1), Squeeze(len), Absorb(len), Squeeze(1)]:
 *       absorb secret, absorb nonce, squeeze ALL len masks, absorb the whole message, squeeze the MAC;
 *       cipher[i] = message[i] + mask[i], cipher[len] = MAC.
 *   P252_CRYPT_DUPLEX (1, what version 0.2 of this library shipped): [Absorb(2), Absorb(1), {Squeeze(c), Absorb(c)}*,
 *       Squeeze(1)] with c = min(4, remaining): squeeze / absorb chunk by chunk.
 * The two are identical for len <= 4 and differ beyond.  bindings/rust/tests/parity.rs decides between them on a
 * machine with the dusk crates.  `tag` as everywhere: pass the real crate's value, or p252_encryption_tag() (UNPINNED). */
#define P252_CRYPT_STREAM 0
#define P252_CRYPT_DUPLEX 1
int p252_encryption_tag(int variant, size_t message_len, uint64_t tag_out[4]);
int p252_encrypt_batch(p252_ctx* ctx, int variant, const uint64_t tag[4], const uint64_t* messages, const uint64_t* secrets,
                       const uint64_t* nonces, size_t len, uint64_t* ciphers, size_t n);
int p252_decrypt_batch(p252_ctx* ctx, int variant, const uint64_t tag[4], const uint64_t* ciphers, const uint64_t* secrets,
                       const uint64_t* nonces, size_t len, uint64_t* messages, uint8_t* ok, size_t n);
int p252_encrypt_batch_device(p252_ctx* ctx, int variant, const uint64_t tag[4], const void* d_messages, const void* d_secrets,
                              const void* d_nonces, size_t len, void* d_ciphers, size_t n, void* hip_stream);
int p252_decrypt_batch_device(p252_ctx* ctx, int variant, const uint64_t tag[4], const void* d_ciphers, const void* d_secrets,
                              const void* d_nonces, size_t len, void* d_messages, void* d_ok, size_t n, void* hip_stream);

/* The same for n messages of DIFFERENT lengths in one call (the reference's encrypt / decrypt take a message of any length).
 * Layout: ONE array of n + 1 uint64 MESSAGE offsets serves both directions: message i = messages[offsets[i] .. offsets[i+1])
 * (L_i scalars), its cipher the L_i + 1 scalars at ciphers[offsets[i] + i ..] — the cipher array holds n_scalars + n scalars and
 * needs no offsets of its own; secrets[n][2], nonces[n], ok[n] bytes as above.  tags: max_len scalars, row L - 1 the tag of a
 * message of L scalars (p252_encryption_tags fills it; a wrong table gives wrong ciphertexts, as a wrong `tag` does above).
 * 1 <= max_len <= P252_CRYPT_RAGGED_MAX_LEN: the schedule keeps one counter per length (longer messages stay with the
 * fixed-length call).  Every message's bytes are those of the fixed-length call at its length.
 *
 * `_device_into` (every result goes into buffers the caller owns, as the forest calls of that name): asynchronous on hip_stream, no
 * host synchronisation, no allocation once the stream's scratch is warm.  n_scalars = the
 * scalars of the message-side array.  Message i is BAD iff offsets[i+1] <= offsets[i] (empty or decreasing), L_i > max_len, or
 * offsets[i+1] > n_scalars: it is counted once in *d_n_bad (a uint32 the caller has zeroed; may be NULL), its output region is left
 * untouched, decrypt sets ok[i] = 0, nothing is read or written through it and its neighbours are unaffected.  Badness depends
 * on the offsets alone, so a caller can find the bad messages itself.  Where offsets that are not non-decreasing make the regions of
 * two valid messages overlap, the contents there are unspecified but stay inside the buffers.  Refused with
 * P252_ERR_INVALID_ARGUMENT: max_len of 0 or above the cap, an unknown variant, a NULL or misaligned buffer (scalars 16 bytes,
 * offsets 8, d_n_bad 4), a size overflow (n_scalars + n included), an output that overlaps any input — in-place use is not
 * possible, the two sides are shifted against each other.  n == 0: P252_OK, nothing enqueued.
 *
 * Host twins: synchronous; the offsets are checked before anything is launched (an empty message: P252_ERR_INVALID_IO_PATTERN;
 * decreasing offsets or a length above max_len: P252_ERR_INVALID_ARGUMENT; p252_last_error names the message), and every
 * library-owned copy of what they were handed is cleared before they return, as p252_{encrypt,decrypt}_batch do. */
#define P252_CRYPT_RAGGED_MAX_LEN 2048
int p252_encryption_tags(int variant, size_t max_len, uint64_t* tags_out); /* row L-1 = p252_encryption_tag(variant, L) */
int p252_encrypt_ragged_device_into(p252_ctx* ctx, int variant, const void* d_tags, size_t max_len, const void* d_messages, size_t n_scalars,
                               const void* d_offsets, const void* d_secrets, const void* d_nonces, void* d_ciphers, size_t n,
                               void* d_n_bad, void* hip_stream);
int p252_decrypt_ragged_device_into(p252_ctx* ctx, int variant, const void* d_tags, size_t max_len, const void* d_ciphers, size_t n_scalars,
                               const void* d_offsets, const void* d_secrets, const void* d_nonces, void* d_messages, void* d_ok, size_t n,
                               void* d_n_bad, void* hip_stream);
int p252_encrypt_ragged(p252_ctx* ctx, int variant, const uint64_t* tags, size_t max_len, const uint64_t* messages, const uint64_t* offsets,
                        const uint64_t* secrets, const uint64_t* nonces, uint64_t* ciphers, size_t n);
int p252_decrypt_ragged(p252_ctx* ctx, int variant, const uint64_t* tags, size_t max_len, const uint64_t* ciphers, const uint64_t* offsets,
                        const uint64_t* secrets, const uint64_t* nonces, uint64_t* messages, uint8_t* ok, size_t n);

/* Openings of a STORED tree, extracted on the device (no hashing; HBM-bound data movement): d_leaves[n_leaves] and d_levels as
 * p252_merkle4_tree_device filled them (all levels, bottom-up); d_indices = k leaf positions (uint32, device).  Writes, in exactly
 * the layout p252_merkle4_path_batch_device reads: d_leaves_out[k] (the leaves at those positions), d_siblings[k][depth][3],
 * d_positions[k][depth] with depth = p252_merkle4_depth(n_leaves); missing siblings of a ragged level are the zero scalar
 * (hash.rs:22-26).  A position >= n_leaves yields an all-zero opening and is counted in *d_n_bad (uint32, device; may be NULL).
 * Re-hashing the result with p252_merkle4_path_batch_device gives the tree's root for every valid position.  Asynchronous. */
size_t p252_merkle4_depth(size_t n_leaves);
int p252_merkle4_openings_device(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_levels, const void* d_indices, size_t k,
                                 void* d_leaves_out, void* d_siblings, void* d_positions, void* d_n_bad, void* hip_stream);
/* The arity-2 twins (Domain::Merkle2 trees as p252_merkle2_tree_device builds them; pass the Merkle2 tag): ONE sibling per level —
 * d_siblings[k][depth], d_positions[k][depth] in 0..1 (1 = the path's node is the right child), depth = p252_merkle2_depth(n_leaves);
 * p252_merkle2_path_batch_device re-hashes n such openings (depth sequential Hash::digest(Domain::Merkle2, [left, right]) per lane); of a
 * position byte it reads the low bit only (THE POSITION BYTE, at p252_merkle4_path_batch_device). */
size_t p252_merkle2_depth(size_t n_leaves);
int p252_merkle2_openings_device(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_levels, const void* d_indices, size_t k,
                                 void* d_leaves_out, void* d_siblings, void* d_positions, void* d_n_bad, void* hip_stream);
int p252_merkle2_path_batch_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, const void* d_siblings,
                                   const void* d_positions, size_t depth, void* d_roots, size_t n, void* hip_stream);

/* Opening::verify in bulk (the downstream poseidon-merkle verifier, AGENTS.md:62-66): the n openings are re-hashed exactly as
 * p252_merkle{4,2}_path_batch_device does and each result is compared with the ONE expected root at d_root (32 bytes, device):
 * d_ok[i] = 1 iff opening i leads to that root — n bytes leave the device instead of n x 32.  Position bytes are masked as there
 * (THE POSITION BYTE, at p252_merkle4_path_batch_device).  The recomputed roots live in the context's scratch of `hip_stream`.
 * Asynchronous. */
int p252_merkle4_verify_batch_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, const void* d_siblings,
                                     const void* d_positions, size_t depth, const void* d_root, void* d_ok, size_t n, void* hip_stream);
int p252_merkle2_verify_batch_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, const void* d_siblings,
                                     const void* d_positions, size_t depth, const void* d_root, void* d_ok, size_t n, void* hip_stream);

/* A FOREST of n_trees independent complete arity-4 trees of leaves_per_tree = 4^k leaves each (the downstream poseidon-merkle
 * shape, AGENTS.md:62-66: many small trees), tree-major in d_leaves.  Level l of all trees is one array of
 * n_trees * 4^(k-l) nodes, tree-major, and each level is ONE launch across all trees — the narrow upper levels of many small
 * trees fill the chip together instead of each tree paying one wave's latency per level (k launches instead of
 * n_trees * k).  d_roots[n_trees] (device) receives tree t's root at index t: identical to p252_merkle4_tree_device of
 * that tree alone.  d_levels (device, may be NULL): all levels bottom-up, level-major —
 * n_trees * p252_merkle4_levels_len(leaves_per_tree) scalars, level l at offset n_trees * (4^(k-1) + ... + 4^(k-l+1)),
 * tree t's nodes of that level at t * 4^(k-l) within it.  Asynchronous on hip_stream. */
int p252_merkle4_forest_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_trees, size_t leaves_per_tree,
                               void* d_roots, void* d_levels, void* hip_stream);
/* the same from HOST leaves (pageable memory is fine), roots to host memory: the first level — three quarters of the work — is hashed
 * chunk by chunk while the leaves stream in through the context's staging lanes (the leaves are never resident as a whole), the
 * upper levels then run once, one launch per level across all trees; synchronous */
int p252_merkle4_forest(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, size_t n_trees, size_t leaves_per_tree,
                        uint64_t* roots);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag): leaves_per_tree = 2^k, p252_merkle2_levels_len per tree */
int p252_merkle2_forest_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_trees, size_t leaves_per_tree,
                               void* d_roots, void* d_levels, void* hip_stream);

/* A forest of n_trees trees of DIFFERENT sizes in one call.  Tree t = d_leaves[offsets[t] .. offsets[t+1]) (n_trees + 1 uint64
 * offsets, device, 8-byte aligned; offsets[0] need not be 0), n_t = offsets[t+1] - offsets[t] leaves; n_leaves = the length of
 * d_leaves in scalars.  d_roots[t] (device) = what p252_merkle4_tree returns for those leaves (each level zero-padded to a multiple
 * of the arity, a single leaf is its own root).  Each level is ONE launch across all trees, as in p252_merkle4_forest_device.
 * d_levels (device, may be NULL = roots only) is TREE-MAJOR, unlike the level-major layout of p252_merkle4_forest_device: tree t's
 * block starts at LO[t] = the sum over good trees s < t of p252_merkle4_levels_len(n_s) and holds byte for byte what
 * p252_merkle4_tree writes for it alone — so a tree's block goes unchanged into p252_merkle4_openings_device, the verify calls and
 * p252_merkle4_update_device (one tree per call; p252_merkle{4,2}_forest_ragged_update_device below updates leaves of any number
 * of trees in one).  A caller with device-only offsets can size d_levels as
 * n_leaves / 3 + n_trees * p252_merkle4_depth(max_leaves) scalars.
 * A tree is bad when n_t == 0, n_t > max_leaves, its offsets decrease, offsets[t+1] > n_leaves, or n_t plus the leaf counts of the
 * trees before it that pass those checks exceed n_leaves (only possible when trees overlap behind decreasing offsets): its root is
 * written as zero, it has no level storage, and *d_n_bad (device uint32 the caller has zeroed; may be NULL) is incremented once per
 * bad tree.  Good trees are unaffected.  max_leaves == 0 -> P252_ERR_INVALID_ARGUMENT; n_trees == 0 -> P252_OK, nothing enqueued.
 * The bookkeeping (scans over the trees) and, without d_levels, the level ping-pong live in the context's scratch of THIS stream
 * (p252_trim / p252_wipe cover it).  Asynchronous on hip_stream: no host synchronisation, no allocation once that scratch is
 * warm — it can be captured into a hipGraph. */
int p252_merkle4_forest_ragged_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                      const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_roots, void* d_levels,
                                      void* d_n_bad, void* hip_stream);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag): p252_merkle2_levels_len per tree, d_levels bound
 * n_leaves + n_trees * p252_merkle2_depth(max_leaves) */
int p252_merkle2_forest_ragged_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                      const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_roots, void* d_levels,
                                      void* d_n_bad, void* hip_stream);
/* host-buffer twins (synchronous): leaves = the scalars offsets[0] .. offsets[n_trees]; every tree is checked first — an empty tree
 * or decreasing offsets -> P252_ERR_INVALID_ARGUMENT (nothing is hashed; p252_last_error names the tree).  roots[n_trees];
 * levels (may be NULL): the tree-major layout above, sum of p252_merkle{4,2}_levels_len(n_t) scalars.  The leaves and offsets go
 * through the context's grow-only device scratch in one piece: there is no chunked pipeline over pageable memory. */
int p252_merkle4_forest_ragged(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, const uint64_t* offsets,
                               size_t n_trees, uint64_t* roots, uint64_t* levels);
int p252_merkle2_forest_ragged(p252_ctx* ctx, const uint64_t tag[4], const uint64_t* leaves, const uint64_t* offsets,
                               size_t n_trees, uint64_t* roots, uint64_t* levels);

/* Openings out of such a forest in one call (no hashing).  d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels: exactly
 * what p252_merkle{4,2}_forest_ragged_device was given (d_levels, tree-major, is required unless every tree is a single leaf; all
 * three sizes > 0).  The call recomputes the per-tree leaf counts and block starts with the build's own validation and scan, so a
 * bad tree means the same in both and nothing is needed from the host.  Opening i = leaf d_leaf_ids[i] (uint64, a position inside
 * the tree) of tree d_tree_ids[i] (uint32); k of each, device.  Every output uses the stride D = p252_merkle4_depth(max_leaves):
 * d_leaves_out[k], d_siblings[k][D][3], d_positions[k][D], d_depths[k] (uint8) = p252_merkle4_depth(n_t).  Rows l < d_depths[i] of
 * opening i are byte for byte what p252_merkle4_openings_device writes for that tree's block alone; rows at or past it are zero.
 * A bad opening (tree id >= n_trees, a bad tree, leaf id >= n_t) is all zero with d_depths[i] = 0xFF — the re-hash and verify calls
 * below refuse that depth, so a zero leaf never "verifies" against a bad tree's zero root — and is counted once in *d_n_bad (device
 * uint32 the caller has zeroed; may be NULL).  D == 0 copies the leaves.  k == 0 -> P252_OK, nothing enqueued.  The forest's index
 * and one 32-byte record per opening live in the context's scratch of THIS stream.  Asynchronous, no host synchronisation, no
 * allocation once that scratch is warm. */
int p252_merkle4_forest_ragged_openings_device(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                                               size_t max_leaves, const void* d_levels, const void* d_tree_ids, const void* d_leaf_ids,
                                               size_t k, void* d_leaves_out, void* d_siblings, void* d_positions, void* d_depths,
                                               void* d_n_bad, void* hip_stream);
/* arity 2: d_siblings[k][D] with D = p252_merkle2_depth(max_leaves), positions in 0..1 */
int p252_merkle2_forest_ragged_openings_device(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                                               size_t max_leaves, const void* d_levels, const void* d_tree_ids, const void* d_leaf_ids,
                                               size_t k, void* d_leaves_out, void* d_siblings, void* d_positions, void* d_depths,
                                               void* d_n_bad, void* hip_stream);
/* The re-hash with a depth per opening: d_roots_out[i] = the root recomputed from the first d_depths[i] levels of opening i (the
 * layout above at stride_depth <= 64; the rows past the depth are not read; position bytes are masked: THE POSITION BYTE, at
 * p252_merkle4_path_batch_device).  d_depths[i] == 0 copies the leaf; d_depths[i] >
 * stride_depth (the 0xFF of a bad opening included) writes a zero root and is counted in *d_n_bad (zeroed by the caller; may be
 * NULL).  With d_depths[i] == stride_depth everywhere the roots are those of p252_merkle{4,2}_path_batch_device.  The openings are
 * sorted by depth on the device first (a wave runs to its deepest lane; P252_RAGGED_SORT=0 turns that off); the order lives in the
 * context's scratch of this stream.  Asynchronous. */
int p252_merkle4_path_ragged_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings,
                                    const void* d_positions, const void* d_depths, size_t stride_depth, void* d_roots_out, size_t k,
                                    void* d_n_bad, void* hip_stream);
int p252_merkle2_path_ragged_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings,
                                    const void* d_positions, const void* d_depths, size_t stride_depth, void* d_roots_out, size_t k,
                                    void* d_n_bad, void* hip_stream);
/* Opening::verify across a forest: d_ok[i] = 1 iff d_depths[i] <= stride_depth, d_tree_ids[i] < n_trees and opening i re-hashes to
 * d_roots[d_tree_ids[i]] (the n_trees roots of the build, device) — k bytes leave the device; the re-hash is that of
 * p252_merkle{4,2}_path_ragged_device, masked position bytes included.  The recomputed roots live in the
 * context's scratch of this stream, as in p252_merkle{4,2}_verify_batch_device.  Asynchronous. */
int p252_merkle4_forest_ragged_verify_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings,
                                             const void* d_positions, const void* d_depths, size_t stride_depth, const void* d_tree_ids,
                                             const void* d_roots, size_t n_trees, void* d_ok, size_t k, void* hip_stream);
int p252_merkle2_forest_ragged_verify_device(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves_in, const void* d_siblings,
                                             const void* d_positions, const void* d_depths, size_t stride_depth, const void* d_tree_ids,
                                             const void* d_roots, size_t n_trees, void* d_ok, size_t k, void* hip_stream);

/* Leaf updates anywhere in such a forest in one call.  d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels: exactly what
 * p252_merkle{4,2}_forest_ragged_device was given (d_levels, tree-major, is required unless every tree is a single leaf; all three
 * sizes > 0); the per-tree leaf counts and block starts are recomputed with the build's own validation and scans, as the openings
 * call does, so a bad tree means the same in all three and nothing is needed from the host.  Update i writes d_new_leaves[i] (one
 * scalar) to leaf d_leaf_ids[i] (uint64, a position inside the tree) of tree d_tree_ids[i] (uint32); k of each, device.  Then every
 * ancestor of a changed leaf is re-hashed, level by level, in place in its tree's block — each dirty node ONCE, however many
 * updates lie below it (p252_merkle4_update_device hashes k nodes on every level).  Afterwards d_leaves and the used part of
 * d_levels are byte for byte what a fresh p252_merkle{4,2}_forest_ragged_device build of the modified leaves writes; nothing
 * outside the touched trees' blocks and nothing past the used length of d_levels is written.  d_roots (device, n_trees scalars,
 * may be NULL): entry t is rewritten for every tree that received a valid update (a single-leaf tree's root is its leaf), the
 * other entries are left alone.  A bad update (tree id >= n_trees, a bad tree, leaf id >= n_t) writes nothing and is counted once
 * in *d_n_bad (device uint32 the caller has zeroed; may be NULL).  The (tree, leaf) pairs must be distinct, with the contract of
 * p252_merkle4_update_device: the same pair twice with the same value is harmless; with different values one of them (or a mix of
 * their 16-byte halves) lands and the levels are consistent with whatever was stored.  *d_n_hashed (device uint64 the caller has
 * zeroed, 8-byte aligned; may be NULL) is incremented by the number of node digests computed = the number of DISTINCT dirty
 * ancestors.  k == 0 -> P252_OK, nothing enqueued.  Scratch, in the context's pair of THIS stream (p252_trim / p252_wipe cover
 * it): the forest's index (16 bytes per tree) and ids only, never a copy of the new leaves — two 16-byte records and at most
 * 32 bytes of claim table per update, i.e. at most 64 bytes per update plus 1 KiB, whatever the size of the forest.
 * Asynchronous on hip_stream: no host synchronisation, no allocation once that scratch is warm — it can be captured into a
 * hipGraph (it holds memset nodes).  Cost: three graph nodes per level, so for a handful of updates of ONE tree
 * p252_merkle4_update_device (one launch per level) is quicker; measured on one 4^12-leaf tree (profiles/forest_update.txt) this
 * call wins from about 2^16 updates (1.1x; 4.2x at 2^20), and above ~N/4 changed leaves of a tree of N, rebuild: a fresh build is
 * then as quick (1.07x at N/4) or quicker (the update takes 1.4x the build's time at k = N).  There is no host-buffer twin: the
 * call acts on a forest that lives on the device. */
int p252_merkle4_forest_ragged_update_device(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, const void* d_offsets,
                                             size_t n_trees, size_t max_leaves, void* d_levels, const void* d_tree_ids,
                                             const void* d_leaf_ids, const void* d_new_leaves, size_t k, void* d_roots, void* d_n_bad,
                                             void* d_n_hashed, void* hip_stream);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag) */
int p252_merkle2_forest_ragged_update_device(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves, const void* d_offsets,
                                             size_t n_trees, size_t max_leaves, void* d_levels, const void* d_tree_ids,
                                             const void* d_leaf_ids, const void* d_new_leaves, size_t k, void* d_roots, void* d_n_bad,
                                             void* d_n_hashed, void* hip_stream);

/* The same update with a JOURNAL, and the swap that plays the journal back: leaving an update again (an orphaned block) and entering
 * it again, without the old leaves and without one digest.  p252_merkle{4,2}_forest_ragged_journal_bound (host, no context): the most
 * journal entries one call with k updates writes, k + the sum over l = 1 .. depth of min(k, n_leaves / arity^l + n_trees), depth =
 * that of a tree of min(max_leaves, n_leaves) leaves; 0 when any of the four sizes is 0, SIZE_MAX when the sum overflows. */
size_t p252_merkle4_forest_ragged_journal_bound(size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);
size_t p252_merkle2_forest_ragged_journal_bound(size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);
/* The journaled update: every argument up to d_n_hashed is the plain update's, in its order and with its meaning, with ONE tightening:
 * the (tree, leaf) pairs go through a claim table at level 0 as the dirty nodes of every upper level do, keyed by the leaf's slot in
 * d_leaves.  Of a pair given several times exactly one update is applied, as a whole scalar, never a mix of halves; the others are
 * dropped and NOT counted in *d_n_bad (which counts what the plain update counts).  (Two good trees whose ranges overlap share
 * slots: of two updates of one slot one is applied, and its tree alone is re-hashed.)  *d_n_hashed means what it means there.
 * The journal, owned by the caller: d_journal_ids (device, 16 bytes per entry, 16-byte aligned), d_journal_values (device, 32 bytes
 * per entry, 16-byte aligned), journal_cap = their capacity in entries, d_journal_len (device uint64, 8-byte aligned, REQUIRED; the
 * call sets it, the caller need not zero it).  journal_cap < p252_merkle{4,2}_forest_ragged_journal_bound(n_leaves, n_trees,
 * max_leaves, k) -> P252_ERR_INVALID_ARGUMENT, nothing enqueued: the device can never run past the journal.  An entry is written
 * for the old 32 bytes of every leaf and every node the call overwrites, BEFORE the overwrite: id = four uint32 {tree id, level + 1,
 * node index low, node index high} (level 0 = the leaves; an all-zero id is void), value = the raw bytes that were stored (a leaf
 * keeps its bytes unreduced, as the build leaves it).  Entries are compact, 0 .. *d_journal_len - 1, the leaves first, then level
 * by level; the order within a level is unspecified; entries past the length are not written.  Entries name DISTINCT nodes, and
 * *d_journal_len = the distinct valid pairs + what *d_n_hashed grows by.  Roots are not journalled: a tree's top node (the leaf of
 * a one-leaf tree) stands for its root.  k == 0 -> P252_OK, *d_journal_len = 0.  As the plain update: asynchronous on hip_stream,
 * no host synchronisation, no allocation once the scratch is warm (the plain update's scratch, in the pair of THIS stream),
 * capturable on one stream (it holds memset nodes), at most three graph nodes per level plus the leaf stage.
 * Measured: profiles/forest_journal.txt. */
int p252_merkle4_forest_ragged_update_journaled_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves,
                                                       const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels,
                                                       const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves, size_t k,
                                                       void* d_roots, void* d_n_bad, void* d_n_hashed, void* d_journal_ids,
                                                       void* d_journal_values, size_t journal_cap, void* d_journal_len, void* hip_stream);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag) */
int p252_merkle2_forest_ragged_update_journaled_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves,
                                                       const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels,
                                                       const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves, size_t k,
                                                       void* d_roots, void* d_n_bad, void* d_n_hashed, void* d_journal_ids,
                                                       void* d_journal_values, size_t journal_cap, void* d_journal_len, void* hip_stream);
/* The swap.  There is no tag: nothing is hashed, the arity only selects the level layout.  For every entry g < min(*d_journal_len,
 * journal_cap) the entry's 32 bytes and the 32 bytes of the node it names change places: the forest gets the journal's value, the
 * journal the forest's.  d_roots (device, n_trees scalars, may be NULL): an entry that is its tree's top also rewrites d_roots[t] —
 * the node's bytes, or for a one-leaf tree the restored leaf reduced, as the update writes it.  After one swap d_leaves, the used
 * part of d_levels and the roots of the touched trees are byte for byte what they were before the journaled update; after a second
 * swap, what they were after it.  The ids and the length never change.  Journals STACK: updates A then B are undone by swap(B),
 * swap(A) and redone by swap(A), swap(B); any other order is the caller's error, and still writes only inside the forest.
 * A JOURNAL IS ONLY MEANINGFUL FOR THE FOREST SHAPE (d_offsets) IT WAS TAKEN ON: the append and resize calls produce a new forest
 * and void every older journal.  The ids are the caller's data, so each is checked against the forest's own index (recomputed as the
 * update recomputes it): an entry writes nothing and is counted once in *d_n_bad (device uint32 the caller has zeroed; may be NULL)
 * when its id is void, its tree id >= n_trees, its tree is a bad tree, its level is above the tree's depth, or its node index is at
 * or past the level's node count.  Ids that name one node twice (no journal of the update does) race with each other inside that
 * node.  The launch is sized by journal_cap and leaves on the device-side length: an all-void or zero-length journal is P252_OK, and
 * journal_cap == 0 enqueues nothing.  d_journal_len is required and read only.  Asynchronous on hip_stream, no host synchronisation,
 * no allocation once the scratch (the forest's index, 16 bytes per tree) is warm, no memset node.  Measured:
 * profiles/forest_journal.txt.  There is no host-buffer twin: both calls act on a forest that lives on the device. */
int p252_merkle4_forest_ragged_journal_swap_device_into(p252_ctx* ctx, void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                                                   size_t max_leaves, void* d_levels, void* d_journal_ids, void* d_journal_values,
                                                   size_t journal_cap, const void* d_journal_len, void* d_roots, void* d_n_bad,
                                                   void* hip_stream);
/* the same for arity 2 */
int p252_merkle2_forest_ragged_journal_swap_device_into(p252_ctx* ctx, void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                                                   size_t max_leaves, void* d_levels, void* d_journal_ids, void* d_journal_values,
                                                   size_t journal_cap, const void* d_journal_len, void* d_roots, void* d_n_bad,
                                                   void* hip_stream);

/* Leaves appended to the trees of such a forest, written INTO a new compact forest.  A tree's size fixes its level layout, so a
 * forest cannot grow in place; but of a tree of n leaves that receives m > 0 more, node j of level l is unchanged iff
 * j < floor(n / A^l) (A = arity), and with m == 0 every node is.  The call moves those nodes at memory speed and hashes only the
 * others: sum over l >= 1 of ceil((n + m) / A^l) - floor(n / A^l) digests per tree that grows.
 * The old forest, read-only: d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels exactly as
 * p252_merkle{4,2}_forest_ragged_device was given and filled them (n_trees == 0: no old forest, the four may be 0 / NULL).  The old
 * leaf count n_t of tree t comes from the build's own validation, as in the openings and update calls: 0 for a tree the build calls
 * bad, and 0 for t >= n_trees.  The new forest has n_trees_new >= n_trees trees (the trees past the old count are new; an old empty
 * tree may start to exist) of at most max_leaves_new >= max_leaves leaves.  Tree t receives d_add[add_offsets[t] ..
 * add_offsets[t + 1]): d_add_offsets = n_trees_new + 1 uint64 (device, 8-byte aligned), m_t = the difference, 0 is fine; d_add =
 * n_add scalars (may be NULL when n_add == 0: a compaction copy).  An append is REFUSED — it counts as m_t = 0, the tree keeps its
 * old leaves and nodes — when its offsets decrease, when add_offsets[t + 1] > n_add, when n_t + m_t > max_leaves_new, or when the
 * appends accepted so far and this one together exceed n_add (only ranges that overlap behind decreasing offsets do that; the rule
 * keeps the new forest within leaves_cap, as the build's own sum rule keeps a forest within n_leaves).
 * Outputs (device): d_offsets_new[0] = 0, d_offsets_new[t + 1] = d_offsets_new[t] + n_t + m_t; d_leaves_new = each tree's old
 * leaves followed by its appended ones, byte for byte as given; the used part of d_levels_new and d_roots[n_trees_new] are byte
 * for byte what a fresh p252_merkle{4,2}_forest_ragged_device(d_leaves_new, leaves_cap, d_offsets_new, n_trees_new, max_leaves_new,
 * ..) writes — the new forest is an ordinary forest, and the openings, verify, update and multiproof calls take it unchanged.
 * leaves_cap >= n_leaves + n_add and levels_cap >= (n_leaves + n_add) / (A - 1) + n_trees_new * depth(max_leaves_new), in scalars;
 * nothing at or past the used lengths is written.  *d_n_bad (device uint32 the caller has zeroed; may be NULL) grows once per tree
 * whose append was refused or that is empty in the new forest (once when both hold); an empty tree gets a zero root and no storage.
 * *d_n_hashed (device uint64 the caller has zeroed, 8-byte aligned; may be NULL) receives the digests computed: exactly the sum
 * above over the trees.  P252_ERR_INVALID_ARGUMENT, nothing enqueued: max_leaves_new < max_leaves or == 0, n_trees_new < n_trees,
 * a cap below the above, a NULL or misaligned buffer (d_levels may be NULL when max_leaves <= 1, d_levels_new when max_leaves_new
 * <= 1), size overflow, or any output range that overlaps any input range (all sizes are known on the host).  n_trees_new == 0 ->
 * P252_OK, nothing enqueued.  Asynchronous on hip_stream: no host synchronisation, no allocation once the scratch is warm, no
 * memset node — it can be captured into a hipGraph.  Scratch, in the context's pair of THIS stream (p252_trim / p252_wipe cover
 * it), ids and counts only: 16 bytes per tree per forest for the indices, 24 + 8 (depth + 1) bytes per new tree, 8 bytes per 512
 * scalars moved, and one 16-byte record per dirty node (at most n_add / A^l + 2 n_trees_new on level l).
 * Cost: a fixed sequence of about 30 small launches plus one digest launch per level; the relocation reads and writes every clean
 * byte once.  Measured (profiles/forest_append.txt) against a fresh build of the same new forest in the same run: 7.2x ahead for 1
 * to 2^16 leaves appended to one 4^12-leaf tree, 5.8x at 2^20 (arity 2, 2^24 leaves: 11x and 7.6x); 20,000 mixed trees: 12.8x with
 * leaves appended to every tree, 12.7x to 1 % of them.  A rebuild is as quick at no fraction of that sweep (up to N/16 appended
 * leaves; larger fractions were not measured).  The relocation moves 4.2-4.5 TB/s read + written, 0.77-0.87 of a device-to-device
 * copy of the same bytes, bookkeeping launches included; one appended leaf still costs 1.9 ms (arity 2: 3.5 ms): one narrow
 * digest launch per level.  There is no host-buffer twin: the call acts on a forest that lives on the device. */
int p252_merkle4_forest_ragged_append_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                                  const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                                  const void* d_add, size_t n_add, const void* d_add_offsets, size_t n_trees_new,
                                                  size_t max_leaves_new, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new,
                                                  void* d_levels_new, size_t levels_cap, void* d_roots, void* d_n_bad, void* d_n_hashed,
                                                  void* hip_stream);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag) */
int p252_merkle2_forest_ragged_append_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                                  const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                                  const void* d_add, size_t n_add, const void* d_add_offsets, size_t n_trees_new,
                                                  size_t max_leaves_new, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new,
                                                  void* d_levels_new, size_t levels_cap, void* d_roots, void* d_n_bad, void* d_n_hashed,
                                                  void* hip_stream);

/* Such a forest rolled back, and forward again, in one call: every tree is cut to its first k_t leaves, then receives its appended
 * ones, and the trailing trees may be dropped — a reorg (the last blocks' notes come off, the competing ones go on), a roll-back to
 * a checkpoint, a prune.  Of a tree cut from n to k leaves (0 < k < n) that receives m more, node j of level l is byte for byte the
 * old node (l, j) iff j < floor(k / A^l): the append is the k = n case of this rule, and this call is the append call with a kept
 * count — the same launcher, kernels, scratch and outputs.  With m = 0 at most ONE node per level of a tree is hashed.
 * Every argument the append call has means what it means there, with these differences.  n_trees_new may be smaller than n_trees:
 * old trees at or past n_trees_new are dropped (trees past n_trees are new, as there).  d_keep = n_trees_new uint64 (device, 8-byte
 * aligned; read-only, it may overlap no output): k_t = min(d_keep[t], n_t), so any value >= n_t, UINT64_MAX included, keeps the
 * tree whole; d_keep == NULL keeps every tree whole.  The append's refusal rules hold with k_t in place of n_t (k_t + m_t >
 * max_leaves_new), and a refused append counts as m_t = 0 while the cut to k_t still applies: it is always valid.  The new tree t
 * holds its first k_t old leaves, then its m_t appended ones; d_offsets_new, d_leaves_new, the used part of d_levels_new and d_roots
 * are byte for byte a fresh build's.  A tree with k_t + m_t == 0 is an empty tree of the new forest: a zero root, no storage, its id
 * kept (no tree is renumbered).  *d_n_bad grows once per tree whose append was refused or that is empty in the new forest;
 * *d_n_hashed receives exactly the sum over l = 1 .. depth(k_t + m_t) of ceil((k_t + m_t) / A^l) - floor(k_t / A^l), over the trees
 * with k_t < n_t or m_t > 0 — an unchanged tree hashes nothing.  max_leaves_new >= max_leaves and the caps (leaves_cap >= n_leaves +
 * n_add, the append's levels_cap) stay as they are: they are known on the host, the kept counts are not.  Asynchronous, no host
 * synchronisation, no allocation once the scratch is warm, no memset node; the scratch is the append's plus 8 bytes per new tree.
 * Measured (profiles/forest_resize.txt) against a fresh build of the same new forest in the same run: one 4^12-leaf tree rolled back
 * by 1 leaf 1.82 ms, 7.5x ahead, by 2^20 leaves 0.62 ms, 20x (arity 2, 2^24 leaves: 3.39 ms / 11x and 1.01 ms / 35x); 20,000 mixed
 * trees cut by 1-16 leaves each 12.8x, 1 % of them 13.1x; a reorg in one call 1.94 ms against 3.93 ms for resize-then-append.  A
 * rebuild is as quick at no point of that sweep.  The relocation alone moves 3.8-4.1 TB/s read + written, 0.71-0.79 of a
 * device-to-device copy of the same bytes; a one-leaf rollback costs that (0.38 ms) plus one one-node digest launch per level,
 * 0.12 ms each.  The append entry points cost what they did before (both builds alternating in one session). */
int p252_merkle4_forest_ragged_resize_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                                  const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                                  const void* d_keep, const void* d_add, size_t n_add, const void* d_add_offsets,
                                                  size_t n_trees_new, size_t max_leaves_new, void* d_leaves_new, size_t leaves_cap,
                                                  void* d_offsets_new, void* d_levels_new, size_t levels_cap, void* d_roots, void* d_n_bad,
                                                  void* d_n_hashed, void* hip_stream);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag) */
int p252_merkle2_forest_ragged_resize_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                                  const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                                  const void* d_keep, const void* d_add, size_t n_add, const void* d_add_offsets,
                                                  size_t n_trees_new, size_t max_leaves_new, void* d_leaves_new, size_t leaves_cap,
                                                  void* d_offsets_new, void* d_levels_new, size_t levels_cap, void* d_roots, void* d_n_bad,
                                                  void* d_n_hashed, void* hip_stream);

/* Any trees of one or two BUILT forests gathered into a new compact forest, in any order: a tree pruned in the middle (the trees
 * behind it renumbered), a freshly built batch merged into the stored forest, a forest split into shards or reordered.  A tree's
 * tree-major block depends on its own leaves only — it holds byte for byte what p252_merkle{4,2}_tree writes for it alone — so NOTHING
 * IS HASHED and there is no tag: leaves, level blocks and roots are relocated at memory speed; the arity only selects the layout
 * (p252_merkle{4,2}_levels_len).
 * Sources A and B (read-only): each exactly what p252_merkle{4,2}_forest_ragged_device was given and filled — d_leaves, n_leaves,
 * d_offsets, n_trees, max_leaves, the tree-major d_levels and the n_trees d_roots.  Each source's leaf counts and block starts are
 * recomputed with the build's own validation, so a bad tree means here what it means there.  B is optional: with n_trees_b == 0 its
 * other six arguments may be 0 / NULL.  d_levels_x may be NULL when max_leaves_x <= 1.
 * d_pick = n_pick uint64 (device, 8-byte aligned): new tree j is tree d_pick[j] of A when the id is below n_trees_a, tree d_pick[j] -
 * n_trees_a of B when it is below n_trees_a + n_trees_b; any order, any tree any number of times.  A pick is REFUSED when its id is
 * >= n_trees_a + n_trees_b, when it names a tree its source's build calls bad, or when — with s_j the leaf count of pick j, 0 for
 * those two — s_0 + .. + s_j exceeds leaves_cap: once the running sum passes the cap every later non-empty pick is refused as well
 * (one scan decides it, and the device stays inside leaves_cap whatever the list holds).  A refused pick is an empty tree of the new
 * forest — a zero root, no storage, its position j kept — and counts once in *d_n_bad (device uint32 the caller has zeroed; may be
 * NULL).
 * Outputs (device): d_offsets_new[0] = 0, d_offsets_new[j + 1] = d_offsets_new[j] + n_j (n_pick + 1 uint64); d_leaves_new, the used
 * part of d_levels_new and d_roots_new[n_pick] are the picked trees' leaves, level blocks and roots byte for byte, hence byte for
 * byte what a fresh p252_merkle{4,2}_forest_ragged_device(d_leaves_new, leaves_cap, d_offsets_new, n_pick, max(max_leaves_a,
 * max_leaves_b), ..) writes: an ordinary forest that every other call takes unchanged.  Nothing at or past the used lengths is
 * written.  P252_ERR_INVALID_ARGUMENT, nothing enqueued: n_trees_a == 0, leaves_cap == 0, levels_cap < leaves_cap / (A - 1) + n_pick *
 * depth(max(max_leaves_a, max_leaves_b)), a NULL or misaligned buffer (scalars 16 bytes, offsets and picks 8, d_n_bad 4; d_levels_new
 * may be NULL when both max_leaves are <= 1), size overflow, or any output range that overlaps an input range or another output
 * range (all sizes are known on the host).  n_pick == 0 -> P252_OK, nothing enqueued.  Asynchronous on hip_stream: no host
 * synchronisation, no allocation once the scratch is warm, no memset node — it can be captured into a hipGraph.  Scratch, in the
 * context's pair of THIS stream (p252_trim / p252_wipe cover it), ids and counts only: 16 bytes per tree of A, of B and of the new
 * forest for the indices, 8 bytes per pick, 8 bytes per 512 scalars of the two capacities.  Cost: about 30 small launches and two
 * relocation launches that are balanced over 512-scalar tiles of the NEW arrays, not over trees.  Measured
 * (profiles/forest_select.txt) against a fresh build of the same new forest and a hipMemcpyDtoDAsync of the same bytes in the same
 * run: 20,000 mixed trees (34 M leaves) kept, 1 % dropped, permuted or merged from two halves in 0.65-0.71 ms, 34-37x ahead of the
 * build, 4.1-4.4 TB/s read + written, 0.78-0.84 of the copy's rate; one 4^12-leaf tree 0.34 ms, 38x (arity 2, 2^24 leaves: 0.46 ms,
 * 80x).  There is no host-buffer twin. */
int p252_merkle4_forest_ragged_select_device_into(p252_ctx* ctx, const void* d_leaves_a, size_t n_leaves_a, const void* d_offsets_a,
                                                  size_t n_trees_a, size_t max_leaves_a, const void* d_levels_a, const void* d_roots_a,
                                                  const void* d_leaves_b, size_t n_leaves_b, const void* d_offsets_b, size_t n_trees_b,
                                                  size_t max_leaves_b, const void* d_levels_b, const void* d_roots_b, const void* d_pick,
                                                  size_t n_pick, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new,
                                                  void* d_levels_new, size_t levels_cap, void* d_roots_new, void* d_n_bad, void* hip_stream);
/* the same for arity 2 (the level layout of p252_merkle2_levels_len) */
int p252_merkle2_forest_ragged_select_device_into(p252_ctx* ctx, const void* d_leaves_a, size_t n_leaves_a, const void* d_offsets_a,
                                                  size_t n_trees_a, size_t max_leaves_a, const void* d_levels_a, const void* d_roots_a,
                                                  const void* d_leaves_b, size_t n_leaves_b, const void* d_offsets_b, size_t n_trees_b,
                                                  size_t max_leaves_b, const void* d_levels_b, const void* d_roots_b, const void* d_pick,
                                                  size_t n_pick, void* d_leaves_new, size_t leaves_cap, void* d_offsets_new,
                                                  void* d_levels_new, size_t levels_cap, void* d_roots_new, void* d_n_bad, void* hip_stream);

/* ---- many leaves of ONE tree behind one shared proof.  The tree is what p252_merkle{4,2}_tree_device stored (d_leaves + d_levels;
 * one tree block of a ragged forest is the same layout); only the proof object is new.  The per-leaf openings above write
 * depth x (arity - 1) siblings for each leaf and their verification hashes k x depth nodes; when the k leaves share a tree most of
 * those siblings follow from other leaves of the batch and most of those digests are the same node again.
 * The format, A = arity: the k positions are STRICTLY ASCENDING, each < n_leaves.  w_0 = n_leaves, w_{l+1} = ceil(w_l / A);
 * S_0 = the positions, S_{l+1} = the distinct i / A of S_l, ascending.  For l = 0, 1, .. while w_l > 1; for every parent p of
 * S_{l+1}, ascending; for every child slot c = pA .. pA + A - 1, ascending: the proof receives node c of level l iff c < w_l and c
 * is not in S_l (slots at or past w_l are the zero scalar, hash.rs:22-26, and never stored).  The proof is the concatenation of
 * these scalars in that order: deterministic, and empty when n_leaves == 1 or k == n_leaves.
 * p252_merkle{4,2}_multiproof_bound: an upper bound of its length in scalars,
 * sum over those levels of min((A - 1) min(k, w_{l+1}), w_l - min(k, w_l)); reached by k == 1 on a complete tree.
 * No host-buffer twin: the calls act on a tree that lives on the device. ---- */
size_t p252_merkle4_multiproof_bound(size_t n_leaves, size_t k);
size_t p252_merkle2_multiproof_bound(size_t n_leaves, size_t k);
/* Extraction (no hashing): d_indices = k uint32 positions (device), d_leaves_out[k] = the leaves at them, d_proof = the proof,
 * *d_proof_len (device uint64, 8-byte aligned) = the scalars the proof NEEDS: nothing is written at or past proof_cap (scalars), so
 * a short buffer costs a second call, never memory; a buffer of _bound scalars always suffices.  d_proof may be NULL when
 * proof_cap == 0.  A position that is >= n_leaves or not greater than its predecessor is bad: counted once in *d_n_bad (device
 * uint32 the caller has zeroed; may be NULL), the call then reports *d_proof_len = 0, reads nothing through a bad position, and
 * leaves the contents of d_leaves_out and d_proof unspecified.  k == 0 or n_leaves == 0 (or either >= 2^32: positions are uint32)
 * -> P252_ERR_INVALID_ARGUMENT.  Asynchronous on hip_stream; scratch (counters, scan tiles, two work lists of 16 bytes per
 * parent: at most 33 bytes per position plus 2 KiB) in the context's pair of THIS stream, covered by p252_trim / p252_wipe.
 * Cost: up to three launches per level, so for a few leaves p252_merkle{4,2}_openings_device (one launch) is quicker. */
int p252_merkle4_multiproof_device(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_levels, const void* d_indices, size_t k,
                                   void* d_leaves_out, void* d_proof, size_t proof_cap, void* d_proof_len, void* d_n_bad, void* hip_stream);
int p252_merkle2_multiproof_device(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_levels, const void* d_indices, size_t k,
                                   void* d_leaves_out, void* d_proof, size_t proof_cap, void* d_proof_len, void* d_n_bad, void* hip_stream);
/* Verification: the structure is derived from (n_leaves, d_indices) alone; every node of S_1, S_2, .. is hashed ONCE with
 * Hash::digest(Domain::Merkle4 / Merkle2, children) (pass that domain's tag), each child taken from the level below, from the
 * proof stream, or as zero.  *d_ok (device, 1 byte) = 1 iff no position is bad, the structure consumes exactly proof_len scalars,
 * and the recomputed root equals *d_root (device, 1 scalar); 0 otherwise (n_leaves == 1: the leaf IS the root and is compared as
 * the 32 bytes it is, so leaf + p is refused; the forest call below compares it mod p).  Positions and proof are untrusted: nothing is read at
 * or past proof_len or k whatever they contain.  d_root_out (device, 1 scalar; may be NULL) receives the recomputed root when the
 * first two conditions hold and is left alone otherwise; *d_n_hashed (device uint64, 8-byte aligned; may be NULL) receives the
 * digests computed, sum over l >= 1 of |S_l| (0 after a bad position); *d_n_bad as above.  d_proof may be NULL when
 * proof_len == 0.  Asynchronous on hip_stream; scratch as for extraction plus two lists of at most min(k, ceil(n_leaves / A))
 * node values, in the same pair.  Cost: up to four launches per level: see profiles/multiproof.txt for the k from which this beats
 * p252_merkle{4,2}_verify_batch_device. */
int p252_merkle4_multiproof_verify_device(p252_ctx* ctx, const uint64_t tag[4], size_t n_leaves, const void* d_indices, const void* d_leaves_in,
                                          size_t k, const void* d_proof, size_t proof_len, const void* d_root, void* d_ok, void* d_root_out,
                                          void* d_n_hashed, void* d_n_bad, void* hip_stream);
int p252_merkle2_multiproof_verify_device(p252_ctx* ctx, const uint64_t tag[4], size_t n_leaves, const void* d_indices, const void* d_leaves_in,
                                          size_t k, const void* d_proof, size_t proof_len, const void* d_root, void* d_ok, void* d_root_out,
                                          void* d_n_hashed, void* d_n_bad, void* hip_stream);

/* ---- the shared proof across a forest of trees of DIFFERENT sizes: k (tree id, leaf id) pairs anywhere in a built ragged forest,
 * one call to extract and one to verify, every launch sized by the whole batch.  The forest arguments (d_leaves, n_leaves, d_offsets,
 * n_trees, max_leaves, d_levels) are exactly those of p252_merkle{4,2}_forest_ragged_device and _forest_ragged_openings_device; n_t and
 * the level block starts are derived on the device, and a bad tree is what it is there (empty, longer than max_leaves, decreasing
 * offsets, past n_leaves).  Pair i = (tree_ids[i]: uint32, leaf_ids[i]: uint64), STRICTLY ASCENDING in (tree id, leaf id).
 * The format: for a tree t with at least one pair, P_t is byte for byte what p252_merkle{A}_multiproof_device writes for that tree's
 * block (leaves[offsets[t] .. offsets[t+1]), its block of d_levels) and its own positions; the forest proof is
 * P_0 | P_1 | .. | P_{n_trees-1} (P_t empty for a tree without pairs, of one leaf, or with every leaf asked for), and
 * proof_offsets (n_trees + 1 uint64) has proof_offsets[0] = 0, proof_offsets[t+1] - proof_offsets[t] = |P_t|,
 * proof_offsets[n_trees] = the proof length.  proof[proof_offsets[t] .. proof_offsets[t+1]) can be cut out and checked alone with
 * p252_merkle{4,2}_multiproof_verify_device.
 * _bound: with D = p252_merkle{4,2}_depth(max_leaves), min(k D (A - 1), n_leaves + n_leaves / (A - 1) + n_trees D) — every proof scalar
 * is a distinct stored node and a pair needs at most D (A - 1) of them; 0 when k, n_leaves or n_trees is 0; reached by one leaf in
 * each complete tree of a forest of equal complete trees. ---- */
size_t p252_merkle4_forest_ragged_multiproof_bound(size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);
size_t p252_merkle2_forest_ragged_multiproof_bound(size_t n_leaves, size_t n_trees, size_t max_leaves, size_t k);
/* Extraction (no hashing): d_leaves_out[i] = the leaf of pair i, byte for byte; d_proof = the forest proof; d_proof_offsets (device,
 * n_trees + 1 uint64, 8-byte aligned) is always written in full, and proof_offsets[n_trees] is the length the proof NEEDS: nothing is
 * written at or past proof_cap (scalars), so a short buffer costs a second call, never memory; a buffer of _bound scalars always
 * suffices.  d_proof may be NULL when proof_cap == 0.  A bad pair — tree id >= n_trees, a bad tree, leaf id >= n_t, or a pair not
 * greater than its predecessor — is counted once in *d_n_bad (device uint32 the caller has zeroed; may be NULL); after any bad pair
 * all of d_proof_offsets is zero, nothing is read through a bad pair, and the contents of d_leaves_out and d_proof are unspecified:
 * the batch is one object.  k, n_trees, n_leaves or max_leaves == 0, k or max_leaves >= 2^32 (a node index is a 32-bit record
 * word), a NULL or misaligned buffer, size overflow -> P252_ERR_INVALID_ARGUMENT, nothing enqueued.  Asynchronous on hip_stream, no
 * host synchronisation, no allocation once the scratch is warm; scratch in the context's pair of THIS stream, covered by p252_trim /
 * p252_wipe: 52 bytes per pair (the elements of level 0, two work lists of 16-byte records with their tree ids, the level widths)
 * and 20 bytes per 256 pairs, 76 bytes per tree (the forest's index, two consumption counters and the total, the first pair, the
 * root) and 16 bytes per 2,048 trees, plus 4 KiB — nothing grows with the forest's leaves.  Cost: the structure pass runs twice (a
 * counting pass, a scan over the trees, a writing pass), up to three launches per level each. */
int p252_merkle4_forest_ragged_multiproof_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                                                 size_t max_leaves, const void* d_levels, const void* d_tree_ids, const void* d_leaf_ids,
                                                 size_t k, void* d_leaves_out, void* d_proof, size_t proof_cap, void* d_proof_offsets,
                                                 void* d_n_bad, void* hip_stream);
int p252_merkle2_forest_ragged_multiproof_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets, size_t n_trees,
                                                 size_t max_leaves, const void* d_levels, const void* d_tree_ids, const void* d_leaf_ids,
                                                 size_t k, void* d_leaves_out, void* d_proof, size_t proof_cap, void* d_proof_offsets,
                                                 void* d_n_bad, void* hip_stream);
/* Verification needs neither leaves nor levels: the structure follows from (d_offsets -> n_t, tree ids, leaf ids) alone.  Every node
 * of every tree's S_1, S_2, .. is hashed ONCE with Hash::digest(Domain::Merkle4 / Merkle2, children) (pass that domain's tag), each
 * child from the level below, from tree t's segment of the proof, or zero.  d_ok (device, n_trees bytes): d_ok[t] = 1 iff tree t has
 * at least one pair, no pair of the batch is bad, proof_offsets[t] <= proof_offsets[t+1] <= proof_len, tree t's structure consumes
 * exactly proof_offsets[t+1] - proof_offsets[t] scalars, and the recomputed root equals d_roots[t] (device, n_trees scalars) as the
 * 32 bytes they are; 0 otherwise, also for a tree nobody asked about.  d_roots_out (n_trees scalars; may be NULL): entry t is written
 * when every condition except the root comparison holds and left alone otherwise; the recomputed root of a one-leaf tree is its leaf
 * mod p (the forest's convention, see the edge-value paragraph above).  *d_n_hashed (device uint64; may be NULL) = the digests
 * computed, the sum over trees and l >= 1 of |S_l| (0 after a bad pair); *d_n_bad as above.  Pairs, proof and proof offsets are
 * untrusted: nothing is read at or past proof_len, k or n_trees + 1 whatever they contain, and a tree whose offsets lie leaves the
 * other trees' verdicts alone.  d_proof may be NULL when proof_len == 0.  Refusals and calling conventions as for extraction;
 * scratch as for extraction plus two lists of k node values (64 bytes per pair) in the same pair.  Cost: up to four launches per
 * level of the deepest tree, whatever the number of trees. */
int p252_merkle4_forest_ragged_multiproof_verify_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_offsets, size_t n_leaves,
                                                        size_t n_trees, size_t max_leaves, const void* d_tree_ids, const void* d_leaf_ids,
                                                        const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_len,
                                                        const void* d_proof_offsets, const void* d_roots, void* d_ok, void* d_roots_out,
                                                        void* d_n_hashed, void* d_n_bad, void* hip_stream);
int p252_merkle2_forest_ragged_multiproof_verify_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_offsets, size_t n_leaves,
                                                        size_t n_trees, size_t max_leaves, const void* d_tree_ids, const void* d_leaf_ids,
                                                        const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_len,
                                                        const void* d_proof_offsets, const void* d_roots, void* d_ok, void* d_roots_out,
                                                        void* d_n_hashed, void* d_n_bad, void* hip_stream);

/* ---- a forest of append-only trees kept ONLY as their frontiers.  Every ragged-forest call above acts on a stored forest: all
 * leaves and all levels.  A consumer that appends and wants the roots (a note-commitment tree, a log per account, one tree too large
 * for the card streamed in chunks) needs O(depth) state per tree.  With A = arity, f_l(n) = floor(n / A^l), c_l(n) = ceil(n / A^l)
 * and d_l(n) = f_l(n) mod A (digit l of n): node j of level l of a tree of n leaves is final iff j < f_l(n), and the final nodes a
 * later append still reads are, per level, the d_l(n) nodes [A f_{l+1}(n), f_l(n)) right of the last complete group.
 * The state of n_trees trees, three device arrays the caller owns: d_counts = n_trees uint64 (8-byte aligned), the leaf counts;
 * d_roots = n_trees scalars; d_frontier = n_trees x p252_merkle{4,2}_forest_frontier_bound(max_leaves) scalars — tree t's part holds
 * rows l = 0 .. D = p252_merkle{4,2}_depth(max_leaves) of A - 1 scalars each (row 0: leaves as they were given; row D is used by a
 * tree of exactly A^D leaves), row l = those d_l(n_t) nodes in index order, the slots past them ZERO: a state is byte-comparable.
 * A count of 0 is an empty tree with a zero root and zero rows, so a caller adds trees by allocating zeroed state.  The bound is
 * (D + 1)(A - 1) scalars per tree, 0 for max_leaves == 0. */
size_t p252_merkle4_forest_frontier_bound(size_t max_leaves);
size_t p252_merkle2_forest_frontier_bound(size_t max_leaves);
/* The append, in place: tree t receives d_add[add_offsets[t] .. add_offsets[t + 1]) (d_add_offsets = n_trees + 1 uint64, device,
 * 8-byte aligned; d_add = n_add scalars, may be NULL when n_add == 0), m_t = the difference.  A tree with m_t == 0 is untouched,
 * root included.  A tree that grows from n to n' = n + m computes, level by level, the nodes [f_l(n), c_l(n')) of level l from the
 * level below — the first d_{l-1}(n) children of node f_l(n) are the frontier's row l - 1, all others were just computed (or are
 * the new leaves), children at or past c_{l-1}(n') are the zero scalar — up to the single node of level depth(n'), the root:
 * sum over l >= 1 of c_l(n') - f_l(n) digests, the count of p252_merkle{4,2}_forest_ragged_append_device_into, with no old leaf
 * or node resident and nothing relocated.  Then row l keeps its entries and gains the new final nodes when f_{l+1} did not move,
 * and is the d_l(n') last final nodes otherwise; n' == 1 has no level: the root is the leaf mod p (as the forest build writes a
 * one-leaf tree's), row 0 the leaf's bytes.  d_counts, d_frontier and d_roots end as the state of the grown trees: d_roots[t] is
 * what p252_merkle{4,2}_tree returns for all leaves so far.
 * An append is REFUSED — counted once in *d_n_bad (device uint32 the caller has zeroed; may be NULL), the tree's count, rows and
 * root untouched — when its offsets decrease, when add_offsets[t + 1] > n_add, when n_t + m_t > max_leaves, when n_t > max_leaves
 * already (a corrupt state is never indexed past its rows; it is counted whatever it is given), or when the appends accepted so
 * far and this one together exceed n_add (the stored append's sum rule: only ranges that overlap behind decreasing offsets do
 * that).  *d_n_hashed (device uint64 the caller has zeroed, 8-byte aligned; may be NULL) receives the digests computed: exactly
 * the sum above over the accepted trees.  P252_ERR_INVALID_ARGUMENT, nothing enqueued: max_leaves == 0; n_add >= 2^32 (a record
 * holds the start of its run of children in 32 bits — a caller with more streams it in smaller chunks, which is what the state is
 * for); a NULL or misaligned buffer (scalars 16 bytes, d_counts / d_add_offsets / d_n_hashed 8, d_n_bad 4); size overflow; d_add or
 * d_add_offsets overlapping d_counts, d_frontier, d_roots, d_n_bad or d_n_hashed.  n_trees == 0 -> P252_OK, nothing enqueued.
 * Asynchronous on hip_stream: no host synchronisation, no allocation once the scratch is warm, no memset node.  Scratch, in the
 * context's pair of THIS stream (p252_trim / p252_wipe cover it): 24 + 8 (D + 1) bytes per tree, and per computed node — at most
 * n_add / A^l + 2 min(n_trees, n_add) on level l, hence n_add / (A - 1) + 2 min(n_trees, n_add) D in all — its 32-byte value, a
 * 16-byte record and a 4-byte width.  Cost: 11 small launches plus one digest launch per level 1 .. D (the stored append: about 30
 * plus one per level); the scans over the trees are the stored append's own, all digests run on the kernels of
 * p252_merkle{4,2}_multiproof_verify_device.  n_trees >= 2^32 is refused as a size overflow (a record names its tree in 32 bits).
 * Measured (profiles/forest_frontier.txt) against the stored append on the same appends in the same run, medians of 20: one
 * 4^12-leaf tree + 1 / 2^16 / 2^20 leaves 1.59 / 1.60 / 2.14 ms against 1.96 / 1.97 / 2.51 ms (0.81-0.85 of it) on 1,384 bytes of state
 * against 716-761 MB stored; arity 2 on 2^24 leaves 2.98 / 3.03 / 4.77 against 3.52 / 3.59 / 5.41 ms (0.84-0.88); 20,000 mixed trees with
 * 1-16 leaves appended to each 1.25 against 1.93 ms, to 1 % of them 0.85 against 1.90 ms, on 16.2 MB against 1.46 GB; 6.9-29x ahead
 * of a fresh build.  One appended leaf still costs one narrow digest launch per level.  Appends above 2^20 leaves were not measured. */
int p252_merkle4_forest_frontier_append_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_counts, void* d_frontier, void* d_roots,
                                                    size_t n_trees, size_t max_leaves, const void* d_add, size_t n_add,
                                                    const void* d_add_offsets, void* d_n_bad, void* d_n_hashed, void* hip_stream);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag) */
int p252_merkle2_forest_frontier_append_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_counts, void* d_frontier, void* d_roots,
                                                    size_t n_trees, size_t max_leaves, const void* d_add, size_t n_add,
                                                    const void* d_add_offsets, void* d_n_bad, void* d_n_hashed, void* hip_stream);
/* The same append with INCREMENTAL WITNESSES: the openings of k marked leaves are kept current while the trees grow underneath them,
 * so a forest kept only as its frontiers can still prove that a leaf is in it.  The state arguments, d_add, d_add_offsets, d_n_bad and
 * d_n_hashed mean, refuse and end exactly as in p252_merkle{4,2}_forest_frontier_append_device_into (byte for byte on the same
 * inputs); k == 0 IS that call (the witness buffers are not looked at and may be NULL).  The witnesses have the layout of
 * p252_merkle{4,2}_forest_ragged_openings_device at the stride D = p252_merkle{4,2}_depth(max_leaves), A = arity: d_wit_tree_ids[k]
 * (uint32) and d_wit_leaf_ids[k] (uint64) are read only; d_wit_leaves[k], d_wit_siblings[k][D][A - 1], d_wit_positions[k][D] and
 * d_wit_depths[k] (uint8) are read and updated in place.  Duplicates and any order are fine: each witness has its own slots.
 * Witness i names leaf p of tree t; n = the tree's count before the call, n' after it (n' == n where nothing was appended or the
 * append was refused).  With f_l(n) = floor(n / A^l) and c_l(n) = ceil(n / A^l) the append computes V_l = the nodes [f_l(n), c_l(n'))
 * of every level l (V_0 = the new leaves); the sibling x of an opening on level l is FINAL (x < f_l(n)), in V_l (x < c_l(n')) or zero.
 *   BAD — t >= n_trees, or p >= n' (a leaf of a refused append included): the witness becomes all zero with depth 0xFF, as the
 *     openings call writes a bad opening, and is counted once in *d_n_bad_witness (device uint32 the caller has zeroed; may be NULL).
 *   CARRIED, p < n, the tree unchanged (n' == n): untouched byte for byte; one whose depth byte is 0xFF already is counted again.
 *   CARRIED, p < n, the tree grown: the input must be the tree's opening at count n.  The one thing the call can check it checks:
 *     d_wit_depths[i] == depth(n), otherwise (an input 0xFF included) the witness is BAD as above.  Rows l < depth(n'): with g = p >>
 *     ((l + 1) log2 A) the path's group and (p >> l log2 A) mod A its slot (the position byte), a row whose whole group is final
 *     (g < f_{l+1}(n)) stays; in any other row the final siblings stay, those below c_l(n') come from V_l, the rest are zero.  Rows
 *     at or past depth(n') stay (they are zero in an opening at n), the leaf stays, the depth byte becomes depth(n').
 *   MARKED in this call, n <= p < n': the input content is ignored.  The leaf is d_add[add_offsets[t] + p - n], bytes as given; a
 *     final sibling x < f_l(n) is the frontier's OLD row l at slot x - A f_{l+1}(n) (the path's node is at or past f_l(n), so its
 *     group is the partly filled one), the others as above; rows at or past depth(n') are zero.
 * Afterwards every witness that is not bad is byte for byte what p252_merkle{4,2}_forest_ragged_openings_device writes for (t, p) on
 * a stored forest of all leaves so far built with the same max_leaves, and goes into p252_merkle{4,2}_path_ragged_device and
 * _forest_ragged_verify_device against d_roots of the state unchanged.  A stored forest hands over with two existing calls: the
 * openings of the leaves to watch, then _forest_frontier_extract_device_into.  Keeping the witnesses current costs NO digest: one
 * launch more between the last digest launch and the update of the state, which gathers out of scratch the append holds anyway — a
 * block takes floor(256 / D) whole witnesses, one lane per (witness, row) — and no scratch of its own.
 * P252_ERR_INVALID_ARGUMENT, nothing enqueued: everything the plain call refuses; with k > 0 a NULL or misaligned witness buffer
 * (scalars 16 bytes, d_wit_leaf_ids 8, d_wit_tree_ids and d_n_bad_witness 4; d_wit_siblings and d_wit_positions may be NULL when
 * D == 0, i.e. max_leaves == 1: only leaves and depth bytes exist); size overflow of k D (A - 1) 32 or of the launch; d_wit_leaves,
 * d_wit_siblings, d_wit_positions, d_wit_depths or d_n_bad_witness overlapping the state, d_add, d_add_offsets, the ids, d_n_bad,
 * d_n_hashed or one another.  n_trees == 0 with k > 0 is a forest in which every witness is bad (the state may be NULL).
 * Asynchronous on hip_stream: no host synchronisation, no allocation beyond the plain call's scratch.
 * Measured (profiles/forest_witness.txt) in one run, medians of 20, as: with witnesses / the plain call / the stored append +
 * p252_merkle{4,2}_forest_ragged_openings_device of the same pairs.  One 4^12-leaf tree + 2^16 leaves with 2^10, 2^16, 2^20 carried
 * witnesses 1.63 / 1.61 / 2.04, 1.63 / 1.62 / 2.06 and 1.78 / 1.63 / 2.76 ms, with the 2^16 new leaves marked 1.67 / 1.61 / 2.05 ms;
 * arity 2 on 2^24 leaves 3.09 / 3.06 / 3.71, 3.12 / 3.09 / 3.76, 3.38 / 3.10 / 4.34 and 3.13 / 3.08 / 3.74 ms; 20,000 mixed trees with
 * 169,761 witnesses 1.30 / 1.27 / 2.06 ms.  The upkeep is one launch, under 10 % of the plain call on every row, but not a copy's
 * speed: at 2^20 witnesses 0.16 ms (arity 2: 0.28 ms) against 0.04 ms (0.02 ms) for a device copy of the bytes it writes — it
 * runs a lane for every row, changed or not. */
int p252_merkle4_forest_frontier_append_witness_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_counts, void* d_frontier,
                                                            void* d_roots, size_t n_trees, size_t max_leaves, const void* d_add, size_t n_add,
                                                            const void* d_add_offsets, const void* d_wit_tree_ids, const void* d_wit_leaf_ids,
                                                            size_t k, void* d_wit_leaves, void* d_wit_siblings, void* d_wit_positions,
                                                            void* d_wit_depths, void* d_n_bad, void* d_n_hashed, void* d_n_bad_witness,
                                                            void* hip_stream);
/* the same for arity 2 (Domain::Merkle2 nodes; pass the Merkle2 tag) */
int p252_merkle2_forest_frontier_append_witness_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_counts, void* d_frontier,
                                                            void* d_roots, size_t n_trees, size_t max_leaves, const void* d_add, size_t n_add,
                                                            const void* d_add_offsets, const void* d_wit_tree_ids, const void* d_wit_leaf_ids,
                                                            size_t k, void* d_wit_leaves, void* d_wit_siblings, void* d_wit_positions,
                                                            void* d_wit_depths, void* d_n_bad, void* d_n_hashed, void* d_n_bad_witness,
                                                            void* hip_stream);
/* The state of a BUILT ragged forest: d_leaves, n_leaves, d_offsets, n_trees, max_leaves_forest, d_levels and d_roots_forest exactly
 * as p252_merkle{4,2}_forest_ragged_device was given and filled them (read-only; d_levels may be NULL when max_leaves_forest <= 1);
 * the leaf counts come from the build's own validation.  Writes d_counts, d_frontier (rows for max_leaves >= max_leaves_forest, so
 * the trees can grow) and d_roots for all n_trees trees: data movement only, nothing is hashed and there is no tag.  A tree the
 * build calls bad gets count 0, zero rows and a zero root and is counted in *d_n_bad (device uint32 the caller has zeroed; may be
 * NULL).  A stored forest can so be dropped down to its accumulator.  P252_ERR_INVALID_ARGUMENT, nothing enqueued:
 * max_leaves_forest == 0, max_leaves < max_leaves_forest, a NULL or misaligned buffer, size overflow, or an output range that
 * overlaps an input range.  n_trees == 0 -> P252_OK.  Asynchronous on hip_stream; scratch: the forest's index, 16 bytes per tree. */
int p252_merkle4_forest_frontier_extract_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                                     size_t n_trees, size_t max_leaves_forest, const void* d_levels,
                                                     const void* d_roots_forest, size_t max_leaves, void* d_counts, void* d_frontier,
                                                     void* d_roots, void* d_n_bad, void* hip_stream);
/* the same for arity 2 (the level layout of merkle2 trees) */
int p252_merkle2_forest_frontier_extract_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                                     size_t n_trees, size_t max_leaves_forest, const void* d_levels,
                                                     const void* d_roots_forest, size_t max_leaves, void* d_counts, void* d_frontier,
                                                     void* d_roots, void* d_n_bad, void* hip_stream);

/* ---- consistency proofs: that a tree of a ragged forest, now of m leaves, is the tree it was at n <= m leaves with leaves appended
 * and nothing before them changed.  With A the arity, f_l(n) = floor(n / A^l) and d_l(n) = f_l(n) mod A: the proof of (tree t, old
 * count n) is the OPENING OF LEAF INDEX n of the tree as it is now, in the layout of p252_merkle{4,2}_forest_ragged_openings_device
 * at stride D = p252_merkle{4,2}_depth(max_leaves).  Its slot on row l is d_l(n), and its siblings left of that slot are the nodes
 * [A f_{l+1}(n), f_l(n)) of level l, which are final at count n — row l of the frontier of the tree at n leaves.  The whole opening
 * re-hashes to the new root in the ordinary way; its left siblings alone re-hash to the old root.  O(depth) scalars per proof and
 * O(depth) digests per check, where replaying the appended leaves through _forest_frontier_append_device_into costs O(m - n). ---- */
/* Extraction.  The forest arguments d_leaves .. d_levels exactly as p252_merkle{4,2}_forest_ragged_openings_device takes them
 * (read-only; n_t comes from the build's own validation).  Proof i is for tree d_tree_ids[i] (uint32) and old count d_old_counts[i]
 * (uint64); it writes d_new_counts_out[i] (uint64), d_leaves_out[i], d_siblings[i][D][arity - 1], d_positions[i][D] (uint8) and
 * d_depths[i] (uint8):
 *   1 <= n < n_t: byte for byte what the openings call writes for (t, leaf id n); d_new_counts_out[i] = n_t.
 *   n == n_t (the tree did not grow): a zero leaf, zero rows and zero positions; the depth byte is depth(n_t); d_new_counts_out[i] = n_t.
 *   BAD — a tree id >= n_trees, a tree the build calls bad, n == 0 or n > n_t: all zero, depth 0xFF, new count 0, counted once in
 *     *d_n_bad (device uint32 the caller has zeroed; may be NULL).
 * Data movement only: nothing is hashed and there is no tag.  P252_ERR_INVALID_ARGUMENT, nothing enqueued: n_leaves, n_trees or
 * max_leaves == 0, a NULL or misaligned buffer (scalars 16 bytes, d_offsets and the counts 8, d_tree_ids and d_n_bad 4; d_levels,
 * d_siblings and d_positions may be NULL when max_leaves == 1), size overflow, or an output range that overlaps an input range or
 * another output.  k == 0 -> P252_OK, nothing enqueued.  Asynchronous on hip_stream; scratch: the forest's index and 32 bytes per
 * proof. */
int p252_merkle4_forest_ragged_consistency_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                                       size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                                       const void* d_old_counts, size_t k, void* d_new_counts_out, void* d_leaves_out,
                                                       void* d_siblings, void* d_positions, void* d_depths, void* d_n_bad, void* hip_stream);
/* the same for arity 2 (the level layout of merkle2 trees) */
int p252_merkle2_forest_ragged_consistency_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                                       size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                                       const void* d_old_counts, size_t k, void* d_new_counts_out, void* d_leaves_out,
                                                       void* d_siblings, void* d_positions, void* d_depths, void* d_n_bad, void* hip_stream);
/* Verification of k such proofs (the four opening arrays at stride_depth <= 64 rows) against claims (old count n, old root, new count
 * m, new root).  d_tree_ids == NULL: claim i is element i of d_old_counts, d_old_roots, d_new_counts and d_new_roots (k entries
 * each; n_trees is not looked at).  d_tree_ids != NULL (uint32[k]): the claim arrays hold n_trees entries and claim i is element
 * d_tree_ids[i]; an id >= n_trees is refused.  So the d_counts / d_roots of a frontier state serve as the old claims and a
 * publisher's counts and roots as the new ones, with no gather.  d_ok[i] (uint8) = 1 iff ALL of:
 *   1 <= n <= m, and d_depths[i] == depth(m) <= stride_depth (otherwise the proof is REFUSED);
 *   n == m: the old and the new root are the same 32 bytes; nothing is hashed and the opening is not read;
 *   n < m: d_positions[i][l] == d_l(n) for every l < depth(m) — the verifier takes the slots from n, never from the proof; the NEW
 *     CHAIN, the ordinary re-hash of the opening over all depth(m) rows, ends in the new root; and the OLD CHAIN ends in the old
 *     root: the carry starts absent; on level l < depth(n), with d = d_l(n), nothing is hashed if d == 0 and there is no carry,
 *     otherwise the carry becomes H(the first d siblings of row l, then the carry if there is one, then zero scalars); after level
 *     depth(n) - 1 the carry is the old root.  n == A^depth(n) hashes nothing for the old side: the old root is sibling 0 of row
 *     depth(n), the final node itself, reduced mod p as a one-leaf tree's root is (n == 1: row 0; a node is left as it is).
 * The roots do not commit to the counts beyond the depth: a new count that differs from the tree's but has its depth describes the
 * same tree followed by zero leaves, and passes.
 * d_old_roots_out[k] / d_new_roots_out[k] (either may be NULL): the recomputed roots; for n == m the claimed roots; zero for a
 * refused proof.  *d_n_hashed (device uint64 the caller has zeroed; may be NULL) gains, for every proof with n < m that was not
 * refused, depth(m) plus the digests of its old chain.  Both chains are walks of the re-hash of p252_merkle{4,2}_path_ragged_device —
 * the old one over a second opening the call lays out in scratch — each sorted by its depths (P252_RAGGED_SORT=0: not sorted).
 * P252_ERR_INVALID_ARGUMENT, nothing enqueued: stride_depth > 64, a NULL or misaligned buffer (scalars 16 bytes, the counts and
 * d_n_hashed 8, d_tree_ids 4; d_siblings and d_positions may be NULL when stride_depth == 0, the claim arrays when d_tree_ids is
 * given and n_trees == 0), size overflow, or an output range that overlaps an input range or another output.  k == 0 -> P252_OK,
 * nothing enqueued.  Asynchronous on hip_stream; scratch: per proof a second opening at stride_depth, two roots and 8 bytes of order. */
int p252_merkle4_forest_consistency_verify_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_old_counts, const void* d_old_roots,
                                                       const void* d_new_counts, const void* d_new_roots, const void* d_leaves_in,
                                                       const void* d_siblings, const void* d_positions, const void* d_depths,
                                                       size_t stride_depth, size_t k, const void* d_tree_ids, size_t n_trees, void* d_ok,
                                                       void* d_old_roots_out, void* d_new_roots_out, void* d_n_hashed, void* hip_stream);
/* the same for arity 2 */
int p252_merkle2_forest_consistency_verify_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_old_counts, const void* d_old_roots,
                                                       const void* d_new_counts, const void* d_new_roots, const void* d_leaves_in,
                                                       const void* d_siblings, const void* d_positions, const void* d_depths,
                                                       size_t stride_depth, size_t k, const void* d_tree_ids, size_t n_trees, void* d_ok,
                                                       void* d_old_roots_out, void* d_new_roots_out, void* d_n_hashed, void* hip_stream);

/* ---- anchors: roots and openings of the trees of a ragged forest AS THEY WERE at earlier leaf counts.  An append-only tree grows
 * with every block, and a party that trusts the root the tree had at count c (its anchor) needs the opening of leaf i < c in the tree
 * of c leaves; the route without this call is one p252_merkle{4,2}_forest_ragged_resize_device_into per distinct anchor into a second
 * copy of the forest.  With A the arity and f_l(c) = floor(c / A^l): node j of level l of the tree at c leaves is the stored node
 * while j < f_l(c); node j == f_l(c) exists iff c mod A^l != 0 and is the PARTIAL node P_l(c) = H(the stored nodes
 * [A f_l(c), f_{l-1}(c)) of level l - 1, then P_{l-1}(c) if it exists, then zero scalars); right of it there is nothing.  The root at c is
 * P_depth(c)(c), or the stored node when c == A^depth(c) (c == 1: the leaf, reduced mod p as a one-leaf tree's root is).  An anchor
 * costs depth(c) - l0 digests, l0 the lowest level whose digit of c is not zero — none when c is a power of A — however many leaves
 * are opened under it.
 * The forest arguments d_leaves .. d_levels exactly as p252_merkle{4,2}_forest_ragged_openings_device takes them (read-only; n_t
 * comes from the build's own validation); tag: the tree's (Merkle4 / Merkle2).
 * ANCHORS.  Anchor a is tree d_anchor_tree_ids[a] (uint32[m]) at count c = d_anchor_counts[a] (uint64[m]); valid iff the tree id is
 * < n_trees, the build does not call the tree bad, and 1 <= c <= n_t.  Then d_anchor_roots[a] is the 32 bytes a fresh build of the
 * tree's first c leaves returns as its root, d_anchor_depths[a] (uint8) = depth(c), and *d_n_hashed (device uint64 the caller has
 * zeroed; may be NULL) gains depth(c) - l0.  A BAD anchor: a zero root, depth 0xFF, counted once in *d_n_bad_anchors (device uint32
 * the caller has zeroed; may be NULL).
 * OPENINGS.  Opening i is leaf d_leaf_ids[i] (uint64[k]) under anchor d_anchor_ids[i] (uint32[k]); valid iff the anchor id is < m, the
 * anchor is valid and the leaf id is < c.  d_leaves_out[i], d_siblings[i][D][arity - 1], d_positions[i][D] and d_depths[i], at stride
 * D = p252_merkle{4,2}_depth(max_leaves), are byte for byte what p252_merkle{4,2}_forest_ragged_openings_device writes for that leaf
 * on a fresh build of the tree's first c leaves: the depth byte is depth(c), rows at and past it are zero, siblings right of the last
 * node of a level are zero, and at most one sibling is a partial node.  A BAD opening: all zero, depth 0xFF, counted once in *d_n_bad
 * (device uint32 the caller has zeroed; may be NULL).
 * VERIFICATION needs nothing new, which is the reason for this layout: the four opening arrays go into
 * p252_merkle{4,2}_path_ragged_device as they stand, and into p252_merkle{4,2}_forest_ragged_verify_device with
 * d_tree_ids := d_anchor_ids, d_roots := d_anchor_roots and n_trees := m.
 * k == 0 with m > 0 is the roots-at-counts call: d_anchor_ids, d_leaf_ids and the four opening arrays may be NULL.  m == 0 with k > 0:
 * every opening is bad (the four anchor arrays may be NULL).  m == 0 and k == 0 -> P252_OK, nothing enqueued.
 * P252_ERR_INVALID_ARGUMENT, nothing enqueued: n_leaves, n_trees or max_leaves == 0, a NULL or misaligned buffer (scalars 16 bytes,
 * d_offsets, the counts, d_leaf_ids and d_n_hashed 8, the ids and the two uint32 counters 4; d_levels, d_siblings and d_positions
 * may be NULL when max_leaves == 1), size overflow (m >= 2^32 among them), or an output range that overlaps an input range or
 * another output.  Asynchronous on hip_stream, no host synchronisation; scratch of the calling stream: the forest's index, 32 bytes
 * per anchor, the partial nodes (m x D x 32 bytes), 48 bytes per opening, one level's children (m x arity x 32 bytes).  The digests
 * run level by level through the library's digest launch, m nodes per level (an anchor with no partial node on a level digests zero
 * children there, and its result is not used); the lane-group or the one-lane build is chosen by m as for every digest batch. */
int p252_merkle4_forest_ragged_anchor_openings_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                                           const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                                           const void* d_anchor_tree_ids, const void* d_anchor_counts, size_t m,
                                                           const void* d_anchor_ids, const void* d_leaf_ids, size_t k, void* d_anchor_roots,
                                                           void* d_anchor_depths, void* d_leaves_out, void* d_siblings, void* d_positions,
                                                           void* d_depths, void* d_n_bad_anchors, void* d_n_bad, void* d_n_hashed,
                                                           void* hip_stream);
/* the same for arity 2 (the level layout of merkle2 trees; pass the Merkle2 tag) */
int p252_merkle2_forest_ragged_anchor_openings_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_leaves, size_t n_leaves,
                                                           const void* d_offsets, size_t n_trees, size_t max_leaves, const void* d_levels,
                                                           const void* d_anchor_tree_ids, const void* d_anchor_counts, size_t m,
                                                           const void* d_anchor_ids, const void* d_leaf_ids, size_t k, void* d_anchor_roots,
                                                           void* d_anchor_depths, void* d_leaves_out, void* d_siblings, void* d_positions,
                                                           void* d_depths, void* d_n_bad_anchors, void* d_n_bad, void* d_n_hashed,
                                                           void* hip_stream);

/* ---- runs: whole runs of leaves of the trees of a ragged forest, proved and checked in one call.  What the readers of a log fetch is
 * chunks: leaves [a, b) of a tree, checked against a root they trust.  Run r is leaves [a, a + len) of tree d_tree_ids[r] (uint32[m])
 * with a = d_first[r] (uint64[m]) and len = d_leaf_offsets[r + 1] - d_leaf_offsets[r] (uint64[m + 1]); its leaves sit at
 * d_leaf_offsets[r] of a flat array of k scalars, the layout of the ragged hash.  With A the arity, a_l = floor(a / A^l),
 * b_l = ceil(b / A^l) and w_l = ceil(n_t / A^l), the nodes of level l that a verifier knows or computes are the interval [a_l, b_l),
 * and the proof holds, level by level from the leaves up, the nodes [A a_{l+1}, a_l) left of it and then [b_l, min(A b_{l+1}, w_l))
 * right of it: at most 2 (A - 1) scalars a level.  That is byte for byte the proof p252_merkle{4,2}_multiproof_device writes for the
 * positions a .. b - 1 of the tree, and p252_merkle{4,2}_multiproof_verify_device accepts it; a run [0, n_t) has an empty proof.
 * A run is BAD when its leaf offsets are bad by the ragged forest's rule for tree offsets with k in the place of n_leaves (decreasing,
 * past k, the cumulative length of the runs before it and itself above k), len == 0, the tree id is >= n_trees, the tree is bad
 * (verification: the claimed count is not in 1 .. max_leaves), or a + len > n_t. */
/* P = 2 (arity - 1) * p252_merkle{4,2}_depth(max_leaves) scalars: room for the proof of any run of a tree of at most max_leaves leaves */
size_t p252_merkle4_forest_range_stride(size_t max_leaves);
size_t p252_merkle2_forest_range_stride(size_t max_leaves);
/* EXTRACTION (no hashing) out of a forest p252_merkle{4,2}_forest_ragged_device built with d_levels: d_leaves, n_leaves, d_offsets,
 * n_trees, max_leaves, d_levels exactly as the build took and filled them.  Row r of d_proof ([m][P] scalars, P = the stride above)
 * receives the proof of run r and zeros behind it, d_proof_lens[r] (uint32[m]) its length in scalars, d_counts_out[r] (uint64[m])
 * n_t, and d_leaves_out (k scalars, may be NULL), at d_leaf_offsets[r], the run's leaves byte for byte.  A BAD run: a zero row,
 * length 0xFFFFFFFF, count 0, no leaf written, counted once in *d_n_bad (device uint32 the caller has zeroed; may be NULL); its
 * neighbours are untouched.
 * P252_ERR_INVALID_ARGUMENT, nothing enqueued: m, k, n_leaves, n_trees or max_leaves == 0; k, m, k + 2 m or max_leaves >= 2^32
 * (record words are 32-bit); a NULL or misaligned buffer (scalars 16 bytes, d_offsets, d_first, d_leaf_offsets and d_counts_out 8,
 * d_tree_ids, d_proof_lens and d_n_bad 4; d_levels and d_proof may be NULL when max_leaves == 1); size overflow.  Asynchronous on
 * hip_stream, no host synchronisation; scratch of the calling stream (covered by p252_trim / p252_wipe): the forest's index
 * (16 bytes a tree), the runs' index and counts (32 bytes a run), 1 KiB. */
int p252_merkle4_forest_ragged_range_proofs_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                                        size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                                        const void* d_first, const void* d_leaf_offsets, size_t m, size_t k,
                                                        void* d_leaves_out, void* d_proof, void* d_proof_lens, void* d_counts_out,
                                                        void* d_n_bad, void* hip_stream);
/* the same for arity 2 (the level layout of merkle2 trees) */
int p252_merkle2_forest_ragged_range_proofs_device_into(p252_ctx* ctx, const void* d_leaves, size_t n_leaves, const void* d_offsets,
                                                        size_t n_trees, size_t max_leaves, const void* d_levels, const void* d_tree_ids,
                                                        const void* d_first, const void* d_leaf_offsets, size_t m, size_t k,
                                                        void* d_leaves_out, void* d_proof, void* d_proof_lens, void* d_counts_out,
                                                        void* d_n_bad, void* hip_stream);
/* VERIFICATION needs no forest, only the claimed leaf count of every run's tree: d_counts[r] (uint64[m]).  Every input is untrusted;
 * nothing is read outside row r's proof_stride scalars of d_proof, the k scalars of d_leaves_in or the m entries of the per-run arrays.
 * d_ok[r] (uint8[m]) = 1 iff run r is good against d_counts[r] (in 1 .. max_leaves), d_proof_lens[r] equals the closed-form length
 * and that length is <= proof_stride, and the run re-hashes to d_roots[d_tree_ids[r]] (n_trees roots) as 32 bytes; a one-leaf tree's
 * root is its leaf mod p, the forest's convention.  d_roots_out[r] ([m] scalars, may be NULL) is written when everything but the
 * comparison holds.  *d_n_hashed (device uint64, may be NULL) is SET to the digests computed: the nodes of [a_l, b_l), l >= 1, summed
 * over the runs that pass the first two conditions; a bad run is counted once in *d_n_bad (device uint32 the caller has zeroed; may
 * be NULL).  A claimed count that differs from the tree's own and leaves every w_l on the run's path alone changes nothing.
 * P252_ERR_INVALID_ARGUMENT, nothing enqueued: m, k, n_trees or max_leaves == 0; k, m, k + 2 m or max_leaves >= 2^32; a NULL or
 * misaligned buffer (scalars 16 bytes, d_counts, d_first, d_leaf_offsets and d_n_hashed 8, d_tree_ids, d_proof_lens and d_n_bad 4;
 * d_proof may be NULL when proof_stride == 0); size overflow.  Asynchronous on hip_stream, no host synchronisation, one record
 * launch and one digest launch per level of depth(max_leaves) whatever m is; scratch of the calling stream (covered by p252_trim /
 * p252_wipe): (64 + 8 depth) bytes a run, 84 bytes per node of the widest level above the leaves — at most
 * min(k + m, k / arity + 2 m) nodes —, 1 KiB. */
int p252_merkle4_forest_range_verify_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_tree_ids, const void* d_counts,
                                                 const void* d_first, const void* d_leaf_offsets, size_t m, size_t max_leaves,
                                                 const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_stride,
                                                 const void* d_proof_lens, const void* d_roots, size_t n_trees, void* d_ok,
                                                 void* d_roots_out, void* d_n_hashed, void* d_n_bad, void* hip_stream);
/* the same for arity 2 (pass the Merkle2 tag) */
int p252_merkle2_forest_range_verify_device_into(p252_ctx* ctx, const uint64_t tag[4], const void* d_tree_ids, const void* d_counts,
                                                 const void* d_first, const void* d_leaf_offsets, size_t m, size_t max_leaves,
                                                 const void* d_leaves_in, size_t k, const void* d_proof, size_t proof_stride,
                                                 const void* d_proof_lens, const void* d_roots, size_t n_trees, void* d_ok,
                                                 void* d_roots_out, void* d_n_hashed, void* d_n_bad, void* hip_stream);

/* ---- sequential updates: k leaf updates of a forest p252_merkle{4,2}_forest_ragged_device built with d_levels, applied IN ORDER in
 * one call, each with its witness — a block of transactions.  d_leaves, n_leaves, d_offsets, n_trees, max_leaves, d_levels, d_roots
 * exactly as p252_merkle{4,2}_forest_ragged_update_device takes them; the forest is updated in place.  Update i writes d_new_leaves[i]
 * to leaf d_leaf_ids[i] (uint64[k], a position inside the tree) of tree d_tree_ids[i] (uint32[k]) and sees the forest as updates
 * 0 .. i - 1 left it; the same pair may occur any number of times.  d_order (uint32[k]) is the indices 0 .. k - 1 sorted by (tree id,
 * leaf id, index) — the stable sort by pair, which p252_pairs_order_device_into makes; this call sorts nothing and checks the order on the device: every entry < k and
 * (tree id, leaf id, index) strictly ascending along it, which makes it a permutation.
 * The witness of update i, in the layout of p252_merkle{4,2}_forest_ragged_openings_device at stride D = depth(max_leaves):
 * d_old_leaves[i] ([k] scalars, may be NULL) the leaf as stored just before update i, byte for byte; d_siblings ([k][D][arity - 1]
 * scalars) and d_positions (uint8[k][D]) its opening in that state, rows at or past the tree's depth zero; d_depths[i] (uint8[k]) =
 * depth(n_t); d_roots_before[i] ([k] scalars, may be NULL) and d_roots_after[i] ([k] scalars) the tree's root just before and just
 * after update i: p252_merkle{4,2}_path_ragged_device over (old leaf, opening) gives the first and over (new leaf, the same opening)
 * the second, and d_roots_before[i] is d_roots_after of the previous update of that tree, or the built root.  A one-leaf tree's root
 * is its leaf mod p, the forest's convention.  Afterwards d_leaves and the used part of d_levels are byte for byte a fresh build of
 * the final leaves, and d_roots[t] ([n_trees] scalars, may be NULL) is rewritten for the trees that received a good update.
 * A BAD update (tree id >= n_trees, a bad tree, leaf id >= n_t) is skipped: zero witness rows and old leaf, depth 0xFF, both roots
 * zero, counted once in *d_n_bad (device uint32 the caller has zeroed; may be NULL); it changes nothing for the others.  An INVALID
 * d_order makes the batch one object: every d_depths[i] = 0xFF, *d_n_bad += k, the forest and every other output untouched.
 * *d_n_hashed (device uint64 the caller has zeroed; may be NULL) grows by depth(n_t) per good update — the digests the result needs;
 * the call computes k per level of D (updates of shallower trees and bad ones digest zeros above their root, results dropped).
 * P252_ERR_INVALID_ARGUMENT, nothing enqueued: k, n_leaves, n_trees or max_leaves == 0; k or max_leaves >= 2^32 (an index and a
 * node are 32-bit words of the sorted list); a NULL or misaligned buffer (scalars 16 bytes, d_offsets, d_leaf_ids and d_n_hashed 8,
 * d_tree_ids, d_order and d_n_bad 4; d_levels, d_siblings and d_positions may be NULL when max_leaves == 1); size overflow; an
 * output that overlaps an input, the forest or another output.  Asynchronous on hip_stream, no host synchronisation, no allocation
 * once the stream's scratch is warm: three launches per level of D (gather, digest, merge rank) and three more whatever k is.
 * Scratch of the calling stream (covered by p252_trim / p252_wipe): the forest's index (16 bytes a tree) and, per update, two sorted
 * lists of 16-byte keys with their 32-byte values, the parents' values, the gathered children and two rank words per child slot:
 * 128 + 40 arity bytes an update (288 at arity 4, 208 at arity 2), 256 bytes. */
int p252_merkle4_forest_ragged_update_sequential_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves,
                                                             const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels,
                                                             const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves,
                                                             const void* d_order, size_t k, void* d_old_leaves, void* d_siblings,
                                                             void* d_positions, void* d_depths, void* d_roots_before, void* d_roots_after,
                                                             void* d_roots, void* d_n_bad, void* d_n_hashed, void* hip_stream);
/* the same for arity 2 (the level layout of merkle2 trees; pass the Merkle2 tag) */
int p252_merkle2_forest_ragged_update_sequential_device_into(p252_ctx* ctx, const uint64_t tag[4], void* d_leaves, size_t n_leaves,
                                                             const void* d_offsets, size_t n_trees, size_t max_leaves, void* d_levels,
                                                             const void* d_tree_ids, const void* d_leaf_ids, const void* d_new_leaves,
                                                             const void* d_order, size_t k, void* d_old_leaves, void* d_siblings,
                                                             void* d_positions, void* d_depths, void* d_roots_before, void* d_roots_after,
                                                             void* d_roots, void* d_n_bad, void* d_n_hashed, void* hip_stream);

/* ---- the order of (tree id, leaf id) pairs, made on the device: what p252_merkle{4,2}_forest_ragged_update_sequential_device_into
 * takes as d_order, what p252_merkle{4,2}_multiproof_device takes as d_indices and what the forest's shared proofs take as their
 * pairs, from pairs in any order with any repeats.  Neither call depends on an arity.  d_leaf_ids is uint64[k]; d_tree_ids is
 * uint32[k], or NULL: every pair is of tree 0 (a single tree's positions).  The key of pair i is the 96-bit number (tree id, leaf
 * id), both parts compared as UNSIGNED, the full width counted: nothing is assumed about the values — a pair outside a forest is
 * its consumer's business.
 * p252_pairs_order_device_into writes d_order (uint32[k]): the indices 0 .. k - 1 sorted by (tree id, leaf id, index), the stable
 * sort by pair — the one permutation the sequential call checks and accepts.
 * p252_pairs_unique_device_into writes the distinct pairs, ascending, into the first *d_n_unique entries of every output that is
 * not NULL: d_tree_ids_out (uint32[k]) and d_leaf_ids_out (uint64[k]) the pair; d_indices_out (uint32[k]) the low word of its leaf
 * id, as the single tree's multiproof takes its positions; d_first (uint32[k]) the lowest input index that holds the pair — gather
 * through it whatever belongs to the pair.  *d_n_unique (a device uint64, required) is always written; entries at and past it are
 * left alone.  At least one of the four arrays must be given.
 * P252_ERR_INVALID_ARGUMENT, nothing enqueued: k == 0; k >= 2^32 (an index is a 32-bit word; no size overflows below that); a NULL
 * required buffer; a misaligned one (d_tree_ids, d_tree_ids_out, d_order, d_indices_out and d_first 4 bytes, d_leaf_ids,
 * d_leaf_ids_out and d_n_unique 8); an output that overlaps an input or another output.
 * The method is a stable radix sort over the 12 bytes of the key, least significant first; a byte that has one value in all k keys
 * costs no pass: its kernels leave at once on a device word (tree ids below 2^16 and leaf ids below 2^24: 5 passes of 12).
 * Asynchronous on hip_stream, no host synchronisation, no allocation once the stream's scratch is warm.  The number and the grids
 * of the launches depend on k alone — 3 + 3 * 12, and 3 more for the distinct pairs — never on the keys: a captured graph replays
 * correctly on other contents of the same buffers.  Scratch of the calling stream (covered by p252_trim / p252_wipe): two arrays of
 * 16-byte records {tree, index, leaf} and the per-tile digit counts, 256 words per 2,048 pairs: 32.5 bytes a pair, 1,280 bytes. */
int p252_pairs_order_device_into(p252_ctx* ctx, const void* d_tree_ids, const void* d_leaf_ids, size_t k, void* d_order, void* hip_stream);
int p252_pairs_unique_device_into(p252_ctx* ctx, const void* d_tree_ids, const void* d_leaf_ids, size_t k, void* d_tree_ids_out,
                                  void* d_leaf_ids_out, void* d_indices_out, void* d_first, void* d_n_unique, void* hip_stream);

/* ---- multi-device: an array of contexts, one per GPU.  Shards are contiguous and independent: no
 * inter-GPU dependence and no collective on the data path.  The calls are synchronous; inside, one host thread drives
 * each context.  A context may appear only once, and when the node has at least n_ctx devices no two contexts may be bound
 * to the same one (P252_MULTI_ALLOW_SHARED_DEVICE=1 lifts that).  The contexts share the process's CPU budget: each uses
 * p252_staging_lanes(n_ctx) staging lanes for pageable buffers.  On failure the error text is on ctxs[0] (p252_last_error). ---- */
/* n digests / sponges, item i of the batch on device floor-split: device t hashes a contiguous n/n_ctx slice (sizes
 * differ by at most one); per-item results identical to p252_hash_batch. */
int p252_hash_batch_multi(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const uint64_t* in, size_t in_len,
                          size_t out_len, uint64_t* out, size_t n);
/* the same on device-resident shards: d_in[t] / d_out[t] live on ctxs[t]'s device and hold n_per_ctx[t] items;
 * asynchronous on hip_streams[t] (hip_streams == NULL: every device's default stream); p252_sync each context. */
int p252_hash_batch_multi_device(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const void* const* d_in, size_t in_len,
                                 size_t out_len, void* const* d_out, const size_t* n_per_ctx, void* const* hip_streams);
/* Sharded arity-4 tree (BASELINE configs[4]: 2^27 leaves = 8 x 4^12): device t reduces the t-th contiguous run of
 * n_leaves / n_ctx leaves — which must be a complete subtree, 4^k leaves — to its root with zero communication; the
 * n_ctx roots (32 bytes each) are gathered on the host and the <= log4(n_ctx) + 1 top levels (zero-padded per
 * hash.rs:22-26) are hashed on ctxs[0].  root == p252_merkle4_tree over the concatenation.  Anything else than
 * n_leaves = n_ctx * 4^k -> P252_ERR_INVALID_ARGUMENT. */
int p252_merkle4_tree_multi(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const uint64_t* leaves, size_t n_leaves,
                            uint64_t root[4]);
/* the same with every device's leaves_per_ctx = 4^k leaves already resident at d_leaves[t]; root is written to host memory.
 * Contexts on distinct devices: the roots are exchanged by ONE ncclAllGather on the devices' streams (the RCCL communicator
 * over the contexts is created on the first such call — or beforehand with p252_comm_create_all — and kept; it is destroyed
 * with its contexts) and every device hashes the top levels, so nothing but the final 32 bytes crosses PCIe.  Contexts
 * that share a device (RCCL wants one device per rank: the single-GPU test configuration), or P252_MULTI_HOST_GATHER=1:
 * the roots are gathered through the host and the top levels run on ctxs[0].
 * ANY array of contexts is accepted, call after call (ctxs[0..8), then ctxs[0..4), a permutation ...): a communicator this
 * entry point made itself over another array is torn down and re-made for the array at hand (communicator creation costs
 * ~0.1-1 s: keep the array stable, or make the communicator once with p252_comm_create_all); contexts that sit in a
 * communicator the CALLER made over another array, and a failing lazy creation, fall back to the host gather.  n_ctx == 1
 * makes no communicator at all. */
int p252_merkle4_tree_multi_device(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const void* const* d_leaves,
                                   size_t leaves_per_ctx, uint64_t root[4]);
/* the RCCL path only, fully asynchronous and device-resident: on return the work is queued on hip_streams[t] (NULL: the
 * default streams) and d_root_out[t] (32 bytes on ctxs[t]'s device; entries, or the array, may be NULL) will hold the
 * root on EVERY device — no host round trip.  P252_ERR_COMM when the contexts cannot form a communicator (shared device,
 * P252_MULTI_HOST_GATHER=1, contexts of a caller-made communicator over another array, RCCL refusing): there is no host path here. */
int p252_merkle4_tree_multi_device_resident(p252_ctx* const* ctxs, size_t n_ctx, const uint64_t tag[4], const void* const* d_leaves,
                                            size_t leaves_per_ctx, void* const* d_root_out, void* const* hip_streams);

/* ---- RCCL communicator (BASELINE north_star: "RCCL broadcast of constants", "RCCL gather of roots").  The path
 * has no data-path collective; a communicator exists for (i) the constant table: on creation rank 0's table is broadcast
 * (ncclBroadcast) and every rank REFUSES it unless it equals the table it derives from its own arc.bin / mds.bin — the rule
 * of p252_tables_import — and (ii) the 32-byte subtree roots of a sharded tree build (ncclAllGather on the rank's stream).
 * One process per GPU: rank 0 calls p252_comm_unique_id and passes the bytes to the other ranks by any host means; every
 * rank calls p252_comm_create_rank with its own context (collective: returns when all `world` ranks have called).
 * One process, several GPUs: p252_comm_create_all over contexts on DISTINCT devices.  A context belongs to at most one
 * communicator; destroy the communicator before its context.  xGMI note: these messages are world x 32 bytes — latency
 * only.  Creation and the sharded build are COLLECTIVE: every rank calls them, in the same order.  Every device allocation
 * of a rank happens before its first collective, so a rank that cannot allocate fails before its peers wait for it; a rank
 * whose subtree build fails later still enters the all-gather (contributing an all-ones root, which is no BlsScalar) and
 * returns its error — peers are never left blocked on the stream.  The healthy ranks DETECT the sentinel on the device: their
 * d_root is overwritten with all-ones as well, and the next p252_comm_check / p252_sync on that rank returns P252_ERR_COMM
 * naming the failed rank (the build itself is asynchronous and has long returned P252_OK by then).  Builds of one communicator
 * queued on different streams run one after the other (event-ordered on the device), never concurrently.
 * RCCL is resolved at run time (ABI 8): without it these entry points return P252_ERR_COMM and p252_last_error lists what was
 * tried; nothing else in this header needs it. ---- */
int p252_comm_unique_id(void* id_out, size_t len /* = P252_COMM_ID_BYTES */);
int p252_comm_create_rank(p252_ctx* ctx, const void* id, size_t len, int rank, int world, p252_comm** out);
int p252_comm_create_all(p252_ctx* const* ctxs, size_t n_ctx, p252_comm** comms_out /* [n_ctx] */);
void p252_comm_destroy(p252_comm* comm);
int p252_comm_rank(const p252_comm* comm);
int p252_comm_size(const p252_comm* comm);
/* waits for hip_stream, then reports whether a sharded build of this communicator met a failed peer since the last check:
 * P252_ERR_COMM (p252_last_error names the rank) once, P252_OK otherwise */
int p252_comm_check(p252_comm* comm, void* hip_stream);
/* which RCCL this process's library calls go to: resolves it if no call has yet, writes the path of the object the symbols
 * came from (NUL-terminated, truncated to len; path_out may be NULL).  P252_ERR_COMM: none found (p252_last_error(NULL)) */
int p252_comm_backend(char* path_out, size_t len);
/* BASELINE configs[4], one rank's part (one process per GPU): this rank's n_leaves_local = 4^k device-resident leaves are
 * reduced to their root with zero communication, the `world` roots are all-gathered (the path's only exchange step, on
 * hip_stream) and the <= log4(world) + 1 top levels (zero-padded per hash.rs:22-26) are hashed on every rank: d_root
 * (32 bytes, device) = the root of the tree over the concatenation of all ranks' leaves, in rank order, on every rank.
 * Asynchronous on hip_stream; collective: every rank of the communicator must call it. */
int p252_merkle4_tree_sharded_device(p252_comm* comm, const uint64_t tag[4], const void* d_leaves, size_t n_leaves_local, void* d_root,
                                     void* hip_stream);

/* ---- constant-table exchange (multi-GPU: rank 0 broadcasts its derived table over RCCL, every
 * rank imports it; byte-identical to what p252_create derives locally) ---- */
size_t p252_tables_size(void);
int p252_tables_export(p252_ctx* ctx, void* host_buf, size_t len);
int p252_tables_import(p252_ctx* ctx, const void* host_buf, size_t len);

/* ---- host helpers mirroring src/hash.rs ---- */
/* From<Domain> for u64 (hash.rs:38-56) */
int p252_domain_separator(int domain, uint64_t* sep_out);
/* io_pattern() validation (hash.rs:62-85) + dusk-safe's pattern rules: 0, or
 * P252_ERR_IO_PATTERN_VIOLATION (Merkle arity mismatch), P252_ERR_INVALID_IO_PATTERN (no absorb,
 * zero-length call, out_len 0). */
int p252_check_io_pattern(int domain, const size_t* absorb_lens, size_t n_absorbs, size_t out_len);
/* UNPINNED convenience: tag = hash_to_scalar(tag_input(io_pattern, domain_sep)). */
int p252_tag(int domain, const size_t* absorb_lens, size_t n_absorbs, size_t out_len, uint64_t tag_out[4]);
/* finalize_truncated post-processing (hash.rs:164-183): canonical value & (2^250 - 1), as the raw
 * limbs handed to JubJubScalar::from_raw.  Host-side, n scalars. */
int p252_truncate250(const uint64_t* scalars, uint64_t* out_raw, size_t n);

/* host-side twins of p252_to_bytes_device / p252_from_bytes_device (no context, no GPU: one multiplication per scalar) */
int p252_to_bytes(const uint64_t* scalars, uint8_t* bytes, size_t n);
int p252_from_bytes(const uint8_t* bytes, uint64_t* scalars, uint8_t* ok, size_t n);

/* ---- measurement aids (bench.py; not on the hashing path) ---- */
/* Launches ONE wave on `hip_stream` that samples the shader-clock counter (s_memtime) and the constant 100 MHz real-time
 * counter (s_memrealtime) before and after sleeping for about spin_us microseconds, and writes
 * d_out6[6] (uint64, device) = {memtime0, realtime0, memtime after a chain of 1,024 dependent v_add_u32, memtime1, realtime1,
 * chain result}: (memtime1 - memtime0) / (realtime1 - realtime0) x 100 MHz = the shader clock over the interval.  On a stream
 * of its own while hashing kernels run it measures the clock under that load. */
int p252_clock_probe_device(p252_ctx* ctx, void* d_out6, unsigned spin_us, void* hip_stream);
/* staging lanes (worker threads) each context uses for pageable host buffers when n_ctx contexts are driven at once by a
 * p252_*_multi call: clamp(floor(usable CPUs / n_ctx), 1, 3) — the driver thread of a context is its first lane, so the
 * call never runs more workers than the process has CPUs (min(affinity, cgroup quota)); n_ctx <= 1: the single-context
 * default (3; 2 below four CPUs).  P252_HOST_LANES overrides both. */
int p252_staging_lanes(size_t n_ctx);

/* library/version introspection */
int p252_abi_version(void); /* P252_ABI_VERSION the library was built from */
const char* p252_version(void);

#ifdef __cplusplus
}
#endif
#endif
