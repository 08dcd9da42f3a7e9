/*
 * boojum_mi355x.h -- C ABI of the MI355X-native witness-commitment hot path
 * (coset LDE over Goldilocks + Poseidon2 Merkle tree with cap).
 *
 * Library: era-boojum_amd/boojum_amd/libboojum_mi355x.so (hipcc, gfx950).
 * Plain C types only: pointers, sizes, u64 field elements.  All field elements
 * crossing this boundary are u64; outputs are canonical (< p = 2^64 - 2^32 + 1),
 * inputs may be any u64 representative (as the reference's GoldilocksField,
 * field/goldilocks/mod.rs:92-94).
 *
 * Return value: 0 on success, a negative errno-style code on failure
 * (BJ_EINVAL for violated preconditions -- the reference asserts/panics on these,
 * fft/mod.rs:399-402, utils.rs:284-287, merkle_tree.rs:83-96 -- BJ_EHIP for a HIP
 * runtime error).  bj_last_error() gives a message for the calling thread.
 * A Rust/ctypes shim maps non-zero to panic!/raise, keeping reference semantics.
 *
 * Two families:
 *   *_d   device-resident batched entry points.  Pointers are device (HBM)
 *         pointers; `stream` is a hipStream_t (NULL = default stream).  Calls are
 *         asynchronous on the stream and never synchronise the device.  These are
 *         what a batched GPU prover calls once per commitment.
 *   *_h   host-pointer entry points with exactly the reference seam's per-call
 *         semantics (in place, synchronous), for drop-in replacement of the
 *         reference functions named in each comment.
 *
 * Thread safety: all entry points are re-entrant (the reference calls its FFT seam
 * concurrently from rayon workers, cs/implementations/utils.rs:295-304,363-379).
 * The only global state is a per-device cache of twiddle tables, filled under a
 * lock on first use of a size (bj_prepare fills it ahead of time; bj_release_tables, which must
 * not run concurrently with other calls, empties it).
 */
#ifndef BOOJUM_MI355X_H
#define BOOJUM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BJ_OK 0
#define BJ_EINVAL (-22)
#define BJ_ENOMEM (-12)
#define BJ_EHIP (-5)

/* Message for the last failure on the calling thread ("" if none). */
const char* bj_last_error(void);
/* ABI version (major << 16 | minor). */
uint32_t bj_abi_version(void);

/* The value in effect of one experiment knob (ABI 2.6; no reference counterpart).  The library's
 * same-binary A/B switches -- BJ_LEAVES_DEFER (default 0), BJ_LEAVES_GROUP (0: one chunk per
 * leaf grid), BJ_INV_FOLD_UNPAIRED (0),
 * BJ_LDE_PASSES (3), BJ_NODE_Q4_MAX (32768), BJ_NODE_FUSED (1) and BJ_LDE_OWN_FUSED (1) -- are read from the environment only when
 * BJ_EXPERIMENTS=1 is set, once per process at the first call that needs one; otherwise each
 * keeps its production value, so a prover's environment cannot change the kernel schedule (the
 * reference's transform_raw_storages_to_lde, cs/implementations/utils.rs:270-403, is a pure
 * function of its inputs).  Every setting gives the same outputs.  name "BJ_EXPERIMENTS" reports
 * the gate (0 / 1).  BJ_EINVAL for an unknown name.  Host-only: touches no device. */
int bj_experiment_knob(const char* name, uint64_t* value);

/* Fill the device twiddle cache for FFT size 2^log_n (forward + inverse tables) on the
 * current device, synchronously.  Twiddle precompute is outside the timed region in
 * the reference's own accounting (prover.rs:313-353 precomputes before "LDE taken").
 * Cached tables stay until bj_release_tables; for 2^13 <= n <= 2^26 a table of one coset shift
 * is n + 1056 (1 + n / 2^13) u64 (36 MiB at 2^22), and an LDE at degree D keeps D of them. */
int bj_prepare(uint32_t log_n);

/* Return the library's cached device workspace to the system (ABI 2.1; no reference
 * counterpart: the reference's Vec workspaces are freed when dropped).  The *_h calls, the
 * host-buffer commit, the collective commit and the LDE's own temporaries take their device
 * workspace from a stream-ordered pool private to the library (one per device); freed blocks
 * stay mapped for the next call (re-mapping C2's 5 GB after every call cost ~20 ms), so after a
 * large call the pool keeps that much reserved -- e.g. ~8.5 GB after a native C3 commit at N = 1.
 * This trims every device's pool to the blocks still in use (hipMemPoolTrimTo(pool, 0)); blocks
 * whose stream-ordered free has not completed yet are released by a later call.  Call it when a
 * long-running prover goes idle.  Twiddle tables (bj_prepare) are not affected. */
int bj_release_workspace(void);

/* Free every cached table (twiddles, coset powers, the LDE passes' factor tables) on every device
 * (ABI 2.3; no reference counterpart: the reference's twiddles are Vecs the caller drops).  The
 * cache only grows: an LDE of 2^22 rows at degree 4 keeps ~180 MiB, one of 2^23 at degree 8
 * ~600 MiB, and a prover that commits many sizes keeps the tables of each.  Each device with
 * tables is synchronised first, so work already queued there has finished with them; no other
 * library call may run concurrently with this one, and a HIP graph captured over library calls
 * holds table addresses, so it must be captured again afterwards.  Later calls rebuild what they
 * need (as on first use; bj_prepare rebuilds ahead of time). */
int bj_release_tables(void);

/* ---------------------------------------------------------------- FFT seam */

/* precompute_twiddles_for_fft::<INVERSED> (cs/implementations/utils.rs:88-125,
 * wrapper fft/mod.rs:625-641): omega_n^i (or omega_n^-i), i < n/2, bit-reversed order.
 * out_d: n/2 u64 (device). */
int bj_precompute_twiddles_d(uint32_t log_n, int inverse, uint64_t* out_d, void* stream);
int bj_precompute_twiddles_h(uint32_t log_n, int inverse, uint64_t* out_h);

/* precompute_twiddles_for_fft_natural (cs/implementations/utils.rs:127-155, wrapper
 * fft/mod.rs:640-657): w^i (or w^-i) for i < n/2 in natural order, canonical; out_d has n/2
 * u64 on the device. */
int bj_precompute_twiddles_natural_d(uint32_t log_n, int inverse, uint64_t* out_d, void* stream);

/* bitreverse_enumeration_inplace (fft/mod.rs:41-155): the bit-reversal permutation of each of
 * n_cols columns of n = 2^log_n, in place; values are moved unchanged. */
int bj_bitreverse_enumeration_d(uint64_t* cols, uint32_t n_cols, size_t col_stride, uint32_t log_n, void* stream);

/* distribute_powers (fft/mod.rs:308-317): col[j] *= element^j, for n_cols columns of
 * 2^log_n elements, column c at cols + c * col_stride. */
int bj_distribute_powers_d(uint64_t* cols, uint32_t n_cols, size_t col_stride, uint32_t log_n,
                           uint64_t element, void* stream);
int bj_distribute_powers_h(uint64_t* col, size_t len, uint64_t element);

/* fft_natural_to_bitreversed (fft/mod.rs:398-411; PrimeFieldLikeVectorized seam
 * field/traits/field_like.rs:111-162): distribute_powers(coset) if coset != 1, then the
 * radix-2 natural->bit-reversed transform (fft/mod.rs:659-734).  In place.
 * twiddles may be NULL (the device cache is used); if given it must be the
 * bj_precompute_twiddles output for this size (it is used as is). */
int bj_fft_natural_to_bitreversed_d(uint64_t* cols, uint32_t n_cols, size_t col_stride, uint32_t log_n,
                                    uint64_t coset, const uint64_t* twiddles_d, void* stream);
int bj_fft_natural_to_bitreversed_h(uint64_t* col, size_t len, uint64_t coset);

/* ifft_natural_to_natural (fft/mod.rs:464-491): inverse transform, bit-reverse, times
 * coset^-j if coset != 1, times n^-1.  In place. */
int bj_ifft_natural_to_natural_d(uint64_t* cols, uint32_t n_cols, size_t col_stride, uint32_t log_n,
                                 uint64_t coset, const uint64_t* inv_twiddles_d, void* stream);
int bj_ifft_natural_to_natural_h(uint64_t* col, size_t len, uint64_t coset);

/* ------------------------------------------------------------------- LDE */

/* transform_raw_storages_to_lde (cs/implementations/utils.rs:270-309 + :311-403, as
 * driven by WitnessStorage::from_base_trace*, witness_storage.rs:18-116):
 *   monomials[c] = ifft_natural_to_natural(trace[c])
 *   lde[c][i]    = fft_natural_to_bitreversed(monomials[c], 7 * w_{nD}^{bitrev(i)})
 * trace:   n_cols columns of n = 2^log_n at trace + c * trace_stride (read only)
 * scratch: n_cols x n device workspace (on return it holds the monomials in bit-reversed
 *          order, c_j at bitrev_n(j) -- the format of bj_lde_coeffs_d)
 * lde:     n_cols x D x n, element (c, i, r) at lde + (c * D + i) * n + r
 *          (the reference's per-column Vec<coset> of ArcGenericLdeStorage)
 * D = 2^log_lde. */
int bj_lde_d(const uint64_t* trace, uint32_t n_cols, size_t trace_stride, uint32_t log_n,
             uint32_t log_lde, uint64_t* scratch, uint64_t* lde, void* stream);

/* bj_lde_d with flags (ABI 2.2).  Without BJ_LDE_KEEP_MONOMIALS, scratch is workspace only and
 * its contents on return are unspecified -- the reference's transform_raw_storages_to_lde
 * (utils.rs:270-403) returns the LDE alone and drops the monomials, and the three-pass path
 * (2^18 <= n <= 2^23) then skips writing them (one pass over n words per column less).
 * bj_lde_d == bj_lde_ex_d(..., BJ_LDE_KEEP_MONOMIALS, ...).  Unknown flags: BJ_EINVAL. */
#define BJ_LDE_KEEP_MONOMIALS 1u
int bj_lde_ex_d(const uint64_t* trace, uint32_t n_cols, size_t trace_stride, uint32_t log_n,
                uint32_t log_lde, uint64_t* scratch, uint64_t* lde, uint32_t flags, void* stream);

/* Coset LDE of already-monomial columns (transform_monomials_to_lde, utils.rs:311-403;
 * also the quotient commit path prover.rs:1471-1482).  monomials read only. */
int bj_monomials_to_lde_d(const uint64_t* monomials, uint32_t n_cols, size_t mono_stride, uint32_t log_n,
                          uint32_t log_lde, uint64_t* lde, void* stream);

/* ------------------------------------------------ coset-sharded LDE (8(e)) */
/* The multi-GPU split of transform_raw_storages_to_lde (utils.rs:270-403) over G = 2^log_shards
 * ranks: the flat leaf domain L = coset * n + row (merkle_tree.rs:112-157 leaf order) is cut
 * into G contiguous ranges of m = n*D/G leaves; rank P owns [P*m, (P+1)*m).
 *
 * Step 1 (every rank, its own trace columns): bj_lde_coeffs_d writes the inverse transform
 *   in the exchange format: column c holds c_j at position bitrev_n(j), where c_j are the
 *   monomials of ifft_natural_to_natural (utils.rs:295-304), canonical.  Ranks all-gather
 *   these columns.
 * Step 2 (every rank, all columns): bj_lde_shard_d evaluates its leaf range:
 *   G <= D: cosets [P*D/G, (P+1)*D/G), each as in bj_lde_d;
 *   G >  D: rows [q*m, (q+1)*m) of coset i = P / (G/D), q = P mod (G/D), as an m-point coset
 *           FFT of the coefficients folded mod Y^m - s'^m, s' = 7 * w_{nD}^{bitrev_{log G}(P)}.
 *   lde: n_cols x m, element (c, L - P*m) at lde + c * m + (L - P*m), identical to the slice
 *   of bj_lde_d's output for those leaves.  work: n_cols x m device scratch (G > D only;
 *   may be NULL when G <= D).  Requires log_shards <= log_n + log_lde and, for G > D,
 *   G / D <= 64. */
int bj_lde_coeffs_d(const uint64_t* trace, uint32_t n_cols, size_t trace_stride, uint32_t log_n,
                    uint64_t* coeffs, size_t coeffs_stride, void* stream);
int bj_lde_shard_d(const uint64_t* coeffs, uint32_t n_cols, size_t coeffs_stride, uint32_t log_n,
                   uint32_t log_lde, uint32_t log_shards, uint32_t shard, uint64_t* work, uint64_t* lde,
                   void* stream);

/* G > D with the fold moved to the sender (all-to-all exchange of m-length columns instead of
 * an all-gather of n-length ones: n/m = G/D times fewer bytes on the wire).
 * bj_lde_fold_shards_d (every rank, its own columns in the bj_lde_coeffs_d format): for every
 *   shard P < G, out + P * out_shard_stride + c * m receives column c folded mod
 *   Y^m - s_P^m, bit-reversed (the h of bj_lde_shard_d's fold step); out_shard_stride >=
 *   n_cols * m.
 * bj_lde_shard_folded_d (rank P, every column folded for P, gathered from all ranks): the
 *   m-point coset transform of the folded columns, the same leaf range and layout as
 *   bj_lde_shard_d.  folded read only. */
int bj_lde_fold_shards_d(const uint64_t* coeffs, uint32_t n_cols, size_t coeffs_stride, uint32_t log_n,
                         uint32_t log_lde, uint32_t log_shards, uint64_t* out, size_t out_shard_stride,
                         void* stream);
int bj_lde_shard_folded_d(const uint64_t* folded, uint32_t n_cols, size_t folded_stride, uint32_t log_n,
                          uint32_t log_lde, uint32_t log_shards, uint32_t shard, uint64_t* lde, void* stream);

/* ---------------------------------------------------------- Poseidon2 / Merkle */

/* poseidon2_permutation (implementations/poseidon2/state_generic_impl.rs:221-249) on
 * `count` independent 12-element states, in place. */
int bj_poseidon2_permute_d(uint64_t* states, size_t count, void* stream);
int bj_poseidon2_permute_h(uint64_t* state12);

/* TreeHasher::hash_into_leaf for GoldilocksPoseidon2Sponge<AbsorptionModeOverwrite>
 * (cs/oracle/mod.rs:141-151, algebraic_props/sponge.rs:224-323) of n_elems elements. */
int bj_hash_into_leaf_h(const uint64_t* elems, size_t n_elems, uint64_t* out4);
/* TreeHasher::hash_into_node (cs/oracle/mod.rs:162-168). */
int bj_hash_into_node_h(const uint64_t* left4, const uint64_t* right4, uint64_t* out4);

/* Leaf hashing of MerkleTreeWithCap::construct (cs/oracle/merkle_tree.rs:78-172):
 * leaf L (flat index coset * n + row) = hash_into_leaf(src[0][L], ..., src[n_cols-1][L]),
 * column c's leaf-domain values at src + c * col_stride.  leaves: n_leaves x 4. */
int bj_merkle_leaves_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                       uint64_t* leaves, void* stream);

/* Leaf hashing of MerkleTreeWithCap::construct_by_chunking (merkle_tree.rs:176-306) and
 * construct_by_chunking_from_flat_sources (:308-386), the FRI oracles' trees (fri/mod.rs:179-187,
 * 258-266): leaf L = hash_into_leaf of, for each column c in order, the elems_per_leaf
 * consecutive elements src[c * col_stride + L * elems_per_leaf + t].  elems_per_leaf is a power
 * of two.  With a [c][coset][row] LDE the flat leaf index runs over the cosets in order, as the
 * reference's per-coset chunks do.  leaves: n_leaves x 4. */
int bj_merkle_leaves_chunked_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                               uint32_t elems_per_leaf, uint64_t* out, void* stream);

/* Leaf hashing over a column range, continuing a sponge (the column-pipelined multi-GPU
 * commit absorbs column chunks as they arrive).  The Overwrite sponge replaces the rate words
 * with each 8-element group, so between groups its whole carried state is the capacity
 * state[8..12].  cap_in: NULL for a fresh sponge (zero state), else n_leaves x 4 capacity words
 * from a previous non-final call.  final_ == 0: n_cols must be a multiple of 8; out receives
 * the capacity words (n_leaves x 4, canonical).  final_ != 0: the remaining columns are
 * absorbed with the reference's padding (sponge.rs:300-323) and out receives the digests, as
 * bj_merkle_leaves_d.  cap_in == out is allowed.  Chaining calls over columns [0, k), [k, C)
 * gives exactly bj_merkle_leaves_d over [0, C). */
int bj_merkle_leaves_partial_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                               const uint64_t* cap_in, uint64_t* out, int final_, void* stream);

/* continue_from_leaf_hashes (merkle_tree.rs:388-449): node levels from n_leaves leaves
 * up to cap_size nodes.  nodes: (n_leaves - cap_size) x 4, the levels concatenated from
 * the leaves upward (node_hashes_enumerated_from_leafs); the cap is the last cap_size
 * digests (get_cap, merkle_tree.rs:451-460, canonical).  Requires n_leaves > cap_size,
 * both powers of two. */
int bj_merkle_nodes_d(const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes,
                      void* stream);

/* ------------------------------------------------ Blake2s256 tree hasher */
/* MerkleTreeWithCap<GoldilocksField, blake2::Blake2s256>: the TreeHasher impl of
 * cs/oracle/mod.rs:179-245, used by the non-recursive prover configs
 * (gadgets/sha256/mod.rs:263-269).  Leaf = BLAKE2s-256 (RFC 7693, no key) of the canonical
 * little-endian bytes of the leaf's elements (as_u64_reduced().to_le_bytes(), :194-197);
 * node = BLAKE2s-256(left || right) (:233-245).  A digest is 32 bytes, stored as 4
 * little-endian u64 words, so leaves / nodes use the same (N x 4) layout as the Poseidon2
 * tree.  Same arguments, layouts and preconditions as the bj_merkle_* calls above. */
int bj_blake2s_leaves_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                        uint64_t* leaves, void* stream);
int bj_blake2s_leaves_chunked_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                                uint32_t elems_per_leaf, uint64_t* out, void* stream);
int bj_blake2s_nodes_d(const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes,
                       void* stream);
/* Column-range continuation (the column pipeline): the carried state is the 32-byte chaining
 * value h plus the byte count, which is 8 * cols_before (a multiple of 64).  state_in: NULL iff
 * cols_before == 0.  final_ == 0: n_cols a multiple of 8, out = chaining values (n_leaves x 4);
 * final_ != 0: out = digests, and n_cols > 0 when cols_before > 0 (the message's last block
 * must be in this range). */
int bj_blake2s_leaves_partial_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                                uint64_t cols_before, const uint64_t* state_in, uint64_t* out, int final_,
                                void* stream);
/* host seams (TreeHasher::hash_into_leaf / hash_into_node) */
int bj_blake2s_leaf_h(const uint64_t* elems, size_t n_elems, uint64_t* out4);
int bj_blake2s_node_h(const uint64_t* left4, const uint64_t* right4, uint64_t* out4);

/* ---------------------------------------------- Keccak256 tree hasher */
/* MerkleTreeWithCap<GoldilocksField, sha3::Keccak256>: the TreeHasher impl of
 * cs/oracle/mod.rs:247-313.  Leaf = Keccak256 (rate 136 bytes, domain byte 0x01) of the
 * canonical little-endian bytes of the leaf's elements; node = Keccak256(left || right).
 * Digests are 32 bytes as 4 little-endian u64 words.  Same arguments, layouts and
 * preconditions as the bj_merkle_* calls. */
int bj_keccak256_leaves_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                          uint64_t* leaves, void* stream);
int bj_keccak256_leaves_chunked_d(const uint64_t* src, uint32_t n_cols, size_t col_stride, size_t n_leaves,
                                  uint32_t elems_per_leaf, uint64_t* out, void* stream);
int bj_keccak256_nodes_d(const uint64_t* leaves, size_t n_leaves, uint32_t cap_size, uint64_t* nodes,
                         void* stream);
int bj_keccak256_leaf_h(const uint64_t* elems, size_t n_elems, uint64_t* out4);
int bj_keccak256_node_h(const uint64_t* left4, const uint64_t* right4, uint64_t* out4);

/* ------------------------------------------------------- whole commitment */

/* Witness commitment, the batched hot path (prover.rs:313-353): the LDE of every column at
 * D = 2^log_lde (used_lde_degree = max(fri_lde_factor, quotient_degree), prover.rs:313), then
 * MerkleTreeWithCap::construct over the first k = 2^log_commit_cosets cosets only
 * (source = subset_for_degree(fri_lde_factor), prover.rs:325-347, polynomial/lde.rs:298-308):
 * leaf L = coset * n + row < k * n, node levels to the cap.  log_commit_cosets <= log_lde; the
 * reference's own proof.json is D = 8 (quotient degree), k = 2 (fri_lde_factor).
 *   scratch  n_cols x n (monomials, as bj_lde_d)
 *   lde      n_cols x D x n, all D cosets (as bj_lde_d)
 *   leaves   k*n x 4;  nodes (k*n - cap_size) x 4, the cap being the last cap_size digests
 * All pointers device; cap additionally copied to cap_h (host, cap_size x 4) if non-NULL
 * (this synchronises the stream).  Requires power-of-two cap_size < k * n. */
int bj_lde_commit_d(const uint64_t* trace, uint32_t n_cols, size_t trace_stride, uint32_t log_n,
                    uint32_t log_lde, uint32_t log_commit_cosets, uint32_t cap_size, uint64_t* scratch,
                    uint64_t* lde, uint64_t* leaves, uint64_t* nodes, uint64_t* cap_h, void* stream);

/* bj_lde_commit_d with flags (ABI 2.4): with BJ_LDE_KEEP_MONOMIALS scratch receives the
 * monomials (bj_lde_d's contract); without it scratch is workspace only, as
 * transform_raw_storages_to_lde drops them (utils.rs:270-403), and the middle LDE pass skips
 * their write-back.  bj_lde_commit_d == bj_lde_commit_ex_d(..., BJ_LDE_KEEP_MONOMIALS, ...).
 * Unknown flags: BJ_EINVAL. */
int bj_lde_commit_ex_d(const uint64_t* trace, uint32_t n_cols, size_t trace_stride, uint32_t log_n,
                       uint32_t log_lde, uint32_t log_commit_cosets, uint32_t cap_size, uint64_t* scratch,
                       uint64_t* lde, uint64_t* leaves, uint64_t* nodes, uint64_t* cap_h, uint32_t flags,
                       void* stream);

/* Host-buffer variant (drop-in for a Rust prover that owns host Vecs): the trace goes in,
 * bj_lde_commit_d's pipeline runs column chunk by column chunk, every output comes back (lde_h
 * n_cols x D x n, leaves_h k*n x 4, nodes_h, cap_h).  Any output pointer may be NULL to skip its
 * copy.  Device workspace comes from the library's own stream-ordered pool (the process's default
 * pool is not touched); pinned staging (3 x 64 MiB + 3 streams per set) comes from a per-device
 * pool of at most 4 sets shared by all calling threads.  PCIe-inclusive; never the headline. */
int bj_lde_commit_h(const uint64_t* trace_h, uint32_t n_cols, uint32_t log_n, uint32_t log_lde,
                    uint32_t log_commit_cosets, uint32_t cap_size, uint64_t* lde_h, uint64_t* leaves_h,
                    uint64_t* nodes_h, uint64_t* cap_h);

/* ------------------------------------- collective sharded commit (8(b), 8(e)) */
/* The whole G-rank witness commitment as one collective call per rank: one process (or
 * thread) per GPU, each calling bj_sharded_commit_d on its own column shard with its own
 * communicator.  It runs the column pipeline of DESIGN.md section 7 natively: local iNTTs,
 * per-chunk exchange on a high-priority stream (G <= D: all-gather of coefficients; G > D:
 * sender-side fold + all-to-all), this rank's coset/sub-coset LDE, the chained leaf sponge,
 * the subtree and the cap all-gather.  It replaces MerkleTreeWithCap::construct over
 * transform_raw_storages_to_lde (utils.rs:270-403, merkle_tree.rs:78-172, prover.rs:313-353)
 * with the leaf domain split over the ranks.
 *
 * Communicators (opaque bj_comm):
 *   bj_comm_rccl_unique_id  ncclGetUniqueId (128 bytes); rank 0 creates it and the caller
 *                           broadcasts it by its own means (torch.distributed, MPI, a file);
 *   bj_comm_init_rccl       ncclCommInitRank on the current device (collective, blocking);
 *   bj_comm_wrap_rccl       an ncclComm_t the caller already owns (not destroyed by us);
 *   bj_comm_local_*         in-process ranks that share one device (threads; device-to-device
 *                           copies through a host barrier): a rehearsal transport that runs the
 *                           same pipeline multi-rank on one GPU.  Not for performance.  If a rank
 *                           fails mid-collective the group is aborted: its peers return an error
 *                           instead of waiting, and the group must be destroyed;
 *   bj_comm_init_callback   the caller's own exchange (gloo, MPI, a test double), called for
 *                           every data exchange from the thread that called the collective.
 *                           kind BJ_XCHG_ALL_GATHER: recv (world x bytes) <- concat over ranks of
 *                           send (bytes); BJ_XCHG_ALL_TO_ALL: recv block p (bytes) <- block `rank`
 *                           of rank p's send (world x bytes).  host_staged != 0: send / recv are
 *                           host buffers (the library synchronises, copies out, calls, copies
 *                           back; stream is NULL).  host_staged == 0: device pointers, and the
 *                           exchange must be ordered on `stream`.  Returns 0 on success.
 * RCCL is resolved at run time (dlopen of librccl.so.1, reusing an already loaded copy), so the
 * library loads without it.  All ranks must call collectives in the same order. */
typedef struct bj_comm bj_comm;
#define BJ_XCHG_ALL_GATHER 0
#define BJ_XCHG_ALL_TO_ALL 1
typedef int (*bj_exchange_fn)(void* user, int kind, const void* send, void* recv, size_t bytes, void* stream);
int bj_comm_rccl_unique_id(uint8_t* id_out128);
int bj_comm_init_rccl(const uint8_t* id128, int world, int rank, bj_comm** out);
int bj_comm_wrap_rccl(void* nccl_comm, int world, int rank, bj_comm** out);
int bj_comm_local_group_create(int world, void** group_out);
int bj_comm_local_group_destroy(void* group);
int bj_comm_init_local(void* group, int rank, bj_comm** out);
int bj_comm_init_callback(int world, int rank, bj_exchange_fn exchange, void* user, int host_staged, bj_comm** out);
int bj_comm_destroy(bj_comm* comm);
/* What a communicator's transport sees (ABI 2.5; no reference counterpart: the reference has no
 * collectives).  kind: BJ_COMM_RCCL / BJ_COMM_LOCAL / BJ_COMM_CALLBACK; world, rank: as the
 * communicator was made; transport_count, transport_rank, device: RCCL's own ncclCommCount,
 * ncclCommUserRank and ncclCommCuDevice (the other transports: world, rank and the device current
 * when the communicator was made); pci_bus_id: hipDeviceGetPCIBusId of that device ("" when this
 * process cannot open it); host: gethostname.  128 bytes. */
#define BJ_COMM_RCCL 0
#define BJ_COMM_LOCAL 1
#define BJ_COMM_CALLBACK 2
#define BJ_COMM_INVALID (-1) /* bj_comm_check_world: the rank could not read its record; reserved[0] = its error */
typedef struct bj_comm_info_t {
    int32_t kind;
    int32_t world, rank;
    int32_t transport_count, transport_rank;
    int32_t device;
    char pci_bus_id[32];
    char host[64];
    int32_t reserved[2];
} bj_comm_info_t;
int bj_comm_info(bj_comm* comm, bj_comm_info_t* out);
/* Collective over `comm` (ordered on `stream`, as bj_comm_exchange_d): all-gathers every rank's
 * bj_comm_info_t into all_out[world] and checks the world the transport formed: slot p holds rank
 * p, and every rank's transport count and rank equal the communicator's world and rank; for RCCL
 * also that no two ranks drive one device (same host and PCI bus id, or same device number where
 * the bus id is unknown).  BJ_EINVAL naming the ranks otherwise (all_out is filled either way once
 * the gather ran).  The local and callback transports may share a device by design.  A rank whose
 * own bj_comm_info fails still enters the gather with a record of kind BJ_COMM_INVALID, so every
 * rank returns BJ_EINVAL; only a failed device allocation (128 * (world + 1) bytes) returns before
 * the gather, and then the peers wait in the transport's collective. */
int bj_comm_check_world(bj_comm* comm, bj_comm_info_t* all_out, void* stream);
/* One data exchange of bj_sharded_commit_d's kinds (BJ_XCHG_ALL_GATHER / BJ_XCHG_ALL_TO_ALL, the
 * layouts above) over `comm`, ordered on `stream`: the transport alone, so a caller can check its
 * communicator before a commit.  Collective; bytes per rank block, a multiple of 8.  An RCCL
 * communicator issues the RCCL call even at world 1 (ncclAllGather; grouped ncclSend/ncclRecv). */
int bj_comm_exchange_d(bj_comm* comm, int kind, const void* send, void* recv, size_t bytes, void* stream);
/* Phase timing of bj_sharded_commit_d on this communicator (no reference counterpart: the
 * reference logs its phase times, merkle_tree.rs:162-167, prover.rs:345).  on != 0: every later
 * call records HIP events on its compute stream around the inverse transforms (+ folds), the
 * LDE evaluations, the leaf hashing and the subtree + cap; waits for the exchange are outside
 * every interval.  Each call first sums the intervals of earlier calls that have completed and
 * frees their events, so the events held are those of calls still in flight.  bj_comm_phase_ms
 * waits for the recorded calls, writes the summed milliseconds {inverse, lde, leaves, nodes} to
 * ms_out[4] and their count to *calls_out, and starts a new sum.  The events cost a little time
 * on the compute stream: time production steps with timing off. */
int bj_comm_set_timing(bj_comm* comm, int on);
int bj_comm_phase_ms(bj_comm* comm, float* ms_out4, int* calls_out);

#define BJ_HASHER_POSEIDON2 0
#define BJ_HASHER_BLAKE2S 1
#define BJ_HASHER_KECCAK256 2

/* Which global trace columns rank `shard` of G = 2^log_shards holds, in the order of its
 * trace_shard rows: the column pipeline deals chunk k (G * c_k consecutive columns, u = 8 /
 * gcd(8, G), c = u, u, then 3/2 (G <= 4) or 2 (G >= 8) times the previous rounded down to u but
 * at least u more, capped at 32 rounded to u) as G runs of c_k; when n_cols / G
 * is not a multiple of u, or the hasher cannot be continued over column ranges (Keccak256),
 * rank P holds columns [P * n_cols / G, (P + 1) * n_cols / G).  cols_out: n_cols / G entries.
 * Host only (no device call). */
int bj_sharded_columns(uint32_t n_cols, uint32_t log_shards, uint32_t shard, int hasher, uint32_t* cols_out);

/* Rank P's part of the G-way commit (G = the communicator's world, a power of two; P its rank).
 * The LDE is at D = 2^log_lde, the tree over the first k = 2^log_commit_cosets cosets
 * (bj_lde_commit_d; prover.rs:313-347).  The committed domain of m_k = k * n leaves is cut into
 * G ranges of m = k * n / G; rank P owns leaf range [P * m, (P + 1) * m) and, so that the LDE
 * work stays balanced, the same range of every other block of k cosets: block j (cosets
 * [j*k, (j+1)*k), j < B = D / k) of the D-coset LDE is itself a k-coset LDE with an extra shift,
 * and rank P holds its part [P * m, (P + 1) * m).
 * trace_shard: n_cols / G columns of n = 2^log_n in bj_sharded_columns order at
 *              trace_shard + j * trace_stride (device, read only).
 * Outputs (device):
 *   lde    B x n_cols x m: block j, global column c at lde + (j * n_cols + c) * m; block 0 is the
 *          committed one, equal to lde_full[c][P*m .. (P+1)*m) of bj_lde_commit_d's flat
 *          coset * n + row index; block j to lde_full[c][j*k*n + P*m ..];
 *   leaves m x 4;
 *   nodes  (m - cap_local) x 4, the subtree levels, cap_local = max(1, cap_size / G);
 *   cap    cap_size x 4, the full gathered cap (identical on every rank).
 * Exchange: G <= D all-gather of the coefficients (8 n n_cols bytes in total); G > D the sender
 * folds its columns for every (block, rank) and all-to-alls deliver them (8 n D / G n_cols bytes
 * received per rank).  Requires n_cols % G == 0, log_lde >= 1, log_commit_cosets <= log_lde,
 * G <= k * n, G / k <= 64, power-of-two cap_size < k * n, m > cap_local.  Asynchronous on
 * `stream`; workspace comes from the library's stream-ordered pool. */
int bj_sharded_commit_d(bj_comm* comm, const uint64_t* trace_shard, size_t trace_stride, uint32_t n_cols,
                        uint32_t log_n, uint32_t log_lde, uint32_t log_commit_cosets, uint32_t cap_size,
                        int hasher, uint64_t* lde, uint64_t* leaves, uint64_t* nodes, uint64_t* cap, void* stream);

/* OracleQuery::construct (proof.rs:65-97) on a bj_sharded_commit_d commit: tree index idx < k * n
 * (flat leaf index coset * n + row of the committed cosets) of the global tree.  The owning rank
 * reads the row of every column and its subtree path; when cap_size < G the top levels over the
 * gathered subtree roots finish the path on every rank.  Collective: every rank passes its own
 * commit outputs and the same idx, and every rank receives, in host memory, leaf_elements
 * (n_cols), leaf_hash (4) and proof (depth x 4, depth = log2(k * n / cap_size),
 * MerkleTreeWithCap::get_proof order, merkle_tree.rs:462-480).  Synchronous. */
int bj_sharded_query_h(bj_comm* comm, const uint64_t* lde, const uint64_t* leaves, const uint64_t* nodes,
                       uint32_t n_cols, uint32_t log_n, uint32_t log_lde, uint32_t log_commit_cosets,
                       uint32_t cap_size, int hasher, uint64_t idx, uint64_t* leaf_elements_h,
                       uint64_t* leaf_hash_h, uint64_t* proof_h, void* stream);

/* ------------------------------------------------------------------- FRI */

/* One FRI fold by 2 of a GoldilocksExt2 codeword stored as base columns c0, c1 of n_src
 * bit-reversed values (fold_multiple, cs/implementations/fri/mod.rs:362-474, as driven by
 * interpolate_independent_cosets :476-585 and interpolate_flattened_cosets :587-682):
 *   dst_i = f(x) + f(-x) + alpha * (f(x) - f(-x)) * roots[i] * coset_inverse,  i < n_src / 2,
 * f(x) = (c0[2i], c1[2i]), f(-x) = (c0[2i+1], c1[2i+1]), alpha = (ch0, ch1), u^2 = 7.
 * roots: the INVERSED bit-reversed twiddles of the full FRI domain (bj_precompute_twiddles_d
 * with inverse = 1), indexed by the flat pair index.  Device pointers; outputs canonical.
 * c0 / c1 at 16-byte-aligned addresses load each (f(x), f(-x)) pair as one 16-byte load; any
 * other 8-byte-aligned address runs the same fold with 8-byte loads. */
int bj_fri_fold_d(const uint64_t* c0, const uint64_t* c1, size_t n_src, const uint64_t* roots,
                  uint64_t coset_inverse, uint64_t ch0, uint64_t ch1, uint64_t* dst_c0, uint64_t* dst_c1,
                  void* stream);

/* One FRI reduction step, a fold by 2^log_fold (log_fold = 1, 2 or 3, the range do_fri allows,
 * fri/mod.rs:204-205), in one launch.  Added after 2.6; detect by symbol (bj_abi_version() is
 * unchanged).  dst_j, j < n_src / 2^log_fold, is the result of log_fold successive fold_multiple
 * steps over the 2^log_fold consecutive values [2^log_fold j, 2^log_fold (j + 1)) of each column.
 * Step s = 0 .. log_fold - 1 folds the pairs at flat index i = 2^(log_fold-1-s) j + t with
 * roots[i], the challenge alpha^(2^s) (squared per step, fri/mod.rs:218-224) and
 * coset_inverse^(2^s) (:554, :651): bit for bit what log_fold calls of bj_fri_fold_d give when
 * the caller squares the challenge and the coset inverse between them, for any u64 inputs.
 * One output per lane with the 2^log_fold inputs of each column in registers, so the
 * intermediate vectors never reach memory: 2 * 2^log_fold values and 2^log_fold - 1 roots in and
 * 2 values out per output.  c0, c1 and roots at 16-byte-aligned addresses load a lane's values as
 * 16-byte words (16, 32 or 64 contiguous bytes per column); any other 8-byte-aligned address
 * runs the same fold with 8-byte loads.  roots holds at least n_src / 2 entries, as for
 * bj_fri_fold_d.  dst_c0 / dst_c1 must not overlap c0, c1 or roots.  Outputs canonical; alpha
 * travels by value, so the call can be captured in a HIP graph.
 * BJ_EINVAL: log_fold 0 or > 3, n_src no multiple of 2^log_fold, a null pointer or one that is
 * not 8-byte aligned (with n_src > 0).  n_src = 0 succeeds and touches nothing.  log_fold = 1
 * runs bj_fri_fold_d's kernel. */
int bj_fri_fold_multi_d(const uint64_t* c0, const uint64_t* c1, size_t n_src, const uint64_t* roots,
                        uint64_t coset_inverse, uint64_t ch0, uint64_t ch1, uint32_t log_fold,
                        uint64_t* dst_c0, uint64_t* dst_c1, void* stream);

/* ------------------------------------------------------------------ DEEP */
/* Evaluations at the out-of-domain point z and the quotening pass that builds the codeword
 * bj_fri_fold_d folds, on LDE columns that stay on the device.  Added after 2.6; detect by symbol
 * (bj_abi_version() is unchanged).  Device pointers are stream-ordered.  GoldilocksExt2 values
 * are pairs (c0, c1) with u^2 = 7 (field/goldilocks/extension.rs:14-40); outputs are canonical. */

/* precompute_for_barycentric_evaluation_in_extension(n, coset, at), utils.rs:907-1021:
 * w[bitrev_n(i)] = C * w_n^i / (at - coset * w_n^i),  C = coset * (at^n - coset^n) / (n * coset^n)
 * w0, w1: n words each (the Ext2 halves), canonical.  log_n = 0: (1, 0).
 * BJ_EINVAL: log_n > 32, a null output, coset = 0.  Precondition (the reference's own, its batch
 * inverse at utils.rs:983; not checked): at is no point of coset * <w_n>. */
int bj_barycentric_weights_d(uint32_t log_n, uint64_t coset, uint64_t at0, uint64_t at1,
                             uint64_t* w0, uint64_t* w1, void* stream);

/* barycentric_evaluate_base_at_extension_for_bitreversed_parallel (utils.rs:1085-1158) for n_cols
 * columns at once, the per-polynomial sums of prover.rs:1501-1780:
 * out[2c], out[2c+1] = sum_r cols[c*col_stride + r] * (w0[r], w1[r]), r < 2^log_n, canonical.
 * (Columns are coset 0 of bj_lde_d's output: col_stride = D * n.)  An Ext2 polynomial held as two
 * base columns is e0 + u * e1 of its columns' results (utils.rs:1160-1200).  Per-block partial
 * sums go through the library's stream-ordered pool and a second launch adds them in a fixed
 * order: no atomics.  BJ_EINVAL: log_n > 32, a null pointer with n_cols > 0, col_stride < 2^log_n. */
int bj_evaluate_at_d(const uint64_t* cols, uint32_t n_cols, size_t col_stride, uint32_t log_n,
                     const uint64_t* w0, const uint64_t* w1, uint64_t* out, void* stream);

/* One opening point of quotening_operation_in_extension (prover.rs:2523-2706, driven by
 * :1823-2050) over rows [row0, row0 + n_rows) of the flat bit-reversed domain of 2^log_domain
 * points (leaf order L = coset * n + row):
 *   x_L = 7 * w_{2^log_domain}^{bitrev(L)}
 *   q   = (sum_c gammas[c] * cols[c*col_stride + (L - row0)] - (k0, k1)) / (x_L - (at0, at1))
 *   dst0/dst1[L - row0] = q (accumulate = 0) or += q (accumulate = 1), canonical.
 * gammas: device, n_cols x 2.  cols and dst are window-relative, so a rank that holds only its
 * leaf range (bj_lde_shard_d's layout) calls it unchanged.  n_cols = 0 is legal (q = -K/(x - at)).
 * The caller folds the sources f_j, values v_j and challenge powers ch_j of the opening point into
 * the coefficients: a base source adds ch_j to its column's gamma, an Ext2 source (c0, c1) adds
 * ch_j to the c0 column's and ch_j * u to the c1 column's, and K = sum_j ch_j * v_j, so
 * sum_j ch_j (f_j(x) - v_j) = sum_c gamma_c col_c(x) - K (the "c1 is None" branch of
 * prover.rs:2523-2539 is the base case).  n_rows = 0 is a no-op.  BJ_EINVAL: log_domain > 32,
 * row0 + n_rows > 2^log_domain, a null dst, null cols or gammas with n_cols > 0, col_stride <
 * n_rows.  Precondition (the reference's own, not checked): x - at != 0 on the whole domain, that
 * is, at is no point of 7 * <w_{2^log_domain}>.  A window that starts and ends on an even row with
 * 16-byte-aligned cols and dst and an even col_stride moves each (x, -x) row pair as one 16-byte
 * access; any other window runs the same arithmetic with 8-byte accesses. */
int bj_deep_quotient_d(const uint64_t* cols, uint32_t n_cols, size_t col_stride, const uint64_t* gammas,
                       uint64_t k0, uint64_t k1, uint64_t at0, uint64_t at1, uint32_t log_domain,
                       size_t row0, size_t n_rows, uint64_t* dst0, uint64_t* dst1, int accumulate,
                       void* stream);

/* Every opening point of the DEEP codeword in one launch (prover.rs:1823-2050): what a chain of
 * bj_deep_quotient_d calls, one per (column group, opening point), leaves in dst, word for word
 * for any u64 input.  Added after 2.6; detect by symbol (bj_abi_version() is unchanged).  Over
 * rows [row0, row0 + n_rows) of the flat bit-reversed domain of 2^log_domain points, with x_L of
 * bj_deep_quotient_d:
 *   dst0/dst1[L - row0] (+)= sum_p (sum_{terms t of p} sum_{c < n_cols_t} gammas[gamma_offset_t + c]
 *       * groups[group_t].cols[(first_col_t + c) * col_stride + (L - row0)] - K_p) / (x_L - at_p)
 * A column group is one tensor of columns over the row window (an oracle's LDE); a term is a
 * column range of one group opened at one point, with its coefficients (the caller folds sources,
 * values and challenge powers into them as for bj_deep_quotient_d) in the one device array
 * `gammas` of n_gammas Ext2 pairs.  Terms are sorted by point; a point with no terms contributes
 * -K / (x - at).  The descriptor is a HOST struct and travels to the kernel by value: nothing is
 * allocated, no table is built on the device and nothing synchronises, so the call can be captured
 * in a HIP graph.  A thread owns the row pair (x, -x), shares x between the points, and performs
 * one base-field inversion for all of them (the product of the norms of every x - at_p and
 * -x - at_p); dst is written once (read once before it when accumulate = 1).  The window and
 * alignment rule of bj_deep_quotient_d's 16-byte accesses holds for every referenced column range.
 * n_rows = 0 is a no-op; n_points = 0 writes zeros (accumulate = 0) or leaves dst as it is.
 * BJ_EINVAL: a null descriptor, counts over the caps, log_domain > 32, row0 + n_rows >
 * 2^log_domain, a term naming a missing group or point, a column range outside its group, a
 * coefficient range outside n_gammas, terms not sorted by point, and with n_rows > 0: a null dst,
 * null cols of a group with n_cols > 0, null gammas with n_gammas > 0, col_stride < n_rows.
 * Precondition (the reference's own, not checked): no at_p is a point of 7 * <w_{2^log_domain}>. */
#define BJ_DEEP_MAX_GROUPS 8
#define BJ_DEEP_MAX_POINTS 8
#define BJ_DEEP_MAX_TERMS 16
typedef struct bj_deep_group {
    const uint64_t* cols; /* column 0 over the row window (device); NULL iff n_cols == 0 */
    size_t col_stride;    /* elements between columns */
    uint32_t n_cols;
    uint32_t reserved;    /* 0 */
} bj_deep_group_t;
typedef struct bj_deep_point {
    uint64_t at0, at1; /* the opening point */
    uint64_t k0, k1;   /* K = sum_j ch_j * v_j over all its terms */
} bj_deep_point_t;
typedef struct bj_deep_term {
    uint32_t group, first_col, n_cols; /* columns [first_col, first_col + n_cols) of groups[group] */
    uint32_t point;
    uint32_t gamma_offset;             /* its first coefficient, in Ext2 pairs */
    uint32_t reserved;                 /* 0 */
} bj_deep_term_t;
typedef struct bj_deep_codeword {
    bj_deep_group_t groups[BJ_DEEP_MAX_GROUPS];
    bj_deep_point_t points[BJ_DEEP_MAX_POINTS];
    bj_deep_term_t terms[BJ_DEEP_MAX_TERMS];
    uint32_t n_groups, n_points, n_terms, log_domain;
    const uint64_t* gammas; /* device, n_gammas x 2 */
    size_t n_gammas;
    size_t row0, n_rows;
    uint64_t* dst0;         /* device, n_rows words each */
    uint64_t* dst1;
    int32_t accumulate;
    uint32_t reserved;      /* 0 */
} bj_deep_codeword_t;
int bj_deep_codeword_d(const bj_deep_codeword_t* desc, void* stream);

/* ------------------------------------------------------------------ stage 2 */
/* The columns of the stage-2 oracle (prover.rs:360-438, committed at :505-554), computed from
 * witness and setup columns that stay on the device: the copy-permutation grand product with its
 * partial products, and the lookup argument's encoding polynomials.  Added after 2.6; detect by
 * symbol (bj_abi_version() is unchanged).  Everything is over the main domain in natural order
 * (row i is x_i = w_n^i: no coset, no LDE, no bit reversal).  Inputs may be any u64 representative;
 * outputs are canonical.  Asynchronous on `stream`, no allocation and no synchronisation, so the
 * calls can be captured in a HIP graph.
 * status_d: device u64[4], rewritten by every call: [0], [1] the product of a over all rows
 * (bj_copy_permutation_d; 0 for the lookup call), [2] the number of zero denominators, [3] 0. */

/* compute_partial_products_in_extension (cs/implementations/copy_permutation.rs:649-774, over
 * pointwise_rational_in_extension :114-248, pointwise_product_in_extension :298-365 and
 * shifted_grand_product_in_extension :425-510; x_poly of utils.rs:690-721), as called at
 * prover.rs:360-392.  With m = ceil(n_cols / chunk) chunks of `chunk` columns (the last may be shorter):
 *   r_j[i] = prod_{c in chunk j} (w_c[i] + beta k_c x_i + gamma) / (w_c[i] + beta sigma_c[i] + gamma)
 *   a[i]   = prod_j r_j[i],   z[0] = 1,   z[i] = prod_{t < i} a[t],
 *   p_j[i] = z[i] prod_{t <= j} r_t[i],   j = 0 .. m - 2
 * in GoldilocksExt2 (u^2 = 7).  vars, sigmas: n_cols device columns of 2^log_n rows, column c at
 * + c * stride.  non_residues: HOST array k_c (bj_non_residues_h).  chunk: the quotient degree, a
 * power of two.  out: 2 m device columns of stride out_stride: z.c0, z.c1, p_0.c0, p_0.c1, ...;
 * they are the call's working memory too.  With m = 1 there is no intermediate: the reference
 * returns its lone per-chunk product there (:747-749), which
 * num_intermediate_partial_product_relations (:14-28) and so the verifier do not count.
 * Where the reference panics, this call reports: status_d[0..1] is the product over all rows
 * (the reference asserts it is one, :485), and a chunk denominator that is zero (batch inverse
 * panic, utils.rs:425-427) is counted in status_d[2] and its r_j[i] taken as 0.
 * BJ_EINVAL: log_n > 32, n_cols = 0, chunk no power of two, a stride below 2^log_n, a null pointer. */
int bj_copy_permutation_d(const uint64_t* vars, size_t vars_stride, const uint64_t* sigmas, size_t sigmas_stride,
                          uint32_t n_cols, uint32_t log_n, const uint64_t* non_residues, uint64_t beta0,
                          uint64_t beta1, uint64_t gamma0, uint64_t gamma1, uint32_t chunk, uint64_t* out,
                          size_t out_stride, uint64_t* status_d, void* stream);

/* The one operation behind compute_lookup_poly_pairs_specialized
 * (cs/implementations/lookup_argument_in_ext.rs:320-700):
 *   out[i] = f[i] / (beta + sum_{t < n_src} g_t srcs[t][i]),  i < 2^log_n,  in GoldilocksExt2.
 * srcs: HOST array of n_src <= 16 device column pointers (they may belong to different buffers:
 * variable columns and a setup constant column, :536-554); g: HOST array of the n_src Ext2
 * coefficients (g_t.c0, g_t.c1), the powers of gamma of :402-418; f: a device column or NULL for 1.
 * A witness encoding (:521-632) is f = NULL over the sub-argument's columns, a multiplicity
 * encoding (:423-518, :635-672) f = the multiplicity column over the table columns.  A zero
 * denominator gives 0 and is counted in status_d[2].
 * BJ_EINVAL: log_n > 32, n_src outside 1..16, a null pointer other than f. */
int bj_lookup_encoding_d(const uint64_t* const* srcs, uint32_t n_src, const uint64_t* g, uint64_t beta0,
                         uint64_t beta1, const uint64_t* f, uint32_t log_n, uint64_t* out_c0, uint64_t* out_c1,
                         uint64_t* status_d, void* stream);

/* non_residues_for_copy_permutation(2^log_n, num) (copy_permutation.rs:512-522): out[0] = 1, then
 * make_non_residues(num - 1, 2^log_n) (utils.rs:636-688): the smallest quadratic non-residues
 * 2, 3, ... outside the domain and in pairwise distinct cosets of it.  Host only, no device call.
 * BJ_EINVAL: log_n > 32, num = 0, null out. */
int bj_non_residues_h(uint32_t num, uint32_t log_n, uint64_t* out);

/* ------------------------------------------------------------------ quotient */
/* The step between the stage-2 commit and the quotient commit (prover.rs:1111-1467): the
 * copy-permutation and lookup terms over the LDE domain, the division by the vanishing polynomial,
 * and the way to monomials.  The gate terms depend on the circuit and are the caller's: they enter
 * as the initial contents of the accumulator, as the reference hands its quotient_c0s /
 * quotient_c1s to this block (prover.rs:1161-1175); a caller without any zeroes it.  Added after
 * 2.6; detect by symbol (bj_abi_version() is unchanged).  Inputs may be any u64 representative;
 * outputs are canonical.  Asynchronous on `stream`, no allocation and no synchronisation, so the
 * calls can be captured in a HIP graph.
 *
 * Domain and layout.  q = 2^log_q is the quotient degree, at most BJ_QUOTIENT_MAX_DEGREE (the
 * per-coset constants travel in the kernel arguments).  The accumulator dst0 / dst1 (the Ext2
 * halves) holds q * n words each in leaf order L = coset * n + row, x_L = 7 * w_{nq}^{bitrev_{log
 * nq}(L)}, bj_deep_quotient_d's x_L.  A source column is a column of bj_lde_d's output at D >= q,
 * given by the address of its coset 0: its value at point L is column[L], because the first q
 * cosets of a bit-reversed D-LDE are the q-LDE (subset_for_degree, lde.rs:298-308).  Columns of
 * one tensor are `stride` = n * D words apart.
 *
 * From stage 2 to bj_monomials_to_lde_d (the quotient commit, prover.rs:1471-1495):
 *   bj_copy_permutation_d, bj_lookup_encoding_d    -> the stage-2 columns      (n each)
 *   bj_lde_d at D >= q on them, the variables, the sigmas, ...                 (D * n each)
 *   dst0, dst1 = 0 or the gate terms                                           (q * n each)
 *   bj_quotient_copy_permutation_d, bj_quotient_lookup_term_d per lookup term  dst += terms
 *   bj_quotient_divide_vanishing_d                                             dst /= x^n - 1
 *   bj_bitreverse_enumeration_d(dst, 2 columns, log_n + log_q): the leaf order is the bit-reversed
 *     enumeration of the whole domain of q * n points (flatten_presumably_bitreversed,
 *     prover.rs:1409-1410), then bj_ifft_natural_to_natural_d(.., log_n + log_q, coset 7)
 *     (prover.rs:1421-1422): q * n monomial coefficients per half.  Their last q are zero for a
 *     satisfied circuit (the reference asserts the last one, "unsatisfied", prover.rs:1424-1439).
 *   chunk i is the slice [i * n, (i + 1) * n) of each half, and the quotient oracle's columns are
 *     chunk_0.c0, chunk_0.c1, chunk_1.c0, ... (prover.rs:1454-1467). */
#define BJ_QUOTIENT_MAX_DEGREE 128u

/* The (z(x) - 1) L_1(x) term (prover.rs:1148-1227; unnormalized_l1_inverse, utils.rs:1585-1665)
 * and compute_quotient_terms_in_extension (cs/implementations/copy_permutation.rs:1000-1249), all
 * m = ceil(n_cols / q) relations, one read and one write of the accumulator.  Per point L:
 *   t_0     = alpha_0 (z(x) - 1) (x^n - 1) / (x - 1)
 *   t_{j+1} = alpha_{j+1} (lhs_j prod_{c in chunk j} (w_c + beta sigma_c + gamma)
 *                          - rhs_j prod_{c in chunk j} (w_c + beta k_c x + gamma)),   j < m
 *   dst    += sum t
 * in GoldilocksExt2, with rhs = [z, p_0, .., p_{m-2}], lhs = [p_0, .., p_{m-2}, z(w x)] and chunk j
 * the columns [j q, min(n_cols, (j + 1) q)), bj_copy_permutation_d's chunks at chunk = q.
 * vars, sigmas: n_cols LDE columns each.  stage2: the LDE of bj_copy_permutation_d's 2 m output
 * columns in its order (z.c0, z.c1, p_0.c0, ...).  z(w x) is read in place, at row
 * bitrev(bitrev(row) + 1 mod n) of the same coset (the reference clones the column,
 * shift_by_omega_assuming_bitreversed, utils.rs:1245-1271).  That row lies half a coset away, so
 * a row window is not self-contained: the call covers the whole domain and takes no window.
 * non_residues: HOST array k_c (bj_non_residues_h).  alphas: HOST array of the m + 1 Ext2
 * challenges (c0, c1), the L_1 term's first.  A trace wider than one launch's kernel arguments
 * hold (128 columns or 64 relations) takes several launches on `stream` that meet on chunk
 * boundaries; only the first adds t_0.
 * BJ_EINVAL: log_n + log_q > 32, q > BJ_QUOTIENT_MAX_DEGREE, n_cols = 0, a stride below q * n, a
 * null pointer. */
int bj_quotient_copy_permutation_d(const uint64_t* vars, size_t vars_stride, const uint64_t* sigmas,
                                   size_t sigmas_stride, const uint64_t* stage2, size_t stage2_stride, uint32_t n_cols,
                                   uint32_t log_n, uint32_t log_q, const uint64_t* non_residues, uint64_t beta0,
                                   uint64_t beta1, uint64_t gamma0, uint64_t gamma1, const uint64_t* alphas,
                                   uint64_t* dst0, uint64_t* dst1, void* stream);

/* The one operation behind both loops of compute_quotient_terms_for_lookup_specialized
 * (cs/implementations/lookup_argument_in_ext.rs:949-1310):
 *   dst[L] += alpha (E[L] (beta + sum_{t < n_src} g_t srcs[t][L]) - f[L]),  L < q * n.
 * srcs: HOST array of n_src <= 16 device pointers to LDE columns (they may belong to different
 * buffers); g: HOST array of the n_src Ext2 coefficients, the powers of gamma (:1000-1014);
 * e_c0, e_c1: the LDE columns of the encoding polynomial; f: an LDE column or NULL for 1.
 * A witness-encoding term (:1115-1229) is f = NULL over the sub-argument's variable columns (and
 * the table-id constant column when it is shared, :1135-1138) with E = A_s; the multiplicity term
 * (:1231-1310) is f = the multiplicity column over the table columns with E = B, so the
 * reference's aggregated_lookup_columns buffer (:1023-1104) is never materialised.
 * BJ_EINVAL: log_n + log_q > 32, q > BJ_QUOTIENT_MAX_DEGREE, n_src outside 1..16, a null pointer
 * other than f. */
int bj_quotient_lookup_term_d(const uint64_t* const* srcs, uint32_t n_src, const uint64_t* g, uint64_t beta0,
                              uint64_t beta1, const uint64_t* e_c0, const uint64_t* e_c1, const uint64_t* f,
                              uint64_t alpha0, uint64_t alpha1, uint32_t log_n, uint32_t log_q, uint64_t* dst0,
                              uint64_t* dst1, void* stream);

/* divide_by_vanishing_for_bitreversed_coset_enumeration (utils.rs:770-817), both halves in one
 * launch: dst[L] *= inv[L >> log_n] with bj_vanishing_inverses_h's constants, which the call
 * computes itself.  BJ_EINVAL: log_n + log_q > 32, q > BJ_QUOTIENT_MAX_DEGREE, a null pointer. */
int bj_quotient_divide_vanishing_d(uint64_t* dst0, uint64_t* dst1, uint32_t log_n, uint32_t log_q, void* stream);

/* out[i] = 1 / (7^n w_{nq}^{n bitrev_{log q}(i)} - 1), i < 2^log_q: the inverse of x^n - 1 on coset
 * i (utils.rs:788-799), canonical.  Host only, no device call, any log_q with log_n + log_q <= 32.
 * BJ_EINVAL: log_n + log_q > 32, null out. */
int bj_vanishing_inverses_h(uint32_t log_n, uint32_t log_q, uint64_t* out);

/* ------------------------------------------------------------------ quotient gate terms */
/* The gate terms of the quotient (the loop prover.rs:560-1085 drives on the CPU) for gates given
 * as captured programs.  The evaluators stay the caller's: what arrives is what
 * gpu_synthesizer/mod.rs records from evaluate_once -- relations Relation::{Add, Double, Sub,
 * Negate, Mul, Square} over Index::{VariablePoly, WitnessPoly, ConstantPoly, TemporaryValue,
 * ConstantValue}, and the operands pushed to the destination -- together with each gate's
 * placement.  Added after 2.6; detect by symbol (bj_abi_version() is unchanged).  For every point
 * L = coset * n + row of the first q cosets (the domain of the calls above)
 *   dst[L] += sum_gates selector_g(L) sum_rep sum_term alpha[k] term(L),
 * k running on across repetitions and gates and restarting per point
 * (BufferedGateEvaluationReducingDestinationChunk::push_evaluation_result / proceed_to_next_gate /
 * advance, buffering_source.rs:157-221, 303-377; evaluate_over_general_purpose_columns,
 * cs/traits/evaluator.rs:376-397).  Terms are base-field values, a term times a challenge is two
 * base products, the selector multiplies each gate's sum once, outputs are canonical.
 * selector_g is the product over the gate's path of constant column i or 1 - column i
 * (compute_selector_subpath, prover.rs:2775-2916); an empty path is 1, which is also the
 * specialized-columns form (prover.rs:651-801).  ConstantPoly(j) of a gate reads constant column
 * constants base + repetition * constants per repetition + j, the base being path length for a
 * general-purpose gate and, for a specialized one, the constants of the general-purpose set plus
 * the gate's initial offset.  A gate without quotient terms (NOP and marker gates,
 * prover.rs:922-994) is not part of a set.
 *
 * The image (u64 words; INTEGRATION.md "Gate programs" describes how to build one from a capture):
 *   [0] 0x3153455441474A42 ("BJGATES1")  [1] segments S  [2 .. 2 + S) word offset of each segment
 *   segment:    [0] gates G  [1] instructions I  [2] writes W  [3] immediates M  [4] alpha base (the
 *               terms of the segments before it)  [5] terms  [6] deepest selector path  [7] kind:
 *               0 interpreted, 1 native Poseidon2 flattened gate, 3 library gates (both below;
 *               2 is no kind), then
 *               G descriptors of 8 words, I instructions, W writes, M immediates
 *   descriptor: [0] instruction begin | end << 32  [1] write begin | end << 32 (in push order)
 *               [2] num_repetitions | path length << 32  [3] path mask, bit i set: column i, clear:
 *               1 - column i  [4] variables base | per repetition << 32  [5] witnesses, [6]
 *               constants likewise  [7] 0 (native Poseidon2 segment: num_witness_columns_used)
 *   instruction: opcode | destination slot << 8 | operand a << 16 | operand b << 40
 *   operand (24 bits): kind << 21 | index; kinds 0 VariablePoly, 1 WitnessPoly, 2 ConstantPoly,
 *               3 slot, 4 immediate (index into the segment's M words); a write is one operand
 *   opcode:     0 Add, 1 Double, 2 Sub, 3 Negate, 4 Mul, 5 Square (Relation's order)
 * A TemporaryValue lives in one of BJ_GATE_MAX_SLOTS slots per point; the caller assigns slots by
 * liveness, so the cap bounds the values live at once (a pushed temporary stays live to the end of
 * its program), not the program's length.  One call is one launch of one segment of at most
 * BJ_GATE_MAX_GATES gates and BJ_GATE_MAX_INSTRUCTIONS instructions (and as many writes and
 * immediates); a larger set is several segments and several calls, which is exact because every
 * call adds to dst.
 *
 * Native segments.  A gate whose capture passes the caps of a launch whatever the split --
 * Poseidon2RoundFunctionFlattenedEvaluator<F, 8, 12, 4> over Goldilocks (cs/gates/poseidon2.rs:166-403)
 * is about 31 matrix layers of 144 relations with more than BJ_GATE_MAX_SLOTS values live -- goes in a
 * segment of its own with a kind other than 0 in word [7], and the two calls below run a written-out
 * kernel on it instead of the interpreter, with the same arguments and the same contract.  Kind 1 is
 * that gate: 130 cells, 118 terms in the reference's push order (36 + 22 + 48 resets, then output -
 * state), degree 7.  Such a segment has G = 1 and I = W = M = 0; its descriptor's [0] is 0, [1] is
 * 0 | 118 << 32 with no writes behind it (so the terms of a gate are read from a descriptor alike for
 * both kinds), [2] .. [6] keep their meaning and [7] is nw = num_witness_columns_used <= 106: S-box
 * output cell s reads witness column s while s < nw and variable column 24 + s - nw after that,
 * variables 0 .. 11 being the input and 12 .. 23 the output.  Variables per repetition must be at
 * least 130 - nw and witnesses per repetition at least nw; terms = 118 * repetitions.  The magic is
 * unchanged, and an image without native segments is word for word what it was.
 *
 * Library segments, kind 3.  The library holds straight-line code for the gates every circuit of the
 * reference uses, generated from their captures (bj_gate_library_find_h names them).  A segment of
 * kind 3 holds 1 .. BJ_GATE_MAX_GATES such gates and no program: I = W = M = 0, [4], [5] and [6] as for
 * every segment.  A descriptor's [0] is the library id (high half 0), [1] is 0 | terms per repetition
 * << 32 with no writes behind it, [2] .. [6] are the placement words, [7] is 0.  The gate computes what
 * the interpreter computes on the capture it was generated from -- the caller compares the digest of
 * its own capture with the library's before it names an entry -- so an image may use either kind for
 * such a gate, with the same columns, challenges and results; which is faster is DESIGN 4.12.3's
 * subject.  Refused: a program area that is not empty, an id outside the table, a term count that is
 * not the entry's, word [7] != 0, and sums of the head that do not add up.
 *
 * Checks, all on the host and none per point: the magic, every range, the caps, an operand outside
 * its space, a slot read before it is written in its gate, a term count or alpha base that does
 * not add up, and opcode 6, Relation::Inverse.  No evaluator in cs/gates records Inverse: its three
 * textual hits (fma_gate_without_constant.rs:353, fma_gate_in_extension_without_constant.rs:451,
 * zero_check.rs:539) are inside witness-computation closures, not in evaluate_once. */
#define BJ_GATE_MAX_SLOTS 16u
#define BJ_GATE_MAX_SELECTOR_DEPTH 8u
#define BJ_GATE_MAX_INSTRUCTIONS 4096u
#define BJ_GATE_MAX_GATES 64u
#define BJ_GATE_MAX_SEGMENTS 64u

/* Validates a HOST image without touching a device.  need (5 words, may be NULL): the variable,
 * witness and constant columns the largest repetition reaches (the selector columns included), the
 * challenges the whole image consumes, the segments.  BJ_EINVAL as listed above. */
int bj_gate_set_check_h(const uint64_t* image, size_t words, uint64_t* need);

/* What a native segment kind is, for a caller that builds images: out[0] the cells of one repetition
 * (130), [1] its terms (118), [2] the constraint degree (7), [3] the most cells that may be witness
 * columns (106).  Added after 2.6; detect by symbol (bj_abi_version() is unchanged): a library
 * without it refuses word [7] != 0.  Host only.  BJ_EINVAL: an unknown kind, null out. */
int bj_gate_native_info_h(uint32_t kind, uint64_t* out);

/* A library gate by the name of its evaluator (fma_gate_in_base_without_constant, boolean_constraint,
 * constants_allocator, reduction_gate_4, selection_gate, zero_check_variable, zero_check_witness,
 * dot_product_gate_4, conditional_swap_gate_1): out[0] the id for descriptor word [0] of a kind-3
 * segment, [1] the terms per repetition, [2], [3], [4] the variable, witness and constant columns one
 * repetition reads (highest index + 1), [5] the 64-bit digest of the capture the code was generated
 * from (FNV-1a-64 over the relations and writes; INTEGRATION.md "Library gates" gives the bytes).
 * Added after 2.6; detect by symbol (bj_abi_version() is unchanged): a library without it refuses
 * kind 3.  Host only.  BJ_EINVAL: an unknown or null name, null out. */
int bj_gate_library_find_h(const char* name, uint64_t* out);

/* bj_gate_set_check_h, then the one upload: allocates words * 8 bytes on the current device, copies
 * the image and synchronises.  *set is the handle the evaluation takes; it keeps the device buffer
 * until bj_gate_set_release (NULL is a no-op).  On failure *set is NULL. */
int bj_gate_set_upload_d(const uint64_t* image, size_t words, void** set);
int bj_gate_set_release(void* set);

/* dst += the gate terms of one segment of an uploaded set: one launch, no copy, no allocation and no
 * synchronisation, so it captures into a HIP graph on `stream`.  vars, wits, consts: the LDE
 * tensors of n_vars, n_wits, n_consts columns (coset 0 of column 0, columns `stride` words apart,
 * D >= q as above), read in place; a kind the set never names may be NULL with count 0.  alphas:
 * DEVICE array of n_alphas Ext2 challenges (c0, c1), the whole set's, indexed from the segment's
 * alpha base.  dst0, dst1 are read once and written once per point.
 * BJ_EINVAL (dst untouched): not a live handle, no such segment, log_n + log_q > 32, an operand
 * that reaches a column index >= its count at the largest repetition, a stride below q * n,
 * n_alphas below the set's terms, a null pointer that is read. */
int bj_quotient_gate_terms_d(const void* set, uint32_t segment, const uint64_t* vars, size_t vars_stride,
                             uint32_t n_vars, const uint64_t* wits, size_t wits_stride, uint32_t n_wits,
                             const uint64_t* consts, size_t consts_stride, uint32_t n_consts, const uint64_t* alphas,
                             uint32_t n_alphas, uint32_t log_n, uint32_t log_q, uint64_t* dst0, uint64_t* dst1,
                             void* stream);

/* Where a witness fails the gates of an uploaded set (CSReferenceAssembly::check_if_satisfied,
 * cs/implementations/satisfiability_test.rs:15-353, which evaluates every gate's evaluate_once on
 * every trace row and panics at the first term that is not zero).  Added after 2.6; detect by symbol
 * (bj_abi_version() is unchanged).  vars, wits, consts: the TRACE columns (Lagrange form on the
 * domain of n rows, row r of column c at [c * stride + r], the tensors the commitment takes, not an
 * LDE), read in place over the rows [row_begin, row_begin + n_rows); a kind the set never names may
 * be NULL with count 0.  Term k of row r is unsatisfied iff selector_g(r) * term_k(r) != 0 in the
 * field, selector_g being the path product of the call above (an empty path is 1) and k the running
 * term index the challenges use: across terms, repetitions, gates and segments (a segment's alpha
 * base carries it on).  With 0 / 1 selector columns that is the reference's rule -- the gate placed
 * on the row, and every specialized gate on every row; a selector that is neither 0 nor 1 next to
 * a non-zero term is reported too, as it would leave a remainder in the quotient.  Any u64
 * representative is accepted, and a value is zero when it is 0 mod p (the word p is zero).
 *
 * status_d: DEVICE u64[4].  [0] the number of unsatisfied (row, term) pairs, [1] the smallest key
 * row << 32 | k among them, or all ones when [0] is 0, [2] the canonical value of that term (the
 * term's, not selector * term; 0 when [0] is 0), [3] 0.  One call checks one segment and COMBINES
 * into the record: the count adds, the key takes the minimum, the value follows the key.  The first
 * call of a check carries BJ_GATE_CHECK_BEGIN in the top bit of `segment`, which initialises the
 * record on the stream before the segment is checked; the other segments of the set (in any order,
 * same columns and window) are further calls on the same record without the bit.
 * Three launches at most (the initialisation, the check at one row per lane, a one-wave launch that
 * re-evaluates the row of the winning key for its value); asynchronous on `stream`, no copy, no
 * allocation and no synchronisation, so it captures into a HIP graph.
 * BJ_EINVAL (status untouched): not a live handle, no such segment, an operand that reaches a
 * column index >= its count at the largest repetition, a null pointer that is read, null status_d,
 * n_rows = 0, row_begin + n_rows > 2^32, a stride below row_begin + n_rows, a set of 2^32 terms or
 * more. */
#define BJ_GATE_CHECK_BEGIN 0x80000000u
int bj_gate_set_satisfied_d(const void* set, uint32_t segment, const uint64_t* vars, size_t vars_stride,
                            uint32_t n_vars, const uint64_t* wits, size_t wits_stride, uint32_t n_wits,
                            const uint64_t* consts, size_t consts_stride, uint32_t n_consts, uint64_t row_begin,
                            uint64_t n_rows, uint64_t* status_d, void* stream);

/* ------------------------------------------------------------------ witness materialisation */
/* The trace columns from a WitnessVec and the circuit's dense copy hints
 * (CSReferenceAssembly::witness_set_from_witness_vec, cs/implementations/witness.rs:387-538; the
 * same loops in materialize_witness_polynomials, :108-385; the hints, cs/implementations/hints/mod.rs),
 * the first step of prove_from_precomputations, and the sigma columns of the setup from the same
 * placement (create_permutation_polys, setup.rs:401-484).  Added after 2.6; detect by symbol
 * (bj_abi_version() is unchanged).  The hints are fixed per circuit and stay on the device; a proof
 * uploads all_values, one word per distinct variable, and the columns appear where the commitment,
 * stage 2 and the satisfiability check read them.
 *
 * A hint is uploaded once.  words: HOST memory, the reference's own words, column-major: cell
 * (c, r) at words[c * stride + r], n_cols columns of n_rows rows.  A Variable or Witness is a u64
 * (cs/mod.rs:159-213): bit 63 marks a placeholder, the low 48 bits hold the index, the other bits
 * are ignored as as_variable_index / as_witness_index ignore them (cs/mod.rs:44-47).  The device
 * copy holds one u32 per cell, 2^32 - 1 standing for the placeholder, which halves the index
 * traffic of every proof; so an index must be below 2^32 - 1, and a word that names a larger one
 * is BJ_EINVAL (the reference's as_variable_index truncates it to 32 bits silently).  The upload
 * packs on the host, records the largest index and the number of placeholders, allocates
 * 4 * n_cols * n_rows bytes on the current device, copies and synchronises.  *hint keeps the device
 * buffer until bj_copy_hint_release (NULL is a no-op); on failure *hint is NULL.
 * BJ_EINVAL: null words or hint, n_cols = 0, n_rows = 0 or above 2^32, stride < n_rows, an index
 * of 2^32 - 1 or more. */
int bj_copy_hint_upload_d(const uint64_t* words, uint32_t n_cols, uint64_t n_rows, size_t stride, void** hint);
int bj_copy_hint_release(void* hint);
/* What the upload recorded; any out pointer may be NULL.  max_index is 0 for a hint of nothing but
 * placeholders.  Host only.  BJ_EINVAL: not a live handle. */
int bj_copy_hint_info(const void* hint, uint32_t* n_cols, uint64_t* n_rows, uint64_t* max_index,
                      uint64_t* n_placeholders);

/* The copy loops of witness_set_from_witness_vec (witness.rs:419-441 for the variables, :466-488 for
 * the witnesses): out[c * out_stride + r] = all_values[index of cell (c, r)], or 0 for a placeholder
 * (:434-436).  all_values: DEVICE array of num_values words, moved bit for bit: a non-canonical word
 * stays as it is, as the LDE accepts such columns.  Words of out between n_rows and out_stride are
 * not written.  The call compares num_values with the hint's largest index on the host, so no lane
 * checks a bound and no kernel can read outside all_values; nothing is copied back.  One launch, no
 * allocation and no synchronisation, the hint travelling by value: it captures into a HIP graph on
 * `stream`, and a replay reads the contents all_values has then.
 * BJ_EINVAL (nothing launched, out untouched): not a live handle, a null pointer,
 * num_values <= max_index, out_stride < n_rows. */
int bj_materialize_columns_d(const void* hint, const uint64_t* all_values, uint64_t num_values, uint64_t* out,
                             size_t out_stride, void* stream);

/* The multiplicity column (witness.rs:493-519): out[i] = mult_u32[i] widened (from_u64_unchecked of
 * the u32, :515) for i < len, 0 for len <= i < n_rows.  mult_u32: DEVICE array, may be NULL when
 * len is 0.  One launch.  BJ_EINVAL: len > n_rows, n_rows = 0, a null pointer that is read. */
int bj_materialize_multiplicities_d(const uint32_t* mult_u32, uint64_t len, uint64_t* out, uint64_t n_rows,
                                    void* stream);

/* create_permutation_polys (setup.rs:401-484) as one elementwise pass.  The identity value of cell
 * (col, row) is non_residues[col] * w_n^row, rows in natural order (materialize_x_by_non_residue_polys,
 * setup.rs:24-76, over materialize_x_poly, utils.rs:690-721).  prev: DEVICE map of n_cols * n_rows
 * u32, cell (c, r) at prev[c * n_rows + r]: the flat index col * n_rows + row of the cell whose
 * identity value the cell takes -- the variable's previous occurrence in (column, row) order, the
 * last occurrence for the first one, and the cell itself for a placeholder or a variable's only
 * occurrence.  That is what the reference's chain of swaps (:428-471) leaves behind.  out[c *
 * out_stride + r] receives the value, canonical: one product of two table entries per cell.  An
 * entry of prev that names no cell gives 0, which is no identity value, and reads nothing.
 * non_residues: HOST array of n_cols words (bj_non_residues_h).  A setup-time call: it takes
 * 8 * (n_cols + n_rows / 2) bytes from the library's pool for its table, filled by the kernel of
 * bj_precompute_twiddles_natural_d, and synchronises `stream` once for the copy of non_residues.
 * BJ_EINVAL: n_rows no power of two or above 2^32, n_cols outside 1..65535, n_cols * n_rows >
 * 2^32, out_stride < n_rows, a null pointer. */
int bj_permutation_polys_d(const uint32_t* prev, uint32_t n_cols, uint64_t n_rows, const uint64_t* non_residues,
                           uint64_t* out, size_t out_stride, void* stream);

/* ------------------------------------------------------------------ queries */
/* The query phase (prover.rs:2161-2266): every OracleQuery of a proof -- the leaf's elements
 * (QuerySource::get_elements, fri/mod.rs:683-927) and its Merkle path (get_proof,
 * merkle_tree.rs:462-480; OracleQuery::construct, proof.rs:64-97) -- for all oracles and all query
 * indices in one launch, from LDEs and trees that stay on the device.  Added after 2.6; detect by
 * symbol (bj_abi_version() is unchanged).  Everything is copied bit for bit, with no arithmetic:
 * elements come back as they are stored and the [u8; 32] digests of Blake2s256 / Keccak256 trees
 * are not reduced.
 *
 * A query index is the flat leaf index coset * n + row of the committed LDE domain, the index of
 * bj_merkle_leaves_d.  An oracle's tree index is index >> index_shift; that one shift is the
 * reference's whole index arithmetic.  For FRI oracle k of the schedule s_0, s_1, ...
 * (prover.rs:2226-2254, proof.rs:89-91):
 *   domain_size_k = n >> (s_0 + ... + s_{k-1}),  inner_k = inner >> (s_0 + ... + s_{k-1}),
 *   tree_idx = (coset << (log2 domain_size_k - s_k)) + (inner_k >> s_k)
 * and since inner < n this is (coset * n + inner) >> (s_0 + ... + s_k). */
#define BJ_QUERY_MAX_ORACLES 16
typedef struct bj_query_oracle {
    const uint64_t* src;         /* column 0 of the leaf sources (device); NULL iff n_cols == 0 */
    size_t col_stride;           /* elements between columns */
    uint32_t n_cols;             /* 0: path only */
    uint32_t log_elems_per_leaf; /* e: leaf L hashes, per column in order, src[c*col_stride + (L<<e) + t], t < 2^e
                                    (bj_merkle_leaves_d: e = 0; bj_merkle_leaves_chunked_d: 2^e = elems_per_leaf) */
    const uint64_t* leaves;      /* n_leaves x 4 */
    const uint64_t* nodes;       /* (n_leaves - cap_size) x 4, bj_merkle_nodes_d's layout; may be NULL iff
                                    n_leaves == cap_size */
    uint64_t n_leaves;
    uint32_t cap_size;
    uint32_t index_shift;        /* tree index = query index >> index_shift */
} bj_query_oracle_t;

/* Words of one query's record of oracle o: (n_cols << e) + 4 + 4 * depth, depth =
 * log2(n_leaves / cap_size).  0 for a null o or sizes that are no powers of two.  Host only. */
size_t bj_oracle_query_words(const bj_query_oracle_t* o);

/* oracles: HOST array of n_oracles descriptors (they travel to the kernel by value); indices_d:
 * n_queries device u64.  Oracle o's block starts at out_d + n_queries * sum_{o' < o} W_o', W =
 * bj_oracle_query_words, and query q's record at + q * W_o.  A record is the leaf's elements
 * (column-major: column 0's 2^e elements, then column 1's, ..., the order of get_elements), the
 * leaf hash (4 words), then the depth siblings in get_proof order: sibling l is entry (t >> l) ^ 1
 * of level l, t the tree index, level 0 the leaves and level l >= 1 after the lower levels in
 * nodes.  n_leaves == cap_size (the last FRI oracle, fri/mod.rs:258-266) gives an empty path.
 * Every oracle of a call covers the same domain: n_leaves << index_shift is equal for all.
 * status_d: device u64[4], rewritten by every call: [0] the number of query indices >=
 * n_leaves << index_shift, [1] the position of the first such index or ~0, [2] = [3] = 0.  Such a
 * query reads nothing and all its records are zero.
 * One launch whatever n_oracles and n_queries; asynchronous on `stream`, no allocation and no
 * synchronisation, so the call can be captured in a HIP graph.
 * BJ_EINVAL: n_oracles outside 1..16, n_queries = 0, a null pointer other than the two allowed
 * above, n_leaves or cap_size no power of two, n_leaves < cap_size, col_stride < n_leaves << e
 * with n_cols > 0, domains that disagree, out_words below n_queries * sum_o W_o. */
int bj_oracle_queries_d(const bj_query_oracle_t* oracles, uint32_t n_oracles, const uint64_t* indices_d,
                        uint32_t n_queries, uint64_t* out_d, size_t out_words, uint64_t* status_d, void* stream);

/* The same batch on trees that bj_sharded_commit_d left sharded: every oracle and every index in
 * one collective call.  Added after 2.6; detect by symbol (bj_abi_version() is unchanged).  With G
 * the communicator's world, m = n_leaves / G and cap_local = max(1, cap_size / G), one oracle is
 * this rank's commit outputs and the GLOBAL tree's geometry. */
typedef struct bj_sharded_query_oracle {
    const uint64_t* src;     /* this rank's block 0 of bj_sharded_commit_d's lde: column c at src + c * col_stride,
                                m rows; NULL iff n_cols == 0 */
    size_t col_stride;       /* >= m */
    uint32_t n_cols;         /* 0: path only */
    int32_t hasher;          /* BJ_HASHER_*: only used to hash the top levels when cap_size < G */
    const uint64_t* leaves;  /* m x 4, this rank's */
    const uint64_t* nodes;   /* (m - cap_local) x 4, this rank's subtree */
    uint64_t n_leaves;       /* of the GLOBAL tree: k * n */
    uint32_t cap_size;       /* of the GLOBAL tree */
    uint32_t reserved;
} bj_sharded_query_oracle_t;

/* Words of one query's record of oracle o: n_cols + 4 + 4 * log2(n_leaves / cap_size), which is
 * bj_oracle_query_words of the unsharded tree with e = 0.  0 for a null o or sizes that are no
 * powers of two.  Host only. */
size_t bj_sharded_query_words(const bj_sharded_query_oracle_t* o);

/* Collective: every rank passes its own shard buffers, the same geometry and the same contents of
 * indices_d (n_queries device u64, tree indices < n_leaves), and every rank receives the same
 * out_d and status_d: word for word what bj_oracle_queries_d writes for the unsharded tree with
 * log_elems_per_leaf = 0 and index_shift = 0.  Oracle o's block starts at out_d + n_queries *
 * sum_{o' < o} W_o', W = bj_sharded_query_words, and query q's record at + q * W_o: the n_cols
 * elements of the row, the leaf hash, then the depth siblings in get_proof order -- the first
 * log2(m / cap_local) from the subtree of the rank that owns the leaf (rank index / m), and when
 * cap_size < G the remaining log2(G / cap_size) from the levels hashed over the gathered subtree
 * roots.  Every oracle of a call has the same n_leaves, so a query has one owner for all of them;
 * cap_size, n_cols and hasher may differ.  status_d[4]: [0] the number of indices >= n_leaves, [1]
 * the position of the first such index or ~0, [2] = [3] = 0; such a query's records are all zero
 * on every rank.
 * Schedule: when an oracle has cap_size < G, one all-gather of those oracles' subtree roots (32
 * bytes per oracle and rank) and the top levels hashed on every rank; one launch in which the
 * owner writes its records; one all-gather of every rank's record buffer (G * n_queries * sum_o
 * W_o * 8 bytes arrive per rank: all ranks' buffers travel, whoever owns the records); one launch
 * that picks each query's owner's copy.  Two launches and at most two exchanges whatever n_queries
 * and n_oracles.  Asynchronous on `stream` (the call itself never synchronises; a host-staged
 * callback transport does inside its exchange); workspace comes from the library's stream-ordered
 * pool.
 * BJ_EINVAL, all checked before the first exchange so that ranks given the same bad arguments all
 * return: a null pointer other than src with n_cols == 0, n_oracles outside 1..16, n_queries = 0,
 * n_leaves or cap_size no power of two, n_leaves that differ between oracles, G > n_leaves,
 * m <= cap_local, col_stride < m with n_cols > 0, an unknown hasher, out_words below n_queries *
 * sum_o W_o. */
int bj_sharded_queries_d(bj_comm* comm, const bj_sharded_query_oracle_t* oracles, uint32_t n_oracles,
                         const uint64_t* indices_d, uint32_t n_queries, uint64_t* out_d, size_t out_words,
                         uint64_t* status_d, void* stream);

/* ------------------------------------------------------------------ proof of work */
/* PoWRunner (cs/implementations/pow.rs:7-32) for Blake2s256 (pow.rs:51-135) and Keccak256
 * (pow.rs:137-221), the step between the last FRI oracle and the queries (prover.rs:2107-2133).
 * Added after 2.6; detect by symbol (bj_abi_version() is unchanged).
 *
 * A nonce passes when u64::from_le_bytes(H(seed || nonce.to_le_bytes())[..8]).trailing_zeros() >=
 * pow_bits (pow.rs:63-67, 127-133), pow_bits <= 32 (pow.rs:53).  H is Blake2s256 (RFC 7693, unkeyed)
 * or Keccak256 (rate 136, domain byte 0x01).  The seed the prover passes is 5 field elements
 * (prover.rs:2115-2118), each as_u64_reduced().to_le_bytes() (pow.rs:10-12): 40 bytes; any length
 * is accepted.  These entries always return the SMALLEST passing nonce of the range they search:
 * that is the reference's serial scan for pow_bits <= 16 (pow.rs:58-71) and one of the answers
 * its race of 2^16-nonce slices may give above that (pow.rs:76-119).  The nonce 2^64 - 1 is never
 * tested: it is the reference's "no result" (pow.rs:48, 61). */
#define BJ_POW_NO_RESULT UINT64_MAX
/* hasher: BJ_HASHER_BLAKE2S or BJ_HASHER_KECCAK256; BJ_HASHER_POSEIDON2 -> BJ_EINVAL (the reference has no such runner) */

/* One launch over [first_nonce, first_nonce + n_nonces): *result_d = min(*result_d, smallest passing nonce of the window).
 * The caller initialises *result_d (BJ_POW_NO_RESULT for a fresh search).  seed is host memory, read before the call
 * returns.  Stream-ordered, no allocation, no synchronise.
 * BJ_EINVAL: pow_bits > 32, a hasher other than the two above, n_nonces == 0, first_nonce + n_nonces > 2^64 - 1, a null
 * seed with seed_len > 0, a null result_d. */
int bj_pow_search_d(uint32_t hasher, const uint8_t* seed, size_t seed_len, uint32_t pow_bits,
                    uint64_t first_nonce, uint64_t n_nonces, uint64_t* result_d, void* stream);

/* PoWRunner::run_from_bytes (pow.rs:52-124, 141-213): the smallest passing nonce >= 0, found window by window;
 * synchronous on the calling thread's library stream.  pow_bits == 0: nonce 0, no launch (the prover skips PoW then,
 * prover.rs:2109).  *nonce_out = BJ_POW_NO_RESULT when no nonce below 2^64 - 1 passes. */
int bj_pow_run_h(uint32_t hasher, const uint8_t* seed, size_t seed_len, uint32_t pow_bits, uint64_t* nonce_out);

/* PoWRunner::verify_from_bytes (pow.rs:126-134, 215-221): 1 passes, 0 fails, negative on an argument error.  Host
 * code only: no device call. */
int bj_pow_verify_h(uint32_t hasher, const uint8_t* seed, size_t seed_len, uint32_t pow_bits, uint64_t nonce);

/* ------------------------------------------------------------- utility */

/* Batched field arithmetic through the device field layer (utility for parity tests of
 * the Goldilocks primitives, field/goldilocks/mod.rs:186-325): out[i] = canonical(a[i] op b[i]),
 * op 0 = mul, 1 = add, 2 = sub, 3 = a + b * 2^32 (a < 2^63, b < 2^63 with b >> 32 < 2^31),
 * 4 = canonical(a).  Device pointers. */
int bj_gl_op_d(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n, void* stream);

/* Bench/test input (not a reference entry point): column-major synthetic trace,
 * x = splitmix64(seed + (first_col + c) * n + r) reduced once mod p. */
int bj_fill_synthetic_d(uint64_t* dst, uint32_t n_cols, size_t col_stride, uint32_t log_n, uint64_t seed,
                        uint64_t first_col, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* BOOJUM_MI355X_H */
