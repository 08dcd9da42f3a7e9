"""boojum_amd -- MI355X-native witness-commitment hot path of era-boojum.

Coset LDE over Goldilocks + Poseidon2 Merkle tree with cap, as hand-written gfx950 HIP
kernels behind the C ABI in include/boojum_mi355x.h (libboojum_mi355x.so).  This
package is the host-side mirror of the reference's interface for that path:

  fft      precompute_twiddles_for_fft, fft_natural_to_bitreversed,
           ifft_natural_to_natural, distribute_powers        (src/fft/mod.rs)
  lde      transform_raw_storages_to_lde, transform_monomials_to_lde,
           ArcGenericLdeStorage, WitnessStorage             (cs/implementations/utils.rs, ...)
  merkle   MerkleTreeWithCap, Poseidon2Sponge (TreeHasher)  (cs/oracle/*)
  commit   witness_commit, CommitWorkspace                   (prover.rs:313-353)
  sharded  multi-GPU commit (one process per GPU)
  deep     precompute_for_barycentric_evaluation_in_extension, barycentric_evaluate_*,
           quotening_operation_in_extension                  (utils.rs:907-1200, prover.rs:1501-2050, 2523-2706)
  stage2   compute_partial_products_in_extension, compute_lookup_poly_pairs_specialized,
           second_stage_trace                                (copy_permutation.rs:649-774,
                                                              lookup_argument_in_ext.rs:320-700, prover.rs:360-438)
  quotient compute_quotient_terms_in_extension, compute_quotient_terms_for_lookup_specialized,
           divide_by_vanishing_for_bitreversed_coset_enumeration, quotient_monomials,
           quotient_from_arguments                           (copy_permutation.rs:1000-1249,
                                                              lookup_argument_in_ext.rs:949-1310, prover.rs:1111-1467)
  gates    Index, Relation, TracingField, capture, GatePlacement, GateSet, evaluate_gate_terms and a
           small library of evaluators                       (gpu_synthesizer/mod.rs, prover.rs:560-1085,
                                                              buffering_source.rs:157-377, cs/gates/*.rs)
  witness  WitnessVec, DenseVariablesCopyHint, DenseWitnessCopyHint, WitnessSet, CopyHint,
           witness_set_from_witness_vec, create_permutation_polys, commit_witness_vec
                                                             (cs/implementations/witness.rs:387-538,
                                                              hints/mod.rs, setup.rs:401-484)
  queries  QueryOracle, construct_queries, OracleQuery, single_round_queries, fri_plan
                                                             (prover.rs:2161-2266, proof.rs:48-116)
  fri      do_fri, FriOracles, fold_by, final_monomials, fold, interpolate
                                                             (cs/implementations/fri/mod.rs:31-682)
  transcript  Poseidon2Transcript                            (cs/implementations/transcript.rs:48-151)
  pow      PoWRunner, Blake2s256, Keccak256, NoPow, search  (cs/implementations/pow.rs, prover.rs:2107-2133)
  openings prove_openings: the opening phase in one call     (prover.rs:1497-2266)
  prover   prepare_setup, prove_commitments, prove: a proof from a circuit's setup and a WitnessVec
                                                             (prover.rs:150-2266, setup_storage.rs:18-70)
"""
from ._lib import BoojumError, load  # noqa: F401
from .field import P, GENERATOR  # noqa: F401

__all__ = ["fft", "lde", "merkle", "commit", "deep", "stage2", "quotient", "gates", "witness", "queries", "pow", "openings", "prover", "field", "BoojumError", "load", "P", "GENERATOR"]
