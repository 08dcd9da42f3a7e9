"""The quotient on the GPU: the step between the stage-2 commit and the quotient commit
(prover.rs:1111-1467), on LDE columns that stay on the device.

* `compute_quotient_terms_in_extension`: the (z(x) - 1) L_1(x) term (prover.rs:1148-1227) and the
  copy-permutation relations (cs/implementations/copy_permutation.rs:1000-1249), one call
  (bj_quotient_copy_permutation_d).
* `compute_quotient_terms_for_lookup_specialized`: the A and B terms of the lookup argument
  (lookup_argument_in_ext.rs:949-1310), one bj_quotient_lookup_term_d per term.
* `divide_by_vanishing_for_bitreversed_coset_enumeration` (utils.rs:770-817).
* `quotient_monomials`: flatten_presumably_bitreversed + ifft_natural_to_natural on the coset 7 and
  the split into [c0, c1] chunks (prover.rs:1399-1467), the input of `commit.quotient_commit`.
* `quotient_from_arguments`: the whole block.

The gate terms depend on the circuit and are the caller's: they enter as the initial contents of
the accumulator.  An accumulator is a pair dst_c0, dst_c1 of q * n words in leaf order
L = coset * n + row; an LDE argument is the (C, D, n) tensor `OracleCommitment.lde` holds, D >= q
(its first q cosets are read), and a list of LDE columns is a list of (D, n) tensors.  Ext2 values
are (c0, c1) pairs of Python integers.  There is no CPU fallback.
"""
import ctypes

import torch

from ._lib import call
from .fft import bitreverse_enumeration_inplace, ifft_natural_to_natural
from .field import GENERATOR, P, ext2_mul, log2_exact, stream_of, to_host
from .stage2 import MAX_LOOKUP_SOURCES, non_residues_for_copy_permutation

MAX_QUOTIENT_DEGREE = 128  # BJ_QUOTIENT_MAX_DEGREE


def _lde_view(t, q):
    """(tensor, C, n, column stride) of a (C, D, n) LDE tensor whose first q cosets are read."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.int64, torch.uint64):
        raise TypeError("expected an int64 CUDA tensor of u64 field elements")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("an LDE is (C, D, n) or, for one column, (D, n)")
    c, d, n = t.shape
    if d < q:
        raise ValueError("the LDE has %d cosets, the quotient degree is %d" % (d, q))
    if t.stride(2) != 1 or (d > 1 and t.stride(1) != n):
        raise ValueError("the cosets of an LDE column must be contiguous")
    return t, c, n, (t.stride(0) if c > 1 else d * n)


def _acc_view(dst, total):
    if not isinstance(dst, torch.Tensor) or not dst.is_cuda or dst.dtype not in (torch.int64, torch.uint64):
        raise TypeError("expected an int64 CUDA tensor of u64 field elements")
    if dst.numel() != total or not dst.is_contiguous():
        raise ValueError("an accumulator half holds q * n = %d contiguous words" % total)
    return dst


def vanishing_inverses(log_n, log_q):
    """1 / (x^n - 1) on each of the q cosets (utils.rs:788-799), Python integers.  Host only."""
    out = (ctypes.c_uint64 * (1 << log_q))()
    call("bj_vanishing_inverses_h", log_n, log_q, out)
    return [int(v) for v in out]


def compute_quotient_terms_in_extension(variables_lde, sigmas_lde, second_stage_lde, beta, gamma, alphas,
                                        quotient_degree, dst_c0, dst_c1):
    """prover.rs:1148-1227 and copy_permutation.rs:1000-1249: dst += the L_1 term and the
    m = ceil(C / quotient_degree) copy-permutation relations.  variables_lde, sigmas_lde: (C, D, n);
    second_stage_lde: the LDE of the stage-2 columns, whose first 2 m columns are z and the
    intermediates (stage2.SecondStageTrace's order); alphas: m + 1 Ext2 challenges, the L_1 term's
    first (the reference takes that one at prover.rs:1180 and the other m at :1241-1250)."""
    log_q = log2_exact(quotient_degree)
    v, c, n, v_stride = _lde_view(variables_lde, quotient_degree)
    s, c2, n2, s_stride = _lde_view(sigmas_lde, quotient_degree)
    z, c3, n3, z_stride = _lde_view(second_stage_lde, quotient_degree)
    m = (c + quotient_degree - 1) // quotient_degree
    if (c, n) != (c2, n2) or n3 != n:
        raise ValueError("variables, sigmas and stage-2 LDE shapes differ")
    if c3 < 2 * m:
        raise ValueError("the stage-2 LDE needs the 2 m = %d copy-permutation columns, got %d" % (2 * m, c3))
    if len(alphas) != m + 1:
        raise ValueError("expected m + 1 = %d challenges, got %d" % (m + 1, len(alphas)))
    log_n = log2_exact(n)
    total = n * quotient_degree
    _acc_view(dst_c0, total), _acc_view(dst_c1, total)
    k = non_residues_for_copy_permutation(n, c)
    a = (ctypes.c_uint64 * (2 * (m + 1)))(*[limb % P for pair in alphas for limb in pair])
    call("bj_quotient_copy_permutation_d", v.data_ptr(), v_stride, s.data_ptr(), s_stride, z.data_ptr(), z_stride, c,
         log_n, log_q, (ctypes.c_uint64 * c)(*k), beta[0] % P, beta[1] % P, gamma[0] % P, gamma[1] % P, a,
         dst_c0.data_ptr(), dst_c1.data_ptr(), stream_of(dst_c0))


def lookup_term(sources, coefficients, beta, encoding, alpha, quotient_degree, dst_c0, dst_c1, f=None):
    """dst += alpha (E (beta + sum_t coefficients[t] sources[t]) - f) (bj_quotient_lookup_term_d):
    sources are up to 16 LDE columns (D, n) of any tensors, encoding the (c0, c1) pair of LDE
    columns of E, f an LDE column or None for 1."""
    log_q = log2_exact(quotient_degree)
    if not 1 <= len(sources) <= MAX_LOOKUP_SOURCES:
        raise ValueError("1..%d source columns, got %d" % (MAX_LOOKUP_SOURCES, len(sources)))
    if len(coefficients) != len(sources):
        raise ValueError("one coefficient per source column")
    cols = [_lde_view(t, quotient_degree) for t in list(sources) + list(encoding) + ([f] if f is not None else [])]
    n = cols[0][2]
    if any(v[1] != 1 or v[2] != n for v in cols):
        raise ValueError("every column must be one LDE column of %d rows per coset" % n)
    total = n * quotient_degree
    _acc_view(dst_c0, total), _acc_view(dst_c1, total)
    ptrs = (ctypes.c_void_p * len(sources))(*[v[0].data_ptr() for v in cols[:len(sources)]])
    g = (ctypes.c_uint64 * (2 * len(sources)))(*[limb % P for pair in coefficients for limb in pair])
    e0, e1 = cols[len(sources)][0], cols[len(sources) + 1][0]
    call("bj_quotient_lookup_term_d", ptrs, len(sources), g, beta[0] % P, beta[1] % P, e0.data_ptr(), e1.data_ptr(),
         cols[-1][0].data_ptr() if f is not None else None, alpha[0] % P, alpha[1] % P, log2_exact(n), log_q,
         dst_c0.data_ptr(), dst_c1.data_ptr(), stream_of(dst_c0))


def compute_quotient_terms_for_lookup_specialized(variables_lde, multiplicities_lde, witness_encodings_lde,
                                                  multiplicity_encodings_lde, constants_lde, tables_lde, beta, gamma,
                                                  alphas, table_id_column_idxes, column_elements_per_subargument,
                                                  num_subarguments, num_multiplicities_polys, variables_offset,
                                                  quotient_degree, dst_c0, dst_c1):
    """lookup_argument_in_ext.rs:949-1310.  The reference's witness, second_stage and setup storages
    come apart into their LDEs: variables_lde, multiplicities_lde (witness), witness_encodings_lde
    and multiplicity_encodings_lde (second stage: lists of (c0, c1) pairs of LDE columns),
    constants_lde and tables_lde (setup); each LDE is a (C, D, n) tensor or a list of (D, n)
    columns.  alphas: num_subarguments + num_multiplicities_polys Ext2 challenges (:973), the
    witness-encoding terms' first.  The table aggregation of :1023-1104 is folded into the
    multiplicity term."""
    if len(alphas) != num_subarguments + num_multiplicities_polys:
        raise ValueError("expected %d challenges, got %d" % (num_subarguments + num_multiplicities_polys, len(alphas)))
    if len(table_id_column_idxes) > 1:
        raise ValueError("at most one shared table-id column (:987-991)")
    capacity = column_elements_per_subargument + len(table_id_column_idxes)   # :998
    if len(tables_lde) != capacity:
        raise ValueError("expected %d table columns, got %d" % (capacity, len(tables_lde)))
    powers = [(1, 0)]   # of gamma, :1000-1014, as stage2.compute_lookup_poly_pairs_specialized builds them
    g = (gamma[0] % P, gamma[1] % P)
    while len(powers) < capacity:
        powers.append(ext2_mul(powers[-1], g))
    for s in range(num_subarguments):   # A_s (beta + sum gamma^t col_t) - 1, :1115-1229
        first = variables_offset + s * column_elements_per_subargument
        sources = [variables_lde[first + t] for t in range(column_elements_per_subargument)]
        if table_id_column_idxes:
            sources.append(constants_lde[table_id_column_idxes[0]])
        lookup_term(sources, powers, beta, witness_encodings_lde[s], alphas[s], quotient_degree, dst_c0, dst_c1)
    tables = [tables_lde[t] for t in range(capacity)]
    for i in range(num_multiplicities_polys):   # B (beta + sum gamma^t table_t) - multiplicity, :1231-1310
        lookup_term(tables, powers, beta, multiplicity_encodings_lde[i], alphas[num_subarguments + i],
                    quotient_degree, dst_c0, dst_c1, f=multiplicities_lde[i])


def divide_by_vanishing_for_bitreversed_coset_enumeration(dst_c0, dst_c1, log_n):
    """utils.rs:770-817 on both halves of the accumulator (q * n words each), in place."""
    log_q = log2_exact(dst_c0.numel()) - log_n
    if log_q < 0:
        raise ValueError("the accumulator is shorter than one coset")
    _acc_view(dst_c1, dst_c0.numel())
    call("bj_quotient_divide_vanishing_d", _acc_view(dst_c0, dst_c0.numel()).data_ptr(), dst_c1.data_ptr(), log_n,
         log_q, stream_of(dst_c0))


def quotient_monomials(dst_c0, dst_c1, log_n):
    """prover.rs:1399-1467 on the divided accumulator, which is left as it is: the leaf order is the
    bit-reversed enumeration of the whole q * n domain, so one bit reversal and one
    ifft_natural_to_natural on the coset 7 give the q * n monomial coefficients of each half.
    Returns (chunks, top_is_zero): chunks the (2 q, n) tensor chunk_0.c0, chunk_0.c1, chunk_1.c0,
    ... that commit.quotient_commit takes, and top_is_zero the pair of booleans the reference
    asserts as "unsatisfied" (prover.rs:1424-1439) -- reported here, not raised; reading them
    synchronises."""
    total = dst_c0.numel()
    n = 1 << log_n
    q = total // n
    if q * n != total:
        raise ValueError("the accumulator is no multiple of a coset")
    log2_exact(q)
    halves = torch.stack([_acc_view(dst_c0, total).reshape(-1), _acc_view(dst_c1, total).reshape(-1)])
    if total > 1:
        bitreverse_enumeration_inplace(halves)
        ifft_natural_to_natural(halves, coset=GENERATOR)
    top = to_host(halves[:, -1])
    chunks = halves.reshape(2, q, n).transpose(0, 1).reshape(2 * q, n)
    return chunks, (int(top[0]) == 0, int(top[1]) == 0)


def quotient_from_arguments(variables_lde, sigmas_lde, second_stage_lde, beta, gamma, challenges, quotient_degree,
                            lookup=None, gate_terms=None, gates=None):
    """The block prover.rs:1145-1467 without the gate evaluation: accumulator (zeros, or the
    caller's gate terms (c0, c1), which are added to in place) -> copy-permutation terms -> lookup
    terms if any -> division -> monomials.  challenges: the Ext2 challenges in the reference's
    order, one for L_1, m for the relations, then the lookup ones.  second_stage_lde: the LDE of
    stage2.SecondStageTrace.trace (z, the intermediates, the witness encodings, the multiplicity
    encodings).  lookup: None, or a dict with variables_lde (default: the variables_lde argument),
    multiplicities_lde, constants_lde, tables_lde, beta, gamma, table_id_column_idxes,
    column_elements_per_subargument, num_subarguments, variables_offset.
    gates: None, or a dict with gate_set (a gates.GateSet), alphas (its Ext2 challenge powers),
    constants_lde, and optionally witnesses_lde and variables_lde (default: the variables_lde
    argument): the gate terms are evaluated into the accumulator before the copy-permutation
    terms (gates.evaluate_gate_terms); with gate_terms as well, both are added.
    Returns what quotient_monomials returns."""
    _, c, n, _ = _lde_view(variables_lde, quotient_degree)
    m = (c + quotient_degree - 1) // quotient_degree
    total = n * quotient_degree
    if gate_terms is None:
        dst_c0 = torch.zeros((total,), dtype=torch.int64, device=variables_lde.device)
        dst_c1 = torch.zeros_like(dst_c0)
    else:
        dst_c0, dst_c1 = gate_terms
    if gates is not None:
        from .gates import evaluate_gate_terms
        evaluate_gate_terms(gates["gate_set"], gates.get("variables_lde", variables_lde), gates.get("witnesses_lde"),
                            gates.get("constants_lde"), gates["alphas"], quotient_degree, dst_c0, dst_c1)
    challenges = list(challenges)
    compute_quotient_terms_in_extension(variables_lde, sigmas_lde, second_stage_lde, beta, gamma,
                                        challenges[:m + 1], quotient_degree, dst_c0, dst_c1)
    used = m + 1
    if lookup is not None:
        reps, n_mult = lookup["num_subarguments"], len(lookup["multiplicities_lde"])
        enc = [(second_stage_lde[2 * m + 2 * i], second_stage_lde[2 * m + 2 * i + 1]) for i in range(reps + n_mult)]
        compute_quotient_terms_for_lookup_specialized(
            lookup.get("variables_lde", variables_lde), lookup["multiplicities_lde"], enc[:reps], enc[reps:],
            lookup["constants_lde"], lookup["tables_lde"], lookup["beta"], lookup["gamma"],
            challenges[used:used + reps + n_mult], lookup["table_id_column_idxes"],
            lookup["column_elements_per_subargument"], reps, n_mult, lookup["variables_offset"], quotient_degree,
            dst_c0, dst_c1)
        used += reps + n_mult
    if used != len(challenges):
        raise ValueError("must exhaust all the challenges (prover.rs:1364): %d given, %d used" % (len(challenges), used))
    divide_by_vanishing_for_bitreversed_coset_enumeration(dst_c0, dst_c1, log2_exact(n))
    return quotient_monomials(dst_c0, dst_c1, log2_exact(n))
