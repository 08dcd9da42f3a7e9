"""Stage 2 on the GPU: the columns of the stage-2 oracle (prover.rs:360-438), computed from witness
and setup columns that stay on the device and laid out so that they go to the commit uncopied.

* Copy permutation (cs/implementations/copy_permutation.rs:649-774, called at prover.rs:360-392):
  the grand product z(x) and the intermediate partial products, over the main domain in natural
  order (bj_copy_permutation_d).
* Lookup (cs/implementations/lookup_argument_in_ext.rs:320-700, the specialized-columns variants):
  the witness encodings A_s = 1 / (beta + sum_t gamma^t col_{s,t}) and the multiplicity encodings
  B = mult / (beta + sum_t gamma^t table_t), both through bj_lookup_encoding_d.
* `second_stage_trace` allocates the (columns, n) tensor of the stage-2 leaf order
  (prover.rs:520-547) once; the two computations fill views of it and the whole tensor goes to
  `commit.commit_trace_columns`.

GoldilocksExt2 values are (c0, c1) pairs of Python integers on the host and pairs of base columns
on the device.  The challenges and their powers are host arithmetic on single field elements, as in
the reference's own driver.
"""
import ctypes
from collections import namedtuple

import torch

from ._lib import BoojumError, call
from .field import P, col_view, ext2_mul, log2_exact, new_status, read_status, stream_of

# LookupParameters::UseSpecializedColumnsWithTableIdAsVariable / ...AsConstant
# (lookup_argument_in_ext.rs:353-383): kind is "variable" or "constant"
LookupParameters = namedtuple("LookupParameters", "kind width num_repetitions")

MAX_LOOKUP_SOURCES = 16


def non_residues_for_copy_permutation(domain_size, num_columns):
    """copy_permutation.rs:512-522: [1] + make_non_residues(num_columns - 1, domain_size)
    (utils.rs:636-688), as Python integers.  Host only."""
    out = (ctypes.c_uint64 * num_columns)()
    call("bj_non_residues_h", num_columns, log2_exact(domain_size), out)
    return [int(v) for v in out]


def num_intermediate_partial_product_relations(num_cols, quotient_degree):
    """copy_permutation.rs:14-28: ceil(num_cols / quotient_degree) - 1, and 0 for one chunk."""
    if num_cols <= quotient_degree:
        return 0
    return (num_cols + quotient_degree - 1) // quotient_degree - 1


def _pairs(t):
    """(2k, n) rows -> [(c0, c1)] views."""
    return [(t[2 * i], t[2 * i + 1]) for i in range(t.shape[0] // 2)]


def compute_partial_products_in_extension(variables, sigmas, beta, gamma, max_degree, out=None, check=True):
    """copy_permutation.rs:649-774.  variables, sigmas: (C, n) device columns in natural order;
    beta, gamma: Ext2 challenges; max_degree: the chunk size (the quotient degree, a power of
    two).  Returns (z, intermediates): z a (c0, c1) pair of (n,) columns and intermediates a list of
    m - 1 such pairs, m = ceil(C / max_degree), all of them views into `out`, a (2 m, n) tensor in
    the order z.c0, z.c1, p_0.c0, p_0.c1, ... (allocated when not given).

    With one chunk (m = 1) there is NO intermediate.  The reference returns its lone per-chunk
    product in that case (copy_permutation.rs:747-749), but
    num_intermediate_partial_product_relations (copy_permutation.rs:14-28) counts 0 relations for
    it and that count is what the verifier uses.

    check=True reads the call's status record, which synchronises, and raises BoojumError where
    the reference panics: on a zero denominator (utils.rs:425-427) and on a product over all rows
    other than one (copy_permutation.rs:485).  check=False leaves the call asynchronous; the status
    tensor of the last call is `compute_partial_products_in_extension.status`."""
    v, c, n, v_stride = col_view(variables)
    s, c2, n2, s_stride = col_view(sigmas)
    if (c, n) != (c2, n2):
        raise ValueError("variables and sigmas shapes differ")
    log_n = log2_exact(n)
    log2_exact(max_degree)
    m = (c + max_degree - 1) // max_degree
    if out is None:
        out = torch.empty((2 * m, n), dtype=torch.int64, device=v.device)
    o, oc, on, o_stride = col_view(out)
    if (oc, on) != (2 * m, n):
        raise ValueError("out must be (%d, %d), got (%d, %d)" % (2 * m, n, oc, on))
    k = non_residues_for_copy_permutation(n, c)
    status = new_status(v.device)
    call("bj_copy_permutation_d", v.data_ptr(), v_stride, s.data_ptr(), s_stride, c, log_n,
         (ctypes.c_uint64 * c)(*k), beta[0] % P, beta[1] % P, gamma[0] % P, gamma[1] % P, max_degree, o.data_ptr(),
         o_stride, status.data_ptr(), stream_of(v))
    compute_partial_products_in_extension.status = status
    if check:
        t0, t1, zeros, _ = read_status(status)
        total = (t0, t1)
        if zeros:
            raise BoojumError("copy permutation: %d zero denominator(s)" % zeros)
        if total != (1, 0):
            raise BoojumError("copy permutation: the grand product over the domain is %r, not one" % (total,))
    pairs = _pairs(o)
    return pairs[0], pairs[1:]


def lookup_encoding(sources, coefficients, beta, out_c0, out_c1, f=None, status=None):
    """out = f / (beta + sum_t coefficients[t] * sources[t]) (bj_lookup_encoding_d): sources are up
    to 16 (n,) device columns of any tensors, coefficients Ext2 pairs, f a device column or None
    for 1.  Returns the status tensor."""
    n = out_c0.shape[-1]
    if not 1 <= len(sources) <= MAX_LOOKUP_SOURCES:
        raise ValueError("1..%d source columns, got %d" % (MAX_LOOKUP_SOURCES, len(sources)))
    if len(coefficients) != len(sources):
        raise ValueError("one coefficient per source column")
    cols = [col_view(t)[0] for t in list(sources) + [out_c0, out_c1] + ([f] if f is not None else [])]
    if any(t.shape != (1, n) for t in cols):
        raise ValueError("every column must have %d rows" % n)
    if status is None:
        status = new_status(out_c0.device)
    ptrs = (ctypes.c_void_p * len(sources))(*[t.data_ptr() for t in cols[:len(sources)]])
    g = (ctypes.c_uint64 * (2 * len(sources)))(*[limb % P for pair in coefficients for limb in pair])
    call("bj_lookup_encoding_d", ptrs, len(sources), g, beta[0] % P, beta[1] % P,
         f.data_ptr() if f is not None else None, log2_exact(n), out_c0.data_ptr(), out_c1.data_ptr(),
         status.data_ptr(), stream_of(out_c0))
    return status


def _lookup_shape(lookup_parameters):
    p = LookupParameters(*lookup_parameters)
    if p.kind == "variable":    # the table id is one more variable column (:354-365)
        return p, p.width + 1, p.width + 1
    if p.kind == "constant":    # the table id is a setup constant column (:366-381)
        return p, p.width, p.width + 1
    raise ValueError("lookup kind must be 'variable' or 'constant' (the general-purpose-columns variant is "
                     "todo!() in the reference's prover, prover.rs:408-438)")


def compute_lookup_poly_pairs_specialized(variables_columns, multiplicities_columns, constant_polys,
                                          lookup_tables_columns, table_id_column_idxes, beta, gamma,
                                          variables_offset, lookup_parameters, out=None, check=True):
    """lookup_argument_in_ext.rs:320-700.  Column arguments are (C, n) device tensors or lists of
    (n,) columns; lookup_parameters is a LookupParameters (kind, width, num_repetitions).  Returns
    (witness_encodings, multiplicity_encodings), lists of (c0, c1) pairs that are views into `out`,
    a (2 (num_repetitions + number of multiplicity columns), n) tensor (allocated when not given).
    check=True synchronises and raises BoojumError on a zero denominator (the reference's batch
    inverse panics, utils.rs:425-427)."""
    p, per_arg, total = _lookup_shape(lookup_parameters)
    if len(lookup_tables_columns) != total:
        raise ValueError("expected %d table columns, got %d" % (total, len(lookup_tables_columns)))
    use_constant = p.kind == "constant"
    if use_constant != bool(len(table_id_column_idxes)):
        raise ValueError("table_id_column_idxes goes with the table-id-as-constant variant only")
    powers = [(1, 0)]   # of gamma, :402-418
    g = (gamma[0] % P, gamma[1] % P)
    while len(powers) < total:
        powers.append(ext2_mul(powers[-1], g))
    n_mult = len(multiplicities_columns)
    n = lookup_tables_columns[0].shape[-1]
    if out is None:
        out = torch.empty((2 * (p.num_repetitions + n_mult), n), dtype=torch.int64,
                          device=lookup_tables_columns[0].device)
    if tuple(out.shape) != (2 * (p.num_repetitions + n_mult), n):
        raise ValueError("out must be (%d, %d)" % (2 * (p.num_repetitions + n_mult), n))
    pairs = _pairs(out)
    statuses = []
    for s in range(p.num_repetitions):
        first = variables_offset + s * per_arg
        sources = [variables_columns[first + t] for t in range(per_arg)]
        if use_constant:
            sources.append(constant_polys[table_id_column_idxes[0]])
        statuses.append(lookup_encoding(sources, powers, beta, *pairs[s]))
    tables = [lookup_tables_columns[t] for t in range(total)]
    for i in range(n_mult):
        statuses.append(lookup_encoding(tables, powers, beta, *pairs[p.num_repetitions + i],
                                        f=multiplicities_columns[i]))
    if check:
        zeros = sum(read_status(st)[2] for st in statuses)
        if zeros:
            raise BoojumError("lookup encodings: %d zero denominator(s)" % zeros)
    return pairs[:p.num_repetitions], pairs[p.num_repetitions:]


class SecondStageTrace:
    """The stage-2 columns in leaf order (prover.rs:520-547): z, the intermediates, the lookup
    witness encodings, the multiplicity encodings, each as c0 then c1, rows of one (columns, n)
    tensor `trace`; `copy_permutation` and `lookup` are the row ranges the two computations fill."""

    def __init__(self, n, num_copy_permutation_columns, quotient_degree, n_witness_enc=0, n_mult_enc=0,
                 device="cuda"):
        m = (num_copy_permutation_columns + quotient_degree - 1) // quotient_degree
        self.trace = torch.empty((2 * (m + n_witness_enc + n_mult_enc), n), dtype=torch.int64, device=device)
        self.copy_permutation = self.trace[:2 * m]
        self.lookup = self.trace[2 * m:]


def second_stage_trace(variables, sigmas, beta, gamma, quotient_degree, lookup=None, check=True):
    """Both stage-2 computations into one tensor.  lookup: None, or a dict of the arguments of
    compute_lookup_poly_pairs_specialized after its challenges: variables_columns,
    multiplicities_columns, constant_polys, lookup_tables_columns, table_id_column_idxes, beta, gamma,
    variables_offset, lookup_parameters (its beta and gamma are the lookup argument's own
    challenges).  Returns the SecondStageTrace; its `trace` goes to commit.commit_trace_columns as
    it is, and `z`, `intermediates`, `witness_encodings`, `multiplicity_encodings` are the views."""
    c, n = variables.shape
    n_w = n_m = 0
    if lookup is not None:
        n_w = LookupParameters(*lookup["lookup_parameters"]).num_repetitions
        n_m = len(lookup["multiplicities_columns"])
    st = SecondStageTrace(n, c, quotient_degree, n_w, n_m, device=variables.device)
    st.z, st.intermediates = compute_partial_products_in_extension(variables, sigmas, beta, gamma, quotient_degree,
                                                                   out=st.copy_permutation, check=check)
    st.witness_encodings, st.multiplicity_encodings = [], []
    if lookup is not None:
        st.witness_encodings, st.multiplicity_encodings = compute_lookup_poly_pairs_specialized(
            out=st.lookup, check=check, **lookup)
    return st
