"""DEEP on the GPU: evaluations at z and the quotening pass that builds the codeword fri.py folds.

* Evaluations at z (prover.rs:1501-1780): every committed polynomial at the out-of-domain point z
  (a few also at z * omega and at 0), as barycentric sums over coset 0 of the LDE
  (cs/implementations/utils.rs:907-1200).  `precompute_for_barycentric_evaluation_in_extension`
  gives the weights (bj_barycentric_weights_d), `barycentric_evaluate_*_for_bitreversed` the sums
  of many columns in one call (bj_evaluate_at_d).
* Quotening (prover.rs:1823-2050, quotening_operation_in_extension :2523-2706): for every point x
  of the whole LDE domain, sum_j c^j (f_j(x) - f_j(at)) / (x - at), accumulated over the opening
  points z, z * omega, 0 and the public-input rows (bj_deep_quotient_d, one call per point).

The kernel sees base columns only.  `quotening_plan` folds the sources of one opening point --
base columns, or Ext2 polynomials held as two base columns (c0, c1) -- into one Ext2 coefficient
per base column and one Ext2 constant:

  sum_j ch_j (f_j(x) - v_j) = sum_k gamma_k col_k(x) - K,

a base source adding ch_j to its column's gamma, an Ext2 source ch_j to the c0 column's and
ch_j * u to the c1 column's, K = sum_j ch_j v_j.  That is host arithmetic on single field elements
(Python integers), as the transcript and the challenge powers are in the reference's own driver.
"""
import numpy as np
import torch

from ._lib import call
from .field import EXT2_NON_RESIDUE, P, col_view, ext2_mul, ext2_mul_by_u, log2_exact, stream_of, to_device, to_host


def materialize_ext_challenge_powers(c, n):
    """[1, c, c^2, ...], n of them, in GoldilocksExt2 (prover.rs:2374-2395), as host integers."""
    c = (c[0] % P, c[1] % P)
    out = [(1, 0)]
    while len(out) < n:
        out.append(ext2_mul(out[-1], c))
    return out[:n]


def precompute_for_barycentric_evaluation_in_extension(n, coset, at, device="cuda"):
    """utils.rs:907-1021: the weights (w0, w1), two (n,) device columns in bit-reversed order, of
    the domain coset * <w_n> at the Ext2 point `at`."""
    log_n = log2_exact(n)
    w0 = torch.empty((n,), dtype=torch.int64, device=device)
    w1 = torch.empty_like(w0)
    call("bj_barycentric_weights_d", log_n, coset % P, at[0] % P, at[1] % P, w0.data_ptr(), w1.data_ptr(),
         stream_of(w0))
    return w0, w1


def barycentric_evaluate_base_at_extension_for_bitreversed(cols_view, w):
    """utils.rs:1085-1158 for every column of `cols_view` in one call: (C, n) (or (n,)) device
    columns in bit-reversed order -- coset 0 of an LDE is lde[:, 0, :] -- and the weights `w` of
    that coset at the point.  Returns [(c0, c1)] per column as host integers."""
    t, c, n, stride = col_view(cols_view)
    w0, w1 = w
    if w0.shape[-1] != n or w1.shape[-1] != n:
        raise ValueError("weights and columns sizes do not match")
    out = torch.empty((c, 2), dtype=torch.int64, device=t.device)
    call("bj_evaluate_at_d", t.data_ptr(), c, stride, log2_exact(n), w0.data_ptr(), w1.data_ptr(), out.data_ptr(),
         stream_of(t))
    return [(int(a), int(b)) for a, b in to_host(out)]


def barycentric_evaluate_extension_at_extension_for_bitreversed(c0_cols, c1_cols, w):
    """utils.rs:1160-1200: Ext2 polynomials held as base columns c0_cols[i], c1_cols[i]: two base
    evaluations combined as e0 + u e1."""
    e0 = barycentric_evaluate_base_at_extension_for_bitreversed(c0_cols, w)
    e1 = barycentric_evaluate_base_at_extension_for_bitreversed(c1_cols, w)
    if len(e0) != len(e1):
        raise ValueError("c0 and c1 column counts differ")
    return [((a[0] + EXT2_NON_RESIDUE * b[1]) % P, (a[1] + b[0]) % P) for a, b in zip(e0, e1)]


def quotening_plan(n_cols, entries):
    """The coefficients of one opening point.  entries: [(col, is_ext, challenge, value_at)], the
    sources in challenge order; is_ext means columns col and col + 1 hold c0 and c1.  Returns
    (gammas, K): n_cols Ext2 coefficients and the Ext2 constant.  Pure Python integers."""
    gammas = [(0, 0)] * n_cols
    k = (0, 0)

    def add(col, g):
        if not 0 <= col < n_cols:
            raise ValueError("column %d outside [0, %d)" % (col, n_cols))
        gammas[col] = ((gammas[col][0] + g[0]) % P, (gammas[col][1] + g[1]) % P)

    for col, is_ext, ch, value in entries:
        ch = (ch[0] % P, ch[1] % P)
        add(col, ch)
        if is_ext:
            add(col + 1, ext2_mul_by_u(ch))
        t = ext2_mul(ch, (value[0] % P, value[1] % P))
        k = ((k[0] + t[0]) % P, (k[1] + t[1]) % P)
    return gammas, k


def quotening_operation_in_extension(dst_c0, dst_c1, storage, entries, at, log_domain, row0=0, accumulate=True):
    """One opening point of prover.rs:2523-2706 over rows [row0, row0 + len(dst)) of the flat
    bit-reversed domain of 2^log_domain points: dst (+)= (sum_j ch_j (f_j(x) - v_j)) / (x - at).
    storage: (C, rows) device columns over the same row window (None with no entries' columns);
    dst_c0, dst_c1: (rows,) device columns, updated in place."""
    n_rows = dst_c0.shape[-1]
    if dst_c1.shape[-1] != n_rows:
        raise ValueError("dst_c0 and dst_c1 sizes differ")
    if storage is None:
        ptr, c, stride = 0, 0, n_rows
    else:
        t, c, n, stride = col_view(storage)
        if n != n_rows:
            raise ValueError("storage and dst row counts differ")
        ptr = t.data_ptr()
    gammas, k = quotening_plan(c, entries)
    g = to_device(np.array(gammas, dtype=np.uint64).reshape(-1), dst_c0.device) if c else None
    call("bj_deep_quotient_d", ptr, c, stride, g.data_ptr() if c else 0, k[0], k[1], at[0] % P, at[1] % P,
         log_domain, row0, n_rows, dst_c0.data_ptr(), dst_c1.data_ptr(), 1 if accumulate else 0, stream_of(dst_c0))
    return dst_c0, dst_c1
