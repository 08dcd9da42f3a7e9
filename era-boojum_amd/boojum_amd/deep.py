"""DEEP on the GPU: evaluations at z and the quotening pass that builds the codeword fri.py folds.

* Evaluations at z (prover.rs:1501-1780): every committed polynomial at the out-of-domain point z
  (a few also at z * omega and at 0), as barycentric sums over coset 0 of the LDE
  (cs/implementations/utils.rs:907-1200).  `precompute_for_barycentric_evaluation_in_extension`
  gives the weights (bj_barycentric_weights_d), `barycentric_evaluate_*_for_bitreversed` the sums
  of many columns in one call (bj_evaluate_at_d).
* Quotening (prover.rs:1823-2050, quotening_operation_in_extension :2523-2706): for every point x
  of the whole LDE domain, sum_j c^j (f_j(x) - f_j(at)) / (x - at), accumulated over the opening
  points z, z * omega, 0 and the public-input rows (bj_deep_quotient_d, one call per point and
  source tensor), or all of them over every source tensor in one launch (`deep_codeword`,
  bj_deep_codeword_d).

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

from ._lib import DEEP_MAX_GROUPS, DEEP_MAX_POINTS, DEEP_MAX_TERMS, DeepCodewordDesc, call
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


def codeword_terms(group_cols, points):
    """The terms of one bj_deep_codeword_d call, host arithmetic only.  group_cols: the column
    count of every group; points: [(at, entries)], entries [(group, col, is_ext, challenge,
    value_at)] in challenge order -- quotening_plan's entries with the group in front.  Per point,
    in order, and per group it has sources in, in group order: quotening_plan over that group's
    entries, trimmed to the column range [first, first + count) the entries touch.  Returns
    (terms, gammas, ks): terms [(group, first_col, n_cols, point, gamma_offset)] sorted by point,
    gammas the flat list of Ext2 coefficients the offsets index, ks the Ext2 constant of every
    point (the sum over its groups)."""
    terms, gammas, ks = [], [], []
    for p, (_, entries) in enumerate(points):
        k = (0, 0)
        for g, n_cols in enumerate(group_cols):
            mine = [e[1:] for e in entries if e[0] == g]
            if not mine:
                continue
            full, kg = quotening_plan(n_cols, mine)
            k = ((k[0] + kg[0]) % P, (k[1] + kg[1]) % P)
            first = min(col for col, _, _, _ in mine)
            end = max(col + (2 if is_ext else 1) for col, is_ext, _, _ in mine)
            terms.append((g, first, end - first, p, len(gammas)))
            gammas += full[first:end]
        for e in entries:
            if not 0 <= e[0] < len(group_cols):
                raise ValueError("group %d outside [0, %d)" % (e[0], len(group_cols)))
        ks.append(k)
    return terms, gammas, ks


def codeword_descriptor(groups, points, terms, ks, gammas_ptr, n_gammas, log_domain, row0, n_rows, dst0, dst1,
                        accumulate):
    """bj_deep_codeword_t from plain values.  groups: [(ptr, n_cols, col_stride)]; points: [(at, _)];
    terms and ks: codeword_terms'; the pointers are integers (0 for NULL)."""
    if len(groups) > DEEP_MAX_GROUPS or len(points) > DEEP_MAX_POINTS or len(terms) > DEEP_MAX_TERMS:
        raise ValueError("%d groups, %d points, %d terms exceed the caps %d, %d, %d of one call"
                         % (len(groups), len(points), len(terms), DEEP_MAX_GROUPS, DEEP_MAX_POINTS, DEEP_MAX_TERMS))
    d = DeepCodewordDesc()
    for i, (ptr, n_cols, stride) in enumerate(groups):
        d.groups[i].cols, d.groups[i].n_cols, d.groups[i].col_stride = ptr or None, n_cols, stride
    for i, ((at, _), k) in enumerate(zip(points, ks)):
        d.points[i].at0, d.points[i].at1, d.points[i].k0, d.points[i].k1 = at[0] % P, at[1] % P, k[0] % P, k[1] % P
    for i, (g, first, count, p, off) in enumerate(terms):
        t = d.terms[i]
        t.group, t.first_col, t.n_cols, t.point, t.gamma_offset = g, first, count, p, off
    d.n_groups, d.n_points, d.n_terms, d.log_domain = len(groups), len(points), len(terms), log_domain
    d.gammas, d.n_gammas, d.row0, d.n_rows = gammas_ptr or None, n_gammas, row0, n_rows
    d.dst0, d.dst1, d.accumulate = dst0 or None, dst1 or None, 1 if accumulate else 0
    return d


def deep_codeword(groups, points, log_domain, row0=0, out=None, accumulate=False):
    """Every opening point of the codeword over rows [row0, row0 + rows) of the flat bit-reversed
    domain of 2^log_domain points in one launch (bj_deep_codeword_d): what one
    quotening_operation_in_extension per (group, point) leaves, word for word.  groups: (C, rows)
    device column views over the same row window (an oracle's LDE, flattened); points: [(at,
    entries)] as codeword_terms takes them; out: None or the pair (dst_c0, dst_c1) of (rows,)
    device columns.  The coefficients of all terms go to the device in one copy.  Returns
    (dst_c0, dst_c1)."""
    import ctypes
    views = [col_view(g) for g in groups]
    if out is None:
        if not views:
            raise ValueError("without groups the row count comes from `out`")
        if accumulate:
            raise ValueError("accumulate needs `out`")
        buf = torch.empty((2, views[0][2]), dtype=torch.int64, device=views[0][0].device)
        out = (buf[0], buf[1])
    dst0, dst1 = out
    n_rows = dst0.shape[-1]
    if dst1.shape[-1] != n_rows or any(v[2] != n_rows for v in views):
        raise ValueError("groups and dst row counts differ")
    terms, gammas, ks = codeword_terms([v[1] for v in views], points)
    g = to_device(np.array(gammas, dtype=np.uint64).reshape(-1), dst0.device) if gammas else None
    d = codeword_descriptor([(v[0].data_ptr(), v[1], v[3]) for v in views], points, terms, ks,
                            g.data_ptr() if gammas else 0, len(gammas), log_domain, row0, n_rows, dst0.data_ptr(),
                            dst1.data_ptr(), accumulate)
    call("bj_deep_codeword_d", ctypes.byref(d), stream_of(dst0))
    return dst0, dst1
