"""Plain-Python-integer model of the quotient block (boojum_amd/quotient.py, csrc/quotient.hip),
written from the reference's formulas on top of stage2_model and oracle/transcript.py's Ext2
arithmetic:

* the (z(x) - 1) L_1(x) term (prover.rs:1148-1227, unnormalized_l1_inverse utils.rs:1585-1665) and
  compute_quotient_terms_in_extension (copy_permutation.rs:1000-1249): `copy_permutation_terms_at`,
  one point at a time, so that the same code answers a point of the LDE domain and a point off it;
* compute_quotient_terms_for_lookup_specialized (lookup_argument_in_ext.rs:949-1310):
  `lookup_term_at`, `lookup_terms`;
* divide_by_vanishing_for_bitreversed_coset_enumeration (utils.rs:770-817): `vanishing_inverses`,
  `divide_by_vanishing`;
* flatten_presumably_bitreversed + ifft_natural_to_natural on the coset 7 and the chunks
  (prover.rs:1399-1467): `monomials_of_leaf_order`, `chunk_columns`;
* a small coset LDE (utils.rs:311-403) for the sizes the tests use: `coset_lde`.

The LDE domain is in leaf order L = coset * n + row with x_L = 7 w_{nq}^(bitrev(L)); Ext2 values are
(c0, c1) tuples."""
import numpy as np

import stage2_model as S
import transcript as T

P = T.P
ONE, ZERO = (1, 0), (0, 0)
GEN = T.GEN


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def e_pow(a, e):
    r = ONE
    while e:
        if e & 1:
            r = T.e_mul(r, a)
        a = T.e_mul(a, a)
        e >>= 1
    return r


# ------------------------------------------------------------------ transforms
def _fft(a, omega):
    """sum_j a[j] omega^(j k), k < len(a), natural order in and out (radix 2, recursive)."""
    n = len(a)
    if n == 1:
        return list(a)
    sq = omega * omega % P
    even, odd = _fft(a[0::2], sq), _fft(a[1::2], sq)
    out, w = [0] * n, 1
    for i in range(n // 2):
        t = w * odd[i] % P
        out[i] = (even[i] + t) % P
        out[i + n // 2] = (even[i] - t) % P
        w = w * omega % P
    return out


def monomials(values):
    """Coefficients of the polynomial of degree < n with the given values on w_n^i, i < n
    (ifft_natural_to_natural, fft/mod.rs:464-491, coset 1)."""
    n = len(values)
    log_n = n.bit_length() - 1
    inv_n = pow(n, P - 2, P)
    return [v * inv_n % P for v in _fft([int(v) % P for v in values], pow(T.domain_generator(log_n), P - 2, P))]


def lde_points(log_n, log_q):
    """x_L, L < q n."""
    bits = log_n + log_q
    w = T.domain_generator(bits)
    return [GEN * pow(w, bitrev(i, bits), P) % P for i in range(1 << bits)]


def evaluate_on_lde(coeffs, log_n, log_q):
    """Values of a polynomial of degree < n on the q-LDE domain in leaf order
    (transform_monomials_to_lde, utils.rs:311-403: coset i is 7 w_{nq}^(bitrev(i)) <w_n>, its rows
    bit-reversed -- together the bit-reversed enumeration of 7 <w_{nq}>)."""
    bits = log_n + log_q
    scaled, g = [], 1
    for c in coeffs:
        scaled.append(c * g % P)
        g = g * GEN % P
    nat = _fft(scaled + [0] * ((1 << bits) - len(scaled)), T.domain_generator(bits))
    return [nat[bitrev(i, bits)] for i in range(1 << bits)]


def coset_lde(values, log_q):
    """Main-domain values of one base column -> its q-LDE in leaf order."""
    return evaluate_on_lde(monomials(values), len(values).bit_length() - 1, log_q)


def ext_lde(poly, log_q):
    """An Ext2 polynomial as main-domain values [(c0, c1)] -> [(c0, c1)] on the LDE domain."""
    return list(zip(coset_lde([v[0] for v in poly], log_q), coset_lde([v[1] for v in poly], log_q)))


def monomials_of_leaf_order(values, log_n, log_q):
    """flatten_presumably_bitreversed (the leaf order is the bit-reversed enumeration of the whole
    domain, prover.rs:1409-1410) and ifft_natural_to_natural with the coset 7 (:1421-1422)."""
    bits = log_n + log_q
    nat = [int(values[bitrev(i, bits)]) % P for i in range(1 << bits)]
    inv_n = pow(1 << bits, P - 2, P)
    raw = _fft(nat, pow(T.domain_generator(bits), P - 2, P))
    ginv, g, out = pow(GEN, P - 2, P), 1, []
    for v in raw:
        out.append(v * inv_n % P * g % P)
        g = g * ginv % P
    return out


def horner(coeffs, at):
    """A base-field polynomial at an Ext2 point."""
    acc = ZERO
    for c in reversed(coeffs):
        acc = T.e_add(T.e_mul(acc, at), (c, 0))
    return acc


def horner_ext(c0, c1, at):
    """c0(at) + u c1(at)."""
    a, b = horner(c0, at), horner(c1, at)
    return T.e_add(a, T.e_mul(b, (0, 1)))


# ------------------------------------------------------------------ terms at one point
def copy_permutation_terms_at(x, w, sigma, z, z_next, inter, beta, gamma, alphas, q, k, n):
    """The sum of t_0 .. t_m at the Ext2 point x.  w, sigma: the C columns' values at x; z, z_next:
    z(x) and z(w_n x); inter: p_0(x) .. p_{m-2}(x); all Ext2.  alphas: m + 1, the L_1 term's first.
      t_0     = alpha_0 (z - 1) (x^n - 1) / (x - 1)               prover.rs:1196-1225, utils.rs:1597-1657
      t_{j+1} = alpha_{j+1} (lhs_j prod (w + beta sigma + gamma) - rhs_j prod (w + beta k x + gamma))
                                                                   copy_permutation.rs:1114-1242
    with rhs = [z] + inter (:1085-1090) and lhs = inter + [z_next] (:1041-1071)."""
    n_cols = len(w)
    m = (n_cols + q - 1) // q
    assert len(alphas) == m + 1 and len(inter) == m - 1
    l1 = T.e_mul(T.e_sub(e_pow(x, n), ONE), T.e_inv(T.e_sub(x, ONE)))
    total = T.e_mul(alphas[0], T.e_mul(T.e_sub(z, ONE), l1))
    rhs, lhs = [z] + list(inter), list(inter) + [z_next]
    for j in range(m):
        d, nm = lhs[j], rhs[j]
        for c in range(j * q, min(n_cols, (j + 1) * q)):
            d = T.e_mul(d, T.e_add(T.e_add(w[c], T.e_mul(beta, sigma[c])), gamma))
            nm = T.e_mul(nm, T.e_add(T.e_add(w[c], T.e_mul(beta, T.e_mul_base(x, k[c]))), gamma))
        total = T.e_add(total, T.e_mul(alphas[j + 1], T.e_sub(d, nm)))
    return total


def lookup_term_at(e, srcs, g, beta, f, alpha):
    """alpha (E (beta + sum_t g_t src_t) - f) at one point, everything Ext2
    (lookup_argument_in_ext.rs:1157-1198 with f = 1, :1266-1287 with f = the multiplicity)."""
    d = beta
    for s, gt in zip(srcs, g):
        d = T.e_add(d, T.e_mul(gt, s))
    return T.e_mul(alpha, T.e_sub(T.e_mul(e, d), f))


def _b(v):
    return (int(v) % P, 0)


def _e(v):
    return (int(v[0]) % P, int(v[1]) % P)


# ------------------------------------------------------------------ terms over the LDE domain
def next_row_index(L, log_n):
    """The leaf holding w_n x_L: same coset, row bitrev(bitrev(row) + 1 mod n)
    (shift_by_omega_assuming_bitreversed, utils.rs:1245-1271)."""
    n = 1 << log_n
    row = L & (n - 1)
    return (L - row) | bitrev((bitrev(row, log_n) + 1) % n, log_n)


def copy_permutation_terms(w_lde, sigma_lde, s2_lde, beta, gamma, alphas, log_n, log_q, k=None):
    """w_lde, sigma_lde: C base columns of q n values; s2_lde: [z, p_0, ..] as lists of q n Ext2
    values.  Returns the q n contributions (L_1 term and all relations)."""
    n, q = 1 << log_n, 1 << log_q
    n_cols = len(w_lde)
    k = k or S.non_residues_for_copy_permutation(n, n_cols)
    beta, gamma, alphas = _e(beta), _e(gamma), [_e(a) for a in alphas]
    xs = lde_points(log_n, log_q)
    out = []
    for L in range(n * q):
        out.append(copy_permutation_terms_at(
            (xs[L], 0), [_b(col[L]) for col in w_lde], [_b(col[L]) for col in sigma_lde], _e(s2_lde[0][L]),
            _e(s2_lde[0][next_row_index(L, log_n)]), [_e(p[L]) for p in s2_lde[1:]], beta, gamma, alphas, q,
            [int(v) % P for v in k], n))
    return out


def lookup_term(e_lde, srcs_lde, g, beta, f_lde, alpha):
    """One bj_quotient_lookup_term_d over the domain: e_lde Ext2 values, srcs_lde base columns,
    f_lde a base column or None for 1."""
    g, beta, alpha = [_e(v) for v in g], _e(beta), _e(alpha)
    return [lookup_term_at(_e(e_lde[L]), [_b(s[L]) for s in srcs_lde], g, beta,
                           ONE if f_lde is None else _b(f_lde[L]), alpha) for L in range(len(e_lde))]


def lookup_terms(variables_lde, mult_lde, wit_enc_lde, mult_enc_lde, constants_lde, tables_lde, beta, gamma, alphas,
                 table_id_column_idxes, per_arg, num_subarguments, variables_offset):
    """compute_quotient_terms_for_lookup_specialized (lookup_argument_in_ext.rs:949-1310): the sum of
    the A terms (:1115-1229) and the B terms (:1231-1310; the table aggregation of :1023-1104 is
    beta + sum gamma^t table_t)."""
    capacity = per_arg + len(table_id_column_idxes)
    assert len(tables_lde) == capacity and len(alphas) == num_subarguments + len(mult_lde)
    powers = S.gamma_powers(gamma, capacity)
    total = [ZERO] * len(tables_lde[0])
    for s in range(num_subarguments):
        first = variables_offset + s * per_arg
        srcs = [variables_lde[first + t] for t in range(per_arg)]
        if table_id_column_idxes:
            srcs.append(constants_lde[table_id_column_idxes[0]])
        total = [T.e_add(a, b) for a, b in zip(total, lookup_term(wit_enc_lde[s], srcs, powers, beta, None, alphas[s]))]
    for i, mcol in enumerate(mult_lde):
        t = lookup_term(mult_enc_lde[i], list(tables_lde), powers, beta, mcol, alphas[num_subarguments + i])
        total = [T.e_add(a, b) for a, b in zip(total, t)]
    return total


# ------------------------------------------------------------------ division, monomials, chunks
def vanishing_inverses(log_n, log_q):
    """utils.rs:788-799: 1 / (7^n w_{nq}^(n i) - 1), i < q, bit-reversed."""
    n, q = 1 << log_n, 1 << log_q
    coset_in_n = pow(T.domain_generator(log_n + log_q), n, P)
    gen_in_n = pow(GEN, n, P)
    powers = [(pow(coset_in_n, i, P) * gen_in_n - 1) % P for i in range(q)]
    return [pow(powers[bitrev(i, log_q)], P - 2, P) for i in range(q)]


def divide_by_vanishing(acc, log_n, log_q):
    inv = vanishing_inverses(log_n, log_q)
    return [T.e_mul_base(v, inv[L >> log_n]) for L, v in enumerate(acc)]


def quotient_monomials(acc, log_n, log_q):
    """The divided accumulator -> (c0 coefficients, c1 coefficients), q n each."""
    return (monomials_of_leaf_order([v[0] for v in acc], log_n, log_q),
            monomials_of_leaf_order([v[1] for v in acc], log_n, log_q))


def chunk_columns(mono, log_n):
    """prover.rs:1454-1467: (2 q, n) uint64, chunk_0.c0, chunk_0.c1, chunk_1.c0, ..."""
    n = 1 << log_n
    c0, c1 = mono
    rows = []
    for i in range(len(c0) // n):
        rows.append(c0[i * n:(i + 1) * n])
        rows.append(c1[i * n:(i + 1) * n])
    return np.array(rows, dtype=np.uint64)


def acc_columns(acc):
    """Ext2 accumulator -> (2, q n) uint64."""
    return S.ext_columns([acc])


# ------------------------------------------------------------------ the whole block
class Quotient:
    """Everything the tests compare, for one (w, sigma) and one optional lookup sub-argument set:
    the stage-2 polynomials (stage2_model), the LDEs, the summed terms, the divided accumulator,
    the monomials and the chunks."""


def lookup_setup(log_n, width, reps, seed, kind="variable"):
    """Random lookup inputs in stage2_model's shapes: variables (1 + (width + 1) reps columns, the
    sub-arguments at offset 1), two constant columns, width + 1 table columns, one multiplicity
    column.  The quotient terms vanish on the domain whatever the values are, because the
    encodings are computed from them."""
    n = 1 << log_n

    def rand(shape, s, high=P):
        return np.random.default_rng(s).integers(0, high, size=shape, dtype=np.uint64)

    return dict(variables=rand((1 + (width + 1) * reps, n), seed), constants=rand((2, n), seed + 1, high=7),
                tables=rand((width + 1, n), seed + 2), mult=rand((1, n), seed + 3, high=100), kind=kind, width=width,
                reps=reps, idxes=[] if kind == "variable" else [1], beta=None, gamma=None)


def lookup_block(d, log_q, alphas, r=None):
    """The lookup side of `quotient` for a lookup_setup dict d with beta and gamma set: the encodings
    (stage2_model), every LDE and the summed terms, as attributes of r."""
    r = r or Quotient()
    r.per_arg = d["width"] + 1 if d["kind"] == "variable" else d["width"]
    r.wit, r.mult, zeros = S.lookup_poly_pairs_specialized(d["variables"], d["mult"], d["constants"], d["tables"],
                                                           d["idxes"], d["beta"], d["gamma"], 1, d["kind"], d["width"],
                                                           d["reps"])
    assert zeros == 0
    r.lk_lde = {name: [coset_lde(col, log_q) for col in d[name]] for name in ("variables", "constants", "tables", "mult")}
    r.wit_lde = [ext_lde(p, log_q) for p in r.wit]
    r.mult_lde = [ext_lde(p, log_q) for p in r.mult]
    r.lk_terms = lookup_terms(r.lk_lde["variables"], r.lk_lde["mult"], r.wit_lde, r.mult_lde, r.lk_lde["constants"],
                              r.lk_lde["tables"], d["beta"], d["gamma"], alphas, d["idxes"], r.per_arg, d["reps"], 1)
    return r


def quotient(w, sigma, beta, gamma, log_q, alphas, lookup=None, lookup_challenges=None, start=None):
    """w, sigma: (C, n) arrays; alphas: m + 1 Ext2; lookup: a lookup_setup dict with beta and gamma
    set, lookup_challenges its reps + 1 alphas; start: the accumulator's initial Ext2 contents."""
    n_cols, n = len(w), len(w[0])
    log_n = n.bit_length() - 1
    q = 1 << log_q
    r = Quotient()
    r.log_n, r.log_q = log_n, log_q
    r.cp = S.copy_permutation(w, sigma, beta, gamma, q)
    r.w_lde = [coset_lde(col, log_q) for col in w]
    r.sigma_lde = [coset_lde(col, log_q) for col in sigma]
    r.s2 = [r.cp.z] + r.cp.intermediates
    r.s2_lde = [ext_lde(p, log_q) for p in r.s2]
    acc = list(start) if start is not None else [ZERO] * (n * q)
    r.cp_terms = copy_permutation_terms(r.w_lde, r.sigma_lde, r.s2_lde, beta, gamma, alphas, log_n, log_q)
    acc = [T.e_add(a, b) for a, b in zip(acc, r.cp_terms)]
    if lookup is not None:
        lookup_block(lookup, log_q, lookup_challenges, r)
        acc = [T.e_add(a, b) for a, b in zip(acc, r.lk_terms)]
    r.terms = acc
    r.divided = divide_by_vanishing(acc, log_n, log_q)
    r.mono = quotient_monomials(r.divided, log_n, log_q)
    r.chunks = chunk_columns(r.mono, log_n)
    return r
