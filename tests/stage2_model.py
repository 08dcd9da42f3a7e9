"""Plain-Python-integer model of stage 2 (boojum_amd/stage2.py, csrc/stage2.hip): the non-residues
(utils.rs:636-688, copy_permutation.rs:512-522), the copy-permutation grand product with its
partial products (copy_permutation.rs:649-774) and the lookup encodings
(lookup_argument_in_ext.rs:320-700), with a generator of valid copy-permutation inputs.  Ext2
values are (c0, c1) tuples; the arithmetic is oracle/transcript.py's."""
from collections import namedtuple

import numpy as np

import transcript as T

P = T.P
ONE, ZERO = (1, 0), (0, 0)


# ------------------------------------------------------------------ non-residues
def make_non_residues(num, domain_size):
    """utils.rs:636-688: the candidates 2, 3, ... that are quadratic non-residues (Legendre symbol
    by Euler's criterion), lie outside the domain (x^n != 1) and in a coset of it that no earlier
    one is in (x^n differs from every earlier k^n, :651-686)."""
    out, powers, cur = [], [], 1
    while len(out) < num:
        cur += 1
        if pow(cur, (P - 1) // 2, P) != P - 1:
            continue
        t = pow(cur, domain_size, P)
        if t == 1 or t in powers:
            continue
        out.append(cur)
        powers.append(t)
    return out


def non_residues_for_copy_permutation(domain_size, num_columns):
    """copy_permutation.rs:512-522."""
    assert num_columns > 0
    return [1] + make_non_residues(num_columns - 1, domain_size)


def num_intermediate_partial_product_relations(num_cols, quotient_degree):
    """copy_permutation.rs:14-28."""
    if num_cols <= quotient_degree:
        return 0
    result = num_cols // quotient_degree
    if num_cols % quotient_degree:
        result += 1
    return result - 1


def domain(log_n):
    omega, x, out = T.domain_generator(log_n), 1, []
    for _ in range(1 << log_n):
        out.append(x)
        x = x * omega % P
    return out


# ------------------------------------------------------------------ inputs
def valid_inputs(n_cols, log_n, seed):
    """Witness and sigma columns (two (C, n) uint64 arrays) of a satisfied copy permutation: a
    seeded random permutation of the C * n cells, witness values constant on each of its cycles,
    and sigma_c[i] = k_c' * w^i' for the image (c', i') of cell (c, i), so that the product of the
    numerators over all cells equals that of the denominators."""
    n = 1 << log_n
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_cols * n)
    values = rng.integers(0, P, size=n_cols * n, dtype=np.uint64)
    k, x = non_residues_for_copy_permutation(n, n_cols), domain(log_n)
    w = np.zeros(n_cols * n, dtype=np.uint64)
    sigma = np.zeros(n_cols * n, dtype=np.uint64)
    seen = np.zeros(n_cols * n, dtype=bool)
    for start in range(n_cols * n):
        cell = start
        while not seen[cell]:
            seen[cell] = True
            w[cell] = values[start]
            image = int(perm[cell])
            sigma[cell] = k[image // n] * x[image % n] % P
            cell = image
    return w.reshape(n_cols, n), sigma.reshape(n_cols, n)


# ------------------------------------------------------------------ copy permutation
def batch_inverse(values):
    """Inverses of Ext2 values with one e_inv; the inverse of zero is taken as zero.  Returns
    (inverses, number of zeros)."""
    prefix, acc = [], ONE
    for v in values:
        prefix.append(acc)
        if v != ZERO:
            acc = T.e_mul(acc, v)
    inv, out, zeros = T.e_inv(acc), [None] * len(values), 0
    for i in range(len(values) - 1, -1, -1):
        if values[i] == ZERO:
            out[i] = ZERO
            zeros += 1
        else:
            out[i] = T.e_mul(inv, prefix[i])
            inv = T.e_mul(inv, values[i])
    return out, zeros


CopyPermutation = namedtuple("CopyPermutation", "z intermediates total zeros num den a")


def copy_permutation(w, sigma, beta, gamma, q, non_residues=None):
    """w, sigma: (C, n) arrays of any u64 representatives.  Returns z (n Ext2 values), the m - 1
    intermediates, the product of a over all rows, the number of zero chunk denominators (their
    r_j taken as 0), and the per-chunk numerators and denominators num[j][i], den[j][i], and a."""
    n_cols, n = len(w), len(w[0])
    log_n = n.bit_length() - 1
    k = non_residues or non_residues_for_copy_permutation(n, n_cols)
    x = domain(log_n)
    b0, b1, g0, g1 = beta[0] % P, beta[1] % P, gamma[0] % P, gamma[1] % P
    m = (n_cols + q - 1) // q
    num, den = [], []
    for j in range(m):
        nj, dj = [ONE] * n, [ONE] * n
        for c in range(j * q, min(n_cols, (j + 1) * q)):
            wc = [int(v) % P for v in w[c]]
            sc = [int(v) % P for v in sigma[c]]
            kc = k[c]
            for i in range(n):
                kx = kc * x[i] % P
                nj[i] = T.e_mul(nj[i], ((wc[i] + b0 * kx + g0) % P, (b1 * kx + g1) % P))
                dj[i] = T.e_mul(dj[i], ((wc[i] + b0 * sc[i] + g0) % P, (b1 * sc[i] + g1) % P))
        num.append(nj)
        den.append(dj)
    inv, zeros = batch_inverse([d for dj in den for d in dj])
    a, prefix = [ONE] * n, []   # prefix[j][i] = r_0[i] .. r_j[i]
    for j in range(m):
        a = [T.e_mul(a[i], T.e_mul(num[j][i], inv[j * n + i])) for i in range(n)]
        prefix.append(a)
    z, acc = [], ONE
    for i in range(n):
        z.append(acc)
        acc = T.e_mul(acc, a[i])
    inter = [[T.e_mul(z[i], prefix[j][i]) for i in range(n)] for j in range(m - 1)]
    return CopyPermutation(z, inter, acc, zeros, num, den, a)


def ext_columns(polys):
    """[Ext2 polynomial as a list of (c0, c1)] -> (2 len, n) uint64 array, c0 then c1 of each."""
    rows = []
    for p in polys:
        rows.append([v[0] for v in p])
        rows.append([v[1] for v in p])
    return np.array(rows, dtype=np.uint64)


def copy_permutation_columns(cp):
    """The out layout of bj_copy_permutation_d: z.c0, z.c1, p_0.c0, p_0.c1, ..."""
    return ext_columns([cp.z] + cp.intermediates)


# ------------------------------------------------------------------ lookup
def lookup_encoding(sources, coefficients, beta, f=None):
    """out[i] = f[i] / (beta + sum_t coefficients[t] * sources[t][i]); the inverse of zero is
    zero.  Returns (values, zeros)."""
    n = len(sources[0])
    b = (beta[0] % P, beta[1] % P)
    dens = []
    for i in range(n):
        d = b
        for src, g in zip(sources, coefficients):
            d = T.e_add(d, T.e_mul_base((g[0] % P, g[1] % P), int(src[i]) % P))
        dens.append(d)
    inv, zeros = batch_inverse(dens)
    if f is not None:
        inv = [T.e_mul_base(v, int(fv) % P) for v, fv in zip(inv, f)]
    return inv, zeros


def gamma_powers(gamma, count):
    out = [ONE]
    while len(out) < count:
        out.append(T.e_mul(out[-1], (gamma[0] % P, gamma[1] % P)))
    return out


def lookup_poly_pairs_specialized(variables, multiplicities, constants, tables, table_id_column_idxes, beta, gamma,
                                  variables_offset, kind, width, num_repetitions):
    """lookup_argument_in_ext.rs:320-700 for kind "variable" (table id as a variable column) or
    "constant" (as the setup constant column table_id_column_idxes[0]).  Returns
    (witness encodings, multiplicity encodings, zeros)."""
    per_arg = width + 1 if kind == "variable" else width
    powers = gamma_powers(gamma, width + 1)
    assert len(tables) == width + 1
    wit, mult, zeros = [], [], 0
    for s in range(num_repetitions):
        first = variables_offset + s * per_arg
        srcs = [variables[first + t] for t in range(per_arg)]
        if kind == "constant":
            srcs.append(constants[table_id_column_idxes[0]])
        v, zc = lookup_encoding(srcs, powers, beta)
        wit.append(v)
        zeros += zc
    for mcol in multiplicities:
        v, zc = lookup_encoding(list(tables), powers, beta, f=mcol)
        mult.append(v)
        zeros += zc
    return wit, mult, zeros
