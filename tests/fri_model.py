"""The FRI commit phase (cs/implementations/fri/mod.rs:49-682) and the verifier's view of it
(verifier.rs:2396-2518) in Python integers -- TEST INFRASTRUCTURE, no GPU and no library.

* `fold_multiple`: one fold by 2 (fri/mod.rs:362-474).
* `fold_by`: the r-step fold of one reduction, written per OUTPUT with the indexing of
  bj_fri_fold_multi_d (step s folds the pairs at flat index 2^(r-1-s) j + t), not as a chain.
* `fold_monomials`: the closed form, one fold maps coefficients to m'_k = 2 (m_2k + alpha m_2k+1).
* `do_fri`: the reference's order over a transcript; trees come from a caller-supplied `cap_of`.
* `chain_check`: what the verifier does with one query's FRI leaves.

A codeword is a pair of lists (c0, c1) over the flat bit-reversed LDE domain: value L is
f(7 w_N^bitrev(L)), N the full size.
"""
P = 0xFFFFFFFF00000001
GEN = 7                                  # multiplicative generator and Ext2 non-residue
ROOT_2_32 = 0x185629dcda58878c           # RADIX_2_SUBGROUP_GENERATOR (goldilocks/mod.rs:108)


def inv(a):
    return pow(a % P, P - 2, P)


def e_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def e_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def e_mul(a, b):
    return ((a[0] * b[0] + GEN * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def e_scale(a, k):
    return (a[0] * k % P, a[1] * k % P)


def log2(n):
    assert n > 0 and n & (n - 1) == 0, n
    return n.bit_length() - 1


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def domain_generator(log_n):
    return pow(ROOT_2_32, 1 << (32 - log_n), P)


def inverse_roots(full_size):
    """precompute_twiddles_for_fft::<true>(full_size): w_N^-bitrev(i), i < N / 2."""
    bits = log2(full_size) - 1
    wi = inv(domain_generator(bits + 1))
    return [pow(wi, bitrev(i, bits), P) for i in range(full_size // 2)]


def challenge_powers(ch, r):
    out = [(ch[0] % P, ch[1] % P)]
    for _ in range(1, r):
        out.append(e_mul(out[-1], out[-1]))
    return out


def fold_pair(fx, fmx, root, coset_inverse, alpha):
    """f(x) + f(-x) + alpha (f(x) - f(-x)) root coset_inverse."""
    diff = e_scale(e_sub(fx, fmx), root * coset_inverse % P)
    return e_add(e_add(e_mul(diff, alpha), fx), fmx)


def fold_multiple(c0, c1, roots, coset_inverse, alpha):
    out = [fold_pair((c0[2 * i], c1[2 * i]), (c0[2 * i + 1], c1[2 * i + 1]), roots[i], coset_inverse, alpha)
           for i in range(len(c0) // 2)]
    return [v[0] for v in out], [v[1] for v in out]


def fold_by(c0, c1, roots, coset_inverse, challenge, r):
    """Output j from the 2^r inputs [2^r j, 2^r (j + 1)): step s folds its 2^(r-1-s) pairs with
    roots[2^(r-1-s) j + t], alpha^(2^s) and coset_inverse^(2^s)."""
    assert len(c0) % (1 << r) == 0
    alphas = challenge_powers(challenge, r)
    d0, d1 = [], []
    for j in range(len(c0) >> r):
        vals = [(c0[(j << r) + t] % P, c1[(j << r) + t] % P) for t in range(1 << r)]
        ci = coset_inverse % P
        for s in range(r):
            m = 1 << (r - 1 - s)
            vals = [fold_pair(vals[2 * t], vals[2 * t + 1], roots[m * j + t], ci, alphas[s]) for t in range(m)]
            ci = ci * ci % P
        d0.append(vals[0][0])
        d1.append(vals[0][1])
    return d0, d1


def fold_monomials(m0, m1, alpha):
    """Coefficients of the folded polynomial: m'_k = 2 (m_2k + alpha m_2k+1)."""
    out = [e_scale(e_add((m0[2 * k], m1[2 * k]), e_mul(alpha, (m0[2 * k + 1], m1[2 * k + 1]))), 2)
           for k in range(len(m0) // 2)]
    return [v[0] for v in out], [v[1] for v in out]


def fold_monomials_by(m0, m1, challenge, r):
    for alpha in challenge_powers(challenge, r):
        m0, m1 = fold_monomials(m0, m1, alpha)
    return m0, m1


def interpolate_bitreversed(values, coset):
    """bitreverse_enumeration_inplace + ifft_natural_to_natural on `coset`, O(n^2): the
    coefficients m with values[L] = sum_k m_k (coset w^bitrev(L))^k."""
    n = len(values)
    bits = log2(n)
    nat = [values[bitrev(i, bits)] % P for i in range(n)]
    wi = inv(domain_generator(bits)) if bits else 1
    n_inv, c_inv = inv(n), inv(coset)
    return [sum(nat[i] * pow(wi, i * k % n, P) for i in range(n)) % P * n_inv % P * pow(c_inv, k, P) % P
            for k in range(n)]


def do_fri(c0, c1, transcript, schedule, lde_degree, cap_size, cap_of):
    """do_fri's order (fri/mod.rs:173-357).  cap_of(rows, elements_per_leaf, cap_size) -> the cap of
    the chunked tree over rows = [c0, c1].  Returns a dict: caps, challenges, leaf_sources (every
    fold result), monomial_forms, low_degree."""
    full = len(c0)
    final_degree = (full // lde_degree) >> sum(schedule)
    assert final_degree > 0
    roots = inverse_roots(full)
    ci = inv(GEN)
    caps, challenges, sources = [], [], []
    cur = (list(c0), list(c1))
    for s in schedule:
        assert 0 < s < 4
        cap = cap_of(cur, 1 << s, cap_size)
        caps.append(cap)
        transcript.witness_merkle_tree_cap(cap)
        ch = (transcript.get_challenge(), transcript.get_challenge())
        challenges.append(ch)
        cur = fold_by(cur[0], cur[1], roots, ci, ch, s)
        ci = pow(ci, 1 << s, P)
        sources.append(cur)
    mono = [interpolate_bitreversed(h, inv(ci)) for h in cur]
    assert final_degree == len(cur[0]) // lde_degree
    low = tuple(not any(m[final_degree:]) for m in mono)
    forms = [m[:final_degree] for m in mono]
    transcript.witness_field_elements(forms[0])
    transcript.witness_field_elements(forms[1])
    return {"caps": caps, "challenges": challenges, "leaf_sources": sources, "monomial_forms": forms,
            "low_degree": low}


def leaf_of(rows, elements_per_leaf, tree_idx):
    """The leaf elements a chunked tree hashes at tree_idx: c0's chunk, then c1's."""
    e = elements_per_leaf
    return [int(v) for row in rows for v in row[tree_idx * e:(tree_idx + 1) * e]]


def chain_check(index, leaves, schedule, challenges, monomial_forms, full_size):
    """verifier.rs:2396-2518 for the flat query index: leaves[k] are oracle k's leaf elements at
    index >> (s_0 + ... + s_k).  Each leaf folds (with the roots at its flat pair indices) to the
    value the next oracle holds at the shifted index; the last fold equals the final monomials at
    the folded point.  AssertionError otherwise."""
    roots = inverse_roots(full_size)
    ci = inv(GEN)
    sub = index
    expected = None
    for k, (s, leaf, ch) in enumerate(zip(schedule, leaves, challenges)):
        deg = 1 << s
        assert len(leaf) == 2 * deg, "leaf %d has %d elements" % (k, len(leaf))
        in_leaf, tree_idx = sub % deg, sub >> s
        vals = [(int(leaf[t]) % P, int(leaf[deg + t]) % P) for t in range(deg)]
        if expected is not None:
            assert vals[in_leaf] == expected, "oracle %d does not hold the fold of oracle %d" % (k, k - 1)
        base = tree_idx * deg // 2
        for alpha in challenge_powers(ch, s):
            vals = [fold_pair(vals[2 * t], vals[2 * t + 1], roots[base + t], ci, alpha) for t in range(len(vals) // 2)]
            base //= 2
            ci = ci * ci % P
        expected, sub = vals[0], tree_idx
    total = sum(schedule)
    x = GEN * pow(domain_generator(log2(full_size)), bitrev(index, log2(full_size)), P) % P
    x = pow(x, 1 << total, P)
    acc = (0, 0)
    for a, b in zip(reversed(monomial_forms[0]), reversed(monomial_forms[1])):
        acc = e_add(e_scale(acc, x), (int(a) % P, int(b) % P))
    assert acc == expected, "the last fold is not the final monomials at the folded point"
