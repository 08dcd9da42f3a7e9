"""The host half of the DEEP step (boojum_amd/deep.py: no device call) against the verifier's
restatement over the reference's own proof (oracle/transcript.py, tests/golden/proof_fri.json)."""
import transcript as T

import deep_groups


def test_plan_reproduces_the_proofs_deep_values():
    """quotening_plan's per-column coefficients and constant, built for the four opening points
    (z, z * omega, 0 and the public-input point) from the 397 leaf columns in the layout
    [witness | stage_2 | quotient | setup], give every query's DEEP value:
    sum_groups (sum_c gamma_c leaf_c - K) / (x - at) == the verifier's quotening (verifier.rs:2526-2565)."""
    fx, rep = deep_groups.proof()
    groups, n_cols = deep_groups.opening_groups(fx, rep)
    assert n_cols == 397 and len(groups) == 4
    assert len(fx["queries"]) == 6
    n_domain = fx["vk"]["domain_size"] * fx["proof_config"]["fri_lde_factor"]
    log_domain = n_domain.bit_length() - 1
    omega = T.domain_generator(log_domain)
    for q, r in zip(fx["queries"], rep["queries"]):
        # the domain convention the kernel uses: x = 7 w_N^bitrev(idx)
        rev = int(format(r["index"], "0%db" % log_domain)[::-1], 2)
        assert r["x"] == 7 * pow(omega, rev, T.P) % T.P
        row = deep_groups.leaf_row(q)
        assert len(row) == n_cols
        assert deep_groups.combine(groups, n_cols, row, r["x"]) == r["deep"], r["index"]


def test_plan_columns_and_zero_coefficients():
    """A base source touches its column alone, an Ext2 source its two columns (the second by
    challenge * u), and columns no source names keep a zero coefficient."""
    from boojum_amd import deep
    ch = [(3, 5), (11, 13)]
    gammas, k = deep.quotening_plan(5, [(0, False, ch[0], (2, 0)), (2, True, ch[1], (17, 19))])
    assert gammas == [(3, 5), (0, 0), (11, 13), (7 * 13, 11), (0, 0)]
    assert k == T.e_add(T.e_mul(ch[0], (2, 0)), T.e_mul(ch[1], (17, 19)))


def test_challenge_powers_match_the_oracle():
    from boojum_amd import deep
    c = (0x123456789abcdef0 % T.P, 0x0fedcba987654321)
    for n in (1, 2, 3, 50):
        assert deep.materialize_ext_challenge_powers(c, n) == T.materialize_ext_challenge_powers(c, n)
