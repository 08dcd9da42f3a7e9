"""The Python-integer side of the prover tests: the verifier's quotient identity at z
(cs/implementations/verifier.rs:1112-1816) over GoldilocksExt2, from the proof's openings, the
challenges, the verification key and the circuit's gates alone -- no column, no LDE.

    sum of every term at z, each times its power of alpha
        == (sum_i chunk_i(z) z^(n i)) (z^n - 1)                       verifier.rs:1799-1815

The powers of alpha are split as the verifier splits them (verifier.rs:1033-1052): the lookup terms
first (A polys, then B polys, :1442-1518), then the gates over specialized columns (:1536-1650),
then the gates over general-purpose columns (:1652-1723), then (z - 1) L_1 and the copy-permutation
relations (:1731-1797).  The gate terms come from running the evaluators of boojum_amd.gates over
Ext2 values (gates_model.ModelField with ExtOps, the verifier's use of them) times the selector
products; the copy-permutation and lookup terms are quotient_model's expressions at one point.

values_at_z is read in the verifier's order (:1112-1230, openings.sources_at_z): variables,
witnesses, constants, sigmas, z and the intermediates, multiplicities, lookup witness encodings,
multiplicity encodings, table columns, quotient chunks."""
import gates_model as M
import quotient_model as Q
import stage2_model as S
import transcript as T

P = T.P


def split_values_at_z(values, g):
    """g: a dict or namedtuple with V W C M L I lookup_setups quotient_degree."""
    g = g if isinstance(g, dict) else g._asdict()
    vals = [(int(v[0]) % P, int(v[1]) % P) for v in values]
    out, at = {}, 0
    for name, count in (("variables", g["V"]), ("witnesses", g["W"]), ("constants", g["C"]), ("sigmas", g["V"]),
                        ("z", 1), ("intermediates", g["I"]), ("multiplicities", g["M"]),
                        ("lookup_witness_encodings", g["L"]), ("multiplicity_encodings", g["M"]),
                        ("tables", g["lookup_setups"]), ("quotient", g["quotient_degree"])):
        out[name] = vals[at:at + count]
        at += count
    assert at == len(vals), "values_at_z has %d entries, the geometry %d" % (len(vals), at)
    return out


def alpha_ranges(g, specialized, general_purpose):
    """verifier.rs:990-1052 -> the four (begin, end) ranges, from the geometry and the placements."""
    g = g if isinstance(g, dict) else g._asdict()
    counts = [g["L"] + g["M"], M.total_terms(specialized), M.total_terms(general_purpose), 1 + 1 + g["I"]]
    out, at = [], 0
    for c in counts:
        out.append((at, at + c))
        at += c
    return out


def quotient_identity(vk, g, specialized, general_purpose, values_at_z, values_at_z_omega, values_at_0, challenges):
    """Both sides of the identity as Ext2 values.  challenges: a dict with beta, gamma, lookup_beta,
    lookup_gamma, alpha, z.  The sum of the lookup encodings at 0 (:1242-1262) is returned third:
    (sum of A(0)) - (sum of B(0)), which the verifier wants zero."""
    gd = g if isinstance(g, dict) else g._asdict()
    n, q = vk["domain_size"], vk["quotient_degree"]
    v = split_values_at_z(values_at_z, gd)
    z = tuple(int(x) % P for x in challenges["z"])
    ranges = alpha_ranges(gd, specialized, general_purpose)
    powers = T.materialize_ext_challenge_powers(tuple(int(x) % P for x in challenges["alpha"]), ranges[-1][1])
    lookup_a, spec_a, general_a, cp_a = (powers[b:e] for b, e in ranges)
    acc = (0, 0)
    # lookup, verifier.rs:1397-1519
    if gd["L"]:
        kind, par = next(iter(vk["lookup_parameters"].items()))
        as_constant = kind == "UseSpecializedColumnsWithTableIdAsConstant"
        per_arg = par["width"] if as_constant else par["width"] + 1
        first = vk["parameters"]["num_columns_under_copy_permutation"]
        beta, gamma = (tuple(int(x) % P for x in challenges[k]) for k in ("lookup_beta", "lookup_gamma"))
        gammas = S.gamma_powers(gamma, len(v["tables"]))
        id_column = vk["parameters"]["num_constant_columns"] + vk["extra_constant_polys_for_selectors"]
        table_id = [v["constants"][id_column]] if as_constant else []
        for s in range(gd["L"]):
            srcs = v["variables"][first + s * per_arg:first + (s + 1) * per_arg] + table_id
            acc = T.e_add(acc, Q.lookup_term_at(v["lookup_witness_encodings"][s], srcs, gammas, beta, (1, 0),
                                                lookup_a[s]))
        for i in range(gd["M"]):
            acc = T.e_add(acc, Q.lookup_term_at(v["multiplicity_encodings"][i], v["tables"], gammas, beta,
                                                v["multiplicities"][i], lookup_a[gd["L"] + i]))
    # gates, verifier.rs:1536-1723
    for placements, alphas in ((specialized, spec_a), (general_purpose, general_a)):
        s, used = M.direct_terms_at(placements, v["variables"], v["witnesses"], v["constants"], alphas, ops=M.ExtOps)
        assert used == len(alphas)
        acc = T.e_add(acc, s)
    # copy permutation, verifier.rs:1726-1797
    beta, gamma = (tuple(int(x) % P for x in challenges[k]) for k in ("beta", "gamma"))
    k = S.non_residues_for_copy_permutation(n, gd["V"])
    z_omega = tuple(int(x) % P for x in values_at_z_omega[0])
    acc = T.e_add(acc, Q.copy_permutation_terms_at(z, v["variables"], v["sigmas"], v["z"][0], z_omega,
                                                   v["intermediates"], beta, gamma, cp_a, q, k, n))
    # the chunks, verifier.rs:1799-1808
    z_n = Q.e_pow(z, n)
    rhs, power = (0, 0), (1, 0)
    for chunk in v["quotient"]:
        rhs = T.e_add(rhs, T.e_mul(chunk, power))
        power = T.e_mul(power, z_n)
    rhs = T.e_mul(rhs, T.e_sub(z_n, (1, 0)))
    at_0 = [tuple(int(x) % P for x in e) for e in values_at_0]
    sums = (0, 0)
    for e in at_0[:gd["L"]]:
        sums = T.e_add(sums, e)
    for e in at_0[gd["L"]:]:
        sums = T.e_sub(sums, e)
    return acc, rhs, sums
