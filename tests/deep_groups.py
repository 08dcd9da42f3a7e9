"""The opening groups of the reference's own proof (tests/golden/proof_fri.json) as inputs of
boojum_amd.deep.quotening_plan -- shared by test_deep_cpu.py and test_gpu_deep.py (a helper, not
a test module).

The 397 leaf columns are laid out [witness | stage_2 | quotient | setup]; the sources of every
opening point come in the order of the verifier's DEEP combination (oracle/transcript.py:324-344),
and the challenge powers run on from one group to the next."""
import json
import os

import transcript as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proof_fri.json")

_CACHE = {}


def proof():
    """(fixture, replay) of proof_fri.json, computed once per process."""
    if not _CACHE:
        fx = json.load(open(FIXTURE))
        _CACHE["v"] = (fx, T.replay(fx))
    return _CACHE["v"]


def leaf_row(q):
    """The 397 leaf values of one query in the column layout [witness | stage_2 | quotient | setup]."""
    return [int(v) % T.P for name in ("witness", "stage_2", "quotient", "setup")
            for v in q[name + "_query"]["leaf_elements"]]


def opening_groups(fx, rep):
    """[(at, entries)] for z, z * omega, 0 and every public-input point; entries are
    (col, is_ext, challenge, value_at) as boojum_amd.deep.quotening_plan takes them.  Also returns
    the number of leaf columns."""
    from boojum_amd import deep
    g = rep["geometry"]
    V, W, C, M, L, I = (g[k] for k in ("V", "W", "C", "M", "L", "I"))
    q0 = fx["queries"][0]
    size = {k: len(q0[k + "_query"]["leaf_elements"]) for k in ("witness", "stage_2", "quotient", "setup")}
    ow = 0
    o2 = ow + size["witness"]
    oq = o2 + size["stage_2"]
    os_ = oq + size["quotient"]
    n_cols = os_ + size["setup"]
    i_off = 2
    lw_off = i_off + 2 * I
    lm_off = lw_off + 2 * L

    def base(first, count):
        return [(first + i, False) for i in range(count)]

    def ext(first, count):
        assert count % 2 == 0
        return [(first + i, True) for i in range(0, count, 2)]

    at_z = (base(ow, V) + base(ow + V, W) + base(os_ + V, C) + base(os_, V) + ext(o2, i_off) +
            ext(o2 + i_off, lw_off - i_off) + base(ow + V + W, M) + ext(o2 + lw_off, lm_off - lw_off) +
            ext(o2 + lm_off, size["stage_2"] - lm_off) + base(os_ + V + C, g["lookup_setups"]) +
            ext(oq, size["quotient"]))
    at_z_omega = ext(o2, i_off)
    at_0 = ext(o2 + lw_off, lm_off - lw_off) + ext(o2 + lm_off, size["stage_2"] - lm_off)
    n = fx["vk"]["domain_size"]
    omega = T.domain_generator(n.bit_length() - 1)
    pi = []
    for (col, row), val in zip(fx["vk"]["public_inputs_locations"], fx["public_inputs"]):
        at = pow(omega, row, T.P)
        for t in pi:
            if t[0] == at:
                t[1].append((col, val))
                break
        else:
            pi.append((at, [(col, val)]))
    ext_v = lambda vals: [(int(v[0]) % T.P, int(v[1]) % T.P) for v in vals]  # noqa: E731
    raw = [(rep["z"], at_z, ext_v(fx["values_at_z"])),
           (T.e_mul_base(rep["z"], omega), at_z_omega, ext_v(fx["values_at_z_omega"])),
           ((0, 0), at_0, ext_v(fx["values_at_0"]))]
    for at, subset in pi:
        raw.append(((at, 0), [(ow + col, False) for col, _ in subset], [(int(v) % T.P, 0) for _, v in subset]))
    total = sum(len(srcs) for _, srcs, _ in raw)
    ch = deep.materialize_ext_challenge_powers(rep["deep_challenge"], total)
    groups, off = [], 0
    for at, srcs, vals in raw:
        assert len(srcs) == len(vals)
        groups.append((at, [(col, is_ext, ch[off + j], vals[j]) for j, (col, is_ext) in enumerate(srcs)]))
        off += len(srcs)
    return groups, n_cols


def combine(groups, n_cols, row, x):
    """sum over the groups of (sum_c gamma_c row[c] - K) / (x - at), in Python integers."""
    from boojum_amd import deep
    acc = (0, 0)
    for at, entries in groups:
        gammas, k = deep.quotening_plan(n_cols, entries)
        s = (0, 0)
        for g, v in zip(gammas, row):
            s = T.e_add(s, T.e_mul_base(g, v))
        acc = T.e_add(acc, T.e_mul(T.e_sub(s, k), T.e_inv(T.e_sub((x, 0), at))))
    return acc
