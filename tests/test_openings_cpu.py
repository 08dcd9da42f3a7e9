"""The host side of the opening phase (boojum_amd/openings.py and what it added to fri.py,
transcript.py and deep.py) without a GPU: compute_fri_schedule and BoolsBuffer against the
checker's restatements (oracle/transcript.py), the term builder of bj_deep_codeword_d against a
Python-integer model, and every BJ_EINVAL of the call, all of which the library decides before it
touches a device."""
import ctypes
import json
import os
import random

import pytest

import numpy as np

import oracle as O
import transcript as T

from boojum_amd import _lib, deep, fri, openings
from boojum_amd import transcript as PT

HERE = os.path.dirname(os.path.abspath(__file__))
P = T.P
BJ_EINVAL = -22


# ------------------------------------------------------------------ schedule
def test_fri_schedule_equals_the_checkers_over_a_grid():
    n = 0
    for security in list(range(8, 100, 3)) + [100]:
        for cap in (1, 2, 4, 8, 16, 32, 64):
            for pow_bits in (0, 1, 2, 3, 5, 7, 12, 20):
                if pow_bits >= security:
                    continue
                for rate in (1, 2, 3, 4):
                    for degree in range(4, 25):
                        want = T.compute_fri_schedule(security, cap, pow_bits, rate, degree)
                        cap_log = cap.bit_length() - 1
                        if (want[3].bit_length() - 1) + rate < cap_log:
                            # the reference asserts here (prover.rs:2364)
                            with pytest.raises(ValueError):
                                fri.compute_fri_schedule(security, cap, pow_bits, rate, degree)
                            continue
                        got = fri.compute_fri_schedule(security, cap, pow_bits, rate, degree)
                        assert got == want, (security, cap, pow_bits, rate, degree)
                        n += 1
    assert n > 100000


def test_fri_schedule_of_the_end_to_end_shape():
    # n = 2^10, LDE factor 2, cap 4, security 8, no PoW: 8 queries, [3, 3, 3] down to degree 2
    assert fri.compute_fri_schedule(8, 4, 0, 1, 10) == (0, 8, [3, 3, 3], 2)
    with pytest.raises(ValueError):
        fri.compute_fri_schedule(8, 4, 8, 1, 10)


# ------------------------------------------------------------------ BoolsBuffer
def feed_until_queries(tr, fx):
    """The verifier's transcript order (verifier.rs:924-1984, oracle/transcript.py replay_with) up
    to the final monomials, on any transcript with the trait's methods."""
    vk = fx["vk"]
    two = lambda: (tr.get_challenge(), tr.get_challenge())  # noqa: E731
    tr.witness_merkle_tree_cap(vk["setup_merkle_tree_cap"])
    for v in fx["public_inputs"]:
        tr.witness_field_elements([v])
    tr.witness_merkle_tree_cap(fx["witness_oracle_cap"])
    for _ in range(4):
        two()
    tr.witness_merkle_tree_cap(fx["stage_2_oracle_cap"])
    two()
    tr.witness_merkle_tree_cap(fx["quotient_oracle_cap"])
    two()
    for s in ("values_at_z", "values_at_z_omega", "values_at_0"):
        for v in fx[s]:
            tr.witness_field_elements(v)
    two()
    for cap in [fx["fri_base_oracle_cap"]] + fx["fri_intermediate_oracles_caps"]:
        tr.witness_merkle_tree_cap(cap)
        two()
    tr.witness_field_elements(fx["final_fri_monomials"][0])
    tr.witness_field_elements(fx["final_fri_monomials"][1])


class HostPermutationTranscript(PT.Poseidon2Transcript):
    """The product transcript with the one call it makes of the library (a permutation, which runs
    on the device) answered by the C oracle's permutation: the absorb / squeeze logic under test is
    the product's own.  tests/test_gpu_openings.py runs the unchanged class end to end."""

    def _round_function(self):
        self.state = [int(x) for x in O.poseidon2_permutation(np.array(self.state, dtype=np.uint64))]


def test_bools_buffer_gives_the_checkers_bits_on_the_reference_proof():
    fx = json.load(open(os.path.join(HERE, "golden", "proof_fri.json")))
    assert fx["proof_config"]["pow_bits"] == 0      # nothing between the monomials and the bits
    n, lde = fx["vk"]["domain_size"], fx["proof_config"]["fri_lde_factor"]
    log_n = n.bit_length() - 1
    max_needed = (n * lde).bit_length() - 1
    ours, theirs = HostPermutationTranscript(), T.Poseidon2Transcript()
    feed_until_queries(ours, fx)
    feed_until_queries(theirs, fx)
    a, b = PT.BoolsBuffer(max_needed), T.BoolsBuffer(max_needed)
    indices = []
    for _ in fx["queries"]:
        bits = a.get_bits(ours, max_needed)
        assert bits == b.get_bits(theirs, max_needed)
        indices.append((PT.u64_from_lsb_first_bits(bits[log_n:]) << log_n) + PT.u64_from_lsb_first_bits(bits[:log_n]))
    assert a.available == b.available
    # the feed above is the verifier's: these are the indices the replay checks the Merkle paths at
    assert indices == [q["index"] for q in T.replay(fx)["queries"]]
    # an uneven request leaves the remainder for the next one
    assert a.get_bits(ours, 5) + a.get_bits(ours, 70) == b.get_bits(theirs, 75)


# ------------------------------------------------------------------ term builder
def rand_ext(r):
    return (r.randrange(P), r.randrange(P))


def test_terms_are_trimmed_sorted_and_equal_the_integer_model():
    r = random.Random(5)
    widths = [12, 17, 12, 8]
    points = [
        # two groups; the Ext2 source (1, 15) ends on the last column of its group, (1, 3) starts a range
        (rand_ext(r), [(0, 4, False, rand_ext(r), rand_ext(r)), (1, 15, True, rand_ext(r), rand_ext(r)),
                       (0, 9, False, rand_ext(r), rand_ext(r)), (1, 3, True, rand_ext(r), rand_ext(r)),
                       (0, 4, False, rand_ext(r), rand_ext(r))]),
        (rand_ext(r), []),                                                    # no terms
        (rand_ext(r), [(2, 0, True, rand_ext(r), rand_ext(r))]),
        # an Ext2 source whose c1 column is the c0 column of the next one: ranges overlap inside a term
        (rand_ext(r), [(2, 10, True, rand_ext(r), rand_ext(r)), (2, 9, True, rand_ext(r), rand_ext(r))]),
        (rand_ext(r), [(3, 7, False, rand_ext(r), rand_ext(r)), (0, 11, False, rand_ext(r), rand_ext(r))]),
    ]
    terms, gammas, ks = deep.codeword_terms(widths, points)
    assert [(t[0], t[1], t[2], t[3]) for t in terms] == [
        (0, 4, 6, 0), (1, 3, 14, 0), (2, 0, 2, 2), (2, 9, 3, 3), (0, 11, 1, 4), (3, 7, 1, 4)]
    assert [t[3] for t in terms] == sorted(t[3] for t in terms)
    offs = [t[4] for t in terms]
    assert offs == [0, 6, 20, 22, 25, 26] and len(gammas) == 27 and len(ks) == len(points)
    # columns inside a range that no source names carry a zero coefficient
    assert gammas[1] == (0, 0) and gammas[0] != (0, 0)
    # the model: at random column values f, sum_t sum_c gamma f - K = sum_j ch_j (F_j - v_j)
    f = [[r.randrange(P) for _ in range(w)] for w in widths]
    for p, (_, entries) in enumerate(points):
        got = (0, 0)
        for g, first, count, pt, off in terms:
            if pt != p:
                continue
            for c in range(count):
                got = T.e_add(got, T.e_mul_base(gammas[off + c], f[g][first + c]))
        got = T.e_sub(got, ks[p])
        want = (0, 0)
        for g, col, is_ext, ch, v in entries:
            val = (f[g][col], f[g][col + 1] if is_ext else 0)
            want = T.e_add(want, T.e_mul(ch, T.e_sub(val, v)))
        assert got == want, p


def test_term_builder_rejects_what_lies_outside():
    with pytest.raises(ValueError):
        deep.codeword_terms([4], [((1, 0), [(0, 3, True, (1, 0), (0, 0))])])    # c1 past the group
    with pytest.raises(ValueError):
        deep.codeword_terms([4], [((1, 0), [(1, 0, False, (1, 0), (0, 0))])])   # no such group
    with pytest.raises(ValueError):
        deep.codeword_descriptor([], [((1, 0), [])] * 9, [], [(0, 0)] * 9, 0, 0, 4, 0, 0, 0, 0, False)


def test_points_are_batched_under_the_caps():
    pts = [((i + 2, 0), [(g, 0, False, (1, 0), (0, 0)) for g in range(3)]) for i in range(11)]
    batches = openings._batches(pts)
    assert [len(b) for b in batches] == [5, 5, 1]       # 16 terms hold five points of three groups
    pts = [((i + 2, 0), [(0, 0, False, (1, 0), (0, 0))]) for i in range(11)]
    assert [len(b) for b in openings._batches(pts)] == [8, 3]


def test_layout_of_the_end_to_end_shape():
    lay = openings.OpeningLayout(V=10, W=1, C=3, M=1, L=2, I=2, lookup_setups=4, quotient_degree=4)
    assert openings.leaf_widths(lay) == (12, 12, 8, 17)
    assert len(openings.sources_at_z(lay)) == 39
    assert len(openings.sources_at_0(lay)) == 3 and openings.sources_at_z_omega(lay) == [(openings.STAGE_2, 0, True)]
    # the one geometry the checker accepts for these leaf sizes
    fx = {"vk": {"parameters": {"num_columns_under_copy_permutation": 10, "num_witness_columns": 1,
                                "num_constant_columns": 2},
                 "lookup_parameters": {"UseSpecializedColumnsWithTableIdAsConstant": {"width": 3, "num_repetitions": 2}},
                 "domain_size": 1 << 10, "total_tables_len": 1 << 10, "quotient_degree": 4,
                 "extra_constant_polys_for_selectors": 1},
          "queries": [{k + "_query": {"leaf_elements": [0] * w} for k, w in
                       zip(("witness", "stage_2", "quotient", "setup"), openings.leaf_widths(lay))}],
          "values_at_z": [0] * 39, "values_at_z_omega": [0], "values_at_0": [0] * 3}
    gs = list(T.geometries(fx))
    assert len(gs) == 1 and openings.OpeningLayout(**gs[0]) == lay
    tuples = openings.public_input_opening_tuples([(0, 0, 5), (3, 0, 6), (1, 7, 8)], 10)
    assert tuples == [(1, [(0, 5), (3, 6)]), (pow(T.domain_generator(10), 7, P), [(1, 8)])]


# ------------------------------------------------------------------ BJ_EINVAL
FAKE = 0x1000   # a pointer the library must never follow: every case fails its check first


def sound(n_rows=8):
    """A descriptor that passes every check: one group of 4 columns, one point, one term."""
    d = deep.codeword_descriptor([(FAKE, 4, 8)], [((3, 0), [])], [(0, 1, 2, 0, 0)], [(0, 0)], FAKE, 2, 3, 0, n_rows,
                                 FAKE, FAKE, False)
    return d


def rc_of(d):
    lib = _lib.load()
    rc = lib.bj_deep_codeword_d(ctypes.byref(d), None)
    return rc, (lib.bj_last_error() or b"").decode()


def test_a_sound_descriptor_of_no_rows_is_a_no_op():
    assert rc_of(sound(0))[0] == 0


def shape_cases():
    def case(name, edit):
        return pytest.param(edit, id=name)
    return [
        case("groups over the cap", lambda d: setattr(d, "n_groups", 9)),
        case("points over the cap", lambda d: setattr(d, "n_points", 9)),
        case("terms over the cap", lambda d: setattr(d, "n_terms", 17)),
        case("missing group", lambda d: setattr(d.terms[0], "group", 1)),
        case("missing point", lambda d: setattr(d.terms[0], "point", 1)),
        case("range past the group", lambda d: setattr(d.terms[0], "n_cols", 4)),
        case("first column past the group", lambda d: setattr(d.terms[0], "first_col", 0xFFFFFFFF)),
        case("coefficients past gammas", lambda d: setattr(d.terms[0], "gamma_offset", 1)),
        case("log_domain 33", lambda d: setattr(d, "log_domain", 33)),
        case("window past the domain", lambda d: setattr(d, "row0", 9)),
    ]


@pytest.mark.parametrize("edit", shape_cases())
def test_shape_errors_are_einval_whatever_the_window(edit):
    d = sound(0)           # no rows: a check that did not fire would be a no-op, never a launch
    edit(d)
    rc, msg = rc_of(d)
    assert rc == BJ_EINVAL and msg


def test_unsorted_terms_are_einval():
    d = deep.codeword_descriptor([(FAKE, 4, 8)], [((3, 0), []), ((4, 0), [])], [(0, 0, 1, 1, 0), (0, 1, 1, 0, 1)],
                                 [(0, 0)] * 2, FAKE, 2, 3, 0, 0, FAKE, FAKE, False)
    assert rc_of(d)[0] == BJ_EINVAL
    d.terms[0].point, d.terms[1].point = 0, 1
    assert rc_of(d)[0] == 0


def test_window_and_pointer_errors_are_einval():
    assert _lib.load().bj_deep_codeword_d(None, None) == BJ_EINVAL
    d = sound()
    d.row0, d.n_rows = 7, 2                     # row0 + n_rows = 9 > 2^3
    assert rc_of(d)[0] == BJ_EINVAL
    d = sound()
    d.row0, d.n_rows = 1, (1 << 64) - 1         # the sum wraps
    assert rc_of(d)[0] == BJ_EINVAL
    for field in ("dst0", "dst1", "gammas"):
        d = sound()
        setattr(d, field, None)
        assert rc_of(d)[0] == BJ_EINVAL, field
    d = sound()
    d.groups[0].cols = None
    assert rc_of(d)[0] == BJ_EINVAL
    d = sound()
    d.groups[0].col_stride = 7                  # < n_rows
    assert rc_of(d)[0] == BJ_EINVAL
    # nothing to point at is fine: no columns, no coefficients
    d = deep.codeword_descriptor([], [((3, 0), [])], [], [(1, 2)], 0, 0, 3, 0, 0, 0, 0, False)
    assert rc_of(d)[0] == 0
