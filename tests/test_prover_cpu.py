"""The host side of the one-call prover (boojum_amd/prover.py) without a GPU: the split of the
powers of alpha, the setup's leaf order, the verification key through the checker's size
calculators, the order in which the front half feeds and draws from the transcript (with every
device call patched out), and the argument errors, which are raised before anything is launched."""
import numpy as np
import pytest
import torch

import gates_check_model as C
import transcript as T

import prover_cases as cases
import prover_model

from boojum_amd import openings, prover as PR

P = T.P


@pytest.fixture(scope="module", params=["A", "B"])
def case(request):
    return cases.Case(request.param)


# ------------------------------------------------------------------ the circuits themselves
def test_the_cases_are_satisfied_and_their_public_inputs_are_read_from_used_cells():
    """At 2^5 rows, where the integer model is quick: every gate of the set holds on every row for
    two witnesses of one circuit, and the multiplicities count the lookups."""
    for kind in "AB":
        case = cases.Case(kind, log_n=5)
        for seed in (1, 2):
            vec, var, wit = case.witness(seed)
            assert C.check(case.set_order, var, wit, case.constants) == (0, None)
            assert all(case.var_idx[c, r] >= 0 for c, r in cases.PUBLIC_INPUTS)
            if kind == "B":
                assert int(np.sum(vec.multiplicities)) == 2 * case.n
        assert not np.array_equal(case.witness(1)[1], case.witness(2)[1])


# ------------------------------------------------------------------ the powers of alpha
def test_alpha_split_counts_and_order(case):
    """prover.rs:608-625.  Terms: the specialized allocator 1 per repetition; FMA 1 x 2, ZeroCheck
    2 x 1, ConstantsAllocator 1 x 2, ConditionalSwap 2 x 1 = 8 over general-purpose columns; the
    copy permutation 1 + 1 + I with I = ceil(V / 4) - 1; the lookup L + M."""
    g = case.layout
    if case.kind == "A":
        assert (g.V, g.I) == (9, 2)
        want = PR.AlphaSplit(lookup=(0, 0), specialized=(0, 1), general_purpose=(1, 9), copy_permutation=(9, 13))
    else:
        assert (g.V, g.I, g.L, g.M) == (17, 4, 2, 1)
        want = PR.AlphaSplit(lookup=(0, 3), specialized=(3, 6), general_purpose=(6, 14), copy_permutation=(14, 20))
    spec = sum(pl.num_terms() for pl in case.placements_specialized)
    general = sum(pl.num_terms() for pl in case.placements_general)
    got = PR.alpha_split(g, spec, general)
    assert got == want
    assert list(got) == prover_model.alpha_ranges(g, case.placements_specialized, case.placements_general)


# ------------------------------------------------------------------ the setup's leaf order
def test_setup_leaf_order_is_the_one_sources_at_z_reads(case):
    g = case.layout
    order = PR.setup_leaf_order(g)
    assert len(order) == openings.leaf_widths(g)[openings.SETUP]
    read = [order[col] for o, col, is_ext in openings.sources_at_z(g) if o == openings.SETUP]
    # verifier.rs:1172-1230: the constants, then the sigmas, then (further on) the table columns
    assert read == [("constant", i) for i in range(g.C)] + [("sigma", i) for i in range(g.V)] + \
        [("table", i) for i in range(g.lookup_setups)]
    assert not any(is_ext for o, _, is_ext in openings.sources_at_z(g) if o == openings.SETUP)


# ------------------------------------------------------------------ the verification key
def stub_fixture(case, vk):
    w = openings.leaf_widths(case.layout)
    g = case.layout
    names = ("witness", "stage_2", "quotient", "setup")
    query = {"%s_query" % k: {"leaf_elements": [0] * w[o]}
             for k, o in zip(names, (openings.WITNESS, openings.STAGE_2, openings.QUOTIENT, openings.SETUP))}
    return {"vk": vk, "queries": [query], "values_at_z": [[0, 0]] * len(openings.sources_at_z(g)),
            "values_at_z_omega": [[0, 0]], "values_at_0": [[0, 0]] * (g.L + g.M)}


def test_vk_goes_through_the_checkers_geometries(case):
    """oracle/transcript.py `geometries` reads a key of the specialized-columns lookup variant only
    (it asserts the kind), so circuit A, whose key says NoLookup as the reference's serde does, has
    no candidates there and is replayed under its layout (tests/test_gpu_prover.py)."""
    from boojum_amd import gates as G
    vk = PR.make_vk(case.layout, G.CSGeometry(**cases.GENERAL), case.lookup, case.n, case.n if case.lookup else 0,
                    cases.EXTRA_SELECTORS, [[0] * 4] * cases.CAP, cases.PUBLIC_INPUTS, case.config(PR))
    assert set(vk) >= {"parameters", "lookup_parameters", "domain_size", "total_tables_len", "quotient_degree",
                       "extra_constant_polys_for_selectors", "setup_merkle_tree_cap", "public_inputs_locations"}
    if case.kind == "A":
        assert vk["lookup_parameters"] == "NoLookup" and vk["total_tables_len"] == 0
        return
    assert list(T.geometries(stub_fixture(case, vk))) == [case.layout._asdict()]


# ------------------------------------------------------------------ the feed order
class Recorder:
    """A transcript that records its calls and answers challenges with a counter."""

    def __init__(self, *a):
        self.calls, self.k = [], 0

    def witness_field_elements(self, els):
        self.calls.append(("elements", [int(e) for e in els]))

    def witness_merkle_tree_cap(self, cap):
        self.calls.append(("cap", [[int(v) for v in d] for d in cap]))

    def get_challenge(self):
        self.calls.append(("challenge",))
        self.k += 1
        return self.k

    def get_challenges(self, n):
        return [self.get_challenge() for _ in range(n)]


class Stub:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def stub_oracle(tag, columns, cosets, n):
    cap = np.arange(cases.CAP * 4, dtype=np.uint64).reshape(cases.CAP, 4) + np.uint64(1000 * tag)
    return Stub(lde=torch.zeros((columns, cosets, n), dtype=torch.int64), get_cap=lambda: cap, cap=cap)


def patch_out_the_device(monkeypatch, case, n, values):
    """prove_commitments' device calls replaced by stubs that hand back tensors of the right shapes
    on the CPU and distinct caps; returns the ProverSetup."""
    g = case.layout
    w = openings.leaf_widths(g)
    oracles = {k: stub_oracle(i + 1, w[o], 4 if k != "quotient" else cases.LDE_FACTOR, n)
               for i, (k, o) in enumerate((("witness", openings.WITNESS), ("stage_2", openings.STAGE_2),
                                           ("quotient", openings.QUOTIENT), ("setup", openings.SETUP)))}

    def commit_witness_vec(vec, *a, **kw):
        total = torch.zeros((w[openings.WITNESS], n), dtype=torch.int64)
        wset = Stub(public_inputs_values=values,
                    public_inputs_with_locations=[(c, r, v) for (c, r), v in zip(cases.PUBLIC_INPUTS, values)],
                    variables=total[:g.V], witness=total[g.V:g.V + g.W], multiplicities=total[g.V + g.W:])
        return oracles["witness"], wset

    def second_stage_trace(*a, **kw):
        assert kw["check"] is False and (kw["lookup"] is None) == (case.lookup is None)
        PR.stage2.compute_partial_products_in_extension.status = "status"
        return Stub(trace=torch.zeros((w[openings.STAGE_2], n), dtype=torch.int64))

    def quotient_from_arguments(v, s, s2, beta, gamma, challenges, q, lookup=None, gates=None):
        assert len(challenges) == 2 + g.I + g.L + g.M and len(gates["alphas"]) == 8 + case.spec_reps
        return torch.zeros((2 * q, n), dtype=torch.int64), (True, True)

    monkeypatch.setattr(PR.witness, "commit_witness_vec", commit_witness_vec)
    monkeypatch.setattr(PR.stage2, "second_stage_trace", second_stage_trace)
    monkeypatch.setattr(PR.commit, "commit_trace_columns", lambda *a, **kw: oracles["stage_2"])
    monkeypatch.setattr(PR.quotient, "quotient_from_arguments", quotient_from_arguments)
    monkeypatch.setattr(PR.commit, "quotient_commit", lambda *a, **kw: oracles["quotient"])
    monkeypatch.setattr(PR, "read_status", lambda s: [1, 0, 0, 0])
    from boojum_amd import gates as G
    vk = PR.make_vk(g, G.CSGeometry(**cases.GENERAL), case.lookup, n, n if case.lookup else 0, cases.EXTRA_SELECTORS,
                    [[int(v) for v in d] for d in oracles["setup"].cap], cases.PUBLIC_INPUTS, case.config(PR))
    setup = PR.ProverSetup(layout=g, config=PR._check_config(case.config(PR)), parameters=G.CSGeometry(**cases.GENERAL),
                           lookup_parameters=case.lookup, n=n, used_lde_degree=4, oracle=oracles["setup"],
                           trace=torch.zeros((w[openings.SETUP], n), dtype=torch.int64), variables_hint=None,
                           witness_hint=None, gate_set=None, num_specialized_terms=case.spec_reps,
                           num_general_purpose_terms=8, public_inputs_locations=cases.PUBLIC_INPUTS,
                           extra_constant_polys_for_selectors=cases.EXTRA_SELECTORS, vk=vk,
                           split=PR.alpha_split(g, case.spec_reps, 8))
    return setup, oracles


def test_feed_order_is_the_verifiers_up_to_the_quotient_cap(case, monkeypatch):
    """prove_commitments over a recording transcript against the calls oracle/transcript.py's
    replay_with makes of its transcript up to the quotient cap (verifier.rs:924-1059).  The checker
    always draws the lookup pair; the prover, as the reference's (prover.rs:395-405), only when the
    circuit has lookups.  Those four draws come out of the eight challenges the witness cap's
    absorption left available and run no round function, so they change nothing after them."""
    n, values = 16, [11, 22, 33]
    setup, oracles = patch_out_the_device(monkeypatch, case, n, values)
    ours = Recorder()
    vec = Stub(public_inputs_locations=cases.PUBLIC_INPUTS, multiplicities=[1] if case.lookup else [])
    front = PR.prove_commitments(setup, vec, ours)
    assert [o is oracles[k] for o, k in zip(front.oracles, ("witness", "stage_2", "quotient", "setup"))] == [True] * 4
    assert front.public_inputs == [(0, 0, 11), (3, 0, 22), (1, 7, 33)]
    assert front.challenges == dict(beta=(1, 2), gamma=(3, 4), lookup_beta=(5, 6) if case.lookup else None,
                                    lookup_gamma=(7, 8) if case.lookup else None,
                                    alpha=(9, 10) if case.lookup else (5, 6))
    theirs = []

    class Recording(Recorder):
        def __init__(self):
            super().__init__()
            theirs.append(self)

    monkeypatch.setattr(T, "Poseidon2Transcript", Recording)
    fx = dict(vk=setup.vk, public_inputs=values, proof_config=dict(fri_lde_factor=2, merkle_tree_cap_size=cases.CAP,
                                                                  security_level=8, pow_bits=0),
              values_at_z=[], values_at_z_omega=[], values_at_0=[],
              **{"%s_oracle_cap" % k: front.caps[k] for k in ("witness", "stage_2", "quotient")})
    with pytest.raises(Exception):   # the stub has no FRI part; the calls before it are what is compared
        T.replay_with(fx, case.layout._asdict())
    want = theirs[0].calls
    end = [i for i, c in enumerate(want) if c[0] == "cap"][3] + 1     # setup, witness, stage 2, quotient
    want = want[:end]
    if case.lookup is None:
        caps = [i for i, c in enumerate(want) if c[0] == "cap"]
        assert want[caps[1] + 1:caps[2]] == [("challenge",)] * 8
        del want[caps[1] + 5:caps[2]]
    assert ours.calls == want
    assert [c[0] for c in ours.calls[:5]] == ["cap", "elements", "elements", "elements", "cap"]


# ------------------------------------------------------------------ argument errors
def test_argument_errors_are_raised_before_anything_is_launched(monkeypatch):
    case = cases.Case("B", log_n=4)

    def launched(*a, **kw):
        raise AssertionError("a device call was made")

    from boojum_amd import gates as G
    monkeypatch.setattr(PR.witness, "create_permutation_polys", launched)
    monkeypatch.setattr(PR.commit, "commit_trace_columns", launched)
    monkeypatch.setattr(G.GateSet, "__init__", launched)
    monkeypatch.setattr(PR.witness.CopyHint, "upload", launched)
    bad = [
        dict(public_inputs_locations=[(0, 0), (case.layout.V, 3)]),          # column out of range
        dict(public_inputs_locations=[(0, case.n)]),                         # row out of range
        dict(lookup_tables=None),                                            # lookup parameters without tables
        dict(config=PR.ProofConfig(3, cases.CAP, cases.SECURITY)),           # fri_lde_factor not a power of two
        dict(config=PR.ProofConfig(2, cases.CAP, cases.SECURITY, hasher="blake2s")),
        dict(layout=case.layout._replace(I=case.layout.I + 1)),
        dict(constants=case.constants[:-1]),
    ]
    for over in bad:
        with pytest.raises(ValueError):
            case.prepare(PR, **over)
    with pytest.raises(AssertionError, match="a device call was made"):   # and good arguments do get that far
        case.prepare(PR)
    with pytest.raises(ValueError):
        PR.prove(None, None, route="other")
