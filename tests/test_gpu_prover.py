"""The one-call prover on the GPU (boojum_amd/prover.py): prepare_setup, prove_commitments, prove.

Two satisfiable circuits (tests/prover_cases.py: A without a lookup, B with a width-3 lookup over
specialized columns, both with a gate over specialized columns and three public inputs) at
n = 2^10, FRI LDE factor 2, quotient degree 4, cap 4, security 8: two cosets committed out of four
computed, three (A) and five (B) copy-permutation chunks, the FRI schedule [3, 3, 3].

1. the checker's replay of the verifier (oracle/transcript.py) accepts the proof and draws what the
   prover drew;
2. the verifier's quotient identity at z, in Python integers (tests/prover_model.py);
3. the driver's words are the parts' words;
4. wrong witnesses give no proof, and the error names the stage;
5. a setup serves many proofs and is left as it was;
6. the library gate segments give the same proof."""
import numpy as np
import pytest

import gates_check_model as C
import transcript as T

import prover_cases as cases
import prover_model

pytestmark = pytest.mark.gpu

P = T.P


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import commit, field, gates, openings, prover, quotient, stage2, transcript, witness
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, commit=commit, gates=gates, openings=openings, prover=prover,
                               quotient=quotient, stage2=stage2, transcript=transcript, witness=witness,
                               BoojumError=boojum_amd.BoojumError))


class Proved:
    def __init__(self, bj, kind):
        self.case = cases.Case(kind)
        self.setup = self.case.prepare(bj.prover)
        self.vec, self.variables, self.witnesses = self.case.witness(1)
        self.proof = bj.prover.prove(self.setup, self.vec)
        self.fx = cases.fixture_of(self.setup, self.proof)


@pytest.fixture(scope="module")
def proved_a(bj):
    return Proved(bj, "A")


@pytest.fixture(scope="module")
def proved_b(bj):
    return Proved(bj, "B")


@pytest.fixture(params=["A", "B"])
def proved(request, proved_a, proved_b):
    return proved_a if request.param == "A" else proved_b


def replay(case, fx):
    """oracle.transcript.replay for B.  Its `geometries` reads a lookup key only (it asserts the
    kind), so for A, whose key says NoLookup, the same checks run under the setup's layout."""
    if case.lookup is None:
        return T.replay_with(fx, case.layout._asdict())
    return T.replay(fx)


# ------------------------------------------------------------------ 1
def test_the_checkers_replay_accepts_the_proof(bj, proved):
    """z is drawn after the setup cap, the public inputs, the three caps and every draw in between
    were absorbed, so equal z pins the whole feed order of the front half."""
    proof, fx, case = proved.proof, proved.fx, proved.case
    assert proof.openings.schedule == [3, 3, 3] and proof.openings.num_queries == 8
    assert proof.openings.low_degree == (True, True)
    assert fx["public_inputs"] == [int(proved.variables[c, r]) for c, r in cases.PUBLIC_INPUTS]
    res = replay(case, fx)
    assert res["geometry"] == case.layout._asdict()
    ch = proof.challenges
    assert tuple(res["beta"]) == ch["beta"] and tuple(res["gamma"]) == ch["gamma"]
    assert tuple(res["alpha"]) == ch["alpha"]
    if case.lookup is not None:
        assert tuple(res["lookup_beta"]) == ch["lookup_beta"] and tuple(res["lookup_gamma"]) == ch["lookup_gamma"]
    else:
        assert ch["lookup_beta"] is None and ch["lookup_gamma"] is None
    assert tuple(res["z"]) == tuple(ch["z"]) and tuple(res["deep_challenge"]) == tuple(ch["deep_challenge"])
    assert [tuple(p[0]) for p in res["fri_challenges"]] == [tuple(c) for c in ch["fri_challenges"]]
    assert [q["index"] for q in res["queries"]] == ch["query_indices"]
    assert len(set(ch["query_indices"])) > 1
    bad = dict(fx, public_inputs=[fx["public_inputs"][0] ^ 1] + fx["public_inputs"][1:])
    with pytest.raises(AssertionError):
        replay(case, bad)


# ------------------------------------------------------------------ 2
def test_the_quotient_identity_holds_at_z(proved):
    """verifier.rs:1112-1816 in Python integers from the openings, the challenges and the key.  The
    powers of alpha are split as at verifier.rs:1033-1052 -- lookup, gates over specialized
    columns, gates over general-purpose columns, copy permutation -- and consumed as at :1442-1518
    (A polys, then B polys), :1536-1650, :1652-1723 and :1731-1797 ((z - 1) L_1, then the chunks)."""
    proof, case, fx = proved.proof, proved.case, proved.fx
    lhs, rhs, sums = prover_model.quotient_identity(
        proved.setup.vk, case.layout, case.placements_specialized, case.placements_general, fx["values_at_z"],
        fx["values_at_z_omega"], fx["values_at_0"], proof.challenges)
    assert lhs == rhs and lhs != (0, 0)
    assert sums == (0, 0)
    # and the model is no tautology: one opening off by one breaks it
    moved = [list(v) for v in fx["values_at_z"]]
    moved[3][0] = (moved[3][0] + 1) % P
    lhs, rhs, _ = prover_model.quotient_identity(
        proved.setup.vk, case.layout, case.placements_specialized, case.placements_general, moved,
        fx["values_at_z_omega"], fx["values_at_0"], proof.challenges)
    assert lhs != rhs


# ------------------------------------------------------------------ 3
def test_the_driver_gives_the_words_of_the_parts(bj, proved):
    """The stages called by hand under the challenges prove_commitments drew, on LDEs of their own:
    the same three caps and the same quotient monomials."""
    case, setup, g = proved.case, proved.setup, proved.case.layout
    front = bj.prover.prove_commitments(setup, proved.vec, bj.transcript.Poseidon2Transcript())
    assert front.caps == {k: proved.fx["%s_oracle_cap" % k] for k in ("witness", "stage_2", "quotient")}
    ch, q, to = front.challenges, g.quotient_degree, bj.field.to_device
    columns = [proved.variables, proved.witnesses]
    if g.M:
        mult = np.zeros((1, case.n), dtype=np.uint64)
        mult[0, :len(proved.vec.multiplicities)] = proved.vec.multiplicities
        columns.append(mult)
    trace = to(np.concatenate(columns))
    assert np.array_equal(bj.field.to_host(front.witness_set.variables), proved.variables)
    o_w = bj.commit.commit_trace_columns(trace, 4, cases.LDE_FACTOR, cases.CAP)
    sigmas, constants, tables = setup.trace[:g.V], setup.trace[g.V:g.V + g.C], setup.trace[g.V + g.C:]
    o_setup = bj.commit.commit_trace_columns(setup.trace.clone(), 4, cases.LDE_FACTOR, cases.CAP)
    first, idxes = cases.GENERAL["num_columns_under_copy_permutation"], [cases.GENERAL_CONSTANTS]
    lookup_s2 = lookup_q = None
    if g.L:
        lookup_s2 = dict(variables_columns=trace[:g.V], multiplicities_columns=trace[g.V + g.W:],
                         constant_polys=constants, lookup_tables_columns=tables, table_id_column_idxes=idxes, beta=ch["lookup_beta"],
                         gamma=ch["lookup_gamma"], variables_offset=first, lookup_parameters=case.lookup)
        lookup_q = dict(multiplicities_lde=o_w.lde[g.V + g.W:], constants_lde=o_setup.lde[g.V:g.V + g.C],
                        tables_lde=o_setup.lde[g.V + g.C:], beta=ch["lookup_beta"], gamma=ch["lookup_gamma"],
                        table_id_column_idxes=idxes, column_elements_per_subargument=3, num_subarguments=2,
                        variables_offset=first)
    st = bj.stage2.second_stage_trace(trace[:g.V], sigmas, ch["beta"], ch["gamma"], q, lookup=lookup_s2, check=True)
    o_s2 = bj.commit.commit_trace_columns(st.trace, 4, cases.LDE_FACTOR, cases.CAP)
    ranges = prover_model.alpha_ranges(g, case.placements_specialized, case.placements_general)
    powers = T.materialize_ext_challenge_powers(ch["alpha"], ranges[-1][1])
    lk, spec, general, cp = (powers[b:e] for b, e in ranges)
    chunks, top = bj.quotient.quotient_from_arguments(
        o_w.lde[:g.V], o_setup.lde[:g.V], o_s2.lde, ch["beta"], ch["gamma"], cp + lk, q, lookup=lookup_q,
        gates=dict(gate_set=bj.gates.GateSet(case.set_order), alphas=spec + general,
                   witnesses_lde=o_w.lde[g.V:g.V + g.W], constants_lde=o_setup.lde[g.V:g.V + g.C]))
    assert top == (True, True)
    o_q = bj.commit.quotient_commit(chunks, cases.LDE_FACTOR, cases.CAP)
    cap = lambda o: [[int(v) for v in d] for d in o.get_cap()]   # noqa: E731
    assert cap(o_setup) == setup.vk["setup_merkle_tree_cap"]
    assert cap(o_w) == front.caps["witness"] and cap(o_s2) == front.caps["stage_2"]
    assert cap(o_q) == front.caps["quotient"]
    got, want = bj.field.to_host(front.monomials), bj.field.to_host(chunks)
    assert np.array_equal(got, want) and want.any()


def test_the_chain_route_gives_the_same_proof(bj, proved):
    other = bj.prover.prove(proved.setup, proved.vec, route="chain")
    assert other.to_json() == proved.proof.to_json() and other.challenges == proved.proof.challenges


# ------------------------------------------------------------------ 4
def test_an_altered_value_gives_no_proof_and_fails_at_the_quotient(bj, proved_a):
    """The variable of cell (3, 0), d of the first FMA of row 0, one up.  It has one occurrence, so
    the copy permutation still holds, the grand product is one, and it is the quotient stage that
    fails.  With diagnose the message is the satisfiability check's, with the model's row and gate."""
    case, setup = proved_a.case, proved_a.setup
    vec, variables, witnesses = case.witness(1)
    at = int(case.var_idx[3, 0])
    assert (case.var_idx == at).sum() == 1
    vec.all_values[at] = (int(vec.all_values[at]) + 1) % P
    result = None
    with pytest.raises(bj.BoojumError, match="prove, quotient: unsatisfied"):
        result = bj.prover.prove(setup, vec)
    assert result is None
    variables[3, 0] = vec.all_values[at]
    count, (row, k, value) = C.check(case.set_order, variables, witnesses, case.constants)
    gate, rep, term = C.locate_brute(case.set_order, k)
    assert (count, row, gate, rep) == (1, 0, 1, 0)
    want = bj.gates.SatisfiabilityReport(count, row, gate, case.set_order[gate].program.evaluator.name, rep, term, k,
                                         value).message()
    assert "row 0 " in want and "fma_gate_in_base_without_constant" in want
    with pytest.raises(bj.BoojumError) as e:
        result = bj.prover.prove(setup, vec, diagnose=True)
    assert result is None and "prove, gates: " in str(e.value) and want in str(e.value)


def test_a_broken_copy_constraint_fails_at_the_grand_product(bj, proved_a):
    """The columns materialised through a hint that is consistent in itself but names another
    variable in a cell the setup's sigmas tie to (0, 0).  No gate reads that cell, so the gates
    hold (diagnose finds nothing) and the grand product over the domain is not one."""
    case, setup = proved_a.case, proved_a.setup
    vec, _, _ = case.witness(1)
    wrong = bj.prover.ProverSetup(**dict(setup.__dict__, variables_hint=bj.witness.CopyHint(case.broken_copy_hint())))
    for diagnose in (False, True):
        result = None
        with pytest.raises(bj.BoojumError, match="prove, stage 2: the grand product over the domain is"):
            result = bj.prover.prove(wrong, vec, diagnose=diagnose)
        assert result is None
    assert bj.prover.prove(setup, vec).to_json() == proved_a.proof.to_json()    # the setup itself is unharmed


# ------------------------------------------------------------------ 5
def test_one_setup_serves_many_proofs(bj, proved):
    case, setup = proved.case, proved.setup
    cap, lde, trace = setup.oracle.tree.nodes, setup.oracle.lde, setup.trace
    before = [bj.field.to_host(t).copy() for t in (cap, lde, trace)]
    vec2, variables2, _ = case.witness(2)
    assert not np.array_equal(variables2, proved.variables)
    second = bj.prover.prove(setup, vec2)
    fx2 = cases.fixture_of(setup, second)
    replay(case, fx2)
    assert fx2["witness_oracle_cap"] != proved.fx["witness_oracle_cap"]
    assert second.challenges["z"] != proved.proof.challenges["z"]
    again = bj.prover.prove(setup, case.witness(1)[0])
    assert again.to_json() == proved.proof.to_json()
    assert setup.oracle.tree.nodes is cap and setup.oracle.lde is lde and setup.trace is trace
    for t, was in zip((cap, lde, trace), before):
        assert np.array_equal(bj.field.to_host(t), was)
    replay(case, proved.fx)


# ------------------------------------------------------------------ 6
def test_library_segments_give_the_same_proof(bj, proved_a):
    case = proved_a.case
    setup = case.prepare(bj.prover, native_library=True)
    kinds = [setup.gate_set.image[setup.gate_set.image[2 + s] + 7] for s in range(setup.gate_set.num_segments)]
    assert bj.gates.KIND_LIBRARY in kinds
    assert setup.vk == proved_a.setup.vk
    proof = bj.prover.prove(setup, proved_a.vec)
    assert proof.to_json() == proved_a.proof.to_json() and proof.challenges == proved_a.proof.challenges
