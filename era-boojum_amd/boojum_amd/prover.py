"""The prover as one call: `prepare_setup` once per circuit, then `prove(setup, witness_vec)`.

`prove_commitments` is the front half of prove_from_precomputations (prover.rs:150-1495), from the
setup cap to the quotient cap, driven by the transcript; `prove` joins it to
`openings.prove_openings` (prover.rs:1497-2266) over the same transcript object.  This module is a
driver: every computation is one of the device calls of witness.py, commit.py, stage2.py,
quotient.py, gates.py and openings.py, called as they stand.  What the host does here is what the
reference's own driver does on single field elements: the transcript, the powers of alpha and
their split, and the bookkeeping of which rows of which tensor a call reads.

The order of the front half (prover.rs line numbers):

1. the setup cap into the transcript (:211);
2. the witness columns from the WitnessVec (witness.commit_witness_vec, LDE at
   used_lde_degree = max(fri_lde_factor, quotient_degree), tree over the first fri_lde_factor
   cosets, :313-347); the public inputs, read from the variable columns, one by one (:264-266),
   then the witness cap (:353);
3. beta and gamma of the copy permutation (:360-363), and beta and gamma of the lookup argument
   when the circuit has lookups (:402-405);
4. stage2.second_stage_trace, commit.commit_trace_columns, the stage-2 cap (:360-554);
5. alpha (:560) and its powers [1, alpha, alpha^2, ..] (:617), split in the reference's order
   (:608-625, the verifier's at verifier.rs:1033-1052): the lookup terms first, then the gates
   over specialized columns, then the gates over general-purpose columns, then the copy
   permutation ((z - 1) L_1 first, then one per chunk);
6. quotient.quotient_from_arguments with the gate set, over the LDEs the commits kept
   (:626-1467), commit.quotient_commit, the quotient cap (:1495).

Where the reference panics the call raises BoojumError naming the stage and returns nothing:
"stage 2" for a zero denominator (utils.rs:425-427) or a grand product other than one
(copy_permutation.rs:485), "quotient" for non-zero top coefficients ("unsatisfied",
prover.rs:1424-1439), "gates" for what `diagnose=True` finds with gates.check_if_satisfied before
stage 2 starts.

Host synchronisations of a front half: the public inputs (one copy), the witness cap, the stage-2
cap with the stage-2 status record right behind it, the quotient's top coefficients, the quotient
cap.  Stage 2 runs with check=False; its grand-product record is read once, after the stage-2 cap
has drained the stream anyway.  (The lookup encodings' zero-denominator counts are not kept by
second_stage_trace under check=False; such a row leaves A(x) d(x) - 1 = -1 in the quotient's
numerator and surfaces as "quotient".)

Not here: the Blake2s and Keccak transcripts, a sharded driver, a captured graph of a proof.
"""
import time
from collections import namedtuple

from . import commit, deep, gates as gates_, openings, quotient, serialization, stage2, witness
from ._lib import BoojumError
from .field import log2_exact, read_status
from .openings import OpeningConfig, OpeningLayout

ProofConfig = namedtuple("ProofConfig", "fri_lde_factor merkle_tree_cap_size security_level pow_bits pow_runner hasher",
                         defaults=(0, None, "poseidon2"))
ProofConfig.__doc__ = """proof.rs ProofConfig's fields that a proof reads, the PoWRunner (pow.Blake2s256,
pow.Keccak256; None = pow.NoPow) and the tree hasher."""

_LOOKUP_SERDE = {"constant": "UseSpecializedColumnsWithTableIdAsConstant",
                 "variable": "UseSpecializedColumnsWithTableIdAsVariable"}


# ------------------------------------------------------------------ host bookkeeping
def setup_leaf_order(layout):
    """[(kind, index)] of the setup oracle's columns: the V sigmas, the C constants, the table
    columns -- the order openings.sources_at_z reads (setup_storage.rs:18-70)."""
    g = OpeningLayout(*layout)
    return [("sigma", i) for i in range(g.V)] + [("constant", i) for i in range(g.C)] + \
        [("table", i) for i in range(g.lookup_setups)]


AlphaSplit = namedtuple("AlphaSplit", "lookup specialized general_purpose copy_permutation")
AlphaSplit.__doc__ = """(begin, end) ranges into the powers of alpha, in the reference's order."""


def alpha_split(layout, num_specialized_terms, num_general_purpose_terms):
    """prover.rs:608-625 / verifier.rs:1033-1052: L + M lookup terms, the terms of the gates over
    specialized columns, those over general-purpose columns, then 1 + 1 + I copy-permutation terms."""
    g = OpeningLayout(*layout)
    counts = (g.L + g.M, num_specialized_terms, num_general_purpose_terms, 2 + g.I)
    out, at = [], 0
    for c in counts:
        out.append((at, at + c))
        at += c
    return AlphaSplit(*out)


def _check_config(config):
    config = ProofConfig(**config) if isinstance(config, dict) else ProofConfig(*config)
    try:
        log2_exact(config.fri_lde_factor)
        log2_exact(config.merkle_tree_cap_size)
    except ValueError as e:
        raise ValueError("ProofConfig: fri_lde_factor and merkle_tree_cap_size are powers of two (%s)" % e)
    if config.hasher != "poseidon2":
        raise ValueError("the transcript that absorbs %s caps is not built: hasher is 'poseidon2'" % config.hasher)
    if not 0 <= config.pow_bits < config.security_level:
        raise ValueError("pow_bits outside 0..security_level")
    if config.pow_runner is None:
        from .pow import NoPow
        config = config._replace(pow_runner=NoPow)
    return config


def _check_geometry(layout, parameters, extra_selectors, lookup_parameters, n_tables, n_rows, locations):
    g = layout
    if min(g) < 0 or g.V < 1 or g.quotient_degree < 1:
        raise ValueError("layout: %r" % (g,))
    log2_exact(g.quotient_degree)
    log2_exact(n_rows)
    if g.I != stage2.num_intermediate_partial_product_relations(g.V, g.quotient_degree):
        raise ValueError("layout.I = %d, %d variables in chunks of %d leave %d intermediate products"
                         % (g.I, g.V, g.quotient_degree,
                            stage2.num_intermediate_partial_product_relations(g.V, g.quotient_degree)))
    if parameters.num_columns_under_copy_permutation > g.V or parameters.num_witness_columns > g.W \
            or parameters.num_constant_columns + extra_selectors > g.C:
        raise ValueError("the general-purpose geometry exceeds the layout")
    if lookup_parameters is None:
        if n_tables or g.L or g.M or g.lookup_setups:
            raise ValueError("lookup tables or lookup columns in the layout without lookup parameters")
    else:
        if not n_tables:
            raise ValueError("lookup parameters without lookup tables")
        p, per_arg, total = stage2._lookup_shape(lookup_parameters)
        if (g.L, g.M, g.lookup_setups) != (p.num_repetitions, 1, total) or n_tables != total:
            raise ValueError("lookup: %d repetitions of width %d need L = %d, M = 1 and %d table columns"
                             % (p.num_repetitions, p.width, p.num_repetitions, total))
        if parameters.num_columns_under_copy_permutation + per_arg * p.num_repetitions > g.V:
            raise ValueError("the lookup columns do not fit behind the general-purpose variables")
        if p.kind == "constant" and parameters.num_constant_columns + extra_selectors >= g.C:
            raise ValueError("no constant column left for the table id")
    for col, row in locations:
        if not (0 <= col < g.V and 0 <= row < n_rows):
            raise ValueError("public input location (%d, %d) outside the %d x %d variables" % (col, row, g.V, n_rows))


class ProverSetup:
    """What the reference keeps per circuit in SetupStorage, plus the verification key.
    oracle: the setup commit.OracleCommitment (its LDE at used_lde_degree, the tree over the first
    fri_lde_factor cosets); trace: the same columns in Lagrange form, (V + C + tables, n), which
    stage 2 and the satisfiability check read; variables_hint, witness_hint: uploaded CopyHints;
    gate_set: the uploaded GateSet, specialized placements first; vk: the verification key under
    the reference's serde names."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def sigmas(self):
        return self.trace[:self.layout.V]

    @property
    def constants(self):
        return self.trace[self.layout.V:self.layout.V + self.layout.C]

    @property
    def tables(self):
        return self.trace[self.layout.V + self.layout.C:]


def prepare_setup(constants, variables_hint, witness_hint, gates, lookup_tables, lookup_parameters,
                  public_inputs_locations, layout, config, parameters, specialized_gates=(),
                  num_specialized_terms=None, extra_constant_polys_for_selectors=None, total_tables_len=None,
                  native_library=False, device="cuda"):
    """Once per circuit.

    constants: the (C, n) constant columns, selector columns first (host array or device tensor);
    variables_hint, witness_hint: the two dense copy hints (Dense*CopyHint, their maps, or
    witness.CopyHint; witness_hint None for no witness columns);
    gates: the placements of the gates over general-purpose columns, with specialized_gates those
    over specialized columns -- or an uploaded gates.GateSet that lists the specialized placements
    first, with num_specialized_terms saying how many of its terms are theirs;
    lookup_tables: the (width + 1, n) table columns with lookup_parameters a
    stage2.LookupParameters, or None and None;
    public_inputs_locations: [(column, row)];
    layout: openings.OpeningLayout; config: ProofConfig;
    parameters: the general-purpose gates.CSGeometry, which the vk carries and which places the
    lookup columns (they start at num_columns_under_copy_permutation) and the table-id constant
    (column num_constant_columns + extra_constant_polys_for_selectors, setup.rs:964-988);
    extra_constant_polys_for_selectors: by default the longest selector path of `gates`.

    Every argument is checked before anything is launched.  Then: the sigma columns
    (witness.create_permutation_polys), constants and tables laid behind them in one tensor, that
    tensor committed at used_lde_degree over fri_lde_factor cosets, the hints and
    the gate set uploaded."""
    import numpy as np
    import torch
    layout = OpeningLayout(**layout) if isinstance(layout, dict) else OpeningLayout(*layout)
    config = _check_config(config)
    if not isinstance(parameters, gates_.CSGeometry):
        parameters = gates_.CSGeometry(**parameters)
    locations = [(int(c), int(r)) for c, r in public_inputs_locations]
    if lookup_parameters is not None:
        lookup_parameters = stage2.LookupParameters(*lookup_parameters)
    if isinstance(gates, gates_.GateSet):
        if specialized_gates or num_specialized_terms is None:
            raise ValueError("an uploaded GateSet comes with num_specialized_terms and no specialized_gates")
        gate_set, placements = gates, gates.placements
        if not 0 <= num_specialized_terms <= gate_set.num_terms:
            raise ValueError("num_specialized_terms outside the set's %d terms" % gate_set.num_terms)
    else:
        if num_specialized_terms is not None:
            raise ValueError("num_specialized_terms goes with an uploaded GateSet")
        gate_set, placements = None, list(specialized_gates) + list(gates)
        num_specialized_terms = sum(pl.num_terms() for pl in specialized_gates)
    if extra_constant_polys_for_selectors is None:
        if placements is None:
            raise ValueError("a GateSet uploaded from an image needs extra_constant_polys_for_selectors")
        extra_constant_polys_for_selectors = max([len(pl.selector_path) for pl in placements], default=0)
    vars_hint = variables_hint if isinstance(variables_hint, witness.CopyHint) else witness.CopyHint(variables_hint)
    wits_hint = witness_hint if witness_hint is None or isinstance(witness_hint, witness.CopyHint) \
        else witness.CopyHint(witness_hint)
    n = vars_hint.n_rows
    n_tables = 0 if lookup_tables is None else len(lookup_tables)
    const_shape = tuple(constants.shape) if hasattr(constants, "shape") else np.asarray(constants).shape
    if const_shape != (layout.C, n):
        raise ValueError("constants are %s, the layout has %d columns of %d rows" % (const_shape, layout.C, n))
    if vars_hint.n_cols != layout.V or (wits_hint.n_cols if wits_hint is not None else 0) != layout.W \
            or (wits_hint is not None and wits_hint.n_rows != n):
        raise ValueError("the hints do not have the layout's %d variable and %d witness columns of %d rows"
                         % (layout.V, layout.W, n))
    _check_geometry(layout, parameters, extra_constant_polys_for_selectors, lookup_parameters, n_tables, n, locations)
    if n_tables and tuple(lookup_tables.shape if hasattr(lookup_tables, "shape") else np.asarray(lookup_tables).shape) \
            != (n_tables, n):
        raise ValueError("lookup tables: %d columns of %d rows" % (n_tables, n))
    if total_tables_len is None:
        total_tables_len = n if n_tables else 0
    if not (n_tables == 0) == (total_tables_len == 0) or total_tables_len > n:
        raise ValueError("total_tables_len %d for %d table columns of %d rows" % (total_tables_len, n_tables, n))
    used_lde_degree = max(config.fri_lde_factor, layout.quotient_degree)
    # -- the device from here on
    if gate_set is None:
        gate_set = gates_.GateSet(placements, native_library=native_library)
    general_terms = gate_set.num_terms - num_specialized_terms
    as_dev = lambda a: a.to(device) if isinstance(a, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).view(np.int64)).to(device)  # noqa: E731
    sigmas = witness.create_permutation_polys(vars_hint, device=device)
    trace = torch.empty((layout.V + layout.C + n_tables, n), dtype=torch.int64, device=sigmas.device)
    trace[:layout.V] = sigmas
    del sigmas
    if layout.C:
        trace[layout.V:layout.V + layout.C] = as_dev(constants)
    if n_tables:
        trace[layout.V + layout.C:] = as_dev(lookup_tables)
    oracle = commit.commit_trace_columns(trace, used_lde_degree, config.fri_lde_factor, config.merkle_tree_cap_size,
                                         hasher=config.hasher)
    vars_hint.upload()
    if wits_hint is not None:
        wits_hint.upload()
    cap = serialization.cap_to_json(oracle.get_cap(), config.hasher)
    vk = make_vk(layout, parameters, lookup_parameters, n, total_tables_len, extra_constant_polys_for_selectors, cap,
                 locations, config)
    return ProverSetup(layout=layout, config=config, parameters=parameters, lookup_parameters=lookup_parameters,
                       n=n, used_lde_degree=used_lde_degree, oracle=oracle, trace=trace, variables_hint=vars_hint,
                       witness_hint=wits_hint, gate_set=gate_set, num_specialized_terms=num_specialized_terms,
                       num_general_purpose_terms=general_terms, public_inputs_locations=locations,
                       extra_constant_polys_for_selectors=extra_constant_polys_for_selectors, vk=vk,
                       split=alpha_split(layout, num_specialized_terms, general_terms))


def make_vk(layout, parameters, lookup_parameters, domain_size, total_tables_len, extra_selectors, setup_cap,
            locations, config):
    """The verification key's fields a verifier of this proof reads, under the reference's serde
    names (verifier.rs:52-120, VerificationKey in proof.rs)."""
    if lookup_parameters is None:
        lookup = "NoLookup"
    else:
        lookup = {_LOOKUP_SERDE[lookup_parameters.kind]: {"width": lookup_parameters.width,
                                                         "num_repetitions": lookup_parameters.num_repetitions,
                                                         "share_table_id": True}}
    return {"parameters": {"num_columns_under_copy_permutation": parameters.num_columns_under_copy_permutation,
                           "num_witness_columns": parameters.num_witness_columns,
                           "num_constant_columns": parameters.num_constant_columns,
                           "max_allowed_constraint_degree": parameters.max_allowed_constraint_degree},
            "lookup_parameters": lookup, "domain_size": domain_size, "total_tables_len": total_tables_len,
            "public_inputs_locations": [list(p) for p in locations],
            "extra_constant_polys_for_selectors": extra_selectors, "quotient_degree": layout.quotient_degree,
            "fri_lde_factor": config.fri_lde_factor, "cap_size": config.merkle_tree_cap_size,
            "setup_merkle_tree_cap": setup_cap}


# ------------------------------------------------------------------ the front half
class FrontHalf:
    """prove_commitments' result.  oracles: the (witness, stage 2, quotient, setup)
    OracleCommitments, the order prove_openings takes; public_inputs: [(column, row, value)];
    caps: {"witness", "stage_2", "quotient"} as JSON; challenges: everything drawn -- beta, gamma,
    lookup_beta, lookup_gamma (None without lookups), alpha; monomials: the (2 q, n) quotient
    chunks; report: {"timings", "top_is_zero", "grand_product", "satisfiability"}."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _two(transcript):
    return (int(transcript.get_challenge()), int(transcript.get_challenge()))


def _lookup_arguments(setup, wset, oracle_w):
    """The `lookup` dicts of second_stage_trace and quotient_from_arguments (without challenges)."""
    g, p = setup.layout, setup.lookup_parameters
    _, per_arg, _ = stage2._lookup_shape(p)
    offset = setup.parameters.num_columns_under_copy_permutation
    idxes = [setup.parameters.num_constant_columns + setup.extra_constant_polys_for_selectors] \
        if p.kind == "constant" else []
    setup_lde = setup.oracle.lde
    trace_side = dict(variables_columns=wset.variables, multiplicities_columns=wset.multiplicities,
                      constant_polys=setup.constants, lookup_tables_columns=setup.tables,
                      table_id_column_idxes=idxes, variables_offset=offset, lookup_parameters=p)
    lde_side = dict(multiplicities_lde=oracle_w.lde[g.V + g.W:], constants_lde=setup_lde[g.V:g.V + g.C],
                    tables_lde=setup_lde[g.V + g.C:], table_id_column_idxes=idxes,
                    column_elements_per_subargument=per_arg, num_subarguments=p.num_repetitions,
                    variables_offset=offset)
    return trace_side, lde_side


def prove_commitments(setup, witness_vec, transcript, diagnose=False):
    """The front half (module doc): from the setup cap to the quotient cap.  transcript: any object
    with witness_field_elements, witness_merkle_tree_cap and get_challenge, fresh.  Returns a
    FrontHalf, or raises BoojumError naming the stage where the reference panics."""
    g, cfg = setup.layout, setup.config
    if [tuple(p) for p in witness_vec.public_inputs_locations] != setup.public_inputs_locations:
        raise ValueError("the WitnessVec's public input locations are not the setup's")
    if bool(len(witness_vec.multiplicities)) != bool(g.M):
        raise ValueError("multiplicities go with a circuit that has lookups, and only with one")
    times, clock = {}, [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        times[name] = now - clock[0]
        clock[0] = now

    cap_json = lambda o: serialization.cap_to_json(o.get_cap(), cfg.hasher)   # noqa: E731
    # 1, 2
    transcript.witness_merkle_tree_cap(setup.vk["setup_merkle_tree_cap"])
    oracle_w, wset = witness.commit_witness_vec(witness_vec, setup.variables_hint, setup.witness_hint,
                                                setup.used_lde_degree, cfg.fri_lde_factor, cfg.merkle_tree_cap_size,
                                                hasher=cfg.hasher, n_multiplicity_columns=g.M,
                                                device=setup.trace.device)
    for value in wset.public_inputs_values:
        transcript.witness_field_elements([value])
    caps = {"witness": cap_json(oracle_w)}
    transcript.witness_merkle_tree_cap(caps["witness"])
    lap("witness_commit")
    report = {"satisfiability": None}
    if diagnose:
        found = gates_.check_if_satisfied(setup.gate_set, wset.variables, wset.witness if g.W else None,
                                          setup.constants if g.C else None)
        report["satisfiability"] = found
        if not found.satisfied:
            raise BoojumError("prove, gates: %s (%d unsatisfied in all)" % (found.message(), found.num_unsatisfied))
        lap("diagnose")
    # 3
    drawn = {"beta": _two(transcript), "gamma": _two(transcript), "lookup_beta": None, "lookup_gamma": None}
    lookup_s2 = lookup_q = None
    if setup.lookup_parameters is not None:
        drawn["lookup_beta"], drawn["lookup_gamma"] = _two(transcript), _two(transcript)
        lookup_s2, lookup_q = _lookup_arguments(setup, wset, oracle_w)
        for d in (lookup_s2, lookup_q):
            d.update(beta=drawn["lookup_beta"], gamma=drawn["lookup_gamma"])
    # 4
    st = stage2.second_stage_trace(wset.variables, setup.sigmas, drawn["beta"], drawn["gamma"], g.quotient_degree,
                                   lookup=lookup_s2, check=False)
    status = stage2.compute_partial_products_in_extension.status
    oracle_s2 = commit.commit_trace_columns(st.trace, setup.used_lde_degree, cfg.fri_lde_factor,
                                            cfg.merkle_tree_cap_size, hasher=cfg.hasher)
    caps["stage_2"] = cap_json(oracle_s2)
    t0, t1, zeros, _ = read_status(status)
    report["grand_product"] = (t0, t1)
    if zeros:
        raise BoojumError("prove, stage 2: copy permutation: %d zero denominator(s)" % zeros)
    if (t0, t1) != (1, 0):
        raise BoojumError("prove, stage 2: the grand product over the domain is %r, not one" % ((t0, t1),))
    transcript.witness_merkle_tree_cap(caps["stage_2"])
    lap("stage2_commit")
    # 5
    drawn["alpha"] = _two(transcript)
    split = setup.split
    powers = deep.materialize_ext_challenge_powers(drawn["alpha"], split.copy_permutation[1])
    take = lambda r: powers[r[0]:r[1]]   # noqa: E731
    # the set lists the specialized placements first, so its running term index is the reference's
    gate_alphas = take((split.specialized[0], split.general_purpose[1]))
    # 6
    lde_w, lde_setup = oracle_w.lde, setup.oracle.lde
    chunks, top_is_zero = quotient.quotient_from_arguments(
        lde_w[:g.V], lde_setup[:g.V], oracle_s2.lde, drawn["beta"], drawn["gamma"],
        take(split.copy_permutation) + take(split.lookup), g.quotient_degree, lookup=lookup_q,
        gates=dict(gate_set=setup.gate_set, alphas=gate_alphas,
                   witnesses_lde=lde_w[g.V:g.V + g.W] if g.W else None,
                   constants_lde=lde_setup[g.V:g.V + g.C] if g.C else None) if gate_alphas else None)
    report["top_is_zero"] = top_is_zero
    if top_is_zero != (True, True):
        raise BoojumError("prove, quotient: unsatisfied, the top coefficient of the quotient is not zero "
                          "(c0 zero: %s, c1 zero: %s)" % top_is_zero)
    oracle_q = commit.quotient_commit(chunks, cfg.fri_lde_factor, cfg.merkle_tree_cap_size, hasher=cfg.hasher)
    caps["quotient"] = cap_json(oracle_q)
    transcript.witness_merkle_tree_cap(caps["quotient"])
    lap("quotient_commit")
    report["timings"] = times
    return FrontHalf(oracles=[oracle_w, oracle_s2, oracle_q, setup.oracle],
                     public_inputs=list(wset.public_inputs_with_locations), caps=caps, challenges=drawn,
                     monomials=chunks, witness_set=wset, report=report)


# ------------------------------------------------------------------ the whole proof
class Proof:
    """proof.rs:118-140 under its serde names (`to_json`), and what the prover drew
    (`challenges`: the front half's and the opening phase's), `front` and `openings` the halves."""

    def __init__(self, setup, front, opening_proof):
        self.front, self.openings = front, opening_proof
        self.config = setup.config
        self.public_inputs = [int(v) for _, _, v in front.public_inputs]
        self.challenges = dict(front.challenges, **opening_proof.challenges)
        self.timings = dict(front.report["timings"], **opening_proof.timings)

    def to_json(self):
        cfg = self.config
        out = {"proof_config": {"fri_lde_factor": cfg.fri_lde_factor, "merkle_tree_cap_size": cfg.merkle_tree_cap_size,
                                "fri_folding_schedule": None, "security_level": cfg.security_level,
                                "pow_bits": cfg.pow_bits},
               "public_inputs": list(self.public_inputs), "witness_oracle_cap": self.front.caps["witness"],
               "stage_2_oracle_cap": self.front.caps["stage_2"], "quotient_oracle_cap": self.front.caps["quotient"]}
        out.update(self.openings.to_json())
        return out


def prove(setup, witness_vec, transcript=None, route="fused", diagnose=False):
    """prove_from_precomputations: prove_commitments, then openings.prove_openings over the same
    transcript (default: a fresh transcript.Poseidon2Transcript).  Returns a Proof; raises
    BoojumError (and returns nothing) where the reference panics."""
    if route not in ("fused", "chain"):
        raise ValueError("route is 'fused' or 'chain'")
    if transcript is None:
        from .transcript import Poseidon2Transcript
        transcript = Poseidon2Transcript()
    cfg = setup.config
    front = prove_commitments(setup, witness_vec, transcript, diagnose=diagnose)
    opening = openings.prove_openings(
        front.oracles, setup.layout, transcript,
        OpeningConfig(cfg.security_level, cfg.pow_bits, cfg.pow_runner, cfg.merkle_tree_cap_size, cfg.fri_lde_factor),
        front.public_inputs, route=route)
    return Proof(setup, front, opening)
