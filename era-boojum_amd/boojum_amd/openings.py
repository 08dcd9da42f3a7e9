"""The opening phase of the prover (prover.rs:1497-2266) in one call, on the device: from the four
committed base oracles and the transcript as it stands after the quotient cap to the queries.

`prove_openings` runs, in the reference's order:

1. z from the transcript (prover.rs:1501-1502);
2. every polynomial at z, the copy-permutation z(x) at z * omega, the lookup encodings at 0, as
   barycentric sums over coset 0 (deep.py, bj_evaluate_at_d), each witnessed (:1504-1800);
3. the public-input openings grouped by row (:1802-1818);
4. the DEEP challenge and its powers (:1826-1850);
5. the codeword over the first fri_lde_factor cosets (:1852-2050): one bj_deep_codeword_d launch
   for every opening point and oracle (`deep.deep_codeword`), or the chain of one
   bj_deep_quotient_d per (oracle, point);
6. `fri.compute_fri_schedule` and `fri.do_fri` (:2052-2105);
7. the proof of work when the schedule leaves it bits (:2107-2133);
8. the query indices from `transcript.BoolsBuffer` (:2161-2183);
9. `queries.single_round_queries` (:2185-2262).

The sources of a leaf, per oracle (the order of :1501-1780, which the verifier reads back at
verifier.rs:2226-2390): witness = V copiable variables, W witness columns, M multiplicities;
setup = V sigmas, C constants, the lookup table columns; stage 2 = z(x), I partial products,
L lookup-witness and M multiplicity encodings, each an Ext2 polynomial as (c0, c1) columns;
quotient = quotient_degree Ext2 chunks.

Not here: everything before the quotient cap (witness, stage 2, quotient in one driver), the
Blake2s and Keccak transcripts, and a driver over sharded oracles.
"""
import time
from collections import namedtuple

import torch

from . import deep, fri, pow as pow_, queries, serialization
from .field import EXT2_NON_RESIDUE, GENERATOR, P, ROOT_OF_UNITY_2_32, TWO_ADICITY, log2_exact
from .transcript import BoolsBuffer, u64_from_lsb_first_bits

WITNESS, STAGE_2, QUOTIENT, SETUP = range(4)   # the order of `oracles`

OpeningLayout = namedtuple("OpeningLayout", "V W C M L I lookup_setups quotient_degree")
OpeningLayout.__doc__ = """The circuit geometry of the leaves: V variables under copy permutation, W witness
columns, C constant columns (selectors included), M multiplicity columns, L lookup sub-arguments,
I intermediate partial products, lookup_setups table columns (width + 1), quotient_degree chunks."""

OpeningConfig = namedtuple("OpeningConfig", "security_level pow_bits pow_runner merkle_tree_cap_size fri_lde_factor")
OpeningConfig.__doc__ = """ProofConfig's fields the phase reads, and the PoWRunner (pow.Blake2s256, pow.Keccak256,
pow.NoPow)."""


def leaf_widths(layout):
    """Base columns of the (witness, stage 2, quotient, setup) leaves."""
    g = layout
    return (g.V + g.W + g.M, 2 * (1 + g.I + g.L + g.M), 2 * g.quotient_degree, g.V + g.C + g.lookup_setups)


def sources_at_z(layout):
    """[(oracle, column, is_ext)] of every polynomial opened at z, in challenge order."""
    g = layout
    lw, lm = 2 + 2 * g.I, 2 + 2 * g.I + 2 * g.L
    out = [(WITNESS, c, False) for c in range(g.V + g.W)]
    out += [(SETUP, g.V + c, False) for c in range(g.C)]
    out += [(SETUP, c, False) for c in range(g.V)]
    out += [(STAGE_2, 2 * k, True) for k in range(1 + g.I)]
    out += [(WITNESS, g.V + g.W + c, False) for c in range(g.M)]
    out += [(STAGE_2, lw + 2 * k, True) for k in range(g.L)]
    out += [(STAGE_2, lm + 2 * k, True) for k in range(g.M)]
    out += [(SETUP, g.V + g.C + c, False) for c in range(g.lookup_setups)]
    out += [(QUOTIENT, 2 * k, True) for k in range(g.quotient_degree)]
    return out


def sources_at_z_omega(layout):
    return [(STAGE_2, 0, True)]


def sources_at_0(layout):
    g = layout
    return [(STAGE_2, 2 + 2 * g.I + 2 * k, True) for k in range(g.L + g.M)]


def domain_generator(log_n):
    """domain_generator_for_size (utils.rs:13-28)."""
    if log_n > TWO_ADICITY:
        raise ValueError("2^%d exceeds the field's 2-adicity" % log_n)
    return pow(ROOT_OF_UNITY_2_32, 1 << (TWO_ADICITY - log_n), P)


def public_input_opening_tuples(public_inputs, log_n):
    """prover.rs:1802-1818: [(omega^row, [(column, value)])], rows in order of first appearance.
    public_inputs: [(column, row, value)]."""
    omega = domain_generator(log_n)
    out = []
    for column, row, value in public_inputs:
        at = pow(omega, row, P)
        for t in out:
            if t[0] == at:
                t[1].append((column, int(value) % P))
                break
        else:
            out.append((at, [(column, int(value) % P)]))
    return out


def opening_points(layout, z, omega, values_at_z, values_at_z_omega, values_at_0, pi_tuples, challenges):
    """deep.codeword_terms' points: every opening point with its sources, values and challenge
    powers, in the order the challenges are handed out (prover.rs:1852-2050)."""
    ch = iter(challenges)
    z_omega = (z[0] * omega % P, z[1] * omega % P)
    points = []
    for at, srcs, vals in ((z, sources_at_z(layout), values_at_z), (z_omega, sources_at_z_omega(layout), values_at_z_omega),
                           ((0, 0), sources_at_0(layout), values_at_0)):
        if len(srcs) != len(vals):
            raise ValueError("%d sources and %d values" % (len(srcs), len(vals)))
        points.append((at, [(o, c, e, next(ch), v) for (o, c, e), v in zip(srcs, vals)]))
    for at, subset in pi_tuples:
        points.append(((at, 0), [(WITNESS, column, False, next(ch), (value, 0)) for column, value in subset]))
    return points


def _batches(points):
    """Split the points over calls that respect the caps of one bj_deep_codeword_d."""
    from ._lib import DEEP_MAX_POINTS, DEEP_MAX_TERMS
    out, cur, terms = [], [], 0
    for pt in points:
        t = len({e[0] for e in pt[1]})
        if cur and (len(cur) == DEEP_MAX_POINTS or terms + t > DEEP_MAX_TERMS):
            out.append(cur)
            cur, terms = [], 0
        cur.append(pt)
        terms += t
    return out + ([cur] if cur else [])


def codeword_fused(groups, points, log_domain, out):
    """The codeword through bj_deep_codeword_d: one launch (one per 8 points or 16 terms)."""
    for k, batch in enumerate(_batches(points)):
        deep.deep_codeword(groups, batch, log_domain, out=out, accumulate=k > 0)
    return out


def codeword_chain(groups, points, log_domain, out):
    """The same codeword as one bj_deep_quotient_d per (group, point), each over the column range
    its sources touch."""
    first = True
    for at, entries in points:
        used = sorted({e[0] for e in entries})
        for g in used or [None]:
            mine = [e[1:] for e in entries if e[0] == g]
            view = None
            if mine:
                lo = min(col for col, _, _, _ in mine)
                hi = max(col + (2 if is_ext else 1) for col, is_ext, _, _ in mine)
                view = groups[g][lo:hi]
                mine = [(col - lo, is_ext, ch, v) for col, is_ext, ch, v in mine]
            deep.quotening_operation_in_extension(out[0], out[1], view, mine, at, log_domain, accumulate=not first)
            first = False
    return out


class OpeningProof:
    """What the phase adds to the proof, under the reference's serde names (proof.rs:118-140), and
    what it drew: `challenges` = {"z", "deep_challenge", "fri_challenges", "query_indices",
    "pow_seed"}.  `low_degree` is do_fri's pair of flags (reported, not raised), `schedule` and
    `new_pow_bits` compute_fri_schedule's, `timings` seconds per step."""

    FIELDS = ("values_at_z", "values_at_z_omega", "values_at_0", "fri_base_oracle_cap",
              "fri_intermediate_oracles_caps", "final_fri_monomials", "pow_challenge", "queries_per_fri_repetition")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def to_json(self):
        return {k: getattr(self, k) for k in self.FIELDS}


def _evaluate(lde, w):
    return deep.barycentric_evaluate_base_at_extension_for_bitreversed(lde[:, 0, :], w)


def _values(evals, srcs):
    out = []
    for o, c, is_ext in srcs:
        a = evals[o][c]
        if is_ext:
            b = evals[o][c + 1]
            a = ((a[0] + EXT2_NON_RESIDUE * b[1]) % P, (a[1] + b[0]) % P)
        out.append([int(a[0]), int(a[1])])
    return out


def prove_openings(oracles, layout, transcript, config, public_inputs, route="fused"):
    """The opening phase.  oracles: the (witness, stage 2, quotient, setup) commit.OracleCommitment,
    each an LDE (C, D, n) with D >= fri_lde_factor and the tree over its first fri_lde_factor
    cosets; layout: OpeningLayout; transcript: any object with witness_field_elements,
    witness_merkle_tree_cap and get_challenge, already fed through the quotient cap; config:
    OpeningConfig; public_inputs: [(column, row, value)].  route: "fused" or "chain" (module doc,
    step 5).  Returns OpeningProof."""
    if route not in ("fused", "chain"):
        raise ValueError("route is 'fused' or 'chain'")
    layout = OpeningLayout(**layout) if isinstance(layout, dict) else OpeningLayout(*layout)
    config = OpeningConfig(**config) if isinstance(config, dict) else OpeningConfig(*config)
    if len(oracles) != 4:
        raise ValueError("four oracles: witness, stage 2, quotient, setup")
    ldes = [o.lde for o in oracles]
    n = ldes[0].shape[2]
    log_n = log2_exact(n)
    lde_factor = config.fri_lde_factor
    log_f = log2_exact(lde_factor)
    for lde, width in zip(ldes, leaf_widths(layout)):
        if lde.dim() != 3 or lde.shape[0] != width or lde.shape[1] < lde_factor or lde.shape[2] != n:
            raise ValueError("an LDE of shape %s where the layout has %d columns of %d rows on at least %d cosets"
                             % (tuple(lde.shape), width, n, lde_factor))
    dev = ldes[0].device
    hasher = oracles[0].tree.hasher
    times = {}
    clock = [time.perf_counter()]

    def lap(name):
        now = time.perf_counter()
        times[name] = now - clock[0]
        clock[0] = now

    # 1, 2
    z = (int(transcript.get_challenge()), int(transcript.get_challenge()))
    omega = domain_generator(log_n)
    z_omega = (z[0] * omega % P, z[1] * omega % P)
    w = deep.precompute_for_barycentric_evaluation_in_extension(n, GENERATOR, z, device=dev)
    values_at_z = _values([_evaluate(lde, w) for lde in ldes], sources_at_z(layout))
    w = deep.precompute_for_barycentric_evaluation_in_extension(n, GENERATOR, z_omega, device=dev)
    values_at_z_omega = _values({STAGE_2: _evaluate(ldes[STAGE_2][:2], w)}, sources_at_z_omega(layout))
    lw = 2 + 2 * layout.I
    values_at_0 = []
    if layout.L + layout.M:
        w = deep.precompute_for_barycentric_evaluation_in_extension(n, GENERATOR, (0, 0), device=dev)
        ev = [(0, 0)] * lw + _evaluate(ldes[STAGE_2][lw:], w)
        values_at_0 = _values({STAGE_2: ev}, sources_at_0(layout))
    for vals in (values_at_z, values_at_z_omega, values_at_0):
        for v in vals:
            transcript.witness_field_elements(v)
    lap("evaluations")
    # 3, 4
    pi_tuples = public_input_opening_tuples(public_inputs, log_n)
    c = (int(transcript.get_challenge()), int(transcript.get_challenge()))
    total = len(values_at_z) + len(values_at_z_omega) + len(values_at_0) + sum(len(s) for _, s in pi_tuples)
    challenges = deep.materialize_ext_challenge_powers(c, total)
    points = opening_points(layout, z, omega, values_at_z, values_at_z_omega, values_at_0, pi_tuples, challenges)
    # 5: the first fri_lde_factor cosets of every column, flat
    rows = lde_factor * n
    groups = [lde.reshape(lde.shape[0], -1)[:, :rows] for lde in ldes]
    codeword = torch.empty((2, rows), dtype=torch.int64, device=dev)
    (codeword_fused if route == "fused" else codeword_chain)(groups, points, log_n + log_f, (codeword[0], codeword[1]))
    torch.cuda.synchronize(dev)
    lap("codeword")
    # 6
    new_pow_bits, num_queries, schedule, final_degree = fri.compute_fri_schedule(
        config.security_level, config.merkle_tree_cap_size, config.pow_bits, log_f, log_n)
    fri_data = fri.do_fri(codeword[0], codeword[1], transcript, schedule, lde_factor, config.merkle_tree_cap_size,
                          hasher=hasher)
    if len(fri_data.monomial_forms[0]) != final_degree:
        raise ValueError("do_fri left %d monomials, the schedule expects %d"
                         % (len(fri_data.monomial_forms[0]), final_degree))
    lap("fri")
    # 7
    pow_challenge, pow_seed = 0, None
    if new_pow_bits:
        pow_seed = [int(transcript.get_challenge()) for _ in range(pow_.NUM_POW_CHALLENGES)]
        pow_challenge = config.pow_runner.run_from_field_elements(pow_seed, new_pow_bits)
        transcript.witness_field_elements(pow_.pow_challenge_to_field_elements(pow_challenge))
    lap("pow")
    # 8
    max_needed = log_n + log_f
    bools = BoolsBuffer(max_needed)
    indices = []
    for _ in range(num_queries):
        bits = bools.get_bits(transcript, max_needed)
        inner, coset = u64_from_lsb_first_bits(bits[:log_n]), u64_from_lsb_first_bits(bits[log_n:])
        indices.append(coset * n + inner)
    # 9
    base = [queries.QueryOracle(o.tree, o.lde) for o in oracles]
    qs = queries.single_round_queries(base[WITNESS], base[STAGE_2], base[QUOTIENT], base[SETUP],
                                      fri_data.query_oracles(codeword[0], codeword[1]), indices)
    lap("queries")
    return OpeningProof(
        values_at_z=values_at_z, values_at_z_omega=values_at_z_omega, values_at_0=values_at_0,
        fri_base_oracle_cap=serialization.cap_to_json(fri_data.base_oracle.get_cap(), hasher),
        fri_intermediate_oracles_caps=[serialization.cap_to_json(t.get_cap(), hasher)
                                       for t in fri_data.intermediate_oracles],
        final_fri_monomials=[[int(v) for v in m] for m in fri_data.monomial_forms],
        pow_challenge=pow_challenge, queries_per_fri_repetition=qs,
        challenges={"z": z, "deep_challenge": c, "fri_challenges": list(fri_data.challenges),
                    "query_indices": indices, "pow_seed": pow_seed},
        low_degree=fri_data.low_degree, schedule=schedule, new_pow_bits=new_pow_bits, num_queries=num_queries,
        route=route, timings=times)
