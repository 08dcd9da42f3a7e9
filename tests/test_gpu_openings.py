"""The opening phase on the GPU (boojum_amd/openings.py, bj_deep_codeword_d in csrc/deep.hip).

* The fused codeword call against the chain of one bj_deep_quotient_d per (group, point), word for
  word, on every path of the kernel: the 16-byte path (full window), the 8-byte path (odd window; a
  group whose pointer is 8- but not 16-byte aligned), one row, the caps (8 points x 16 terms), a
  column walk with and without the unrolled-by-8 body, several blocks (2^11 rows = 4 blocks), and
  16 rows against Python integers.
* The call captured in a graph and replayed.
* prove_openings end to end through the checker's replay of the verifier (oracle/transcript.py),
  its negative cases, and the proof of work.

Everything is at n = 2^10 with FRI LDE factor 2 (log_domain 11)."""
import ctypes

import numpy as np
import pytest

import oracle as O
import transcript as T

from test_openings_cpu import feed_until_queries

pytestmark = pytest.mark.gpu

P = O.P
LOG_N, LDE_FACTOR, LOG_DOMAIN = 10, 2, 11
N, DOMAIN = 1 << LOG_N, 1 << LOG_DOMAIN
WIDTHS = [12, 17, 12, 8]


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, commit, deep, field, merkle, openings, pow as pow_, transcript
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, deep=deep, commit=commit, lib=_lib, openings=openings,
                               transcript=transcript, pow=pow_, merkle=merkle))


def rand_words(shape, seed):
    """Random u64 words, every eighth one non-canonical (>= p) and a few 2^64 - 1."""
    r = np.random.default_rng(seed)
    a = r.integers(0, P, size=shape, dtype=np.uint64)
    flat = a.reshape(-1)
    flat[::8] = r.integers(P, 1 << 64, size=flat[::8].shape, dtype=np.uint64)
    flat[3::61] = np.uint64((1 << 64) - 1)
    return a


def rand_ext(r):
    return (int(r.integers(0, P, dtype=np.uint64)), int(r.integers(0, P, dtype=np.uint64)))


def six_points(seed):
    """One point with sources in two groups, one with none, two sharing a group (one of them with
    the walk's remainder loop only, the other with Ext2 sources), one over a whole group of 17
    columns (two unrolled bodies and a remainder), and a base-field point."""
    r = np.random.default_rng(seed)
    e = lambda g, c, x: (g, c, x, rand_ext(r), rand_ext(r))  # noqa: E731
    return [
        (rand_ext(r), [e(0, c, False) for c in range(12)] + [e(3, 0, True), e(3, 5, False), e(0, 2, False)]),
        (rand_ext(r), []),
        (rand_ext(r), [e(2, 4, True), e(2, 6, True), e(2, 11, False)]),
        (rand_ext(r), [e(2, 0, True)]),
        (rand_ext(r), [e(1, c, False) for c in range(17)]),
        ((int(r.integers(2, 1 << 20)), 0), [e(0, 3, False), e(0, 7, False)]),
    ]


@pytest.fixture(scope="module")
def columns(bj):
    """The four groups over the whole domain, host and device; group 1 sits one word into its
    allocation, so its pointer is 8- but not 16-byte aligned (its stride is even)."""
    host = [rand_words((w, DOMAIN), 10 + i) for i, w in enumerate(WIDTHS)]
    dev = [bj.field.to_device(h) for h in host]
    buf = bj.torch.empty((WIDTHS[1] * DOMAIN + 1,), dtype=bj.torch.int64, device="cuda")
    odd = buf[1:].view(WIDTHS[1], DOMAIN)
    odd.copy_(dev[1])
    assert odd.data_ptr() % 16 == 8
    return host, dev, odd


def chain(bj, groups, points, row0, n_rows, dst):
    """The yardstick: quotening_operation_in_extension (one bj_deep_quotient_d) per (point, group)
    over the whole group, coefficients from quotening_plan; accumulating into dst."""
    for at, entries in points:
        used = sorted({e[0] for e in entries})
        for g in used or [None]:
            mine = [e[1:] for e in entries if e[0] == g]
            bj.deep.quotening_operation_in_extension(dst[0], dst[1], None if g is None else groups[g], mine, at,
                                                     LOG_DOMAIN, row0=row0, accumulate=True)
    return bj.field.to_host(dst)


def both(bj, groups, points, row0, n_rows, accumulate):
    start = rand_words((2, n_rows), 77)
    window = [g[:, row0:row0 + n_rows] for g in groups]
    want_dst = bj.field.to_device(start if accumulate else np.zeros_like(start))
    want = chain(bj, window, points, row0, n_rows, want_dst)
    got_dst = bj.field.to_device(start)        # without accumulate the call must overwrite this
    bj.deep.deep_codeword(window, points, LOG_DOMAIN, row0=row0, out=(got_dst[0], got_dst[1]), accumulate=accumulate)
    got = bj.field.to_host(got_dst)
    assert (got < np.uint64(P)).all()
    return got, want


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("window", ["full", "odd", "one_row", "misaligned"])
def test_fused_call_equals_the_chain_word_for_word(bj, columns, window, accumulate):
    _, dev, odd = columns
    groups = list(dev)
    row0, n_rows = {"full": (0, DOMAIN), "odd": (37, 91 + 512), "one_row": (5, 1), "misaligned": (0, DOMAIN)}[window]
    if window == "misaligned":
        groups[1] = odd
    if window == "full":
        assert all(g.data_ptr() % 16 == 0 for g in groups)   # the 16-byte path
    got, want = both(bj, groups, six_points(3), row0, n_rows, accumulate)
    assert np.array_equal(got, want)


def test_fused_call_at_the_caps(bj, columns):
    """8 points x 2 terms = 16 terms."""
    _, dev, _ = columns
    r = np.random.default_rng(9)
    points = []
    for p in range(8):
        g0, g1 = p % 4, (p + 1) % 4
        points.append((rand_ext(r), [(g0, p % WIDTHS[g0], False, rand_ext(r), rand_ext(r)),
                                     (g1, 0, True, rand_ext(r), rand_ext(r)),
                                     (g1, WIDTHS[g1] - 1, False, rand_ext(r), rand_ext(r))]))
    terms, _, _ = bj.deep.codeword_terms(WIDTHS, points)
    assert len(terms) == bj.lib.DEEP_MAX_TERMS and len(points) == bj.lib.DEEP_MAX_POINTS
    for row0, n_rows in ((0, DOMAIN), (1, 255)):
        got, want = both(bj, list(dev), points, row0, n_rows, False)
        assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        bj.deep.deep_codeword(list(dev), points + [points[0]], LOG_DOMAIN)


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def test_sixteen_rows_equal_python_integers(bj, columns):
    host, dev, _ = columns
    points = six_points(3)
    row0 = DOMAIN - 16
    window = [g[:, row0:] for g in dev]
    d0, d1 = bj.deep.deep_codeword(window, points, LOG_DOMAIN, row0=row0)
    got = list(zip((int(v) for v in bj.field.to_host(d0)), (int(v) for v in bj.field.to_host(d1))))
    w = T.domain_generator(LOG_DOMAIN)
    for i, L in enumerate(range(row0, DOMAIN)):
        x = 7 * pow(w, bitrev(L, LOG_DOMAIN), P) % P
        want = (0, 0)
        for at, entries in points:
            num = (0, 0)
            for g, col, is_ext, ch, v in entries:
                f = (int(host[g][col, L]) % P, int(host[g][col + 1, L]) % P if is_ext else 0)
                num = T.e_add(num, T.e_mul(ch, T.e_sub(f, v)))
            want = T.e_add(want, T.e_mul(num, T.e_inv(T.e_sub((x, 0), at))))
        assert got[i] == want, L


def test_call_captured_in_a_graph_replays_the_same_words(bj, columns):
    torch = bj.torch
    _, dev, _ = columns
    points = six_points(4)
    want0, want1 = bj.deep.deep_codeword(list(dev), points, LOG_DOMAIN)
    want = bj.field.to_host(torch.stack([want0, want1]))
    terms, gammas, ks = bj.deep.codeword_terms(WIDTHS, points)
    g = bj.field.to_device(np.array(gammas, dtype=np.uint64).reshape(-1))
    dst = torch.zeros((2, DOMAIN), dtype=torch.int64, device="cuda")
    d = bj.deep.codeword_descriptor([(t.data_ptr(), t.shape[0], t.stride(0)) for t in dev], points, terms, ks,
                                    g.data_ptr(), len(gammas), LOG_DOMAIN, 0, DOMAIN, dst[0].data_ptr(),
                                    dst[1].data_ptr(), False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bj.lib.call("bj_deep_codeword_d", ctypes.byref(d), bj.field.stream_of(dst))
    for _ in range(2):
        dst.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bj.field.to_host(dst), want)


# ------------------------------------------------------------------ end to end
LAYOUT = dict(V=10, W=1, C=3, M=1, L=2, I=2, lookup_setups=4, quotient_degree=4)
CAP, SECURITY = 4, 8
PUBLIC_INPUTS = [(0, 0), (3, 0), (1, 7)]     # (column, row): two in one row, one in another


class Circuit:
    """Four committed oracles of random columns of degree < n at the end-to-end shape, and the
    verifier-side data that does not depend on the opening phase."""

    def __init__(self, bj, bad_column=None):
        widths = bj.openings.leaf_widths(bj.openings.OpeningLayout(**LAYOUT))
        assert widths == (12, 12, 8, 17)
        r = np.random.default_rng(2024)
        traces = [r.integers(0, P, size=(w, N), dtype=np.uint64) for w in widths]
        wit, s2, quo, setup = traces
        self.witness = bj.commit.commit_trace_columns(bj.field.to_device(wit), 4, LDE_FACTOR, CAP)
        if bad_column is not None:
            # + a on coset 0, + b on coset 1: alpha + beta x^n with beta != 0, so degree exactly n
            lde = bj.field.to_host(self.witness.lde).copy()
            for coset, add in ((0, 1), (1, 2)):
                lde[bad_column, coset] = (lde[bad_column, coset].astype(object) + add) % P
            lde = bj.field.to_device(lde)
            tree = bj.merkle.MerkleTreeWithCap.construct(lde, CAP, num_cosets=LDE_FACTOR)
            self.witness = bj.commit.OracleCommitment(lde, tree)
        self.stage_2 = bj.commit.commit_trace_columns(bj.field.to_device(s2), 4, LDE_FACTOR, CAP)
        self.quotient = bj.commit.quotient_commit(bj.field.to_device(quo), LDE_FACTOR, CAP)
        self.setup = bj.commit.commit_trace_columns(bj.field.to_device(setup), 4, LDE_FACTOR, CAP)
        self.oracles = [self.witness, self.stage_2, self.quotient, self.setup]
        self.public_inputs = [(c, row, int(wit[c, row]) + (1 if c == bad_column and row == 0 else 0))
                              for c, row in PUBLIC_INPUTS]
        cap = lambda o: [[int(v) for v in d] for d in o.get_cap()]  # noqa: E731
        self.fx = {
            "vk": {"parameters": {"num_columns_under_copy_permutation": 10, "num_witness_columns": 1,
                                  "num_constant_columns": 2},
                   "lookup_parameters": {"UseSpecializedColumnsWithTableIdAsConstant":
                                         {"width": 3, "num_repetitions": 2}},
                   "domain_size": N, "total_tables_len": N, "quotient_degree": 4,
                   "extra_constant_polys_for_selectors": 1, "setup_merkle_tree_cap": cap(self.setup),
                   "public_inputs_locations": [list(p) for p in PUBLIC_INPUTS]},
            "public_inputs": [v for _, _, v in self.public_inputs],
            "witness_oracle_cap": cap(self.witness), "stage_2_oracle_cap": cap(self.stage_2),
            "quotient_oracle_cap": cap(self.quotient),
        }

    def transcript(self, bj):
        """The product transcript fed as the prover feeds it up to the quotient cap."""
        tr, fx = bj.transcript.Poseidon2Transcript(), self.fx
        tr.witness_merkle_tree_cap(fx["vk"]["setup_merkle_tree_cap"])
        for v in fx["public_inputs"]:
            tr.witness_field_elements([v])
        tr.witness_merkle_tree_cap(fx["witness_oracle_cap"])
        tr.get_multiple_challenges(8)
        tr.witness_merkle_tree_cap(fx["stage_2_oracle_cap"])
        tr.get_multiple_challenges(2)
        tr.witness_merkle_tree_cap(fx["quotient_oracle_cap"])
        return tr

    def prove(self, bj, pow_bits=0, runner=None, route="fused"):
        cfg = bj.openings.OpeningConfig(SECURITY, pow_bits, runner or bj.pow.NoPow, CAP, LDE_FACTOR)
        proof = bj.openings.prove_openings(self.oracles, LAYOUT, self.transcript(bj), cfg, self.public_inputs,
                                           route=route)
        fx = dict(self.fx)
        fx["proof_config"] = {"fri_lde_factor": LDE_FACTOR, "merkle_tree_cap_size": CAP, "security_level": SECURITY,
                              "pow_bits": pow_bits}
        fx.update(proof.to_json())
        fx["queries"] = fx["queries_per_fri_repetition"]
        return proof, fx


@pytest.fixture(scope="module")
def circuit(bj):
    return Circuit(bj)


@pytest.fixture(scope="module")
def proved(bj, circuit):
    return circuit.prove(bj)


def test_the_checkers_replay_accepts_the_opening_phase(bj, proved):
    proof, fx = proved
    assert proof.schedule == [3, 3, 3] and len(proof.final_fri_monomials[0]) == 2 and proof.num_queries == 8
    assert len(proof.values_at_z) == 39 and len(proof.values_at_z_omega) == 1 and len(proof.values_at_0) == 3
    assert proof.low_degree == (True, True) and proof.pow_challenge == 0
    res = T.replay(fx)
    assert res["geometry"] == LAYOUT
    ch = proof.challenges
    assert tuple(res["z"]) == tuple(ch["z"]) and tuple(res["deep_challenge"]) == tuple(ch["deep_challenge"])
    assert [tuple(p[0]) for p in res["fri_challenges"]] == [tuple(c) for c in ch["fri_challenges"]]
    assert [q["index"] for q in res["queries"]] == ch["query_indices"]
    assert len(set(ch["query_indices"])) > 1


def test_the_chain_route_gives_the_same_proof(bj, circuit, proved):
    proof, _ = proved
    other, _ = circuit.prove(bj, route="chain")
    assert other.to_json() == proof.to_json() and other.challenges == proof.challenges


def test_replay_rejects_an_altered_value_at_z(proved):
    _, fx = proved
    bad = dict(fx)
    bad["values_at_z"] = [list(v) for v in fx["values_at_z"]]
    bad["values_at_z"][17][1] = (bad["values_at_z"][17][1] + 1) % P
    with pytest.raises(AssertionError):
        T.replay(bad)


def test_a_column_of_degree_n_is_reported_and_rejected(bj):
    proof, fx = Circuit(bj, bad_column=5).prove(bj)
    assert False in proof.low_degree
    with pytest.raises(AssertionError):
        T.replay(fx)


def test_proof_of_work_is_absorbed_before_the_query_bits(bj, circuit, proved):
    plain, _ = proved
    proof, fx = circuit.prove(bj, pow_bits=4, runner=bj.pow.Blake2s256)
    assert proof.new_pow_bits == 4 and proof.num_queries == 4
    seed, nonce = proof.challenges["pow_seed"], proof.pow_challenge
    assert len(seed) == 5
    assert bj.pow.Blake2s256.verify_from_field_elements(seed, 4, nonce)
    assert proof.challenges["query_indices"] != plain.challenges["query_indices"][:4]
    # the checker's transcript over the same proof: seed, then the nonce's halves, then the bits
    tr = T.Poseidon2Transcript()
    feed_until_queries(tr, fx)
    assert tr.get_challenges(5) == seed
    tr.witness_field_elements([nonce & 0xFFFFFFFF, nonce >> 32])
    bools, indices = T.BoolsBuffer(LOG_DOMAIN), []
    for _ in range(4):
        bits = bools.get_bits(tr, LOG_DOMAIN)
        indices.append((T.u64_from_lsb_first_bits(bits[LOG_N:]) << LOG_N) + T.u64_from_lsb_first_bits(bits[:LOG_N]))
    assert indices == proof.challenges["query_indices"]
