"""FRI folding of the DEEP codeword (cs/implementations/fri/mod.rs:179-300) on the GPU.

The codeword is a GoldilocksExt2 vector held as two base columns c0, c1 over the full LDE
domain, bit-reversed (cosets one after another). One fold by 2 (`fold`, bj_fri_fold_d)
is fold_multiple (fri/mod.rs:362-474). `interpolate` chains folds the way
interpolate_independent_cosets / interpolate_flattened_cosets (:476-682) do:
* the root table is the INVERSED bit-reversed twiddles of the full domain;
* it is indexed by the flat pair index at every step;
* the coset inverse starts at 7^-1 (fri/mod.rs:194) and is squared after each fold.

The oracles over the folded vectors are MerkleTreeWithCap.construct_by_chunking(_from_flat_sources)
(merkle.py). For `fold` and `interpolate` the challenges are inputs. Scalar setup (challenge
powers, the coset inverse) is host arithmetic on single field elements, as in the reference's own
driver loop.

The commit phase as one call is `do_fri` (fri/mod.rs:49-357): oracle, cap into the transcript,
challenge, `fold_by` (one launch per reduction step of 2, 4 or 8, bj_fri_fold_multi_d), and at
the end `final_monomials`. Its result goes into queries.single_round_queries through
FriOracles.query_oracles.
"""
import torch

from ._lib import call
from .fft import bitreverse_enumeration_inplace, ifft_natural_to_natural
from .field import GENERATOR, P, ext2_square, log2_exact, stream_of, to_host


def compute_fri_schedule(security_bits, cap_size, pow_bits, rate_log_two, initial_degree_log_two):
    """compute_fri_schedule (prover.rs:2281-2372) -> (new_pow_bits, num_queries, schedule,
    final_degree).  PoW bits that buy no whole query are dropped; folding goes by 3 while it can,
    then by 2 or 1, down to max(1, cap_size >> rate_log_two) coefficients, and stops before a tree
    would be no larger than its cap.  ValueError where the reference asserts."""
    if security_bits <= pow_bits:
        raise ValueError("security_bits must exceed pow_bits (prover.rs:2293)")
    if rate_log_two < 1:
        raise ValueError("rate_log_two is at least 1")
    log2_exact(cap_size)
    new_pow_bits = pow_bits
    short = (security_bits - pow_bits) % rate_log_two
    if short and new_pow_bits >= rate_log_two - short:
        new_pow_bits -= rate_log_two - short        # there is no point to do so much PoW
    num_queries = -(-(security_bits - new_pow_bits) // rate_log_two)
    stop_log = log2_exact(max(1, cap_size >> rate_log_two))
    cap_log = log2_exact(cap_size)
    degree = initial_degree_log_two
    schedule = []
    while degree > stop_log and degree + rate_log_two > cap_log:
        step = min(3, degree - stop_log)
        degree -= step
        schedule.append(step)
        if step == 1:
            break
    if degree + rate_log_two < cap_log:
        raise ValueError("the last tree is smaller than the cap (prover.rs:2364)")
    return new_pow_bits, num_queries, schedule, 1 << degree


def challenge_powers(challenge, reduction_degree_log_2):
    """[alpha, alpha^2, alpha^4, ...] as fri/mod.rs:206-226 builds them for one reduction step."""
    out = [(challenge[0] % P, challenge[1] % P)]
    for _ in range(1, reduction_degree_log_2):
        out.append(ext2_square(out[-1]))
    return out


def precompute_roots(full_size, device="cuda"):
    """precompute_twiddles_for_fft::<INVERSED = true>(full_size) (fri/mod.rs:191-192)."""
    log_n = log2_exact(full_size)
    out = torch.empty((full_size // 2,), dtype=torch.int64, device=device)
    call("bj_precompute_twiddles_d", log_n, 1, out.data_ptr(), stream_of(out))
    return out


def fold(c0, c1, roots, coset_inverse, challenge):
    """One fold by 2: (N,) device columns -> (N/2,) each."""
    n = c0.shape[-1]
    if c1.shape[-1] != n or roots.shape[-1] < n // 2:
        raise ValueError("c0, c1 and roots sizes do not match")
    d0 = torch.empty((n // 2,), dtype=torch.int64, device=c0.device)
    d1 = torch.empty_like(d0)
    call("bj_fri_fold_d", c0.data_ptr(), c1.data_ptr(), n, roots.data_ptr(), coset_inverse % P, challenge[0] % P,
         challenge[1] % P, d0.data_ptr(), d1.data_ptr(), stream_of(c0))
    return d0, d1


def interpolate(c0, c1, challenges, roots, coset_inverse=None):
    """Fold len(challenges) times (interpolate_independent_cosets + interpolate_flattened_cosets).
    c0, c1: (N,) flat bit-reversed codeword columns (cosets in order). Returns
    (c0', c1', coset_inverse after the folds)."""
    ci = pow(GENERATOR, P - 2, P) if coset_inverse is None else coset_inverse % P
    for ch in challenges:
        c0, c1 = fold(c0.reshape(-1), c1.reshape(-1), roots, ci, ch)
        ci = ci * ci % P
    return c0, c1, ci


def fold_by(c0, c1, roots, coset_inverse, challenge, reduction_degree_log_2, out=None):
    """One reduction step of do_fri, a fold by 2^reduction_degree_log_2 (1..3), in one launch
    (bj_fri_fold_multi_d): what `interpolate` gives over challenge_powers(challenge, r) from
    `coset_inverse`, bit for bit, without the r - 1 intermediate vectors.  c0, c1: (N,) device
    columns; out: None or the pair (d0, d1) of (N / 2^r,) device columns to write, which must not
    overlap the sources.  Returns (d0, d1); the coset inverse of the result is
    coset_inverse^(2^r).  Nothing else is allocated and nothing synchronises, so with `out` the
    call can be captured in a graph."""
    r = int(reduction_degree_log_2)
    c0, c1 = c0.reshape(-1), c1.reshape(-1)
    n = c0.shape[0]
    if c1.shape[0] != n or roots.shape[-1] < n // 2:
        raise ValueError("c0, c1 and roots sizes do not match")
    if out is None:
        n_out = n >> r if 1 <= r <= 3 else 0
        d0 = torch.empty((n_out,), dtype=torch.int64, device=c0.device)
        d1 = torch.empty_like(d0)
    else:
        d0, d1 = out
        if 1 <= r <= 3 and (d0.numel() != n >> r or d1.numel() != n >> r):
            raise ValueError("out holds %d and %d elements, the fold gives %d" % (d0.numel(), d1.numel(), n >> r))
    call("bj_fri_fold_multi_d", c0.data_ptr(), c1.data_ptr(), n, roots.data_ptr(), coset_inverse % P,
         challenge[0] % P, challenge[1] % P, r, d0.data_ptr(), d1.data_ptr(), stream_of(c0))
    return d0, d1


def _final_halves(c0, c1, coset_inverse):
    """bit reversal + iFFT on the coset coset_inverse^-1 of copies of both halves, as one (2, len)
    tensor (fri/mod.rs:312-321)."""
    halves = torch.stack([c0.reshape(-1), c1.reshape(-1)])
    if halves.shape[1] > 1:
        bitreverse_enumeration_inplace(halves)
        ifft_natural_to_natural(halves, coset=pow(coset_inverse % P, P - 2, P))
    return halves


def _split_monomials(halves_host, lde_degree):
    length = halves_host.shape[1]
    if lde_degree < 1 or length % lde_degree:
        raise ValueError("%d values are no multiple of the lde degree %d" % (length, lde_degree))
    final_degree = length // lde_degree
    low = tuple(not halves_host[k, final_degree:].any() for k in range(2))
    return final_degree, low


def final_monomials(c0, c1, coset_inverse, lde_degree):
    """fri/mod.rs:312-343 on the last fold's result, which is left as it is: copies are bit-reversed
    and interpolated on the coset coset_inverse^-1.  Returns (m0, m1, low_degree): m* the first
    len / lde_degree coefficients of each half (device), low_degree the pair of booleans "every
    coefficient from len / lde_degree on is zero" that the reference asserts as its self-check
    (:325-334) -- reported here, not raised; reading them synchronises."""
    halves = _final_halves(c0, c1, coset_inverse)
    final_degree, low = _split_monomials(to_host(halves), lde_degree)
    return halves[0, :final_degree], halves[1, :final_degree], low


def _paired_rows(c0, c1):
    """c0, c1 (flat) as the two rows of one (2, N) tensor, which is what the tree builders and
    QueryOracle read: a view when c1 lies behind c0 in the same allocation (the rows of a (2, N)
    or (2, D, n) tensor), a stacked copy otherwise."""
    c0, c1 = c0.reshape(-1), c1.reshape(-1)
    n = c0.shape[0]
    if c1.shape[0] != n or c0.device != c1.device:
        raise ValueError("c0 and c1 differ in size or device")
    if c0.untyped_storage().data_ptr() == c1.untyped_storage().data_ptr():
        delta = c1.storage_offset() - c0.storage_offset()
        if delta >= n:
            return torch.as_strided(c0, (2, n), (delta, 1))
    return torch.stack([c0, c1])


class FriOracles:
    """do_fri's result (FriOracles, fri/mod.rs:31-47): base_oracle, the fold results
    leaf_sources_for_intermediate_oracles [(c0, c1)] (every step's, the last one included),
    intermediate_oracles and monomial_forms (two numpy uint64 arrays), plus `challenges` (the Ext2
    pair drawn per step) and `low_degree` (see final_monomials)."""

    def __init__(self, base_oracle, leaf_sources, intermediate_oracles, monomial_forms, challenges, low_degree,
                 schedule, log_n, log_lde):
        self.base_oracle = base_oracle
        self.leaf_sources_for_intermediate_oracles = leaf_sources
        self.intermediate_oracles = intermediate_oracles
        self.monomial_forms = monomial_forms
        self.challenges = challenges
        self.low_degree = low_degree
        self.schedule, self.log_n, self.log_lde = list(schedule), log_n, log_lde

    def query_oracles(self, c0, c1):
        """The queries.QueryOracle of every FRI oracle in schedule order, for
        queries.single_round_queries / construct_queries.  c0, c1: the codeword do_fri was given
        (the reference keeps no leaf sources for the base oracle either).  The shifts are
        queries.fri_plan's."""
        from .queries import QueryOracle, fri_plan
        plan = fri_plan(self.log_n, self.log_lde, self.schedule)
        trees = [self.base_oracle] + list(self.intermediate_oracles)
        sources = [_paired_rows(c0, c1)] + [_paired_rows(a, b) for a, b in
                                            self.leaf_sources_for_intermediate_oracles[:-1]]
        return [QueryOracle(t, s, e, shift) for t, s, (e, shift, _) in zip(trees, sources, plan)]


def do_fri(c0, c1, transcript, interpolation_log2s_schedule, lde_degree, cap_size, hasher="poseidon2"):
    """do_fri (fri/mod.rs:49-357) on the device.  c0, c1: the (D, n) or flat (D * n,) device columns
    of the DEEP codeword, bit-reversed cosets one after another; transcript: any object with the
    reference trait's witness_merkle_tree_cap(cap), get_challenge() and witness_field_elements(els)
    (transcript.Poseidon2Transcript is the recursive-mode one).  The reference's order: base oracle
    (construct_by_chunking, 2^schedule[0] values per leaf) -> its cap into the transcript -> two
    challenges -> fold_by; per later step the oracle over the previous result
    (construct_by_chunking_from_flat_sources) -> cap -> challenges -> fold_by; then the final
    monomials, witnessed c0 then c1.  The only host round trips are each cap, and one copy that
    brings the monomials and the low-degree flags.  Returns FriOracles.  ValueError where the
    reference asserts: a schedule entry outside 1..3, final_degree == 0.
    Outside this function: Blake2s / Keccak transcripts and hashing the next oracle's leaves inside
    the fold kernel; the schedule is `compute_fri_schedule`, and openings.prove_openings runs the
    DEEP codeword into this call and the queries out of it."""
    from .merkle import MerkleTreeWithCap
    schedule = [int(s) for s in interpolation_log2s_schedule]
    if not schedule:
        raise ValueError("the schedule is empty")
    for s in schedule:
        if not 1 <= s <= 3:
            raise ValueError("a folding step of %d is outside 1..3 (fri/mod.rs:204-205)" % s)
    rows = _paired_rows(c0, c1)
    full_size = rows.shape[1]
    log_full, log_lde = log2_exact(full_size), log2_exact(lde_degree)
    if log_lde > log_full or (full_size // lde_degree) >> sum(schedule) == 0:
        raise ValueError("final_degree is 0 (fri/mod.rs:82)")
    log_n = log_full - log_lde
    base_oracle = MerkleTreeWithCap.construct_by_chunking(rows, 1 << schedule[0], cap_size, hasher=hasher)
    roots = precompute_roots(full_size, device=rows.device)
    ci = pow(GENERATOR, P - 2, P)
    sources, oracles, challenges = [], [], []
    cur, tree = rows, base_oracle
    for k, s in enumerate(schedule):
        if k:
            tree = MerkleTreeWithCap.construct_by_chunking_from_flat_sources(cur, 1 << s, cap_size, hasher=hasher)
            oracles.append(tree)
        transcript.witness_merkle_tree_cap(tree.get_cap())
        ch = (int(transcript.get_challenge()), int(transcript.get_challenge()))
        challenges.append(ch)
        nxt = torch.empty((2, cur.shape[1] >> s), dtype=torch.int64, device=rows.device)
        fold_by(cur[0], cur[1], roots, ci, ch, s, out=(nxt[0], nxt[1]))
        ci = pow(ci, 1 << s, P)
        sources.append((nxt[0], nxt[1]))
        cur = nxt
    halves = to_host(_final_halves(cur[0], cur[1], ci))
    final_degree, low = _split_monomials(halves, lde_degree)
    m0, m1 = halves[0, :final_degree].copy(), halves[1, :final_degree].copy()
    transcript.witness_field_elements(m0)
    transcript.witness_field_elements(m1)
    return FriOracles(base_oracle, sources, oracles, [m0, m1], challenges, low, schedule, log_n, log_lde)
