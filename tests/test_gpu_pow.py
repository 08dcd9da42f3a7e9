"""bj_pow_search_d / bj_pow_run_h / boojum_amd.pow on the GPU against tests/pow_model.py, the
reference's serial scan (pow.rs:61-70) on hashlib's Blake2s and the oracle's Keccak256.  Every
expectation comes from the model, never from the library."""
import pytest

import pow_model as M

pytestmark = pytest.mark.gpu

HASHERS = (M.BLAKE2S, M.KECCAK256)
NO_RESULT = M.NO_RESULT
# seed lengths: the prover's 40 bytes (the kernels' fast path), the empty seed, a nonce that ends a
# Blake2s block (56), straddles two (57, 63), follows a host-absorbed prefix block (64, 100); for
# Keccak's 136-byte rate the padding in the block's last byte (127), a whole padding block (128), a
# straddling nonce (129, 135) and a prefix block (136, 200)
SEED_LENS = {M.BLAKE2S: (0, 40, 56, 57, 63, 64, 100),
             M.KECCAK256: (0, 40, 56, 57, 63, 64, 100, 127, 128, 129, 135, 136, 200)}
CASES = [(h, n) for h in HASHERS for n in SEED_LENS[h]]
# the 40-byte seed of the 16- and 20-bit cases: tag 2 has a short scan in the model for both hashers
# (2.7e5 and 4.5e5 nonces at 20 bits; the model hashes 2e5 to 8e5 nonces a second)
LONG_SEED = M.make_seed(40, 2)


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import pow as W
    boojum_amd.load()
    runners = {M.BLAKE2S: W.Blake2s256, M.KECCAK256: W.Keccak256}

    def search(hasher, seed, pow_bits, first, n, init=NO_RESULT):
        """One launch on a fresh result word; the value it leaves."""
        res = torch.tensor([init - (1 << 64) if init >= 1 << 63 else init], dtype=torch.int64, device="cuda")
        W.search(hasher, seed, pow_bits, first, n, res)
        return int(res.cpu()[0]) & ((1 << 64) - 1)

    return type("BJ", (), dict(torch=torch, W=W, runners=runners, search=staticmethod(search)))


@pytest.mark.parametrize("pow_bits", (1, 4, 8, 12))
@pytest.mark.parametrize("hasher,seed_len", CASES)
def test_smallest_nonce(bj, hasher, seed_len, pow_bits):
    seed = M.make_seed(seed_len)
    want = M.smallest_nonce(hasher, seed, pow_bits)
    assert want != NO_RESULT
    assert bj.runners[hasher].run_from_bytes(seed, pow_bits) == want


@pytest.mark.parametrize("pow_bits", (16, 20))
@pytest.mark.parametrize("hasher", HASHERS)
def test_smallest_nonce_at_the_prover_sizes(bj, hasher, pow_bits):
    """16 bits is the last size of the reference's serial scan, 20 its default (prover.rs:70)."""
    want = M.smallest_nonce(hasher, LONG_SEED, pow_bits)
    assert want != NO_RESULT
    assert bj.runners[hasher].run_from_bytes(LONG_SEED, pow_bits) == want


@pytest.mark.parametrize("pow_bits", (24, 28))
@pytest.mark.parametrize("hasher", HASHERS)
def test_validity_at_24_and_28_bits(bj, hasher, pow_bits):
    """The returned nonce passes in the model; the model cannot scan this far for minimality."""
    seed = M.make_seed(40, 7)
    nonce = bj.runners[hasher].run_from_bytes(seed, pow_bits)
    assert nonce != NO_RESULT
    assert M.passes(hasher, seed, pow_bits, nonce)
    assert M.trailing_zeros(hasher, seed, nonce) >= pow_bits


@pytest.mark.parametrize("hasher,seed_len", [(M.BLAKE2S, 40), (M.BLAKE2S, 61), (M.KECCAK256, 40), (M.KECCAK256, 131)])
def test_many_solutions_in_one_launch(bj, hasher, seed_len):
    """A quarter of all nonces pass: every wave reduces its lanes and most waves have a minimum
    to offer."""
    seed = M.make_seed(seed_len, 1)
    assert bj.search(hasher, seed, 2, 0, 1 << 16) == M.smallest_nonce(hasher, seed, 2)
    first = 12345
    assert bj.search(hasher, seed, 2, first, 1 << 16) == M.smallest_nonce(hasher, seed, 2, first)


@pytest.mark.parametrize("n_nonces", (1, 255, 257, 65537))
@pytest.mark.parametrize("hasher", HASHERS)
def test_ragged_windows(bj, hasher, n_nonces):
    """The window ends one nonce before the first that passes: lanes past its end test nothing."""
    passing = M.smallest_nonce(hasher, LONG_SEED, 20)   # nothing below it passes 20 bits
    assert passing >= n_nonces
    first = passing - n_nonces
    assert bj.search(hasher, LONG_SEED, 20, first, n_nonces) == NO_RESULT
    assert bj.search(hasher, LONG_SEED, 20, first, n_nonces + 1) == passing
    assert bj.search(hasher, LONG_SEED, 20, passing, 1) == passing


@pytest.mark.parametrize("first", ((1 << 32) - 1000, (1 << 63) + 12345, (1 << 64) - 1 - 4096))
@pytest.mark.parametrize("hasher,seed_len", [(M.BLAKE2S, 40), (M.BLAKE2S, 63), (M.KECCAK256, 40), (M.KECCAK256, 135)])
def test_the_carry_into_the_high_word(bj, hasher, seed_len, first):
    """first_nonce + offset carries into the nonce's high word inside the window (2^32 - 1000), the
    high word is not zero (>= 2^63), and the window ends at the last nonce there is, 2^64 - 2."""
    seed = M.make_seed(seed_len, 5)
    want = M.smallest_nonce(hasher, seed, 8, first, 4096)
    got = bj.search(hasher, seed, 8, first, 4096)
    assert got == want
    if first == (1 << 32) - 1000:
        # the model's first solution past the carry, from a window that starts before it
        past = M.smallest_nonce(hasher, seed, 8, 1 << 32, 4096)
        assert past != NO_RESULT and bj.search(hasher, seed, 8, 1 << 32, 4096) == past
        assert bj.search(hasher, seed, 8, (1 << 32) - 64, past - (1 << 32) + 65) == min(
            M.smallest_nonce(hasher, seed, 8, (1 << 32) - 64, 64), past)


@pytest.mark.parametrize("hasher", HASHERS)
def test_many_tiles_with_early_exit_live(bj, hasher):
    """2^22 nonces are 4096 tiles, about 2^14 of the nonces pass, and the waves that see one of
    them stop: the answer is still the window's smallest."""
    seed = M.make_seed(40, 9)
    want = M.smallest_nonce(hasher, seed, 8)
    for _ in range(3):
        assert bj.search(hasher, seed, 8, 0, 1 << 22) == want
    first = 1 << 20
    assert bj.search(hasher, seed, 8, first, 1 << 22) == M.smallest_nonce(hasher, seed, 8, first)


@pytest.mark.parametrize("hasher", HASHERS)
def test_min_combining(bj, hasher):
    seed = M.make_seed(40, 11)
    smallest = M.smallest_nonce(hasher, seed, 8)
    second = M.smallest_nonce(hasher, seed, 8, smallest + 1)
    assert smallest < second != NO_RESULT
    # pre-set below every solution of the window: unchanged (a passing or a failing value alike)
    assert bj.search(hasher, seed, 8, smallest + 1, 1 << 16, init=smallest) == smallest
    assert bj.search(hasher, seed, 8, 0, 1 << 16, init=0) == 0
    # pre-set above: replaced by the window's minimum
    assert bj.search(hasher, seed, 8, 0, 1 << 16, init=second) == smallest
    assert bj.search(hasher, seed, 8, 0, 1 << 16, init=NO_RESULT - 1) == smallest
    # pre-set between two solutions of the window
    assert bj.search(hasher, seed, 8, smallest + 1, 1 << 16, init=second + 1) == second


@pytest.mark.parametrize("hasher", HASHERS)
def test_the_window_start_is_honoured(bj, hasher):
    seed = M.make_seed(40, 13)
    smallest = M.smallest_nonce(hasher, seed, 10)
    nxt = M.smallest_nonce(hasher, seed, 10, smallest + 1)
    assert nxt != NO_RESULT
    assert bj.search(hasher, seed, 10, smallest + 1, 1 << 16) == nxt
    assert bj.search(hasher, seed, 10, smallest, 1 << 16) == smallest


@pytest.mark.parametrize("hasher", HASHERS)
def test_run_from_field_elements(bj, hasher):
    """Five elements (NUM_POW_CHALLENGES), one of them >= p: the seed is the canonical bytes."""
    elements = [0x1122334455667788, M.P + 3, 0, M.P - 1, 0xDEADBEEF]
    canonical = [0x1122334455667788, 3, 0, M.P - 1, 0xDEADBEEF]
    assert len(elements) == bj.W.NUM_POW_CHALLENGES
    seed = M.seed_bytes(canonical)
    want = M.smallest_nonce(hasher, seed, 12)
    runner = bj.runners[hasher]
    assert runner.run_from_field_elements(elements, 12) == want
    assert runner.run_from_field_elements(canonical, 12) == want
    assert runner.verify_from_field_elements(elements, 12, want)
    assert bj.W.pow_challenge_to_field_elements(want) == (want & 0xFFFFFFFF, want >> 32)
