"""The host side of the proof of work (boojum_amd.pow, bj_pow_verify_h and the argument checks of
bj_pow_search_d / bj_pow_run_h) against tests/pow_model.py.  bj_pow_verify_h is host code of the
library: the midstate over the seed's full blocks, the tail block(s) and the shared predicate run
on the CPU exactly as the kernels run them, so every block-boundary case is checked here without
a GPU."""
import ctypes

import pytest

import pow_model as M

P = M.P
BJ_EINVAL = -22
NONCES = (0, 1, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2)
HASHERS = (M.BLAKE2S, M.KECCAK256)


@pytest.fixture(scope="module")
def lib():
    import boojum_amd
    return boojum_amd.load()


def test_module_is_exported():
    import boojum_amd
    from boojum_amd import pow as W
    assert "pow" in boojum_amd.__all__
    for name in ("PoWRunner", "Blake2s256", "Keccak256", "NoPow", "search", "NUM_POW_CHALLENGES",
                 "pow_challenge_to_field_elements"):
        assert hasattr(W, name), name
    for name in ("run_from_field_elements", "run_from_bytes", "verify_from_field_elements", "verify_from_bytes"):
        assert hasattr(W.PoWRunner, name), name


@pytest.mark.parametrize("hasher", HASHERS)
def test_verify_matches_the_model_at_every_seed_length(lib, hasher):
    """seed_len 0..280 crosses, for Blake2s (64-byte blocks), a nonce inside one block, ending a
    block (mod 64 == 56), straddling two (57..63) and starting one (0) after 0..4 prefix blocks;
    for Keccak (136-byte rate) the same with the padding in the nonce's block, in the last byte
    (mod 136 == 127), a whole padding block (128) and a straddling nonce (129..135)."""
    for seed_len in range(281):
        seed = M.make_seed(seed_len)
        for nonce in NONCES:
            tz = M.trailing_zeros(hasher, seed, nonce)
            for pow_bits in range(33):
                got = lib.bj_pow_verify_h(hasher, seed, seed_len, pow_bits, nonce)
                assert got == (1 if tz >= pow_bits else 0), (seed_len, nonce, pow_bits, tz)


@pytest.mark.parametrize("hasher", HASHERS)
def test_verify_accepts_and_rejects_at_32_bits(lib, hasher):
    """pow_bits = 0 always passes; pow_bits = 32 fails on a digest whose first word is not zero,
    and the mask has no shift by 32 in it: a first word of 0x80000000 passes 31 bits, not 32."""
    seed = M.make_seed(40)
    for nonce in range(64):
        tz = M.trailing_zeros(hasher, seed, nonce)
        assert lib.bj_pow_verify_h(hasher, seed, 40, 0, nonce) == 1
        assert lib.bj_pow_verify_h(hasher, seed, 40, 32, nonce) == (1 if tz >= 32 else 0)
        assert lib.bj_pow_verify_h(hasher, seed, 40, min(tz, 32), nonce) == 1
        if tz < 32:
            assert lib.bj_pow_verify_h(hasher, seed, 40, tz + 1, nonce) == 0


def test_python_runners_verify(lib):
    from boojum_amd import pow as W
    for cls, hasher in ((W.Blake2s256, M.BLAKE2S), (W.Keccak256, M.KECCAK256)):
        seed = M.make_seed(40, 3)
        nonce = M.smallest_nonce(hasher, seed, 8)
        assert cls.verify_from_bytes(seed, 8, nonce) is True
        assert all(cls.verify_from_bytes(seed, 8, k) is False for k in range(nonce))
        assert cls.verify_from_bytes(bytearray(seed), 8, nonce) is True


def test_verify_from_field_elements(lib):
    """pow.rs:18-30: elements are reduced, then 8 little-endian bytes each."""
    from boojum_amd import pow as W
    canonical = [1, 0x0102030405060708, P - 1, 0, 0xFFFFFFFE]
    shifted = [1 + P, 0x0102030405060708, P - 1, P, 0xFFFFFFFE + P]   # three of them >= p, all < 2^64
    assert all(v < 1 << 64 for v in shifted)
    seed = M.seed_bytes(canonical)
    assert len(seed) == 40 and seed[8:16] == bytes([8, 7, 6, 5, 4, 3, 2, 1])
    assert W.seed_from_field_elements(canonical) == seed == W.seed_from_field_elements(shifted)
    for cls, hasher in ((W.Blake2s256, M.BLAKE2S), (W.Keccak256, M.KECCAK256)):
        nonce = M.smallest_nonce(hasher, seed, 6)
        for elements in (canonical, shifted):
            assert cls.verify_from_field_elements(elements, 6, nonce) is True
            if nonce:  # the model's nonce is the smallest, so the one before it fails
                assert cls.verify_from_field_elements(elements, 6, nonce - 1) is False
        # the bytes of the unreduced values are another seed
        raw = b"".join(v.to_bytes(8, "little") for v in shifted)
        assert raw != seed


def test_constants_and_challenge_split():
    from boojum_amd import pow as W
    assert W.NUM_POW_CHALLENGES == 5
    assert W.pow_challenge_to_field_elements(0xAABBCCDD_11223344) == (0x11223344, 0xAABBCCDD)
    assert W.pow_challenge_to_field_elements(0) == (0, 0)
    assert W.NO_RESULT == (1 << 64) - 1


def test_no_pow():
    from boojum_amd import pow as W
    assert W.NoPow.run_from_bytes(b"seed", 0) == 0
    assert W.NoPow.run_from_field_elements([1, 2, 3, 4, 5], 0) == 0
    assert W.NoPow.verify_from_bytes(b"seed", 0, 0) is True
    with pytest.raises(ValueError):
        W.NoPow.run_from_bytes(b"seed", 1)
    with pytest.raises(ValueError):
        W.NoPow.verify_from_bytes(b"seed", 20, 0)
    with pytest.raises(ValueError):
        W.NoPow.run_from_field_elements([1, 2, 3, 4, 5], 20)


def test_argument_errors(lib):
    """Every check comes before the first device call, so these run without a GPU.  result_d is
    never dereferenced by a call that fails its checks."""
    seed = M.make_seed(40)
    out = ctypes.c_uint64(123)
    res = ctypes.c_void_p(0x1000)  # a non-null placeholder: the call must fail before it launches

    def einval(rc, word):
        assert rc == BJ_EINVAL
        msg = lib.bj_last_error().decode()
        assert word in msg, msg

    for hasher in HASHERS:
        einval(lib.bj_pow_verify_h(hasher, seed, 40, 33, 0), "pow_bits")
        einval(lib.bj_pow_run_h(hasher, seed, 40, 33, ctypes.byref(out)), "pow_bits")
        einval(lib.bj_pow_search_d(hasher, seed, 40, 33, 0, 16, res, None), "pow_bits")
        einval(lib.bj_pow_search_d(hasher, seed, 40, 8, 0, 0, res, None), "n_nonces")
        einval(lib.bj_pow_search_d(hasher, seed, 40, 8, (1 << 64) - 16, 16, res, None), "overflow")
        einval(lib.bj_pow_search_d(hasher, seed, 40, 8, 1, (1 << 64) - 1, res, None), "overflow")
        einval(lib.bj_pow_search_d(hasher, None, 5, 8, 0, 16, res, None), "null seed")
        einval(lib.bj_pow_verify_h(hasher, None, 5, 8, 0), "null seed")
        einval(lib.bj_pow_run_h(hasher, None, 5, 8, ctypes.byref(out)), "null seed")
        einval(lib.bj_pow_search_d(hasher, seed, 40, 8, 0, 16, None, None), "result_d")
        einval(lib.bj_pow_run_h(hasher, seed, 40, 8, None), "nonce_out")
    for hasher in (0, 7):  # BJ_HASHER_POSEIDON2 (the reference has no such runner) and an unknown one
        einval(lib.bj_pow_verify_h(hasher, seed, 40, 8, 0), "hasher" if hasher else "Poseidon2")
        einval(lib.bj_pow_run_h(hasher, seed, 40, 8, ctypes.byref(out)), "hasher" if hasher else "Poseidon2")
        einval(lib.bj_pow_search_d(hasher, seed, 40, 8, 0, 16, res, None), "hasher" if hasher else "Poseidon2")
    assert out.value == 123
    # a null seed of length 0 is the empty seed
    assert lib.bj_pow_verify_h(M.BLAKE2S, None, 0, 0, 5) == 1


def test_run_with_zero_bits_needs_no_device(lib):
    """bj_pow_run_h with pow_bits == 0 returns nonce 0 without a launch."""
    from boojum_amd import pow as W
    for cls in (W.Blake2s256, W.Keccak256):
        assert cls.run_from_bytes(M.make_seed(40), 0) == 0
        assert cls.run_from_field_elements([1, 2, 3, 4, P + 5], 0) == 0
