"""The reference's proof of work (cs/implementations/pow.rs) restated on Python integers, the
expectation of tests/test_pow_cpu.py and tests/test_gpu_pow.py.  Blake2s256 is hashlib's, Keccak256
(domain byte 0x01) the oracle's, which tests/test_oracle_keccak.py pins to its known answers."""
import functools
import hashlib

import oracle as O

BLAKE2S, KECCAK256 = 1, 2  # BJ_HASHER_*
P = 0xFFFFFFFF00000001
NO_RESULT = (1 << 64) - 1  # pow.rs:48, 137


def digest(hasher, seed, nonce):
    """H(seed || nonce.to_le_bytes()) (pow.rs:63-64, 127-129)."""
    data = bytes(seed) + int(nonce).to_bytes(8, "little")
    if hasher == BLAKE2S:
        return hashlib.blake2s(data, digest_size=32).digest()
    if hasher == KECCAK256:
        return O.keccak256(data)
    raise ValueError("no PoW runner for hasher %r" % (hasher,))


def trailing_zeros(hasher, seed, nonce):
    """u64::from_le_bytes(digest[..8]).trailing_zeros() (pow.rs:65-67); 64 for zero."""
    v = int.from_bytes(digest(hasher, seed, nonce)[:8], "little")
    return 64 if v == 0 else (v & -v).bit_length() - 1


def passes(hasher, seed, pow_bits, nonce):
    return trailing_zeros(hasher, seed, nonce) >= pow_bits


@functools.lru_cache(maxsize=None)
def smallest_nonce(hasher, seed, pow_bits, first=0, limit=1 << 26):
    """The serial scan of pow.rs:61-70 from `first`: the smallest passing nonce in
    [first, first + limit), or NO_RESULT."""
    seed = bytes(seed)
    mask = (1 << pow_bits) - 1
    for nonce in range(first, min(first + limit, NO_RESULT)):
        if int.from_bytes(digest(hasher, seed, nonce)[:8], "little") & mask == 0:
            return nonce
    return NO_RESULT


def seed_bytes(elements):
    """pow.rs:9-13: as_u64_reduced().to_le_bytes() of every element."""
    return b"".join((int(e) % P).to_bytes(8, "little") for e in elements)


def make_seed(length, tag=0):
    """A fixed pseudo-random seed of `length` bytes."""
    return hashlib.shake_128(b"pow seed %d %d" % (length, tag)).digest(length) if length else b""
