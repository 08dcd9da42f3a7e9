"""Proof-of-work grinding (cs/implementations/pow.rs, prover.rs:2107-2133) on the GPU.

After the last FRI oracle the prover draws NUM_POW_CHALLENGES field elements from the transcript,
lays them out as 40 seed bytes and looks for a nonce with

    u64::from_le_bytes(H(seed || nonce.to_le_bytes())[..8]).trailing_zeros() >= pow_bits,

H = Blake2s256 or Keccak256 (rate 136, domain byte 0x01).  The runners here keep the reference's
names and always return the smallest passing nonce: the reference's serial scan for pow_bits <= 16
(pow.rs:58-71) and one of the answers its race may give above that (pow.rs:76-119).

* `Blake2s256`, `Keccak256`, `NoPow`: the `PoWRunner` impls (`run_from_field_elements`,
  `run_from_bytes`, `verify_from_field_elements`, `verify_from_bytes`).
* `search`: one launch of bj_pow_search_d over a window of nonces, asynchronous.
* `pow_challenge_to_field_elements`: what the prover feeds back to the transcript.

The transcript itself is outside this path; the seed is an argument, as the FRI challenges are in
fri.py.  Verification is host code of the library (bj_pow_verify_h) and needs no GPU.
"""
import ctypes

from ._lib import call, load
from .field import P

# prover.rs:2115-2118: num_challenges = 256 / F::CHAR_BITS = 4, and `if num_challenges %
# F::CHAR_BITS != 0 { num_challenges += 1 }` tests 4 % 64, not 256 % 64, so it is always 5
NUM_POW_CHALLENGES = 256 // 64 + (1 if (256 // 64) % 64 != 0 else 0)

NO_RESULT = (1 << 64) - 1        # BJ_POW_NO_RESULT (pow.rs:48, 137)
HASHER_BLAKE2S, HASHER_KECCAK256 = 1, 2   # BJ_HASHER_*


def seed_from_field_elements(seed):
    """pow.rs:9-13: every element as_u64_reduced().to_le_bytes(), concatenated."""
    return b"".join((int(el) % P).to_bytes(8, "little") for el in seed)


def pow_challenge_to_field_elements(nonce):
    """prover.rs:2122-2126: (low, high) = (nonce as u32, (nonce >> 32) as u32), the two field
    elements the prover witnesses to the transcript after the search."""
    return nonce & 0xFFFFFFFF, (nonce >> 32) & 0xFFFFFFFF


def search(hasher, seed, pow_bits, first_nonce, n_nonces, result):
    """bj_pow_search_d on the current stream of `result`'s device: result[0] = min(result[0], the
    smallest passing nonce of [first_nonce, first_nonce + n_nonces)).  `result` is a one-element
    uint64 (or int64) CUDA tensor the caller initialises (NO_RESULT for a fresh search).
    Asynchronous: nothing is allocated or synchronised."""
    import torch
    from .field import stream_of
    if not isinstance(result, torch.Tensor) or not result.is_cuda or result.numel() != 1 or \
            result.dtype not in (torch.uint64, torch.int64):
        raise TypeError("result must be a one-element uint64 CUDA tensor")
    seed = bytes(seed)
    call("bj_pow_search_d", hasher, seed, len(seed), pow_bits, first_nonce, n_nonces, result.data_ptr(),
         stream_of(result))


class PoWRunner:
    """pow.rs:7-32.  Subclasses set HASHER (a BJ_HASHER_* value)."""
    HASHER = None

    @classmethod
    def run_from_field_elements(cls, seed, pow_bits):
        return cls.run_from_bytes(seed_from_field_elements(seed), pow_bits)

    @classmethod
    def verify_from_field_elements(cls, seed, pow_bits, challenge):
        return cls.verify_from_bytes(seed_from_field_elements(seed), pow_bits, challenge)

    @classmethod
    def run_from_bytes(cls, seed, pow_bits):
        """The smallest passing nonce (bj_pow_run_h); NO_RESULT if none below 2^64 - 1 passes."""
        seed = bytes(seed)
        out = ctypes.c_uint64(0)
        call("bj_pow_run_h", cls.HASHER, seed, len(seed), pow_bits, ctypes.byref(out))
        return out.value

    @classmethod
    def verify_from_bytes(cls, seed, pow_bits, challenge):
        seed = bytes(seed)
        rc = load().bj_pow_verify_h(cls.HASHER, seed, len(seed), pow_bits, challenge)
        if rc < 0:
            from ._lib import check
            check(rc, "bj_pow_verify_h")
        return rc == 1


class Blake2s256(PoWRunner):
    """pow.rs:51-135: the runner of the non-recursive prover."""
    HASHER = HASHER_BLAKE2S


class Keccak256(PoWRunner):
    """pow.rs:137-221."""
    HASHER = HASHER_KECCAK256


class NoPow(PoWRunner):
    """pow.rs:34-46: asserts pow_bits == 0.  With pow_bits == 0 the prover never calls a runner
    and writes pow_challenge = 0 (prover.rs:2109, 2133); here run returns that 0 and verify holds."""

    @classmethod
    def run_from_bytes(cls, seed, pow_bits):
        if pow_bits != 0:
            raise ValueError("NoPow with pow_bits = %d (pow.rs:38)" % pow_bits)
        return 0

    @classmethod
    def verify_from_bytes(cls, seed, pow_bits, challenge):
        if pow_bits != 0:
            raise ValueError("NoPow with pow_bits = %d (pow.rs:43)" % pow_bits)
        return True
