"""GoldilocksPoisedon2Transcript (cs/implementations/transcript.rs:48-151): the recursive-mode
transcript, AlgebraicSpongeBasedTranscript<GoldilocksField, 8, 12, 4, Poseidon2Goldilocks,
AbsorptionModeOverwrite>, over the library's Poseidon2 permutation
(merkle.Poseidon2Sponge.poseidon2_permutation, bj_poseidon2_permute_h).

The 12-word state lives on the host and every round function is one call of the host seam (a
single permutation on the device): a transcript absorbs a few caps and field elements per proof,
and what it feeds on (caps, evaluations, the final FRI monomials) is already on the host when it
is witnessed.  fri.do_fri takes any object with these three methods.

`BoolsBuffer` (transcript.rs:369-417) draws the query indices' bits from it.

Not here: the Blake2s and Keccak transcripts (transcript.rs:153-367), and with them BoolsBuffer's
byte branch.
"""
from .field import P
from .merkle import Poseidon2Sponge

RATE = 8        # AW
WIDTH = 12      # SW
CAPACITY = 4    # CW, the words of a cap element


class Poseidon2Transcript:
    """Transcript<GoldilocksField>: witness_field_elements, witness_merkle_tree_cap, get_challenge.
    Elements are buffered until a challenge is asked for; then the buffer is padded with ONE and
    zeros to a multiple of 8 and absorbed in Overwrite mode (each chunk of 8 replaces state[..8],
    then one permutation; sponge.rs:241-283), and state[..8] becomes the 8 available challenges
    (finalize with nothing pending, :300-323).  When they run out and nothing was witnessed in
    between, one more round function gives the next 8 (:287-298)."""

    def __init__(self):
        self.buffer = []
        self.available_challenges = []
        self.state = [0] * WIDTH

    def _round_function(self):
        self.state = [int(x) for x in Poseidon2Sponge.poseidon2_permutation(self.state)]

    def witness_field_elements(self, field_els):
        self.buffer.extend(int(e) % P for e in field_els)

    def witness_merkle_tree_cap(self, cap):
        for el in cap:
            self.witness_field_elements(el)

    def get_challenge(self):
        while True:
            if self.buffer:
                to_absorb, self.buffer = self.buffer + [1], []      # rescue-prime padding
                to_absorb += [0] * (-len(to_absorb) % RATE)
                for at in range(0, len(to_absorb), RATE):
                    self.state[:RATE] = to_absorb[at:at + RATE]
                    self._round_function()
                self.available_challenges = self.state[:RATE]
            elif not self.available_challenges:
                self._round_function()
                self.available_challenges = self.state[:RATE]
            else:
                return self.available_challenges.pop(0)

    def get_multiple_challenges(self, n):
        return [self.get_challenge() for _ in range(n)]


class BoolsBuffer:
    """BoolsBuffer (transcript.rs:369-417), the branch of an algebraic transcript: when fewer bits
    are left than asked for, one more challenge gives its 64 - max_needed least significant bits
    (of the reduced u64, lowest first), appended to what is left."""

    def __init__(self, max_needed):
        if not 0 <= max_needed <= 64:
            raise ValueError("max_needed outside 0..64")
        self.available = []
        self.max_needed = max_needed

    def get_bits(self, transcript, num_bits):
        while len(self.available) < num_bits:
            if self.max_needed == 64:
                raise ValueError("a challenge gives no bits with max_needed = 64")
            el = int(transcript.get_challenge()) % P
            self.available += [bool((el >> i) & 1) for i in range(64 - self.max_needed)]
        give, self.available = self.available[:num_bits], self.available[num_bits:]
        return give


def u64_from_lsb_first_bits(bits):
    """The integer whose bit i is bits[i] (prover.rs:2272-2279)."""
    return sum(int(b) << i for i, b in enumerate(bits))
