"""The lazy S-box hand-off of the Poseidon2 full rounds, executed on the CPU (no GPU).

tools/gen_gl_asm.py emits glasm::mul_lazy_x4: a Goldilocks product that stops once its partial
products are combined and hands the external MDS two 64-bit limbs, with
    Lin + Hin 2^32 - LAZY_OFF == a b (mod p),   Lin < 3 * 2^32,   Hin < 2^33
for any u64 a, b.  csrc/poseidon2.hpp runs the MDS on those limbs, takes the offset out in the
next round's one constant add (or, where no constant follows, as a small add into each limb)
and reduces.  This file interprets the committed header's asm text with the interpreter of
tests/test_mi_layers_asm.py, extended by the carry-chain instructions the products use; a carry
written to the sink operand (never read) must be zero, so no discarded intermediate exceeds its
register.  Chained as `permute` chains the blocks, the full rounds must give the reference
permutation's values (tests/test_poseidon2_sched.py) on its known answers, on random states
and on all-ones words, with the limb bounds stated in poseidon2.hpp.
"""
import random
import re

import pytest

from test_mi_layers_asm import FN, Lane, M32, M64, device_partial_rounds
from test_poseidon2_sched import M4, P, RC, RC26, reference_permutation

EPS = M32
LAZY_OFF = 2 * EPS
SINK = "q64"  # the generator's JUNK pair s[64:65] as a compiler operand
FULL_RC_BOUND = 2 ** 64 - 2 ** 41
LIMB_RC_BOUND = 2 ** 63 + 2 ** 62
LAZY = sorted(n for n in FN if n.startswith("mul_lazy_x"))


class CarryLane(Lane):
    """Lane plus v_addc / v_subb / v_not / v_mov and carry-outs of v_mad_u64_u32."""

    def _carry_out(self, c, bit, ins):
        name = c[2:-1]
        if name == SINK:
            assert bit == 0, "a discarded carry is set: " + ins
        self.op[name] = bit

    def run(self, instrs):
        for ins in instrs:
            mn, _, rest = ins.partition(" ")
            a = [x.strip() for x in rest.split(",")] if rest else []
            if mn == "v_mad_u64_u32":
                d, c, x, y, s = a
                r = self.get32(x) * self.get32(y) + self.get64(s)
                self._carry_out(c, r >> 64, ins)
                self.set64(d, r & M64)
            elif mn == "v_add_co_u32":
                d, c, x, y = a
                r = self.get32(x) + self.get32(y)
                self.set32(d, r)
                self._carry_out(c, r >> 32, ins)
            elif mn == "v_addc_co_u32":
                d, c, x, y, ci = a
                r = self.get32(x) + self.get32(y) + self.op[ci[2:-1]]
                self.set32(d, r)
                self._carry_out(c, r >> 32, ins)
            elif mn == "v_subb_co_u32":
                d, c, x, y, ci = a
                r = self.get32(x) - self.get32(y) - self.op[ci[2:-1]]
                self.set32(d, r)
                self._carry_out(c, 1 if r < 0 else 0, ins)
            elif mn == "v_not_b32":
                self.set32(a[0], ~self.get32(a[1]))
            elif mn == "v_mov_b32":
                self.set32(a[0], self.get32(a[1]))
            else:
                Lane.run(self, [ins])


def call(name, **operands):
    lane = CarryLane(operands)
    lane.run(FN[name])
    return lane.op


def mul_lazy(name, pairs):
    """The block `name` on its n operand pairs -> [(Lin, Hin)]."""
    ops = {}
    for k, (a, b) in enumerate(pairs):
        ops.update({"a0%d" % k: a & M32, "a1%d" % k: a >> 32, "b0%d" % k: b & M32, "b1%d" % k: b >> 32})
    r = call(name, **ops)
    return [(r["Lin%d" % k], r["Hin%d" % k]) for k in range(len(pairs))]


def mul4(xs, ys):
    ops = {}
    for k, (a, b) in enumerate(zip(xs, ys)):
        ops.update({"a0%d" % k: a & M32, "a1%d" % k: a >> 32, "b0%d" % k: b & M32, "b1%d" % k: b >> 32})
    r = call("mul_x4", **ops)
    return [r["z0%d" % k] | (r["z1%d" % k] << 32) for k in range(4)]


def reduce4(L, H):
    ops = {}
    for k in range(4):
        ops.update({"L%d" % k: L[k], "Hlo%d" % k: H[k] & M32, "Hhi%d" % k: H[k] >> 32})
    r = call("reduce_x4", **ops)
    return [r["z%d" % k] for k in range(4)]


EDGES = [0, 1, 2 ** 32 - 1, 2 ** 32, P - 1, P, 2 ** 64 - 1]


def _pairs():
    rng = random.Random(11)
    out = [(a, b) for a in EDGES for b in EDGES]
    out += [(rng.randrange(2 ** 64), rng.randrange(2 ** 64)) for _ in range(4000)]
    # operands with extreme words: the carries and the complemented words at their ends
    words = [0, 1, M32 - 1, M32]
    out += [(rng.choice(words) | rng.choice(words) << 32, rng.choice(words) | rng.choice(words) << 32)
            for _ in range(400)]
    return out


def test_lazy_blocks_present():
    assert "mul_lazy_x4" in LAZY


@pytest.mark.parametrize("name", LAZY)
def test_lazy_product_identity_and_bounds(name):
    n = int(re.fullmatch(r"mul_lazy_x(\d+)", name).group(1))
    pairs = _pairs()
    pairs += pairs[:(-len(pairs)) % n]
    for g in range(0, len(pairs), n):
        grp = pairs[g:g + n]
        for (a, b), (lin, hin) in zip(grp, mul_lazy(name, grp)):
            assert (lin + (hin << 32) - LAZY_OFF - a * b) % P == 0, (hex(a), hex(b))
            assert lin < 3 * 2 ** 32 and hin < 2 ** 33, (hex(a), hex(b))


# ---- the full rounds as poseidon2.hpp chains them ----

def _me_matrix():
    return [[(2 if i // 4 == j // 4 else 1) * M4[i % 4][j % 4] for j in range(12)] for i in range(12)]


ME = _me_matrix()
ROW_SUM = [sum(r) for r in ME]


def lazy_off(i):
    return ROW_SUM[i] * LAZY_OFF


def test_offsets_and_constants():
    """The header's compile-time facts, restated: row sums 64 / 48, every constant a lazy round
    takes at least its offset and below the one-add bound, the two-limb form of -offset."""
    assert ROW_SUM == [64, 48] * 6
    for r in (1, 2, 3, 27, 28, 29):
        for i in range(12):
            assert lazy_off(i) <= RC[r][i] and RC[r][i] - lazy_off(i) < FULL_RC_BOUND
    assert lazy_off(0) <= RC[4][0] < FULL_RC_BOUND
    for i in range(12):
        lo, hi = 1 + 2 * ROW_SUM[i], EPS - 2 * ROW_SUM[i]
        assert lo + (hi << 32) + lazy_off(i) == P
    # the reduction's W = Hhi EPS + L + c < 2^64 with the limbs' bounds after a lazy MDS
    assert (2 ** 39 >> 32) * EPS + 2 ** 40 + FULL_RC_BOUND <= 2 ** 64


def me_limbs(X):
    out = [sum(c * x for c, x in zip(row, X)) for row in ME]
    assert max(out) <= M64
    return out


def full_round(L, H, consts, track):
    """reduce(L + c, H); x^7 with the last product lazy; M_E on its limbs."""
    if consts is not None:
        L = [l + c for l, c in zip(L, consts)]
    z = []
    for q in range(3):
        z += reduce4(L[4 * q:4 * q + 4], H[4 * q:4 * q + 4])
    Lin, Hin = [], []
    for q in range(3):
        x = z[4 * q:4 * q + 4]
        x2 = mul4(x, x)
        x3 = mul4(x2, x)
        x4 = mul4(x2, x2)
        for lin, hin in mul_lazy("mul_lazy_x4", list(zip(x3, x4))):
            Lin.append(lin)
            Hin.append(hin)
    L, H = me_limbs(Lin), me_limbs(Hin)
    track["L"] = max(track.get("L", 0), max(L))
    track["H"] = max(track.get("H", 0), max(H))
    return L, H


def lazy_fix(L, H, idx):
    L, H = list(L), list(H)
    for i in idx:
        L[i] += 1 + 2 * ROW_SUM[i]
        H[i] += EPS - 2 * ROW_SUM[i]
    return L, H


def rcl(r):
    return [RC[r][i] - (lazy_off(i) if r in (1, 2, 3, 27, 28, 29) else 0) for i in range(12)]


def device_permutation(x, track=None):
    """poseidon2.hpp permute<OUT_ALL> on 12 u64 words (any representatives)."""
    track = {} if track is None else track
    L, H = me_limbs([v & M32 for v in x]), me_limbs([v >> 32 for v in x])
    for r in range(4):
        L, H = full_round(L, H, rcl(r), track)
    L[0] += RC[4][0] - lazy_off(0)
    L, H = lazy_fix(L, H, range(1, 12))
    z = []
    for q in range(3):
        z += reduce4(L[4 * q:4 * q + 4], H[4 * q:4 * q + 4])
    _, Lo, Ho = device_partial_rounds(z)
    L, H = [Lo[i] for i in range(12)], [Ho[i] for i in range(12)]
    for i in range(12):
        if RC26[i] < LIMB_RC_BOUND:
            L[i] += RC26[i]
        else:
            L[i] += RC26[i] & M32
            H[i] += RC26[i] >> 32
    L, H = full_round(L, H, None, track)
    for r in range(27, 30):
        L, H = full_round(L, H, rcl(r), track)
    L, H = lazy_fix(L, H, range(12))
    z = []
    for q in range(3):
        z += reduce4(L[4 * q:4 * q + 4], H[4 * q:4 * q + 4])
    return [v % P for v in z]


def test_chained_rounds_known_answers():
    assert [hex(v) for v in device_permutation(list(range(12)))[:4]] == [
        "0x5d82c16b87f07f98", "0x3655af22bb2f037d", "0x82c1535dfb4bdf90", "0x4d318cfdafd2378e"]
    assert [hex(v) for v in device_permutation([0] * 12)[:4]] == [
        "0x78e86c27e831c353", "0xc4c13a505ffd93b8", "0xc3a6d7d7f7971adc", "0xf6ff8f53ab94d8c7"]


def test_chained_rounds_equal_reference():
    rng = random.Random(3)
    track = {}
    states = [[P - 1] * 12, [M64] * 12, [M32] * 12, [M32 << 32] * 12, [1] + [0] * 11]
    states += [[rng.randrange(2 ** 64) for _ in range(12)] for _ in range(12)]
    for x in states:
        assert device_permutation(x, track) == reference_permutation([v % P for v in x])
    assert track["L"] < 2 ** 40 and track["H"] < 2 ** 39


def test_limb_bounds_after_mds_at_all_ones():
    """The largest limbs mul_lazy can hand on (every word of Lin's three terms and Hin's two at
    2^32 - 1) through M_E: below the bounds the one-add constant form relies on."""
    L = me_limbs([3 * EPS] * 12)
    H = me_limbs([2 * EPS] * 12)
    assert max(L) < 2 ** 40 and max(H) < 2 ** 39
    assert ((max(H) + EPS) >> 32) * EPS + max(L) + FULL_RC_BOUND < 2 ** 64
