"""Witness materialisation without a GPU: the integer model itself (tests/witness_model.py), the
host-side previous-occurrence map of boojum_amd.witness against the model's chain of swaps, the wire
formats, and the argument errors the library raises before it touches a device."""
import ctypes
import io
import struct

import numpy as np
import pytest

import witness_model as W

from boojum_amd import BoojumError, serialization as ser, witness
from boojum_amd import _lib

P = W.P
PH = W.PH


def identity_index(n_cols, log_n):
    """identity value -> flat cell; the values are distinct (cosets of distinct non-residues)."""
    n = 1 << log_n
    ident = W.identity_polys(n_cols, log_n)
    index = {ident[c][r]: c * n + r for c in range(n_cols) for r in range(n)}
    assert len(index) == n_cols * n
    return ident, index


def hints():
    """(name, maps, log_n): random hints with placeholders and single-use variables, one with a
    variable that fills a whole column, one of placeholders only, one where every cell is index 0."""
    out = [("random-5x64", W.random_maps(5, 64, 40, seed=1), 6),
           ("sparse-vars-3x32", W.random_maps(3, 32, 500, seed=2), 5),   # most variables used once
           ("one-column", W.random_maps(1, 16, 5, seed=3), 4)]
    m = W.random_maps(4, 32, 20, seed=4)
    m[2, :] = 7                                                           # a variable fills column 2 ...
    m[0, 3] = 7                                                           # ... and is used before it
    m[3, 31] = 7                                                          # ... and after it
    out.append(("whole-column", m, 5))
    out.append(("placeholders-only", np.full((2, 8), PH, dtype=np.uint64), 3))
    out.append(("all-index-0", np.zeros((3, 8), dtype=np.uint64), 3))
    m = W.random_maps(2, 8, 6, seed=5, placeholders=0.0)
    m[0, 0] = 0                                                           # index 0 first, and again later
    m[1, 5] = 0
    out.append(("index-0", m, 3))
    return out


HINTS = hints()
IDS = [h[0] for h in HINTS]


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("name,maps,log_n", HINTS, ids=IDS)
def test_sigma_model_is_a_permutation_whose_cycles_are_the_occurrence_sets(name, maps, log_n):
    n_cols, n = maps.shape
    ident, index = identity_index(n_cols, log_n)
    sigma = W.create_permutation_polys(maps, log_n)
    flat = [v for col in sigma for v in col]
    assert sorted(flat) == sorted(index)            # a permutation of the identity values
    image = [index[v] for v in flat]                # cell -> the cell whose identity value it holds
    seen, cycles = set(), []
    for start in range(n_cols * n):
        if start in seen:
            continue
        cycle, cell = set(), start
        while cell not in cycle:
            cycle.add(cell)
            cell = image[cell]
        seen |= cycle
        cycles.append(frozenset(cycle))
    want = {frozenset(s) for s in W.occurrence_sets(maps).values()}
    want |= {frozenset([c * n + r]) for c in range(n_cols) for r in range(n) if W.is_placeholder(maps[c][r])}
    assert set(cycles) == want


def test_copy_model():
    maps = [[3, PH, 0, 3 | 1 << 62], [PH, 1, 2, 2]]
    values = [10, 11, P, (1 << 64) - 1]
    assert W.copy_columns(maps, values) == [[(1 << 64) - 1, 0, 10, (1 << 64) - 1], [0, 11, P, P]]
    assert W.multiplicities_column([5, 0, 2 ** 32 - 1], 4) == [5, 0, 2 ** 32 - 1, 0]
    assert W.public_inputs([(1, 2), (0, 0)], [[1, 2, 3], [4, 5, 6]]) == ([6, 1], [(1, 2, 6), (0, 0, 1)])


# ------------------------------------------------------------------ prev_map against the model
@pytest.mark.parametrize("name,maps,log_n", HINTS, ids=IDS)
def test_prev_map_matches_the_swap_chain(name, maps, log_n):
    n_cols, n = maps.shape
    ident, _ = identity_index(n_cols, log_n)
    prev = witness.prev_map(maps)
    assert prev.dtype == np.uint32 and prev.shape == (n_cols, n)
    got = [[ident[int(s) // n][int(s) % n] for s in col] for col in prev]
    assert got == W.create_permutation_polys(maps, log_n)


def test_prev_map_rules():
    maps = np.array([[4, PH, 9, 4], [9, 4, PH, 2]], dtype=np.uint64)
    #       cells:    0   1  2  3     4  5   6  7
    # 4 at cells 0, 3, 5: 0 <- 5 (the last), 3 <- 0, 5 <- 3; 9 at 2, 4: 2 <- 4, 4 <- 2; 2 once; 1, 6 placeholders
    assert witness.prev_map(maps).reshape(-1).tolist() == [5, 1, 4, 0, 2, 3, 6, 7]
    assert witness.prev_map(witness.DenseVariablesCopyHint(maps.tolist())).tolist() == witness.prev_map(maps).tolist()


def test_prev_map_ignores_the_bits_above_the_index():
    maps = np.array([[5, 5 | 1 << 62, 5 | 1 << 50, PH | 5]], dtype=np.uint64)
    assert witness.prev_map(maps).tolist() == [[2, 0, 1, 3]]


# ------------------------------------------------------------------ wire formats
def test_witness_vec_byte_layout():
    wv = witness.WitnessVec([(2, 7), (0, 1)], np.array([1, P, (1 << 64) - 1], dtype=np.uint64),
                            np.array([3, 2 ** 32 - 1], dtype=np.uint32))
    f = io.BytesIO()
    ser.write_witness_vec(f, wv)
    want = struct.pack("<Q", 2) + struct.pack("<QQQQ", 2, 7, 0, 1)        # write_vec_into_buffer of (usize, usize)
    want += struct.pack("<Q", 3) + struct.pack("<QQQ", 1, P, (1 << 64) - 1)  # Vec<F>, words as they are
    want += struct.pack("<Q", 2) + struct.pack("<II", 3, 2 ** 32 - 1)     # the u32 counts, 4 bytes each
    assert f.getvalue() == want
    back = ser.read_witness_vec(io.BytesIO(want))
    assert back.public_inputs_locations == [(2, 7), (0, 1)]
    assert back.all_values.dtype == np.uint64 and back.all_values.tolist() == [1, P, (1 << 64) - 1]
    assert back.multiplicities.dtype == np.uint32 and back.multiplicities.tolist() == [3, 2 ** 32 - 1]


def test_witness_vec_empty_and_truncated():
    f = io.BytesIO()
    ser.write_witness_vec(f, witness.WitnessVec([], [], []))
    assert f.getvalue() == struct.pack("<QQQ", 0, 0, 0)
    back = ser.read_witness_vec(io.BytesIO(f.getvalue()))
    assert (back.public_inputs_locations, back.all_values.size, back.multiplicities.size) == ([], 0, 0)
    with pytest.raises(EOFError):
        ser.read_witness_vec(io.BytesIO(struct.pack("<QQQ", 0, 0, 2) + b"\x00" * 7))


@pytest.mark.parametrize("kind", [witness.DenseVariablesCopyHint, witness.DenseWitnessCopyHint])
def test_copy_hint_byte_layout(kind):
    maps = [[1, PH, 5 | 1 << 62], [PH, 0, (1 << 48) - 1]]
    want = struct.pack("<Q", 2)
    for col in maps:
        want += struct.pack("<Q", 3) + struct.pack("<QQQ", *col)
    for hint in (kind(maps), np.array(maps, dtype=np.uint64), witness.CopyHint(kind(maps))):
        f = io.BytesIO()
        ser.write_copy_hint(f, hint)
        assert f.getvalue() == want
    back = ser.read_copy_hint(io.BytesIO(want), kind)
    assert isinstance(back, kind) and [[int(v) for v in col] for col in back.maps] == maps
    assert isinstance(ser.read_copy_hint(io.BytesIO(want)), witness.DenseVariablesCopyHint)
    with pytest.raises(EOFError):
        ser.read_copy_hint(io.BytesIO(want[:-1]))


# ------------------------------------------------------------------ errors that need no device
def upload(words, n_cols, n_rows, stride):
    arr = (ctypes.c_uint64 * len(words))(*words)
    handle = ctypes.c_void_p(1)
    rc = _lib.load().bj_copy_hint_upload_d(arr, n_cols, n_rows, stride, ctypes.byref(handle))
    return rc, handle.value, _lib.load().bj_last_error().decode()


@pytest.mark.parametrize("index", [2 ** 32 - 1, 2 ** 32, 2 ** 48 - 1])
def test_upload_rejects_an_index_that_does_not_fit_the_packed_cell(index):
    rc, handle, msg = upload([0, 1, index, 2], 2, 2, 2)
    assert rc == -22 and handle is None
    assert "column 1 row 0" in msg and str(index) in msg
    with pytest.raises(BoojumError, match=r"\(-22\)"):
        witness.CopyHint(np.array([[0, index]], dtype=np.uint64)).upload()


def test_upload_rejects_bad_shapes():
    assert upload([0, 1], 0, 2, 2)[0] == -22
    assert upload([0, 1], 1, 0, 2)[0] == -22
    assert upload([0, 1, 2, 3], 2, 2, 1)[0] == -22     # a stride below n_rows
    assert _lib.load().bj_copy_hint_upload_d(None, 1, 1, 1, ctypes.byref(ctypes.c_void_p())) == -22
    assert _lib.load().bj_copy_hint_release(None) == 0


def test_multiplicities_longer_than_the_trace():
    dummy = ctypes.c_void_p(8)   # never read: the lengths are compared first
    lib = _lib.load()
    assert lib.bj_materialize_multiplicities_d(dummy, 9, dummy, 8, None) == -22
    assert "more counts than rows" in lib.bj_last_error().decode()
    assert lib.bj_materialize_multiplicities_d(dummy, 0, dummy, 0, None) == -22


def test_hint_shapes_that_disagree():
    with pytest.raises(ValueError, match="disagree on the number of rows"):
        witness.CopyHint([[1, 2, 3], [4, 5]])
    with pytest.raises(ValueError):
        witness.CopyHint([])
    v, w = witness.CopyHint(np.zeros((2, 8), dtype=np.uint64)), witness.CopyHint(np.zeros((1, 4), dtype=np.uint64))
    wv = witness.WitnessVec([], [1], [])
    with pytest.raises(ValueError, match="disagree on the number of rows"):
        witness.witness_set_from_witness_vec(wv, v, w)
    with pytest.raises(ValueError, match="9 multiplicities for 8 rows"):
        witness.witness_set_from_witness_vec(witness.WitnessVec([], [1], [0] * 9), v, None)
    with pytest.raises(ValueError, match="power of two"):
        witness.create_permutation_polys(np.zeros((1, 6), dtype=np.uint64))


def test_calls_reject_what_is_no_hint():
    lib = _lib.load()
    dummy = ctypes.c_void_p(8)
    assert lib.bj_materialize_columns_d(None, dummy, 1, dummy, 8, None) == -22
    assert lib.bj_copy_hint_info(None, None, None, None, None) == -22
    assert lib.bj_permutation_polys_d(dummy, 1, 6, (ctypes.c_uint64 * 1)(1), dummy, 8, None) == -22   # 6 rows
    assert lib.bj_permutation_polys_d(dummy, 0, 8, (ctypes.c_uint64 * 1)(1), dummy, 8, None) == -22
    assert lib.bj_permutation_polys_d(dummy, 1, 8, (ctypes.c_uint64 * 1)(1), dummy, 4, None) == -22   # stride
