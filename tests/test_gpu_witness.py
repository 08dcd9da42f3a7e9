"""Witness materialisation on the device (boojum_amd.witness, csrc/witness.hip) against the integer
model (tests/witness_model.py), bit for bit.

The gather takes one row per lane, 256 rows per workgroup and 4 columns per thread, so the sizes are
n = 2^10 rows (four row blocks, padded to a group of eight) and 2^3 (a partly filled wave), with 1, 5
and 9 columns (below a column tile, one past one, one past two).  Every output starts from a pattern,
so a placeholder has to write its 0 and the words between n and the column stride have to survive.
No test feeds a kernel an index outside all_values."""
import ctypes

import numpy as np
import pytest

import witness_model as W

from boojum_amd import BoojumError, witness

pytestmark = pytest.mark.gpu

P = W.P
PH = W.PH
PATTERN = 0xA5A5A5A5DEADBEEF
SHAPES = [(3, 1), (3, 5), (3, 9), (10, 1), (10, 5), (10, 9)]
SPECIAL = [P - 1, P, (1 << 64) - 1]


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import _lib, field
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, lib=_lib))


def rand_values(count, seed):
    """Random words, the non-canonical ones among them."""
    v = np.random.default_rng(seed).integers(0, P, size=count, dtype=np.uint64)
    v[:len(SPECIAL)] = SPECIAL[:count]
    return v


def patterned(bj, n_cols, stride):
    return bj.field.to_device(np.full((n_cols, stride), PATTERN, dtype=np.uint64))


def gather(bj, maps, values, pad=0, num_values=None):
    """bj_materialize_columns_d into a patterned (C, n + pad) buffer -> the whole buffer on the host."""
    maps = np.asarray(maps, dtype=np.uint64)
    n_cols, n = maps.shape
    hint = witness.CopyHint(maps)
    vals = bj.field.to_device(np.asarray(values, dtype=np.uint64))
    out = patterned(bj, n_cols, n + pad)
    try:
        bj.lib.call("bj_materialize_columns_d", hint.upload(), vals.data_ptr(),
                    len(values) if num_values is None else num_values, out.data_ptr(), n + pad,
                    bj.field.stream_of(out))
        return bj.field.to_host(out), hint
    finally:
        hint.release()


def assert_gather(bj, maps, values, pad=0):
    got, hint = gather(bj, maps, values, pad)
    n = np.asarray(maps).shape[1]
    assert got[:, :n].tolist() == W.copy_columns(maps, values)
    assert (got[:, n:] == PATTERN).all()
    return hint


# ------------------------------------------------------------------ gather: sizes
@pytest.mark.parametrize("log_n,n_cols", SHAPES)
@pytest.mark.parametrize("pad", [0, 3])
def test_gather_sizes(bj, log_n, n_cols, pad):
    n = 1 << log_n
    n_vars = max(4, n_cols * n // 4)
    maps = W.random_maps(n_cols, n, n_vars, seed=log_n * 16 + n_cols)
    hint = assert_gather(bj, maps, rand_values(n_vars, seed=n_cols), pad)
    occ = W.occurrence_sets(maps)
    assert (hint.n_cols, hint.n_rows, hint.max_index) == (n_cols, n, max(occ))
    assert hint.n_placeholders == sum(W.is_placeholder(v) for col in maps for v in col)


# ------------------------------------------------------------------ gather: contents
@pytest.mark.parametrize("log_n", [3, 10])
def test_placeholders_first_row_last_row_and_a_whole_column(bj, log_n):
    n = 1 << log_n
    maps = W.random_maps(5, n, 50, seed=11, placeholders=0.0)
    maps[:, 0] = PH
    maps[:, n - 1] = PH
    maps[3, :] = PH
    got, _ = gather(bj, maps, rand_values(50, 12))
    assert got.tolist() == W.copy_columns(maps, rand_values(50, 12))
    assert not got[:, 0].any() and not got[:, n - 1].any() and not got[3].any()


def test_hint_of_placeholders_only(bj):
    got, hint = gather(bj, np.full((2, 8), PH, dtype=np.uint64), [7])
    assert not got.any() and (hint.max_index, hint.n_placeholders) == (0, 16)


@pytest.mark.parametrize("log_n", [3, 10])
def test_every_cell_names_the_same_index(bj, log_n):
    maps = np.full((5, 1 << log_n), 2, dtype=np.uint64)
    got, _ = gather(bj, maps, [1, 2, (1 << 64) - 1])
    assert (got == np.uint64((1 << 64) - 1)).all()


def test_the_last_index_and_one_value(bj):
    maps = W.random_maps(5, 1 << 10, 300, seed=21)
    maps[4, 1023] = 299                      # num_values - 1, in the last lane of the last block
    assert_gather(bj, maps, rand_values(300, 22)).max_index == 299
    got, hint = gather(bj, np.zeros((5, 8), dtype=np.uint64), [P])   # num_values = 1
    assert (got == np.uint64(P)).all() and hint.max_index == 0


def test_words_are_copied_verbatim(bj):
    values = SPECIAL + [0, 1]
    maps = np.array([[0, 1, 2, 3, 4, 2, 1, 0]], dtype=np.uint64)
    got, _ = gather(bj, maps, values)
    assert got.tolist() == [[P - 1, P, (1 << 64) - 1, 0, 1, (1 << 64) - 1, P, P - 1]]


def test_bits_above_the_index_are_ignored(bj):
    maps = np.array([[1 | 1 << 62, 2 | 1 << 50, PH | 1, 0]], dtype=np.uint64)
    got, _ = gather(bj, maps, [10, 11, 12])
    assert got.tolist() == [[11, 12, 0, 10]]


# ------------------------------------------------------------------ gather: errors
def test_too_few_values_launch_nothing(bj):
    maps = W.random_maps(5, 64, 40, seed=31)
    maps[2, 17] = 39
    with pytest.raises(BoojumError, match=r"\(-22\).*names index 39 and all_values holds 39"):
        gather(bj, maps, rand_values(40, 32), num_values=39)   # num_values = max_index
    hint = witness.CopyHint(maps)
    vals = bj.field.to_device(rand_values(40, 32))
    out = patterned(bj, 5, 64)
    rc = bj.lib.load().bj_materialize_columns_d(hint.upload(), vals.data_ptr(), 39, out.data_ptr(), 64, None)
    assert rc == -22
    rc = bj.lib.load().bj_materialize_columns_d(hint.upload(), vals.data_ptr(), 40, out.data_ptr(), 63, None)
    assert rc == -22                                            # a stride below n_rows
    bj.torch.cuda.synchronize()
    assert (bj.field.to_host(out) == PATTERN).all()
    hint.release()
    assert bj.lib.load().bj_copy_hint_info(hint._handle, None, None, None, None) == -22


# ------------------------------------------------------------------ multiplicities
@pytest.mark.parametrize("n,length", [(1 << 10, 0), (1 << 10, 1 << 10), (1 << 10, 300), (8, 5)])
def test_multiplicities(bj, n, length):
    m = np.random.default_rng(n + length).integers(0, 1 << 32, size=length, dtype=np.uint64).astype(np.uint32)
    if length:
        m[length - 1] = 2 ** 32 - 1
    out = patterned(bj, 1, n)[0]
    witness.materialize_multiplicities(m, out)
    assert bj.field.to_host(out).tolist() == W.multiplicities_column(m, n)
    with pytest.raises(BoojumError, match=r"\(-22\)"):
        witness.materialize_multiplicities(np.zeros(n + 1, dtype=np.uint32), out)


# ------------------------------------------------------------------ sigma
@pytest.mark.parametrize("log_n,n_cols", SHAPES)
def test_permutation_polys(bj, log_n, n_cols):
    n = 1 << log_n
    maps = W.random_maps(n_cols, n, max(4, n_cols * n // 4), seed=40 + log_n + n_cols)
    if n_cols > 1:
        maps[1, :] = 3       # a variable that fills a column
    got = bj.field.to_host(witness.create_permutation_polys(witness.DenseVariablesCopyHint(maps)))
    assert got.tolist() == W.create_permutation_polys(maps, log_n)


def test_permutation_polys_stride_and_stray_entries(bj):
    """A column stride above n leaves the padding alone; an entry of prev that names no cell gives 0."""
    n, n_cols = 8, 2
    prev = np.arange(n_cols * n, dtype=np.uint32).reshape(n_cols, n)
    prev[0, 1], prev[1, 7], prev[1, 0] = 9, n_cols * n, 2 ** 32 - 1
    from boojum_amd.stage2 import non_residues_for_copy_permutation
    k = non_residues_for_copy_permutation(n, n_cols)
    prev_d = bj.torch.from_numpy(prev.view(np.int32)).to("cuda")
    out = patterned(bj, n_cols, n + 3)
    bj.lib.call("bj_permutation_polys_d", prev_d.data_ptr(), n_cols, n, (ctypes.c_uint64 * n_cols)(*k), out.data_ptr(),
                n + 3, bj.field.stream_of(out))
    got = bj.field.to_host(out)
    want = np.array(W.identity_polys(n_cols, 3), dtype=np.uint64)
    want[0, 1], want[1, 7], want[1, 0] = want[1, 1], 0, 0
    assert got[:, :n].tolist() == want.tolist() and (got[:, n:] == PATTERN).all()


# ------------------------------------------------------------------ the reference's entry point
def test_witness_set_from_witness_vec(bj):
    n = 1 << 10
    v_maps, w_maps = W.random_maps(5, n, 700, seed=51), W.random_maps(2, n, 700, seed=52)
    values = rand_values(700, 53)
    mult = np.arange(1, 301, dtype=np.uint32)
    locations = [(4, 1023), (0, 0), (2, 517)]
    wv = witness.WitnessVec(locations, values, mult)
    ws = witness.witness_set_from_witness_vec(wv, witness.DenseVariablesCopyHint(v_maps),
                                              witness.DenseWitnessCopyHint(w_maps))
    variables = W.copy_columns(v_maps, values)
    assert bj.field.to_host(ws.variables).tolist() == variables
    assert bj.field.to_host(ws.witness).tolist() == W.copy_columns(w_maps, values)
    assert bj.field.to_host(ws.multiplicities).tolist() == [W.multiplicities_column(mult, n)]
    assert (ws.public_inputs_values, ws.public_inputs_with_locations) == W.public_inputs(locations, variables)
    # LookupParameters::NoLookup, no witness columns, all_values already on the device
    wv = witness.WitnessVec([], bj.field.to_device(values), [])
    ws = witness.witness_set_from_witness_vec(wv, witness.CopyHint(v_maps), None)
    assert bj.field.to_host(ws.variables).tolist() == variables
    assert tuple(ws.witness.shape) == (0, n) and tuple(ws.multiplicities.shape) == (0, n)
    assert (ws.public_inputs_values, ws.public_inputs_with_locations) == ([], [])


# ------------------------------------------------------------------ end to end
class Circuit:
    """n = 2^10 rows, C = 5 variable columns: an FMA gate on columns 0..3 (its two coefficients in
    constant columns 0 and 1) and a boolean constraint on column 4, both on every row.  a, b and c
    draw from 64 shared input variables, d is a variable of its own per row, the boolean column
    names one variable of value 0 or one of value 1; every 16th row is placeholders only."""

    def __init__(self, log_n=10, seed=61):
        from boojum_amd import gates as G
        n = self.n = 1 << log_n
        rng = np.random.default_rng(seed)
        inputs = rng.integers(0, P, size=64, dtype=np.uint64)
        self.constants = rng.integers(0, P, size=(2, n), dtype=np.uint64)
        self.maps = np.empty((5, n), dtype=np.uint64)
        self.maps[:3] = rng.integers(0, 64, size=(3, n), dtype=np.uint64)
        self.maps[3] = 66 + np.arange(n, dtype=np.uint64)
        self.maps[4] = 64 + rng.integers(0, 2, size=n, dtype=np.uint64)
        self.maps[:, ::16] = PH
        values = [int(v) for v in inputs] + [0, 1]
        for r in range(n):
            a, b, c = (values[int(self.maps[j, r])] if r % 16 else 0 for j in range(3))
            values.append((int(self.constants[0, r]) * a * b + int(self.constants[1, r]) * c) % P)
        self.values = np.array(values, dtype=np.uint64)
        fma, boolean = G.FmaGateInBaseFieldWithoutConstant(), G.BooleanConstraintGate()
        self.placements = [G.GatePlacement(G.capture(fma), 1, fma.per_chunk_offset, (), 0),
                           G.GatePlacement(G.capture(boolean), 1, G.PerChunkOffset(1, 0, 0), (), 0,
                                           G.PerChunkOffset(4, 0, 0))]


@pytest.fixture(scope="module")
def circuit():
    return Circuit()


BETA, GAMMA = (0x1234567890ABCDEF % P, 77), (0x0FEDCBA987654321, 5)


def test_end_to_end_copy_permutation(bj, circuit):
    from boojum_amd import stage2
    hint = witness.CopyHint(witness.DenseVariablesCopyHint(circuit.maps))
    sigmas = witness.create_permutation_polys(hint)
    ws = witness.witness_set_from_witness_vec(witness.WitnessVec([], circuit.values, []), hint, None)
    stage2.compute_partial_products_in_extension(ws.variables, sigmas, BETA, GAMMA, 4, check=True)
    total = bj.field.to_host(stage2.compute_partial_products_in_extension.status)
    assert [int(total[0]), int(total[1])] == [1, 0]
    # one cell from another variable with another value, against the same sigmas
    maps = circuit.maps.copy()
    other = (int(maps[0, 5]) + 1) % 64
    assert circuit.values[other] != circuit.values[int(maps[0, 5])]
    maps[0, 5] = other
    bad = witness.witness_set_from_witness_vec(witness.WitnessVec([], circuit.values, []), maps, None)
    with pytest.raises(BoojumError, match="grand product"):
        stage2.compute_partial_products_in_extension(bad.variables, sigmas, BETA, GAMMA, 4, check=True)


def test_end_to_end_satisfied_and_committed(bj, circuit):
    from boojum_amd import commit, gates as G
    wv = witness.WitnessVec([(3, 7)], circuit.values, [])
    ws = witness.witness_set_from_witness_vec(wv, witness.DenseVariablesCopyHint(circuit.maps), None)
    model = W.copy_columns(circuit.maps, circuit.values)
    assert ws.public_inputs_with_locations == [(3, 7, model[3][7])]
    gate_set = G.GateSet(circuit.placements)
    report = G.check_if_satisfied(gate_set, ws.variables, None, bj.field.to_device(circuit.constants))
    assert report.satisfied, report
    bad = circuit.values.copy()
    bad[66 + 9] = (int(bad[66 + 9]) + 1) % P        # d of row 9
    ws_bad = witness.witness_set_from_witness_vec(witness.WitnessVec([], bad, []), circuit.maps, None)
    report = G.check_if_satisfied(gate_set, ws_bad.variables, None, bj.field.to_device(circuit.constants))
    assert (report.num_unsatisfied, report.row, report.gate) == (1, 9, 0)
    got = commit.commit_trace_columns(ws.variables, 4, 2, 16)
    want = commit.commit_trace_columns(bj.field.to_device(np.array(model, dtype=np.uint64)), 4, 2, 16)
    assert got.get_cap().tolist() == want.get_cap().tolist()


def test_commit_witness_vec_is_in_the_oracles_leaf_order(bj, circuit):
    from boojum_amd import commit
    n = circuit.n
    w_maps = W.random_maps(2, n, len(circuit.values), seed=71)
    mult = np.arange(100, dtype=np.uint32)
    wv = witness.WitnessVec([(0, 1)], circuit.values, mult)
    oracle, ws = witness.commit_witness_vec(wv, witness.CopyHint(circuit.maps), witness.CopyHint(w_maps), 4, 2, 16)
    columns = W.copy_columns(circuit.maps, circuit.values) + W.copy_columns(w_maps, circuit.values) \
        + [W.multiplicities_column(mult, n)]
    want = commit.commit_trace_columns(bj.field.to_device(np.array(columns, dtype=np.uint64)), 4, 2, 16)
    assert oracle.get_cap().tolist() == want.get_cap().tolist()
    assert tuple(oracle.lde.shape) == (8, 4, n)
    assert bj.field.to_host(ws.multiplicities).tolist() == [columns[7]]
    assert ws.public_inputs_values == [columns[0][1]]


# ------------------------------------------------------------------ capture
def test_gather_replays_in_a_graph_with_new_values(bj):
    torch = bj.torch
    n, n_cols = 1 << 10, 5
    maps = W.random_maps(n_cols, n, 300, seed=81)
    first, second = rand_values(300, 82), rand_values(300, 83)[::-1].copy()
    hint = witness.CopyHint(maps)
    hint.upload()                                   # the allocation and the copy stay outside the capture
    values = bj.field.to_device(first)
    out = patterned(bj, n_cols, n)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        witness.materialize_columns(hint, values, out)
    graph.replay()
    torch.cuda.synchronize()
    assert bj.field.to_host(out).tolist() == W.copy_columns(maps, first)
    values.copy_(bj.field.to_device(second))
    graph.replay()
    torch.cuda.synchronize()
    assert bj.field.to_host(out).tolist() == W.copy_columns(maps, second)
