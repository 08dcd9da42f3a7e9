"""Python-integer restatements of witness_set_from_witness_vec (cs/implementations/witness.rs:387-538)
and create_permutation_polys (cs/implementations/setup.rs:401-484), the models the witness tests
compare the library with.  The sigma model is the reference's sequential chain of swaps, not the
sort boojum_amd.witness.prev_map uses."""
import numpy as np

import stage2_model as S2

P = S2.P
PLACEHOLDER_BIT_MASK = 1 << 63   # cs/mod.rs:44
LOW_U48_MASK = (1 << 48) - 1     # cs/mod.rs:47
PH = PLACEHOLDER_BIT_MASK        # Variable::placeholder() / Witness::placeholder(), cs/mod.rs:159-161, 192-194


def is_placeholder(word):
    """cs/mod.rs:172-175, 205-208."""
    return int(word) & PLACEHOLDER_BIT_MASK != 0


def as_index(word):
    """as_variable_index / as_witness_index (cs/mod.rs:163-170, 196-203) for an index below 2^32,
    where the two agree."""
    return int(word) & LOW_U48_MASK


def copy_columns(maps, all_values):
    """The copy loops, witness.rs:419-441 (variables) and :466-488 (witnesses): a zeroed column
    (:402, :454), then *dst = all_values[index] for every cell that is no placeholder.  Words are
    moved as they are.  -> list of columns of Python integers."""
    out = []
    for column in maps:
        dst = [0] * len(column)
        for row, var in enumerate(column):
            if not is_placeholder(var):
                dst[row] = int(all_values[as_index(var)])
        out.append(dst)
    return out


def multiplicities_column(multiplicities, n):
    """witness.rs:493-519: a zeroed column of the trace length, the counts widened into its head
    (zip stops at the shorter, :510-516)."""
    dst = [0] * n
    for i, src in zip(range(n), multiplicities):
        dst[i] = int(src)
    return dst


def public_inputs(locations, variables_columns):
    """witness.rs:521-529 -> (public_inputs_values, public_inputs_with_locations)."""
    with_values = [(column, row, variables_columns[column][row]) for column, row in locations]
    return [v for _, _, v in with_values], with_values


def identity_polys(n_cols, log_n):
    """materialize_x_by_non_residue_polys (setup.rs:24-76): column c is k_c * w^row, rows in natural
    order (materialize_x_poly, utils.rs:690-721), k_0 = 1 and the rest make_non_residues."""
    n = 1 << log_n
    k, x = S2.non_residues_for_copy_permutation(n, n_cols), S2.domain(log_n)
    return [[kc * xi % P for xi in x] for kc in k]


def create_permutation_polys(maps, log_n, num_places=None):
    """setup.rs:401-484 line by line: the scratch of (value, first place) per variable index
    (:425-426; num_places is next_available_place_idx), the walk over the columns that swaps each
    occurrence's identity value with the one parked in the scratch (:428-455), and the final pass
    that writes the last occurrence's value into the first place (:459-471).  "Never seen" is the
    parked value being zero (:441, :461); an identity value is a product of units, so the test is
    exact for every index, 0 included."""
    result = identity_polys(len(maps), log_n)
    if num_places is None:
        num_places = 1 + max([as_index(v) for col in maps for v in col if not is_placeholder(v)], default=0)
    scratch = [[0, (0, 0)] for _ in range(num_places)]
    for column_idx, (column, poly) in enumerate(zip(maps, result)):
        for row, var in enumerate(column):
            if is_placeholder(var):
                continue
            previous = scratch[as_index(var)]
            if previous[0] == 0:
                assert previous[1] == (0, 0)
                previous[0], previous[1] = poly[row], (column_idx, row)
            else:
                previous[0], poly[row] = poly[row], previous[0]
    for value, (first_column, first_row) in scratch:
        if value == 0:
            continue
        result[first_column][first_row] = value
    return result


# ------------------------------------------------------------------ inputs
def random_maps(n_cols, n, n_vars, seed, placeholders=0.1):
    """A dense hint of n_cols x n words over the variable indices [0, n_vars): uniformly random
    cells, a share of placeholders, index 0 and index n_vars - 1 used at least once when there is
    room, and bits 48..62 set in some words (the index is the low 48 bits only)."""
    rng = np.random.default_rng(seed)
    maps = rng.integers(0, n_vars, size=(n_cols, n), dtype=np.uint64)
    maps[rng.random((n_cols, n)) < placeholders] = PH
    flat = maps.reshape(-1)
    if flat.size >= 2:
        flat[rng.integers(0, flat.size)] = 0
        flat[rng.integers(0, flat.size)] = n_vars - 1
    return maps


def occurrence_sets(maps):
    """variable index -> the set of flat cells col * n + row that name it."""
    n = len(maps[0])
    out = {}
    for c, column in enumerate(maps):
        for r, var in enumerate(column):
            if not is_placeholder(var):
                out.setdefault(as_index(var), set()).add(c * n + r)
    return out
