"""Witness materialisation on the GPU: the trace columns from a WitnessVec and the circuit's dense
copy hints (bj_materialize_columns_d, csrc/witness.hip), and the sigma columns of the setup from
the same placement (bj_permutation_polys_d).

The reference's production entry point, prove_from_precomputations, takes a WitnessVec and the
per-circuit DenseVariablesCopyHint / DenseWitnessCopyHint and builds the columns itself
(witness_set_from_witness_vec, cs/implementations/witness.rs:387-538).  Here the hints are uploaded
once per circuit (`CopyHint`) and stay on the device; a proof uploads `all_values`, one word per
distinct variable, and the columns appear where the commitment, stage 2 and the satisfiability
check read them.

* `WitnessVec`, `DenseVariablesCopyHint`, `DenseWitnessCopyHint`, `WitnessSet`: the reference's
  names and fields (witness.rs:21-40, hints/mod.rs:10-20).
* `CopyHint(maps)`: the upload (bj_copy_hint_upload_d) and `prev_map()`, the previous-occurrence
  map the sigma kernel reads.  `prev_map` is index bookkeeping, built once on the host with a
  stable sort by variable index; it is host only in the sense `gates.compile_gate_set` is.
* `witness_set_from_witness_vec`, `create_permutation_polys` (setup.rs:401-484),
  `commit_witness_vec` (prover.rs:313-347).

There is no CPU fallback: nothing here copies a value or forms an identity value on the host.
"""
import ctypes

import numpy as np
import torch

from ._lib import call, load
from .field import stream_of, to_device, to_host

PLACEHOLDER_BIT = 1 << 63        # cs/mod.rs:44
LOW_U48_MASK = (1 << 48) - 1     # cs/mod.rs:47
PACKED_PLACEHOLDER = 0xFFFFFFFF  # the device copy's reserved cell value


def placeholder():
    """Variable::placeholder() / Witness::placeholder() (cs/mod.rs:159-161, 192-194)."""
    return PLACEHOLDER_BIT


class WitnessVec:
    """witness.rs:29-40.  all_values may be host data (uploaded per call) or an int64 device tensor
    (read in place)."""

    def __init__(self, public_inputs_locations, all_values, multiplicities):
        self.public_inputs_locations = [(int(c), int(r)) for c, r in public_inputs_locations]
        self.all_values = all_values
        self.multiplicities = multiplicities


class DenseVariablesCopyHint:
    """hints/mod.rs:10-14: maps[column][row] is a Variable's u64 word."""

    def __init__(self, maps):
        self.maps = maps


class DenseWitnessCopyHint:
    """hints/mod.rs:16-20: maps[column][row] is a Witness's u64 word."""

    def __init__(self, maps):
        self.maps = maps


class WitnessSet:
    """witness.rs:21-27.  variables and witness are (C, n) device tensors (a (0, n) one for no
    columns), multiplicities a (k, n) one with k the number of multiplicity columns (0 or 1)."""

    def __init__(self, public_inputs_values, public_inputs_with_locations, variables, witness, multiplicities):
        self.public_inputs_values = public_inputs_values
        self.public_inputs_with_locations = public_inputs_with_locations
        self.variables = variables
        self.witness = witness
        self.multiplicities = multiplicities


def hint_words(maps):
    """A hint's maps (a Dense*CopyHint, or its maps as nested lists or a (C, n) array) -> the
    (C, n) uint64 array of its words.  ValueError when the columns disagree on the number of rows."""
    maps = getattr(maps, "maps", maps)
    if isinstance(maps, np.ndarray):
        words = maps
    else:
        cols = [np.asarray(col, dtype=np.uint64) for col in maps]
        if not cols:
            raise ValueError("a dense hint holds at least one column")
        if any(col.ndim != 1 or col.shape != cols[0].shape for col in cols):
            raise ValueError("the columns of a dense hint disagree on the number of rows")
        words = np.stack(cols)
    if words.ndim != 2 or words.shape[0] == 0 or words.shape[1] == 0:
        raise ValueError("a dense hint is (columns, rows) with at least one of each")
    return np.ascontiguousarray(words, dtype=np.uint64)


def prev_map(maps):
    """The previous-occurrence map of a variables hint, a (C, n) uint32 array: cell (c, r) holds
    the flat index col * n + row of the variable's previous occurrence in (column, row) order, the
    first occurrence holds the last one's, and a placeholder or a variable's only occurrence holds
    its own.  That is where the reference's chain of swaps (setup.rs:428-471) takes each cell's
    identity value from.  One stable sort by variable index; host only."""
    words = hint_words(maps)
    c, n = words.shape
    if c * n > 1 << 32:
        raise ValueError("more than 2^32 cells")
    flat = words.reshape(-1)
    prev = np.arange(c * n, dtype=np.uint32)
    cells = np.nonzero((flat >> np.uint64(63)) == 0)[0]
    if cells.size:
        index = flat[cells] & np.uint64(LOW_U48_MASK)
        order = cells[np.argsort(index, kind="stable")]   # by variable, then by (column, row)
        var = index[np.argsort(index, kind="stable")]
        first = np.ones(order.size, dtype=bool)
        first[1:] = var[1:] != var[:-1]
        last = np.ones(order.size, dtype=bool)
        last[:-1] = first[1:]
        before = np.empty_like(order)
        before[1:] = order[:-1]
        before[first] = order[last]   # the groups are in one order in both selections
        prev[order] = before.astype(np.uint32)
    return prev.reshape(c, n)


class CopyHint:
    """One dense hint on the device.  The words are checked and packed by the library
    (bj_copy_hint_upload_d) at the first use or at `upload()`; the handle keeps the device buffer
    until it is collected or `release()`d.  n_cols, n_rows are known from the start; max_index and
    n_placeholders (bj_copy_hint_info) after the upload."""

    def __init__(self, maps):
        self._handle = None
        self.words = hint_words(maps)
        self.n_cols, self.n_rows = self.words.shape
        self.max_index = self.n_placeholders = None

    def upload(self):
        if self._handle is None:
            handle = ctypes.c_void_p()
            call("bj_copy_hint_upload_d", self.words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), self.n_cols,
                 self.n_rows, self.n_rows, ctypes.byref(handle))
            self._handle = handle
            n_cols, n_rows, max_index, n_ph = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            call("bj_copy_hint_info", handle, ctypes.byref(n_cols), ctypes.byref(n_rows), ctypes.byref(max_index),
                 ctypes.byref(n_ph))
            assert (n_cols.value, n_rows.value) == (self.n_cols, self.n_rows)
            self.max_index, self.n_placeholders = max_index.value, n_ph.value
        return self._handle

    def prev_map(self):
        return prev_map(self.words)

    def release(self):
        if self._handle is not None:
            handle, self._handle = self._handle, None
            load().bj_copy_hint_release(handle)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _as_copy_hint(hint):
    return hint if hint is None or isinstance(hint, CopyHint) else CopyHint(hint)


def _values_tensor(all_values, device):
    if isinstance(all_values, torch.Tensor):
        if not all_values.is_cuda or all_values.dtype not in (torch.int64, torch.uint64) or all_values.dim() != 1 \
                or not all_values.is_contiguous():
            raise TypeError("all_values: a contiguous 1-d int64 CUDA tensor of u64 words, or host data")
        return all_values
    return to_device(np.asarray(all_values, dtype=np.uint64).reshape(-1), device)


def materialize_columns(hint, all_values, out):
    """out[c, r] = all_values[index of cell (c, r)], 0 for a placeholder (bj_materialize_columns_d):
    one launch on the current stream, nothing copied back.  all_values: a 1-d int64 device tensor;
    out: a (C, >= n) int64 device tensor (or a view of one) with unit-stride rows."""
    if out.dim() != 2 or out.shape[0] != hint.n_cols or out.shape[1] != hint.n_rows or out.stride(1) != 1:
        raise ValueError("out must be (%d, %d) with contiguous rows" % (hint.n_cols, hint.n_rows))
    stride = out.stride(0) if hint.n_cols > 1 else hint.n_rows
    call("bj_materialize_columns_d", hint.upload(), all_values.data_ptr(), all_values.numel(), out.data_ptr(), stride,
         stream_of(out))
    return out


def materialize_multiplicities(multiplicities, out):
    """out[i] = multiplicities[i] widened, 0 past their end (bj_materialize_multiplicities_d).
    multiplicities: u32 counts on the host, or an int32 device tensor; out: an (n,) device row."""
    if isinstance(multiplicities, torch.Tensor):
        if not multiplicities.is_cuda or multiplicities.dtype not in (torch.int32, torch.uint32) \
                or not multiplicities.is_contiguous():
            raise TypeError("multiplicities: a contiguous int32 CUDA tensor of u32 counts, or host data")
        m = multiplicities
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(multiplicities, dtype=np.uint32)).view(np.int32)).to(
            out.device)
    if out.dim() != 1 or out.stride(0) != 1:
        raise ValueError("out must be one contiguous row")
    call("bj_materialize_multiplicities_d", m.data_ptr() if m.numel() else None, m.numel(), out.data_ptr(),
         out.numel(), stream_of(out))
    return out


def _materialize(witness_vec, vars_hint, wits_hint, n_multiplicity_columns, device):
    """The variables, the witnesses and the multiplicities in one (C_total, n) tensor, in that
    order, and the three views."""
    vars_hint, wits_hint = _as_copy_hint(vars_hint), _as_copy_hint(wits_hint)
    hints = [h for h in (vars_hint, wits_hint) if h is not None]
    if not hints:
        raise ValueError("neither a variables hint nor a witness hint")
    n = hints[0].n_rows
    if any(h.n_rows != n for h in hints):
        raise ValueError("the hints disagree on the number of rows: %s" % [h.n_rows for h in hints])
    n_mult = len(witness_vec.multiplicities)
    if n_multiplicity_columns is None:
        n_multiplicity_columns = 1 if n_mult else 0
    if n_multiplicity_columns not in (0, 1):
        raise ValueError("the reference has one multiplicity column at most (witness.rs:500-501)")
    if n_mult > n:
        raise ValueError("%d multiplicities for %d rows" % (n_mult, n))
    c_v = vars_hint.n_cols if vars_hint is not None else 0
    c_w = wits_hint.n_cols if wits_hint is not None else 0
    values = _values_tensor(witness_vec.all_values, device)
    total = torch.empty((c_v + c_w + n_multiplicity_columns, n), dtype=torch.int64, device=values.device)
    variables, witness, mult = total[:c_v], total[c_v:c_v + c_w], total[c_v + c_w:]
    if c_v:
        materialize_columns(vars_hint, values, variables)
    if c_w:
        materialize_columns(wits_hint, values, witness)
    if n_multiplicity_columns:
        materialize_multiplicities(witness_vec.multiplicities, mult[0])
    return total, variables, witness, mult


def _public_inputs(witness_vec, variables):
    """witness.rs:521-529: the values at the public input locations, read back in one copy."""
    locations = witness_vec.public_inputs_locations
    if not locations:
        return [], []
    c, n = variables.shape
    for col, row in locations:
        if not (0 <= col < c and 0 <= row < n):
            raise IndexError("public input location (%d, %d) outside the %d x %d variables" % (col, row, c, n))
    index = torch.tensor([col * n + row for col, row in locations], dtype=torch.int64)
    values = [int(v) for v in to_host(variables.reshape(-1)[index.to(variables.device)])]
    return values, [(col, row, v) for (col, row), v in zip(locations, values)]


def witness_set_from_witness_vec(witness_vec, vars_hint, wits_hint, n_multiplicity_columns=None, device="cuda"):
    """CSReferenceAssembly::witness_set_from_witness_vec (witness.rs:387-538) on the device.
    vars_hint, wits_hint: `CopyHint`s (uploaded once per circuit), Dense*CopyHints (uploaded
    here), or None for no columns of that kind.  n_multiplicity_columns: 0 for
    LookupParameters::NoLookup, 1 otherwise; by default 1 iff the WitnessVec carries
    multiplicities.  Returns a WitnessSet of device tensors; the public inputs are read back from
    the variable columns in one copy, which synchronises (none: nothing is copied)."""
    _, variables, witness, mult = _materialize(witness_vec, vars_hint, wits_hint, n_multiplicity_columns, device)
    values, with_locations = _public_inputs(witness_vec, variables)
    return WitnessSet(values, with_locations, variables, witness, mult)


def create_permutation_polys(vars_hint, device="cuda"):
    """create_permutation_polys (setup.rs:401-484): the (C, n) sigma tensor of a variables hint,
    the argument `stage2.compute_partial_products_in_extension` takes.  The previous-occurrence map
    is built on the host (`prev_map`), the values on the device (bj_permutation_polys_d)."""
    from .stage2 import non_residues_for_copy_permutation
    prev = vars_hint.prev_map() if isinstance(vars_hint, CopyHint) else prev_map(vars_hint)
    c, n = prev.shape
    if n & (n - 1):
        raise ValueError("the trace length must be a power of two, got %d" % n)
    k = non_residues_for_copy_permutation(n, c)
    prev_d = torch.from_numpy(prev.view(np.int32)).to(device)
    out = torch.empty((c, n), dtype=torch.int64, device=prev_d.device)
    call("bj_permutation_polys_d", prev_d.data_ptr(), c, n, (ctypes.c_uint64 * c)(*k), out.data_ptr(), n,
         stream_of(out))
    return out


def commit_witness_vec(witness_vec, vars_hint, wits_hint, lde_degree, fri_lde_factor, cap_size, hasher="poseidon2",
                       n_multiplicity_columns=None, device="cuda"):
    """The witness oracle from a WitnessVec (prover.rs:313-347).  The variables, the witnesses and
    the multiplicities are materialised into one (C_total, n) tensor in the oracle's leaf order --
    variables_columns, then witness_columns, then lookup_multiplicities_polys (the three
    `source.extend` of prover.rs:325-343) -- so there is no stacking copy, and the tensor goes to
    `commit.commit_trace_columns`.  Returns (OracleCommitment, WitnessSet); the set's tensors are
    views into the committed one."""
    from .commit import commit_trace_columns
    total, variables, witness, mult = _materialize(witness_vec, vars_hint, wits_hint, n_multiplicity_columns, device)
    oracle = commit_trace_columns(total, lde_degree, fri_lde_factor, cap_size, hasher=hasher)
    values, with_locations = _public_inputs(witness_vec, variables)
    return oracle, WitnessSet(values, with_locations, variables, witness, mult)
