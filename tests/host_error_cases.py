"""The rejected calls of the collective, host-commit and tree ABI whose return code and bj_last_error()
text tests/golden/host_errors.json pins (tests/test_host_errors.py checks them, tools/record_host_errors.py
records them from a library built at the commit before a change of the host code).

A case is a name and a function of the loaded library (ctypes, _lib.SIGNATURES applied) that returns the
call's code.  HOST cases return before any runtime call that needs a device; DEVICE cases make a local
group (its events) first.  No case launches anything: device pointers are null wherever the null check
comes last, and where a non-null pointer is needed to reach a later check it is only compared, with a later
check of the same call violated as well (out_words 0, a null trace, zero leaves) so the call returns even
if the check under test were lost.  The pair cases violate two adjacent checks at once: which message
wins pins their order.
"""
import ctypes

from boojum_amd import _lib

POSEIDON2, BLAKE2S, KECCAK = 0, 1, 2
ALL_GATHER, ALL_TO_ALL = 0, 1
# bj::tree_leaves_partial (csrc/bj_internal.hpp), the one route to a Keccak leaf call with a state or a
# non-final range: every ABI entry point passes Keccak whole leaves
TREE_LEAVES_PARTIAL = "_ZN2bj19tree_leaves_partialEiPKmjmmmS1_PmbP12ihipStream_t"

_keep = []  # callbacks and buffers the communicators and cases point to
_comms = []  # communicators made by the cases, destroyed at the end of run()


def _noop_exchange(user, kind, send, recv, nbytes, stream):
    return 0


def comm(L, world, rank=0):
    """A callback communicator: it makes no runtime objects."""
    fn = _lib.EXCHANGE_FN(_noop_exchange)
    _keep.append(fn)
    out = ctypes.c_void_p()
    rc = L.bj_comm_init_callback(world, rank, fn, None, 1, ctypes.byref(out))
    assert rc == 0, L.bj_last_error()
    _comms.append(out)
    return out


def _ptr():
    """A non-null address (four host words) for arguments that are compared with null, never read."""
    b = (ctypes.c_uint64 * 4)()
    _keep.append(b)
    return ctypes.addressof(b)


def _commit(L, c, n_cols=2, log_n=4, log_lde=2, log_k=1, cap=2, hasher=POSEIDON2, stride=16):
    # every buffer null: the null check is the call's last
    return L.bj_sharded_commit_d(c, None, stride, n_cols, log_n, log_lde, log_k, cap, hasher, None, None, None, None,
                                 None)


def _query(L, c, n_cols=2, log_n=4, log_lde=2, log_k=1, cap=2, hasher=POSEIDON2, idx=0):
    return L.bj_sharded_query_h(c, None, None, None, n_cols, log_n, log_lde, log_k, cap, hasher, idx, None, None,
                                None, None)


def _oracle(**kw):
    d = dict(src=_ptr(), col_stride=16, n_cols=2, hasher=POSEIDON2, leaves=_ptr(), nodes=_ptr(), n_leaves=16,
             cap_size=2, reserved=0)
    d.update(kw)
    return _lib.ShardedQueryOracleDesc(**d)


def _queries(L, c, oracles=None, n_oracles=None, indices=True, n_queries=1):
    oracles = [_oracle()] if oracles is None else oracles
    arr = (_lib.ShardedQueryOracleDesc * len(oracles))(*oracles)
    # out_words 0 everywhere: the size check is the call's last
    return L.bj_sharded_queries_d(c, arr, len(oracles) if n_oracles is None else n_oracles,
                                  _ptr() if indices else None, n_queries, _ptr(), 0, _ptr(), None)


def _commit_h(L, n_cols=2, log_n=4, log_lde=2, log_k=1, cap=2):
    # the trace null: the null check is the last before the call takes a device
    return L.bj_lde_commit_h(None, n_cols, log_n, log_lde, log_k, cap, None, None, None, None)


def _b2s_partial(L, n_cols=8, cols_before=0, state=False, final=1):
    return L.bj_blake2s_leaves_partial_d(None, n_cols, 0, 0, cols_before, _ptr() if state else None, None, final, None)


def _keccak_partial(L, state, final):
    fn = getattr(L, TREE_LEAVES_PARTIAL)
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint64,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_bool, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn(KECCAK, None, 8, 0, 0, 0, _ptr() if state else None, None, final, None)


def _init_callback(L, world, rank, null_fn=False):
    fn = _lib.EXCHANGE_FN() if null_fn else _lib.EXCHANGE_FN(_noop_exchange)
    _keep.append(fn)
    out = ctypes.c_void_p()
    rc = L.bj_comm_init_callback(world, rank, fn, None, 1, ctypes.byref(out))
    assert rc != 0 and not out.value
    return rc


def _columns(L, n_cols, log_shards, shard, hasher):
    out = (ctypes.c_uint32 * 64)()
    return L.bj_sharded_columns(n_cols, log_shards, shard, hasher, out)


def _group_create(L, world):
    g = ctypes.c_void_p()
    rc = L.bj_comm_local_group_create(world, ctypes.byref(g))
    assert rc != 0 and not g.value
    return rc


# (name, call) in the order of the entry points' checks
HOST = [
    ("init_callback/world_3", lambda L: _init_callback(L, 3, 0)),
    ("init_callback/rank_eq_world", lambda L: _init_callback(L, 2, 2)),
    ("init_callback/null_fn", lambda L: _init_callback(L, 2, 0, null_fn=True)),
    ("init_callback/pair_null_fn_world_3", lambda L: _init_callback(L, 3, 0, null_fn=True)),
    ("local_group_create/world_3", lambda L: _group_create(L, 3)),
    ("local_group_create/world_128", lambda L: _group_create(L, 128)),
    ("exchange/null_comm", lambda L: L.bj_comm_exchange_d(None, ALL_GATHER, None, None, 0, None)),
    ("exchange/unknown_kind", lambda L: L.bj_comm_exchange_d(comm(L, 1), 7, None, None, 0, None)),
    ("exchange/bytes_12", lambda L: L.bj_comm_exchange_d(comm(L, 1), ALL_TO_ALL, None, None, 12, None)),
    ("exchange/null_buffer_bytes_8", lambda L: L.bj_comm_exchange_d(comm(L, 1), ALL_GATHER, None, None, 8, None)),
    ("exchange/pair_null_comm_unknown_kind", lambda L: L.bj_comm_exchange_d(None, 7, None, None, 12, None)),
    ("exchange/pair_unknown_kind_bytes_12", lambda L: L.bj_comm_exchange_d(comm(L, 1), 7, None, None, 12, None)),
    ("exchange/pair_bytes_12_null_buffer", lambda L: L.bj_comm_exchange_d(comm(L, 2), ALL_GATHER, None, None, 12, None)),
    ("sharded_columns/log_shards_17", lambda L: _columns(L, 8, 17, 0, POSEIDON2)),
    ("sharded_columns/n_cols_6_of_4", lambda L: _columns(L, 6, 2, 0, POSEIDON2)),
    ("sharded_columns/hasher_7", lambda L: _columns(L, 8, 2, 0, 7)),
    ("sharded_columns/pair_log_shards_17_n_cols_6", lambda L: _columns(L, 6, 17, 0, POSEIDON2)),
    ("sharded_columns/pair_n_cols_6_hasher_7", lambda L: _columns(L, 6, 2, 0, 7)),
    # bj_sharded_commit_d, one case per check in source order
    ("sharded_commit/null_comm", lambda L: _commit(L, None)),
    ("sharded_commit/unknown_hasher", lambda L: _commit(L, comm(L, 1), hasher=7)),
    ("sharded_commit/n_cols_0", lambda L: _commit(L, comm(L, 1), n_cols=0)),
    ("sharded_commit/n_cols_3_of_2", lambda L: _commit(L, comm(L, 2), n_cols=3)),
    ("sharded_commit/log_lde_0", lambda L: _commit(L, comm(L, 1), log_lde=0, log_k=0)),
    ("sharded_commit/log_k_gt_log_lde", lambda L: _commit(L, comm(L, 1), log_lde=1, log_k=2)),
    ("sharded_commit/log_n_31", lambda L: _commit(L, comm(L, 1), log_n=31)),
    ("sharded_commit/shards_gt_leaves", lambda L: _commit(L, comm(L, 4), n_cols=4, log_n=1, log_k=0)),
    ("sharded_commit/g_over_k_128", lambda L: _commit(L, comm(L, 128), n_cols=128, log_n=8, log_k=0)),
    ("sharded_commit/cap_3", lambda L: _commit(L, comm(L, 1), cap=3)),
    ("sharded_commit/cap_eq_nk", lambda L: _commit(L, comm(L, 1), cap=32)),
    ("sharded_commit/cap_slice_ge_m", lambda L: _commit(L, comm(L, 2), log_n=1, log_lde=1, log_k=0, cap=1, stride=2)),
    ("sharded_commit/stride_lt_n", lambda L: _commit(L, comm(L, 1), stride=15)),
    ("sharded_commit/null_buffer", lambda L: _commit(L, comm(L, 1))),
    ("sharded_commit/pair_null_comm_hasher", lambda L: _commit(L, None, hasher=7)),
    ("sharded_commit/pair_hasher_n_cols", lambda L: _commit(L, comm(L, 1), hasher=7, n_cols=0)),
    ("sharded_commit/pair_n_cols_log_lde", lambda L: _commit(L, comm(L, 1), n_cols=0, log_lde=0, log_k=0)),
    ("sharded_commit/pair_log_lde_log_k", lambda L: _commit(L, comm(L, 1), log_lde=0, log_k=1)),
    ("sharded_commit/pair_log_k_log_n", lambda L: _commit(L, comm(L, 1), log_lde=1, log_k=2, log_n=31)),
    ("sharded_commit/pair_log_n_g_over_k", lambda L: _commit(L, comm(L, 128), n_cols=128, log_n=31, log_k=0)),
    ("sharded_commit/pair_g_over_k_cap", lambda L: _commit(L, comm(L, 128), n_cols=128, log_n=8, log_k=0, cap=3)),
    ("sharded_commit/pair_cap_cap_slice",
     lambda L: _commit(L, comm(L, 2), log_n=1, log_lde=1, log_k=0, cap=3, stride=2)),
    ("sharded_commit/pair_cap_slice_stride",
     lambda L: _commit(L, comm(L, 2), log_n=1, log_lde=1, log_k=0, cap=1, stride=1)),
    # bj_sharded_query_h
    ("sharded_query/null_comm", lambda L: _query(L, None)),
    ("sharded_query/unknown_hasher", lambda L: _query(L, comm(L, 1), hasher=7)),
    ("sharded_query/log_k_gt_log_lde", lambda L: _query(L, comm(L, 1), log_k=3)),
    ("sharded_query/log_n_31", lambda L: _query(L, comm(L, 1), log_n=31)),
    ("sharded_query/shards_gt_leaves", lambda L: _query(L, comm(L, 2), log_n=0, log_k=0)),
    ("sharded_query/n_cols_0", lambda L: _query(L, comm(L, 1), n_cols=0)),
    ("sharded_query/cap_3", lambda L: _query(L, comm(L, 1), cap=3)),
    ("sharded_query/cap_eq_nl", lambda L: _query(L, comm(L, 1), cap=32)),
    ("sharded_query/cap_slice_ge_m", lambda L: _query(L, comm(L, 2), log_n=1, log_k=0, cap=1)),
    ("sharded_query/idx_eq_nl", lambda L: _query(L, comm(L, 1), idx=32)),
    ("sharded_query/null_buffer", lambda L: _query(L, comm(L, 1))),
    ("sharded_query/pair_null_comm_hasher", lambda L: _query(L, None, hasher=7)),
    ("sharded_query/pair_hasher_log_k", lambda L: _query(L, comm(L, 1), hasher=7, log_k=3)),
    ("sharded_query/pair_log_k_geometry", lambda L: _query(L, comm(L, 1), log_k=3, n_cols=0)),
    ("sharded_query/pair_geometry_cap", lambda L: _query(L, comm(L, 1), n_cols=0, cap=3)),
    ("sharded_query/pair_cap_cap_slice", lambda L: _query(L, comm(L, 2), log_n=1, log_k=0, cap=3)),
    ("sharded_query/pair_cap_slice_idx", lambda L: _query(L, comm(L, 2), log_n=1, log_k=0, cap=1, idx=5)),
    # bj_sharded_queries_d
    ("sharded_queries/null_comm", lambda L: _queries(L, None)),
    ("sharded_queries/null_indices", lambda L: _queries(L, comm(L, 1), indices=False)),
    ("sharded_queries/n_oracles_0", lambda L: _queries(L, comm(L, 1), n_oracles=0)),
    ("sharded_queries/n_oracles_17", lambda L: _queries(L, comm(L, 1), n_oracles=17)),
    ("sharded_queries/n_queries_0", lambda L: _queries(L, comm(L, 1), n_queries=0)),
    ("sharded_queries/oracle_null_leaves", lambda L: _queries(L, comm(L, 1), [_oracle(leaves=None)])),
    ("sharded_queries/oracle_null_src", lambda L: _queries(L, comm(L, 1), [_oracle(src=None)])),
    ("sharded_queries/n_leaves_6", lambda L: _queries(L, comm(L, 1), [_oracle(n_leaves=6)])),
    ("sharded_queries/cap_3", lambda L: _queries(L, comm(L, 1), [_oracle(cap_size=3)])),
    ("sharded_queries/oracle_1_n_leaves_differs", lambda L: _queries(L, comm(L, 1), [_oracle(), _oracle(n_leaves=32)])),
    ("sharded_queries/more_ranks_than_leaves", lambda L: _queries(L, comm(L, 4), [_oracle(n_leaves=2, cap_size=1)])),
    ("sharded_queries/cap_slice_ge_m", lambda L: _queries(L, comm(L, 1), [_oracle(cap_size=16)])),
    ("sharded_queries/col_stride_lt_m", lambda L: _queries(L, comm(L, 1), [_oracle(col_stride=8)])),
    ("sharded_queries/unknown_hasher", lambda L: _queries(L, comm(L, 1), [_oracle(hasher=7)])),
    ("sharded_queries/oracle_1_unknown_hasher", lambda L: _queries(L, comm(L, 1), [_oracle(), _oracle(hasher=7)])),
    ("sharded_queries/out_words_0", lambda L: _queries(L, comm(L, 1))),
    ("sharded_queries/pair_null_comm_null_indices", lambda L: _queries(L, None, indices=False)),
    ("sharded_queries/pair_null_indices_n_oracles", lambda L: _queries(L, comm(L, 1), indices=False, n_oracles=0)),
    ("sharded_queries/pair_n_oracles_n_queries", lambda L: _queries(L, comm(L, 1), n_oracles=0, n_queries=0)),
    ("sharded_queries/pair_n_queries_oracle_null",
     lambda L: _queries(L, comm(L, 1), [_oracle(leaves=None)], n_queries=0)),
    ("sharded_queries/pair_oracle_null_pow2", lambda L: _queries(L, comm(L, 1), [_oracle(leaves=None, n_leaves=6)])),
    ("sharded_queries/pair_pow2_differs", lambda L: _queries(L, comm(L, 1), [_oracle(), _oracle(n_leaves=6)])),
    ("sharded_queries/pair_cap_slice_col_stride",
     lambda L: _queries(L, comm(L, 1), [_oracle(cap_size=16, col_stride=8)])),
    ("sharded_queries/pair_col_stride_hasher", lambda L: _queries(L, comm(L, 1), [_oracle(col_stride=8, hasher=7)])),
    # bj_lde_commit_h
    ("lde_commit_h/log_n_plus_log_lde_33", lambda L: _commit_h(L, log_n=31)),
    ("lde_commit_h/log_k_gt_log_lde", lambda L: _commit_h(L, log_lde=1, log_k=2)),
    ("lde_commit_h/cap_0", lambda L: _commit_h(L, cap=0)),
    ("lde_commit_h/cap_3", lambda L: _commit_h(L, cap=3)),
    ("lde_commit_h/cap_eq_nl", lambda L: _commit_h(L, cap=32)),
    ("lde_commit_h/log_lde_0", lambda L: _commit_h(L, log_lde=0, log_k=0)),
    ("lde_commit_h/null_trace", lambda L: _commit_h(L)),
    ("lde_commit_h/pair_log_n_log_k", lambda L: _commit_h(L, log_n=31, log_k=3)),
    ("lde_commit_h/pair_log_k_cap", lambda L: _commit_h(L, log_lde=1, log_k=2, cap=3)),
    ("lde_commit_h/pair_cap_log_lde", lambda L: _commit_h(L, log_lde=0, log_k=0, cap=3)),
    # the trees (capi_tree.hip); zero leaves, so a call that lost its check would have nothing to hash
    ("merkle_nodes/n_leaves_6", lambda L: L.bj_merkle_nodes_d(None, 6, 2, None, None)),
    ("merkle_nodes/n_leaves_eq_cap", lambda L: L.bj_merkle_nodes_d(None, 4, 4, None, None)),
    ("merkle_nodes/cap_3", lambda L: L.bj_merkle_nodes_d(None, 8, 3, None, None)),
    ("blake2s_nodes/n_leaves_6", lambda L: L.bj_blake2s_nodes_d(None, 6, 2, None, None)),
    ("keccak256_nodes/n_leaves_eq_cap", lambda L: L.bj_keccak256_nodes_d(None, 4, 4, None, None)),
    ("merkle_leaves_chunked/elems_3", lambda L: L.bj_merkle_leaves_chunked_d(None, 2, 0, 0, 3, None, None)),
    ("merkle_leaves_chunked/leaf_over_2_32", lambda L: L.bj_merkle_leaves_chunked_d(None, 1 << 31, 0, 0, 4, None, None)),
    ("merkle_leaves_chunked/pair_elems_3_leaf_over_2_32",
     lambda L: L.bj_merkle_leaves_chunked_d(None, 1 << 31, 0, 0, 3, None, None)),
    ("keccak256_leaves_chunked/elems_3", lambda L: L.bj_keccak256_leaves_chunked_d(None, 2, 0, 0, 3, None, None)),
    ("merkle_leaves_partial/non_final_3_cols",
     lambda L: L.bj_merkle_leaves_partial_d(None, 3, 0, 0, None, None, 0, None)),
    ("merkle_leaves_partial/final_continued_empty",
     lambda L: L.bj_merkle_leaves_partial_d(None, 0, 0, 0, _ptr(), None, 1, None)),
    ("blake2s_leaves_partial/cols_before_3", lambda L: _b2s_partial(L, cols_before=3, state=True)),
    ("blake2s_leaves_partial/cols_before_without_state", lambda L: _b2s_partial(L, cols_before=8)),
    ("blake2s_leaves_partial/state_without_cols_before", lambda L: _b2s_partial(L, state=True)),
    ("blake2s_leaves_partial/non_final_3_cols", lambda L: _b2s_partial(L, n_cols=3, final=0)),
    ("blake2s_leaves_partial/final_continued_empty", lambda L: _b2s_partial(L, n_cols=0, cols_before=8, state=True)),
    ("blake2s_leaves_partial/pair_cols_before_3_no_state", lambda L: _b2s_partial(L, cols_before=3)),
    ("blake2s_leaves_partial/pair_no_state_non_final_3",
     lambda L: _b2s_partial(L, n_cols=3, cols_before=8, final=0)),
    ("keccak256_leaves_partial/state", lambda L: _keccak_partial(L, True, True)),
    ("keccak256_leaves_partial/non_final", lambda L: _keccak_partial(L, False, False)),
]


def _init_local(L, world, rank):
    g = ctypes.c_void_p()
    rc = L.bj_comm_local_group_create(world, ctypes.byref(g))
    assert rc == 0, L.bj_last_error()
    out = ctypes.c_void_p()
    rc = L.bj_comm_init_local(g, rank, ctypes.byref(out))
    msg = L.bj_last_error()
    assert rc != 0 and not out.value
    assert L.bj_comm_local_group_destroy(g) == 0
    return rc, msg


# these make a local group: 2 * world events on the current device
DEVICE = [
    ("init_local/rank_eq_world", lambda L: _init_local(L, 2, 2)),
    ("init_local/rank_negative", lambda L: _init_local(L, 4, -1)),
]


def run(L, cases):
    """{name: {"rc": code, "error": bj_last_error() after the call}}"""
    out = {}
    for name, fn in cases:
        r = fn(L)
        rc, msg = r if isinstance(r, tuple) else (r, L.bj_last_error())
        out[name] = {"rc": rc, "error": (msg or b"").decode()}
    while _comms:
        assert L.bj_comm_destroy(_comms.pop()) == 0
    return out
