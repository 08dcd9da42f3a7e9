"""The node levels of the three tree hashers through bj_*_nodes_d alone (csrc/tree_hasher.hpp: one
per-lane level kernel and one one-workgroup tail, instantiated per hasher; csrc/merkle.hip: the
Poseidon2 quad-lane and fused levels), every level bit-exact against the oracle's node hash over
random canonical digests, and the argument checks the tree entry points share
(csrc/capi_tree.hip), with their error texts."""
import ctypes
import os

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
EINVAL = -22

# hasher -> (nodes, chunked leaves, node seam, leaf seam)
ENTRY = {
    "poseidon2": ("bj_merkle_nodes_d", "bj_merkle_leaves_chunked_d", "bj_hash_into_node_h", "bj_hash_into_leaf_h"),
    "blake2s": ("bj_blake2s_nodes_d", "bj_blake2s_leaves_chunked_d", "bj_blake2s_node_h", "bj_blake2s_leaf_h"),
    "keccak256": ("bj_keccak256_nodes_d", "bj_keccak256_leaves_chunked_d", "bj_keccak256_node_h",
                  "bj_keccak256_leaf_h"),
}

# (N, cap): one node; the tail at its limit of 4096 digests (Blake2s, Keccak); one per-lane level,
# then a tail that stops after one level; a level and a multi-level tail; Poseidon2 only: one
# per-lane level above the quad threshold (2^15 nodes), then the quad and fused levels
SHAPES = [(2, 1), (4096, 1), (8192, 2048), (8192, 8)]
CASES = [(h, n, c) for h in ENTRY for n, c in SHAPES] + [("poseidon2", 1 << 17, 16)]


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import field
    return type("BJ", (), dict(torch=torch, field=field, lib=boojum_amd.load()))


@pytest.mark.parametrize("hasher,n,cap", CASES)
def test_every_level_matches_oracle(bj, hasher, n, cap):
    digests = np.random.default_rng(n + cap).integers(0, O.P, size=(n, 4), dtype=np.uint64)
    src = bj.field.to_device(digests)
    out = bj.torch.empty((n - cap, 4), dtype=bj.torch.int64, device="cuda")
    assert getattr(bj.lib, ENTRY[hasher][0])(src.data_ptr(), n, cap, out.data_ptr(), 0) == 0, bj.lib.bj_last_error()
    got = bj.field.to_host(out)
    want, _ = O.merkle_nodes(digests, cap, threads=THREADS, hasher=hasher)
    assert got.shape == want.shape
    off, m = 0, n // 2
    while m >= cap:
        bad = np.argwhere(got[off:off + m] != want[off:off + m])
        assert bad.size == 0, "level of %d nodes: first mismatches at %s" % (m, bad[:5].tolist())
        off, m = off + m, m // 2
    assert off == n - cap


def rejected(bj, fn, *args):
    rc = getattr(bj.lib, fn)(*args)
    return rc, bj.lib.bj_last_error().decode()


@pytest.mark.parametrize("hasher", list(ENTRY))
def test_shared_argument_checks(bj, hasher):
    f_nodes, f_chunked, f_node_h, f_leaf_h = ENTRY[hasher]
    buf = bj.torch.zeros((8, 4), dtype=bj.torch.int64, device="cuda")
    p = buf.data_ptr()
    nodes_msg = "need power-of-two n_leaves > cap_size (merkle_tree.rs:83-96)"
    assert rejected(bj, f_nodes, p, 6, 1, p, 0) == (EINVAL, nodes_msg)   # N not a power of two
    assert rejected(bj, f_nodes, p, 4, 4, p, 0) == (EINVAL, nodes_msg)   # N == cap
    assert rejected(bj, f_nodes, p, 8, 3, p, 0) == (EINVAL, nodes_msg)   # cap not a power of two
    assert rejected(bj, f_chunked, p, 1, 8, 2, 3, p, 0) == (
        EINVAL, "elements_to_take_per_leaf must be a power of two")
    # 2^31 columns of 2 elements: one more than a 32-bit leaf length (rejected before any launch)
    assert rejected(bj, f_chunked, p, 1 << 31, 8, 1, 2, p, 0) == (EINVAL, "leaf too long")
    out = np.zeros(4, dtype=np.uint64)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert rejected(bj, f_leaf_h, None, 1 << 32, outp) == (EINVAL, "leaf too long")
    # the node seam is the (2, 1) tree through the same check
    lr = np.random.default_rng(7).integers(0, O.P, size=(2, 4), dtype=np.uint64)
    lp = lr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    rp = ctypes.cast(lr.ctypes.data + 32, ctypes.POINTER(ctypes.c_uint64))
    assert getattr(bj.lib, f_node_h)(lp, rp, outp) == 0, bj.lib.bj_last_error()
    assert np.array_equal(out, O.merkle_nodes(lr, 1, hasher=hasher)[0][0])
