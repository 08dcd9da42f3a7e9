"""GPU parity of the Poseidon2 full rounds' lazy S-box hand-off (csrc/poseidon2.hpp: the last
product of each full-round S-box goes to the external MDS as unreduced limbs,
glasm::mul_lazy_x4), bit for bit against the CPU oracle at the smallest shapes that reach every
output form of the permutation:
* all 12 words (bj_poseidon2_permute) on edge and random states, where the offsets the limbs
  carry and the words' extremes meet;
* leaves of 1..33 columns: the digest form alone, capacity forms followed by a digest form,
  and the zero-padded last group;
* a small tree over such leaves.
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

P = O.P


@pytest.fixture(scope="module")
def bj():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import boojum_amd
    from boojum_amd import field, merkle
    boojum_amd.load()
    return type("BJ", (), dict(torch=torch, field=field, merkle=merkle))


def rand(shape, seed):
    return np.random.default_rng(seed).integers(0, P, size=shape, dtype=np.uint64)


def test_permute_256_states(bj):
    from boojum_amd._lib import call
    st = rand((256, 12), 29)
    st[0] = 0
    st[1] = P - 1
    st[2] = np.uint64(0xFFFFFFFF)
    st[3] = np.uint64(0xFFFFFFFF) << np.uint64(32)
    st[4] = np.uint64(2**64 - 1)  # non-canonical
    t = bj.field.to_device(st)
    call("bj_poseidon2_permute_d", t.data_ptr(), st.shape[0], bj.field.stream_of(t))
    got = bj.field.to_host(t)
    want = np.stack([O.poseidon2_permutation(np.array([int(x) % P for x in row], dtype=np.uint64)) for row in st])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("c", [1, 7, 8, 9, 16, 17, 33])
def test_leaves_64_rows(bj, c):
    src = rand((c, 64), 100 + c)
    src[:, 0] = 0
    src[:, 1] = P - 1
    src[:, 2] = np.uint64(0xFFFFFFFF)
    tree = bj.merkle.MerkleTreeWithCap.construct(bj.field.to_device(src), 1)
    leaves = O.merkle_construct(src, 1, threads=1)[0]
    assert np.array_equal(bj.field.to_host(tree.leaf_hashes), leaves)


def test_tree_1024_leaves_16_columns_cap_4(bj):
    src = rand((16, 1 << 10), 7)
    tree = bj.merkle.MerkleTreeWithCap.construct(bj.field.to_device(src), 4)
    leaves, nodes, _, cap = O.merkle_construct(src, 4, threads=4)
    assert np.array_equal(bj.field.to_host(tree.leaf_hashes), leaves)
    assert np.array_equal(bj.field.to_host(tree.nodes), nodes)
    assert np.array_equal(np.asarray(tree.get_cap(), dtype=np.uint64), np.asarray(cap, dtype=np.uint64))
