"""The query phase (prover.rs:2161-2266) on the GPU: every OracleQuery of a proof from one launch
and one device-to-host copy (bj_oracle_queries_d).

An OracleQuery (proof.rs:48-97) is the elements a leaf hashed (QuerySource::get_elements,
fri/mod.rs:683-927) and the leaf's Merkle path (MerkleTreeWithCap::get_proof,
merkle_tree.rs:462-480).  A query index here is the flat leaf index coset_idx * domain_size +
inner_idx of the committed LDE domain; an oracle's tree index is that index shifted right by the
oracle's `index_shift`, which is all of the reference's index arithmetic (`fri_plan`).

* `QueryOracle` describes one oracle: its tree and the tensor its leaves were hashed from.
* `construct_queries` answers a batch of indices for up to 16 oracles that cover one domain.
* `OracleQuery.construct` takes the reference's arguments and runs a batch of one.
* `single_round_queries` returns the proof's `queries_per_fri_repetition` in the serde shape.

The transcript that draws the indices and the proof of work are outside this path; the indices are
inputs, as the FRI challenges are in fri.py.
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._lib import QUERY_MAX_ORACLES, BoojumError, QueryOracleDesc, call
from . import serialization
from .field import STATUS_WORDS, log2_exact


# ------------------------------------------------------------------ layout (host arithmetic only)

def fri_plan(log_n, log_lde, schedule):
    """The FRI oracles of a folding schedule s_0, s_1, ... over the 2^(log_n + log_lde) domain, as
    [(elements_per_leaf, index_shift, n_leaves)] per oracle.  Oracle k chunks 2^s_k values of each
    of its two columns into a leaf (fri/mod.rs:179-187, 258-266) and its tree index is
      (coset << (log2 domain_size_k - s_k)) + (inner_k >> s_k),
    domain_size_k = n >> (s_0 + ... + s_{k-1}), inner_k = inner >> (s_0 + ... + s_{k-1})
    (prover.rs:2226-2254, proof.rs:89-91).  Because inner < n that is the flat index coset * n +
    inner shifted right by s_0 + ... + s_k."""
    out, shift = [], 0
    for s in schedule:
        if s < 1:
            raise ValueError("a folding step is at least 1")
        shift += s
        if shift > log_n:
            raise ValueError("the schedule folds more than the 2^%d rows of a coset" % log_n)
        out.append((1 << s, shift, 1 << (log_n + log_lde - shift)))
    return out


def query_words(n_cols, elements_per_leaf, n_leaves, cap_size):
    """bj_oracle_query_words: the leaf's n_cols * elements_per_leaf elements, the leaf hash, and
    4 words for each of the log2(n_leaves / cap_size) siblings."""
    log2_exact(elements_per_leaf)
    depth = log2_exact(n_leaves) - log2_exact(cap_size)
    if depth < 0:
        raise ValueError("n_leaves < cap_size")
    return n_cols * elements_per_leaf + 4 + 4 * depth


def block_offsets(words, n_queries):
    """Where each oracle's block starts in the output (words[o] = the oracle's record words):
    n_queries * the record words of the oracles before it; the last entry is the total."""
    out, at = [], 0
    for w in words:
        out.append(at)
        at += n_queries * w
    return out + [at]


OracleQueries = namedtuple("OracleQueries", "leaf_elements leaf_hash proof")


def parse_queries(buf, shapes, n_queries):
    """Split the output of bj_oracle_queries_d: buf a flat uint64 array, shapes one
    (leaf elements, depth) per oracle.  Returns per oracle OracleQueries(leaf_elements (Q, C * E),
    leaf_hash (Q, 4), proof (Q, depth, 4)), views of buf."""
    buf = np.asarray(buf, dtype=np.uint64).reshape(-1)
    words = [n_el + 4 + 4 * depth for n_el, depth in shapes]
    offs = block_offsets(words, n_queries)
    if buf.size < offs[-1]:
        raise ValueError("buffer of %d words is shorter than the %d the oracles need" % (buf.size, offs[-1]))
    out = []
    for (n_el, depth), w, at in zip(shapes, words, offs):
        rec = buf[at: at + n_queries * w].reshape(n_queries, w)
        out.append(OracleQueries(rec[:, :n_el], rec[:, n_el: n_el + 4],
                                 rec[:, n_el + 4:].reshape(n_queries, depth, 4)))
    return out


# ------------------------------------------------------------------ device side

class QueryOracle:
    """One oracle of a query batch: `tree` (merkle.MerkleTreeWithCap) and the tensor its leaves were
    hashed from.  `sources` takes what MerkleTreeWithCap.construct* take: a (C, D, n) LDE tensor (a
    tree over the first k of its D cosets reads the same tensor through the column stride) or
    (C, L) flat rows; None answers paths only.  elements_per_leaf is 1 for `construct` trees and
    the chunk size for the `construct_by_chunking*` ones.  The tree index of a query index is
    index >> index_shift."""

    def __init__(self, tree, sources=None, elements_per_leaf=1, index_shift=0):
        from .merkle import _leaf_sources
        self.tree, self.sources = tree, sources
        self.elements_per_leaf, self.index_shift = elements_per_leaf, index_shift
        self.log_e = log2_exact(elements_per_leaf)
        self.n_leaves, self.cap_size = tree.n_leaves, tree.cap_size
        self.n_cols, self.col_stride, self._src = 0, 0, None
        if sources is not None:
            src, c, stride, total = _leaf_sources(sources)
            if total < self.n_leaves * elements_per_leaf:
                raise ValueError("sources hold %d elements per column, the tree's leaves hash %d"
                                 % (total, self.n_leaves * elements_per_leaf))
            if src.device != tree.leaf_hashes.device:
                raise ValueError("sources and tree are on different devices")
            self.n_cols, self.col_stride, self._src = c, stride, src
        self.depth = log2_exact(self.n_leaves) - log2_exact(self.cap_size)
        self.n_elements = self.n_cols * elements_per_leaf
        self.words = query_words(self.n_cols, elements_per_leaf, self.n_leaves, self.cap_size)

    @property
    def domain(self):
        return self.n_leaves << self.index_shift

    def descriptor(self):
        t = self.tree
        return QueryOracleDesc(self._src.data_ptr() if self.n_cols else None, self.col_stride, self.n_cols, self.log_e,
                               t.leaf_hashes.data_ptr(), t.nodes.data_ptr() if self.depth else None,
                               self.n_leaves, self.cap_size, self.index_shift)


def _descriptors(oracles):
    if not 1 <= len(oracles) <= QUERY_MAX_ORACLES:
        raise ValueError("1..%d oracles, got %d" % (QUERY_MAX_ORACLES, len(oracles)))
    return (QueryOracleDesc * len(oracles))(*[o.descriptor() for o in oracles])


def oracle_query_words(oracle):
    """bj_oracle_query_words of a QueryOracle, asked of the library."""
    from ._lib import load
    return int(load().bj_oracle_query_words(ctypes.byref(oracle.descriptor())))


def launch_queries(oracles, indices_d, out_d, status_d):
    """The bare bj_oracle_queries_d call on the current stream of out_d's device: asynchronous,
    nothing allocated, so it can be captured in a graph.  indices_d: (Q,) int64 device tensor;
    out_d: at least Q * sum of the oracles' words; status_d: (4,)."""
    from .field import stream_of
    call("bj_oracle_queries_d", _descriptors(oracles), len(oracles), indices_d.data_ptr(), indices_d.numel(),
         out_d.data_ptr(), out_d.numel(), status_d.data_ptr(), stream_of(out_d))


def construct_queries(oracles, indices):
    """Every oracle's query at every index: one call, one device-to-host copy.  oracles: 1..16
    QueryOracle over one domain; indices: flat leaf indices (a sequence of ints, or an int64 device
    tensor).  Returns per oracle OracleQueries(leaf_elements (Q, C * E), leaf_hash (Q, 4),
    proof (Q, depth, 4)) as numpy uint64.  Raises BoojumError when an index is outside the
    domain."""
    import torch
    from .field import to_host
    dev = oracles[0].tree.leaf_hashes.device
    if isinstance(indices, torch.Tensor):
        idx = indices.reshape(-1).to(device=dev, dtype=torch.int64)
    else:
        idx = torch.from_numpy(np.ascontiguousarray(np.asarray(indices, dtype=np.uint64)).view(np.int64)).to(dev)
    q = idx.numel()
    total = q * sum(o.words for o in oracles)
    # the status record rides behind the records, so one copy brings both
    buf = torch.empty((total + STATUS_WORDS,), dtype=torch.int64, device=dev)
    launch_queries(oracles, idx, buf[:total], buf[total:])
    host = to_host(buf)
    status = host[total:]
    if status[0]:
        raise BoojumError("%d query index(es) outside the domain of %d leaves, the first at position %d"
                          % (int(status[0]), oracles[0].domain, int(status[1])))
    return parse_queries(host[:total], [(o.n_elements, o.depth) for o in oracles], q)


class OracleQuery(namedtuple("OracleQuery", "leaf_elements proof")):
    """proof.rs:48-63: leaf_elements (k,) and proof (depth, 4), numpy uint64."""

    @classmethod
    def construct(cls, tree, source, lde_factor, coset_idx, domain_size, inner_idx, num_elements):
        """OracleQuery::construct (proof.rs:64-97) with the reference's arguments: the leaf that
        holds row inner_idx of coset coset_idx, num_elements values of every column of `source` per
        leaf; tree index (coset_idx << (log2 domain_size - log2 num_elements)) + inner_idx /
        num_elements.  A batch of one."""
        log2_exact(domain_size)
        if not 0 <= coset_idx < lde_factor or not 0 <= inner_idx < domain_size:
            raise ValueError("coset_idx or inner_idx out of range")
        o = QueryOracle(tree, source, num_elements, log2_exact(num_elements))
        r = construct_queries([o], [coset_idx * domain_size + inner_idx])[0]
        return cls(r.leaf_elements[0], r.proof[0])

    def to_json(self, hasher="poseidon2"):
        return serialization.oracle_query_to_json(self.leaf_elements, self.proof, hasher)


def single_round_queries(witness, stage_2, quotient, setup, fri_oracles, indices):
    """queries_per_fri_repetition (prover.rs:2161-2266, SingleRoundQueries of proof.rs:99-116) in
    the serde shape: for each index {"witness_query", "stage_2_query", "quotient_query",
    "setup_query", "fri_queries": [...]}, every query through serialization.oracle_query_to_json.
    The arguments are QueryOracle; fri_oracles in schedule order (`fri_plan` gives their shifts)."""
    oracles = [witness, stage_2, quotient, setup] + list(fri_oracles)
    res = construct_queries(oracles, indices)
    n_queries = res[0].leaf_hash.shape[0]

    def one(o, q):
        return serialization.oracle_query_to_json(res[o].leaf_elements[q], res[o].proof[q], oracles[o].tree.hasher)

    return [{"witness_query": one(0, q), "stage_2_query": one(1, q), "quotient_query": one(2, q),
             "setup_query": one(3, q), "fri_queries": [one(o, q) for o in range(4, len(oracles))]}
            for q in range(n_queries)]
