"""CPU model of bj_sharded_queries_d (csrc/collective.hip, csrc/queries.hip): pure numpy, no GPU and
no library.

A tree is (leaves (nl, 4), nodes (nl - cap, 4)) in bj_merkle_nodes_d's layout: level l >= 1 holds
nl >> l digests and follows the lower levels in `nodes`; the last level is the cap.  The node
function is a parameter: the model only moves digests, so any function of (left, right) will do.

* `build_tree` hashes a full tree; `plain_records` are the get_proof-order records the call must
  reproduce (bj_oracle_queries_d's, e = 0, index_shift = 0).
* `shard_tree` cuts rank P's leaves and subtree out of the full tree.
* `sharded_queries` restates the call's schedule over G ranks: top levels, owner records, gather,
  select.  It returns every rank's (out, status).
"""
import numpy as np

U64 = np.uint64


def log2(n):
    if n <= 0 or n & (n - 1):
        raise ValueError("size must be a power of two, got %d" % n)
    return n.bit_length() - 1


def mix_node(left, right):
    """A cheap stand-in node function on (k, 4) uint64 digests (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        return (left * U64(0x9E3779B97F4A7C15) + np.roll(right, 1, axis=1) * U64(0xC2B2AE3D27D4EB4F)
                + (left >> U64(29)) + U64(1))


def tree_nodes(leaves, cap, node=mix_node):
    """bj::tree_nodes: the levels over `leaves` down to `cap` digests, concatenated."""
    levels, cur = [], np.asarray(leaves, dtype=U64)
    while cur.shape[0] > cap:
        cur = node(cur[0::2], cur[1::2])
        levels.append(cur)
    return np.concatenate(levels) if levels else np.zeros((0, 4), dtype=U64)


def build_tree(leaves, cap, node=mix_node):
    return np.asarray(leaves, dtype=U64), tree_nodes(leaves, cap, node)


def level(leaves, nodes, lvl):
    """Level lvl of a tree in the layout above: level 0 the leaves, level l >= 1 at digest
    n - (n >> (l - 1)) of nodes."""
    n = leaves.shape[0]
    if lvl == 0:
        return leaves
    start = n - (n >> (lvl - 1))
    return nodes[start: start + (n >> lvl)]


def words(n_cols, n_leaves, cap):
    """bj_sharded_query_words."""
    return n_cols + 4 + 4 * (log2(n_leaves) - log2(cap))


def plain_records(src, leaves, nodes, cap, indices):
    """The unsharded records, (Q, W): the row of src (C, nl) or nothing for src None, the leaf
    hash, then sibling l = entry (t >> l) ^ 1 of level l (MerkleTreeWithCap::get_proof order).  An
    index >= nl gives a zero record."""
    nl = leaves.shape[0]
    depth = log2(nl) - log2(cap)
    n_cols = 0 if src is None else src.shape[0]
    out = np.zeros((len(indices), n_cols + 4 + 4 * depth), dtype=U64)
    for q, t in enumerate(indices):
        if t >= nl:
            continue
        parts = [src[:, t]] if n_cols else []
        parts.append(leaves[t])
        parts += [level(leaves, nodes, l)[(t >> l) ^ 1] for l in range(depth)]
        out[q] = np.concatenate(parts)
    return out


def shard_tree(leaves, nodes, cap, G, P):
    """Rank P's (leaves (m, 4), nodes (m - cap_local, 4)) of a G-way commit of the full tree
    (leaves, nodes, cap): local level l is the P-th slice of global level l, down to
    cap_local = max(1, cap / G) digests (the relation check_rank of test_gpu_native_sharded.py
    asserts of bj_sharded_commit_d's outputs).  With cap < G the global levels above the G subtree
    roots belong to no shard.  Works on numpy arrays and on torch tensors alike (slices only)."""
    nl = leaves.shape[0]
    m, cap_local = nl // G, max(1, cap // G)
    if m <= cap_local:
        raise ValueError("each shard needs more leaves than its cap slice")
    local, l = [], 1
    while (m >> l) >= cap_local:
        cnt = m >> l
        local.append(level(leaves, nodes, l)[P * cnt: (P + 1) * cnt])
        l += 1
    if isinstance(leaves, np.ndarray):
        return leaves[P * m: (P + 1) * m], np.concatenate(local)
    import torch
    return leaves[P * m: (P + 1) * m], torch.cat(local)


def status_record(indices, nl):
    bad = [q for q, t in enumerate(indices) if t >= nl]
    return np.array([len(bad), bad[0] if bad else 2 ** 64 - 1, 0, 0], dtype=U64)


def sharded_queries(oracles, G, indices, node=mix_node, fill=0xDEAD):
    """The schedule of bj_sharded_queries_d over G ranks.  oracles: one dict per oracle with
    "shards" (per rank (src (C, m) or None, leaves, nodes)), "n_leaves", "cap" and optionally "node".
    Returns per rank (out (Q * sum W,), status (4,)).  Staging buffers start as `fill`, so a slot
    that no owner wrote shows if it is ever selected."""
    nl = oracles[0]["n_leaves"]
    assert all(o["n_leaves"] == nl for o in oracles)
    m, nq = nl // G, len(indices)
    W = [words(0 if o["shards"][0][0] is None else o["shards"][0][0].shape[0], nl, o["cap"]) for o in oracles]
    at = [nq * sum(W[:i]) for i in range(len(oracles) + 1)]

    # 1. top levels: the subtree roots of the oracles with cap < G, gathered together, then the
    #    levels over each such oracle's G roots (the same on every rank)
    top_of = [i for i, o in enumerate(oracles) if o["cap"] < G]
    sent = [np.concatenate([oracles[i]["shards"][P][2][-1:] for i in top_of]) if top_of else None for P in range(G)]
    tops = {}
    for t, i in enumerate(top_of):
        roots = np.stack([sent[P][t] for P in range(G)])
        tops[i] = (roots, tree_nodes(roots, oracles[i]["cap"], oracles[i].get("node", node)))

    # 2. every rank writes the records it owns at their final offsets of its staging buffer
    staging = np.full((G, at[-1]), fill, dtype=U64)
    for P in range(G):
        for i, o in enumerate(oracles):
            src, leaves, nodes = o["shards"][P]
            cap_local = max(1, o["cap"] // G)
            local_depth = log2(m) - log2(cap_local)
            top_depth = log2(G) - log2(o["cap"]) if o["cap"] < G else 0
            for q, idx in enumerate(indices):
                if idx >= nl or idx // m != P:
                    continue
                loc = idx % m
                parts = [src[:, loc]] if src is not None else []
                parts.append(leaves[loc])
                parts += [level(leaves, nodes, l)[(loc >> l) ^ 1] for l in range(local_depth)]
                parts += [level(*tops[i], l)[(P >> l) ^ 1] for l in range(top_depth)]
                rec = np.concatenate(parts)
                assert rec.size == W[i]
                staging[P, at[i] + q * W[i]: at[i] + (q + 1) * W[i]] = rec
    # 3. one all-gather: every rank holds all G staging buffers; 4. select the owner's copy
    outs = []
    for P in range(G):
        gathered = staging.copy()
        out = np.empty(at[-1], dtype=U64)
        for i in range(len(oracles)):
            for q, idx in enumerate(indices):
                lo, hi = at[i] + q * W[i], at[i] + (q + 1) * W[i]
                out[lo:hi] = gathered[idx // m, lo:hi] if idx < nl else 0
        outs.append((out, status_record(indices, nl)))
    return outs
