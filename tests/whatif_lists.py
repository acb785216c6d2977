"""Checker of what-if change lists (spf_whatif_changes), in numpy.

The oracle has no list call: the pin is its digest.  A failure's list is
right when the unfailed result patched with it has the oracle's digest for
that failure -- the hash of include/openr_spf.h recomputed here from its
definition over every node, listed or not, and n_dist_changed /
n_nh_changed recounted from the entries against the base.
"""

import numpy as np

U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
_FNV_OFFSET = np.uint64(0xCBF29CE484222325)
_FNV_PRIME = np.uint64(0x100000001B3)


def mix64(z):
    """splitmix64's finaliser over a u64 array (mod 2^64)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def fnv_rows(nh):
    """FNV-1a 64 over each row's u32 words: nh [n, W] -> [n] u64."""
    nh = np.asarray(nh, np.uint32)
    f = np.full(nh.shape[0], _FNV_OFFSET, np.uint64)
    with np.errstate(over="ignore"):
        for w in range(nh.shape[1]):
            f = (f ^ nh[:, w].astype(np.uint64)) * _FNV_PRIME
    return f


def result_hash(dist, nh) -> int:
    """sum over reachable v of mix(mix(v + 1) + metric(v)) ^ fnv1a64(nh(v)), mod 2^64."""
    dist = np.asarray(dist, np.uint64)
    ok = dist != U64_MAX
    v = np.arange(1, len(dist) + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(mix64(v) + dist) ^ fnv_rows(nh)
        return int(h[ok].sum(dtype=np.uint64))


def neighbours(rp, col, s):
    """The distinct up neighbours of s, ascending id: the bitset's bit order."""
    return sorted(set(int(x) for x in col[int(rp[s]): int(rp[s + 1])]) - {int(s)})


def words_of(k: int) -> int:
    return max(1, (k + 31) // 32)


def base_from_oracle(orc, names, rp, col, s):
    """OracleLinkState.spf(names[s]) as (dist[N] u64, nh[N, W] u32)."""
    nbrs = neighbours(rp, col, s)
    bit = {names[v]: j for j, v in enumerate(nbrs)}
    index = {n: i for i, n in enumerate(names)}
    dist = np.full(len(names), U64_MAX, np.uint64)
    nh = np.zeros((len(names), words_of(len(nbrs))), np.uint32)
    for node, e in orc.spf(names[s]).items():
        v = index[node]
        dist[v] = e["metric"]
        for hop in e["nextHops"]:
            j = bit[hop]
            nh[v, j >> 5] |= np.uint32(1 << (j & 31))
    return dist, nh


def patched(base_dist, base_nh, node, dist, nh):
    d, n = base_dist.copy(), base_nh.copy()
    d[node] = dist
    n[node] = nh
    return d, n


def check_failure(base_dist, base_nh, node, dist, nh, want, where=""):
    """One failure's list against the oracle's digest `want` =
    (n_dist_changed, n_nh_changed, hash)."""
    node = np.asarray(node, np.int64)
    assert len(np.unique(node)) == len(node), f"{where}: a node is listed twice"
    gone = dist == U64_MAX
    assert not nh[gone].any(), f"{where}: an unreachable entry has next-hop words"
    d_ch = dist != base_dist[node]
    # nextHops() changed: the words differ, or the node became unreachable
    n_ch = (nh != base_nh[node]).any(axis=1) | (gone & (base_dist[node] != U64_MAX))
    assert (d_ch | n_ch).all(), f"{where}: a listed node equals the base"
    nd, nn = int(d_ch.sum()), int(n_ch.sum())
    assert max(want[0], want[1]) <= len(node) <= want[0] + want[1], (where, len(node), want)
    d, n = patched(base_dist, base_nh, node, dist, nh)
    got = (nd, nn, result_hash(d, n))
    assert got == tuple(want), f"{where}: patched result {got}, oracle {tuple(want)}"
