"""Checker of what-if route lists (spf_whatif_routes), in numpy.

A set's route is the reference's selection restated: the min of the metrics
over its reachable members (getMinCostNodes, Decision.cpp:1082-1105) and the OR
of the next-hop words of the members at that min (getNextHopsWithMetric without
LFA).  A set that holds the source is the source's own prefix: metric 0, no
next hops.  For failure i the plan's unfailed result is patched with list i
(whatif_lists.patched) and the expected route list is exactly the sets whose
(min_metric, nh) differs from the base's.  The lists themselves are pinned to
the CPU oracle by whatif_lists.check_failure, which the GPU tests call on the
same failures first.
"""

import numpy as np

import whatif_lists as L

U64_MAX = L.U64_MAX


def flatten(sets):
    """(ptr, nodes) of a list of member sequences, as the C-ABI takes them."""
    ptr = np.zeros(len(sets) + 1, np.int64)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    nodes = np.array([int(v) for s in sets for v in s], np.int64)
    return ptr, nodes


def routes(dist, nh, sets, src):
    """Every set's (min_metric[n_sets] u64, nh[n_sets, W] u32) on one result;
    `sets` as member sequences or flattened already."""
    W = nh.shape[1]
    ptr, nodes = sets if isinstance(sets, tuple) else flatten(sets)
    m = np.full(len(ptr) - 1, U64_MAX, np.uint64)
    words = np.zeros((len(ptr) - 1, W), np.uint32)
    size = np.diff(ptr)
    full = np.nonzero(size)[0]  # reduceat over the non-empty sets: their starts ascend strictly
    if len(full) == 0:
        return m, words
    at = ptr[full]
    d = dist[nodes]  # (a repeated member changes neither a min nor an OR)
    lo = np.minimum.reduceat(d, at)
    mine = np.logical_or.reduceat(nodes == src, at)
    at_min = (d == np.repeat(lo, size[full])) & (d != U64_MAX)
    for w in range(W):
        words[full, w] = np.bitwise_or.reduceat(np.where(at_min, nh[nodes, w], np.uint32(0)), at)
    m[full] = np.where(mine, np.uint64(0), lo)
    words[full[mine]] = 0
    return m, words


def expected(base_dist, base_nh, node, dist, nh, sets, src, base=None):
    """Failure's route list from its change list: (set ids ascending,
    min_metric, nh words) of the sets whose route differs from the base's."""
    bm, bw = base if base is not None else routes(base_dist, base_nh, sets, src)
    d, n = L.patched(base_dist, base_nh, np.asarray(node, np.int64), dist, nh)
    m, w = routes(d, n, sets, src)
    ids = np.nonzero((m != bm) | (w != bw).any(axis=1))[0]
    return ids.astype(np.uint32), m[ids], w[ids]


SEED = 11  # of case_sets; checked against the oracle in test_whatif_routes_host.py


def case_sets(n_nodes, src, seed=SEED):
    """The destination sets of the GPU tests over one graph, and where each
    family starts: {name: first set id}."""
    rng = np.random.default_rng(seed)
    others = np.array([v for v in range(n_nodes) if v != src])
    sets, at = [], {}
    at["a"] = len(sets)  # one set per node (the source's own included)
    sets += [[v] for v in range(n_nodes)]
    at["b"] = len(sets)  # anycast: 64 sets of 2 to 8 members
    for _ in range(64):
        sets.append([int(v) for v in rng.choice(others, int(rng.integers(2, 9)), replace=False)])
    at["c"] = len(sets)  # every node but the source (with it, the set would be the source's own)
    sets.append([int(v) for v in others])
    at["d"] = len(sets)  # 100 members (drawn with replacement where the graph is smaller)
    sets.append([int(v) for v in rng.choice(others, 100, replace=len(others) < 100)])
    at["e"] = len(sets)  # empty
    sets.append([])
    at["f"] = len(sets)  # two identical sets
    sets += [list(sets[at["b"]]), list(sets[at["b"]])]
    at["g"] = len(sets)  # a repeated member
    x, y = (int(v) for v in rng.choice(others, 2, replace=False))
    sets.append([x, y, x, x])
    at["h"] = len(sets)  # the source among others
    sets.append([int(others[0]), int(src), int(others[-1])])
    return sets, at


def changed_nodes(base, res):
    """The change list that turns the result `base` into `res`: (node, dist, nh)."""
    node = np.nonzero((base[0] != res[0]) | (base[1] != res[1]).any(axis=1))[0]
    return node, res[0][node], res[1][node]
