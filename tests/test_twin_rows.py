"""The facts class rows rest on, pinned on the CPU against the
oracle's all-sources distances (OracleLinkState.dense), no device:

 1. for a fixed source s, d(s, v) for v != s depends only on the class of v
    (false twins: nodes with equal distinct-neighbour sets);
 2. for twins s, s', d(s, .) and d(s', .) agree at every node outside {s, s'};
 3. every member of s's class other than s lies at one distance t_C: 2 when
    some neighbour forwards (is not drained), longer or unreachable otherwise.

On the 19-node and 592-node fabrics of test_gpu_msbfs_quotient.py: undrained,
a drained rack switch whose twins are not, a class drained as a whole, and
every neighbour of one class drained."""

import numpy as np
import pytest

from oracle import OracleLinkState
from openr_amd import topology as T
from openr_amd.engine import graph_from_lsdb
from openr_amd.lsdb import PackedLsdb

INF = np.iinfo(np.uint64).max


def small_fabric():
    return T.fabric(2 * 2 + 3 * (2 + 3), ssw_per_plane=2, fsw_per_pod=2, rsw_per_pod=3)


def mid_fabric():
    return T.fabric(4 * 4 + 24 * (4 + 20), ssw_per_plane=4, fsw_per_pod=4, rsw_per_pod=20)


def drained(lsdb, names):
    dbs = lsdb.dbs.copy()
    all_names = [bytes(lsdb.blob[o: o + n]).decode() for o, n in zip(dbs["name_off"], dbs["name_len"])]
    for n in names:
        dbs["is_overloaded"][all_names.index(n)] = 1
    return PackedLsdb(lsdb.blob, dbs, lsdb.adjs.copy())


STATES = {
    "small": (small_fabric, {"undrained": [], "twin": ["3-1-2"], "class": ["3-1-0", "3-1-1", "3-1-2"],
                             "neighbours": ["2-1-0", "2-1-1"]}),
    "mid": (mid_fabric, {"undrained": [], "twin": ["3-5-7"], "class": [f"3-5-{r}" for r in range(20)],
                         "neighbours": [f"2-9-{f}" for f in range(4)]}),
}
CASES = [(g, s) for g, (_, states) in STATES.items() for s in states]


@pytest.mark.parametrize("graph,state", CASES, ids=[f"{g}-{s}" for g, s in CASES])
def test_distances_are_functions_of_classes(graph, state):
    make, states = STATES[graph]
    lsdb = drained(make().lsdb, states[state])
    names, rp, col, met, lid, ovl = graph_from_lsdb(lsdb)
    n = len(names)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    D, _ = orc.dense(names, list(range(n)))
    nbrs = [frozenset(int(x) for x in col[int(rp[v]): int(rp[v + 1])]) for v in range(n)]
    ids = {}
    cls = np.array([ids.setdefault(nbrs[v], len(ids)) for v in range(n)])
    members = [np.nonzero(cls == c)[0] for c in range(len(ids))]
    assert len(ids) < n  # twins exist
    for s in range(n):
        for c, m in enumerate(members):  # fact 1 (and 3: c = s's class, one distance t_C)
            others = m[m != s]
            if len(others):
                assert len(set(int(x) for x in D[s, others])) == 1, (names[s], c)
        twins = members[cls[s]]
        for t in twins[twins > s]:  # fact 2
            keep = np.ones(n, bool)
            keep[[s, t]] = False
            assert np.array_equal(D[s, keep], D[int(t), keep]), (names[s], names[int(t)])
        others = twins[twins != s]
        if len(others):  # fact 3: t_C
            forwards = any(not ovl[x] for x in nbrs[s])
            t_c = int(D[s, others[0]])
            assert (t_c == 2) if forwards else (t_c > 2), (names[s], t_c)
    if state == "neighbours":  # the state exists to make some t_C differ from 2
        c = names.index("3-1-0" if graph == "small" else "3-9-0")
        t = members[cls[c]]
        assert int(D[c, t[t != c][0]]) != 2
