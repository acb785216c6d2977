"""Link-metric what-if batches without a device: the numpy restatement of the
device's classify rule (cold / root / delta) and of its slack-bounded growth
of the affected set D (tests/whatif_metrics.py), against full oracle re-runs
on the changed LSDB.

On about 200 random (graph, change) pairs:
  * a change the rule calls cold leaves the oracle's result as it was;
  * every node whose metric or next hops the change moves lies in the grown D
    (the superset argument of DESIGN 4.9), the source never does, and no node
    becomes unreachable;
  * no node improves by more than delta.
"""

import numpy as np
import pytest

import whatif_lists as L
import whatif_metrics as WM
from openr_amd import topology as T
from openr_amd.link_state import LinkState

GRAPHS = {
    # metrics 1-3 and 20 % parallel links: ties and parallel links bite
    "m40": lambda: T.random_graph(40, 100, 75, max_metric=3, parallel_frac=0.2),
    "rand0": lambda: T.random_graph(70, 180, 300, max_metric=5, parallel_frac=0.2,
                                    overload_frac=0.1, link_overload_frac=0.05),
    "rand3": lambda: T.random_graph(70, 180, 303, max_metric=5, parallel_frac=0.2,
                                    overload_frac=0.1, link_overload_frac=0.05),
    "wan200": lambda: T.wan(200, 100, seed=6),
}
PER_GRAPH = 50


def flat(topo, s=0):
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names, rp, col, met, lid, ovl = ls.flatten()
    exp = WM.Expected(topo.lsdb, ls, names, rp, col, s)
    return ls, names, exp, (rp, col, met, lid, ovl)


def random_changes(rng, exp, edges, n):
    """(link, m_lo, m_hi): raises, lowers and mixed ones, one direction kept now and then."""
    links = sorted(edges)
    out = []
    for _ in range(n):
        l = int(rng.choice(links))
        cur = exp.current(l)
        new = []
        for w in cur:
            kind = int(rng.integers(0, 4))
            new.append(WM.KEEP if kind == 0 else int(rng.integers(1, w + 1)) if kind == 1
                       else w + int(rng.integers(1, 6)) if kind == 2 else int(rng.integers(1, 9)))
        out.append((l, new[0], new[1]))
    return out


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_changed_nodes_lie_in_the_grown_set(name):
    ls, names, exp, (rp, col, met, lid, ovl) = flat(GRAPHS[name]())
    s = exp.s
    bd = exp.base[0]
    edges = WM.link_edges(rp, col, lid)
    rng = np.random.default_rng(7)
    seen = {"cold": 0, "raise": 0, "tie": 0, "lower": 0}
    for l, m_lo, m_hi in random_changes(rng, exp, edges, PER_GRAPH):
        new = exp.resolved(l, m_lo, m_hi)
        # the CSR's metrics are the advertised ones, direction by direction
        assert (int(met[edges[l][0]]), int(met[edges[l][1]])) == exp.current(l)
        res = exp.metric_result(l, m_lo, m_hi)
        moved = WM.changed_nodes(exp.base, res)
        assert not ((res[0] == L.U64_MAX) & (bd != L.U64_MAX)).any()  # nobody becomes unreachable
        root, delta = WM.classify(rp, col, met, ovl, bd, s, edges[l], new)
        if root is None:
            assert not moved, (l, m_lo, m_hi)
            seen["cold"] += 1
            continue
        D = WM.grow(rp, col, met, ovl, bd, s, edges[l], new, root, delta)
        assert moved <= D, (l, m_lo, m_hi, sorted(moved - D))
        assert s not in D
        ok = bd != L.U64_MAX
        gain = bd[ok].astype(np.int64) - res[0][ok].astype(np.int64)
        raised = new[0 if root == edges[l][0] else 1] > int(met[root])
        if raised:
            assert delta == 0 and (gain <= 0).all()
            seen["raise"] += 1
        else:
            assert (gain <= delta).all() and (gain >= 0).all()
            seen["tie" if delta == 0 else "lower"] += 1
    assert seen["cold"] and seen["raise"] and seen["lower"], seen


def test_a_drained_tail_is_cold_and_a_drained_source_is_not():
    topo = T.random_graph(50, 120, 17, max_metric=4, overload_frac=0.2)
    ls, names, exp, (rp, col, met, lid, ovl) = flat(topo)
    edges = WM.link_edges(rp, col, lid)
    drained = [int(x) for x in np.nonzero(ovl)[0]]
    assert drained
    n_cold = 0
    for l, (e_lo, e_hi) in sorted(edges.items()):
        for e, k in ((e_lo, 0), (e_hi, 1)):
            a = WM.tail_of(rp, e)
            if a in drained and a != exp.s and int(met[e]) > 1:
                m = [WM.KEEP, WM.KEEP]
                m[k] = 1  # lowering the direction out of a drained node
                assert exp.metric_digest(l, *m) == exp.base_digest
                assert WM.classify(rp, col, met, ovl, exp.base[0], exp.s, (e_lo, e_hi),
                                   exp.resolved(l, *m))[0] is None
                n_cold += 1
    assert n_cold
    # the same graph from a drained source: its own links are expanded
    s = drained[0]
    exp2 = WM.Expected(topo.lsdb, ls, names, rp, col, s)
    n_hot = 0
    for e in range(int(rp[s]), int(rp[s + 1])):
        b, l = int(col[e]), int(lid[e])
        if b == s or int(met[e]) == 1:
            continue
        k = 0 if s < b else 1
        m = [WM.KEEP, WM.KEEP]
        m[k] = 1
        root, delta = WM.classify(rp, col, met, ovl, exp2.base[0], s, edges[l], exp2.resolved(l, *m))
        assert root == e and delta == int(exp2.base[0][b]) - 1  # 0 + 1 <= d(b): always hot
        moved = WM.changed_nodes(exp2.base, exp2.metric_result(l, *m))
        assert moved <= WM.grow(rp, col, met, ovl, exp2.base[0], s, edges[l],
                                exp2.resolved(l, *m), root, delta)
        n_hot += bool(moved)
    assert n_hot
