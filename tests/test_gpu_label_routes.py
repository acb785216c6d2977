"""Every node's node-label MPLS routes from a resident all-sources pass
(spf_mplan_label_routes, include/openr_spf.h): what buildRouteDb computes at
Decision.cpp:586-674 for every node, with no SPF per node.

The expectation comes from the oracle's restatement of getNextHopsWithMetric /
getNextHopsThrift (oracle.nexthops), never from the code under test: per me
and label the candidates are walked in ascending name; the first that is me
owns the label (POP_AND_LOOKUP), otherwise the first with a non-empty next-hop
set owns it and those rows are the route.  The reference resolves a label
collision this way (the smaller name wins only when it has a route), and so
do the two host solvers: the comparison with SpfSolver.buildRouteDb runs on
shared labels too (tests/test_gpu_label_collisions.py pins the host solvers
themselves to the oracle).
"""

import ctypes as C
import functools

import numpy as np
import pytest

from helpers import expected_from, label_candidates
from oracle import OracleLinkState
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.link_state import LinkState
from openr_amd.lsdb import create_adj_db, create_adjacency, pack, pack_fast
from openr_amd.spf_solver import MPLS_LABEL_MAX, PrefixState, SpfSolver

pytestmark = pytest.mark.gpu


# ---- the graphs -----------------------------------------------------------------
def graph_a():
    """Two components, 13 nodes.  b1..b9: parallel links (b1-b2 at equal
    metrics, b4-b7 at different ones), b3 drained, the b5-b8 link overloaded.
    a1, a2, c1, c2: a ring nobody in b* reaches (a* sort before b*, c* after).
    Labels: 100 on a1 and b5 (from b*: the smaller name is unreachable, the
    larger owns it), 101 on b2 and b7 (both reachable; from b7: me and a
    smaller-named reachable node), 102 on b9 and c1, none on b4 (0), an
    invalid one on b6."""
    links = [  # (u, v, metric u->v, metric v->u, overloaded)
        ("b1", "b2", 1, 1, False), ("b1", "b2", 1, 1, False), ("b2", "b3", 1, 1, False),
        ("b3", "b4", 1, 1, False), ("b2", "b4", 3, 3, False), ("b4", "b5", 1, 2, False),
        ("b5", "b6", 2, 2, False), ("b6", "b7", 1, 1, False), ("b7", "b8", 1, 1, False),
        ("b8", "b9", 1, 3, False), ("b9", "b1", 2, 2, False), ("b5", "b8", 2, 2, True),
        ("b4", "b7", 2, 2, False), ("b4", "b7", 5, 5, False),
        ("a1", "a2", 1, 1, False), ("a2", "c1", 1, 1, False), ("c1", "c2", 1, 1, False),
        ("c2", "a1", 2, 2, False),
    ]
    label = {"a1": 100, "a2": 22, "b1": 11, "b2": 101, "b3": 13, "b4": 0, "b5": 100,
             "b6": MPLS_LABEL_MAX + 8, "b7": 101, "b8": 18, "b9": 102, "c1": 102, "c2": 32}
    adjs = {n: [] for n in label}
    seen = {}
    for i, (u, v, mu, mv, ovl) in enumerate(links):
        k = seen.get((u, v), 0)
        seen[(u, v)] = k + 1
        a = create_adjacency(v, f"{u}/{v}/{k}", f"{v}/{u}/{k}", f"fe80::{i + 1:x}", f"10.0.{i}.1", mu,
                             50000 + 2 * i)
        b = create_adjacency(u, f"{v}/{u}/{k}", f"{u}/{v}/{k}", f"fe80::1:{i + 1:x}", f"10.0.{i}.2", mv,
                             50001 + 2 * i)
        a.isOverloaded = ovl
        adjs[u].append(a)
        adjs[v].append(b)
    dbs = [create_adj_db(n, adjs[n], label[n], overLoadBit=(n == "b3")) for n in label]
    return pack(dbs), label, None


def graph_b(shared=True):
    """test_gpu_routes_resident's rand0; seeded labels: about 10 % zeros and
    (shared) five labels advertised by two nodes each."""
    topo = T.random_graph(60, 170, 12, max_metric=6, parallel_frac=0.25, overload_frac=0.1,
                          link_overload_frac=0.05)
    rng = np.random.default_rng(2024)
    n = len(topo.nodes)
    lab = 1000 + rng.permutation(n).astype(np.int32)
    lab[rng.random(n) < 0.1] = 0
    if shared:
        pick = rng.choice(np.nonzero(lab)[0], 10, replace=False)
        lab[pick[5:]] = lab[pick[:5]]
    topo.lsdb.dbs["node_label"] = lab
    return topo.lsdb, dict(zip(topo.nodes, lab.tolist())), None


def hub_graph(leaves=300, n_me=8):
    """A hub with `leaves` leaves and a second, parallel link to 20 of them (10
    at the same metric, 10 at a larger one); me: the hub and n_me seeded
    leaves."""
    nodes = ["hub"] + [f"l{i:03d}" for i in range(leaves)]
    src, dst, met, ifs, oifs = [], [], [], [], []
    for i in range(1, leaves + 1):
        for k in range(2 if i <= 20 else 1):
            m = 2 if (k == 1 and i > 10) else 1
            for a, b in ((0, i), (i, 0)):
                src.append(a)
                dst.append(b)
                met.append(m)
                ifs.append(f"{nodes[a]}/{nodes[b]}/{k}")
                oifs.append(f"{nodes[b]}/{nodes[a]}/{k}")
    lab = np.arange(1, len(nodes) + 1, dtype=np.int32)
    lsdb = pack_fast(nodes, np.asarray(src), np.asarray(dst), ifs, oifs, np.asarray(met, np.int32),
                     node_label=lab)
    rng = np.random.default_rng(5)
    mes = ["hub"] + [nodes[int(i)] for i in rng.choice(np.arange(1, leaves + 1), n_me, replace=False)]
    return lsdb, dict(zip(nodes, lab.tolist())), mes


def graph_c():
    """A hub with 300 leaves and a second, parallel link to 20 of them (10 at
    the same metric, 10 at a larger one): 320 links at the hub (more than one
    256-link staging chunk), 301 labels (more than one 256-thread block)."""
    return hub_graph(300)


def graph_d():
    """fabric1000 (960 nodes), label = node id + 1, 12 seeded me."""
    topo = T.fabric(1000, full=True)
    rank = {s: i for i, s in enumerate(sorted(topo.nodes))}
    lab = np.array([rank[s] + 1 for s in topo.nodes], np.int32)
    topo.lsdb.dbs["node_label"] = lab
    rng = np.random.default_rng(11)
    mes = [topo.nodes[int(i)] for i in rng.choice(len(topo.nodes), 12, replace=False)]
    return topo.lsdb, dict(zip(topo.nodes, lab.tolist())), mes


GRAPHS = {"A": graph_a, "B": graph_b, "C": graph_c, "D": graph_d}


@functools.lru_cache(maxsize=None)
def graph(key):
    return GRAPHS[key]()


@functools.lru_cache(maxsize=None)
def expected(key, lfa):
    """expected_from for a graph of GRAPHS; computed once per (graph, lfa) and
    shared by the member counts."""
    lsdb, label_of, mes = graph(key)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    return expected_from(orc, label_of, mes, lfa)


def expand(ls, flat, me, labels, owner, ptr, rec):
    """One node's records -> {label: (owner name, rows)} in the oracle's shape."""
    names, _rp, col, _met, lid, _ovl = flat
    out = {}
    for g, lab in enumerate(labels.tolist()):
        o = int(owner[g])
        if o == N.SPF_UNREACHABLE:
            assert ptr[g] == ptr[g + 1]
            continue
        rows = set()
        edges = []
        for r in rec[int(ptr[g]): int(ptr[g + 1])].tolist():
            e, m = r & 0xFFFFFFFF, r >> 32
            edges.append(e)
            link = ls._link(int(lid[e]))
            nb = link.getOtherNodeName(me)
            assert names[int(col[e])] == nb
            php = int(col[e]) == o
            rows.add((link.getIfaceFromNode(me), m - (1 << 32) if m >= 1 << 31 else m, nb,
                      "PHP" if php else "SWAP", None if php else lab))
        assert edges == sorted(set(edges)), "records not in me's link order"
        assert len(rows) == len(edges)
        out[lab] = (names[o], rows)
    return out


def member_pools(mp, n_members):
    """[(me slots, records)] of every member (spf_mplan_label_route_buffers)."""
    out = []
    for r in range(n_members):
        k, nrec = C.c_uint32(), C.c_uint64()
        po, pp, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        N.raise_for(N.lib.spf_mplan_label_route_buffers(C.c_void_p(mp), r, C.byref(po), C.byref(pp),
                                                        C.byref(pr), C.byref(nrec), None, 0, C.byref(k)),
                    N.global_error())
        slots = np.zeros(max(1, k.value), np.uint32)
        N.raise_for(N.lib.spf_mplan_label_route_buffers(C.c_void_p(mp), r, None, None, None, None,
                                                        N.ptr(slots), k.value, None), N.global_error())
        assert bool(po.value) == bool(k.value) == bool(pp.value) == bool(pr.value)
        out.append((slots[: k.value].tolist(), int(nrec.value)))
    return out


@pytest.mark.parametrize("key", sorted(GRAPHS))
@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_label_routes_match_oracle(key, members, lfa):
    lsdb, label_of, me_names = graph(key)
    want = expected(key, lfa)
    cands = label_candidates(label_of)
    with LinkState(devices=[0] * members) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        flat = ls.flatten()
        names = list(flat[0])
        assert names == sorted(label_of)
        id_of = {s: i for i, s in enumerate(names)}
        me_names = names if me_names is None else me_names
        mes = np.array([id_of[s] for s in me_names], np.uint32)
        calls = []
        for _ in range(2):
            labels, n_records, pool_bytes, ms = ls.allSourcesLabelRoutes(lfa, mes)
            assert ms >= 0
            dbs = [ls.allSourcesLabelRouteDb(t) for t in range(len(mes))]
            calls.append((labels, n_records, pool_bytes, dbs))
        pools = member_pools(N.lib.ls_all_sources_plan(ls._h), members)
        G = len(labels)
        assert labels.tolist() == list(cands)
        got = {}
        seen = 0
        for t, me in enumerate(me_names):
            owner, ptr, rec = dbs[t]
            assert len(owner) == G and len(ptr) == G + 1
            assert ptr[0] == 0 and np.all(np.diff(ptr.astype(np.int64)) >= 0)
            assert int(ptr[G]) == len(rec)  # sum(count) == len(rec)
            seen += len(rec)
            for lab, val in expand(ls, flat, me, labels, owner, ptr, rec).items():
                got[(me, lab)] = val
    assert seen == n_records
    # the exactly sized pools: per member with a me, 8 records + 8 (n G + 1) + 4 n G
    assert sorted(t for slots, _ in pools for t in slots) == list(range(len(mes)))
    assert sum(r for _, r in pools) == n_records
    assert pool_bytes == sum(8 * r + 8 * (len(s) * G + 1) + 4 * len(s) * G for s, r in pools if s)
    # a second call gives identical arrays
    (l0, n0, b0, d0), (l1, n1, b1, d1) = calls
    assert np.array_equal(l0, l1) and n0 == n1 and b0 == b1
    for x, y in zip(d0, d1):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    # owners and next hops equal the oracle's
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (bad[:3], [(got[k], want[k]) for k in bad[:1]])


def test_graph_a_covers_the_collision_cases():
    """What graph A is for, checked on the oracle's expectation: a shared
    label goes past an unreachable smaller name, to the smaller of two
    reachable names, and to a smaller reachable name rather than me."""
    want = expected("A", False)
    assert want[("b1", 100)][0] == "b5" and want[("c2", 100)][0] == "a1"
    assert want[("b1", 101)][0] == "b2" and want[("b7", 101)][0] == "b2"
    assert want[("b2", 101)] == ("b2", set())
    assert want[("b4", 102)][0] == "b9" and want[("a2", 102)][0] == "c1"
    assert ("b1", 22) not in want and ("a1", 11) not in want


def test_mpls_routes_equal_build_route_db():
    """allSourcesMplsRoutes(t) (the records expanded, adjacency labels from
    the host) equals SpfSolver.buildRouteDb(me).mplsRoutes for every me, on
    graph B without and with shared labels and on graph A (two components,
    shared labels with an unreachable smaller name), shortest paths only."""
    ps = PrefixState()
    # (graph, routes per me at least: most of B's ~54 labels are routable from
    # most nodes; A has 9 node labels, about half of them routable per me, and
    # its adjacency labels)
    for lsdb, least in ((graph_b(shared=False)[0], 10), (graph("B")[0], 10), (graph("A")[0], 4)):
        with LinkState(devices=[0, 0]) as ls:
            ls.updateAdjacencyDatabases(lsdb)
            ls.prefetchAllSources()
            names = list(ls.flatten()[0])
            ls.allSourcesLabelRoutes(False)
            routes = 0
            for t, me in enumerate(names):
                got = ls.allSourcesMplsRoutes(t)
                want = SpfSolver(me, False, False).buildRouteDb(me, {"0": ls}, ps).mplsRoutes
                assert got == want, me
                routes += len(got)
        assert routes > least * len(names)


def test_label_routes_error_paths():
    lsdb, _label_of, _ = graph("A")
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        with pytest.raises(RuntimeError):
            ls.allSourcesLabelRoutes(False)
        with pytest.raises(RuntimeError):
            ls.allSourcesLabelRouteDb(0)
        with pytest.raises(RuntimeError):
            ls.allSourcesMplsRoutes(0)
        ls.prefetchAllSources(useLinkMetric=False)  # a hop-count plan
        with pytest.raises(N.UnsupportedInput) as ei:
            ls.allSourcesLabelRoutes(False)
        assert ei.value.status == N.SPF_E_UNSUPPORTED
