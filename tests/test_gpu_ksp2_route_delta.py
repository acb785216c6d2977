"""KSP2 route databases on the GPU: snapshot, delta and update payload
(spf_ksp2_route_snapshot / _delta / _update, include/openr_spf.h).

Expected values never come from the code under test: both generations are read
back with spf_ksp2_route_db (pinned to the oracle by test_gpu_ksp2_routes.py),
every route becomes a frozenset of (link_hash[link_id[edge]], cost, stack), and
DecisionRouteDb::calculateUpdate's three rules are applied in Python:
unchanged (both empty, or equal sets), DELETE (only the old side has next
hops), UPDATE (the new side has next hops and the route is new or differs).
Lists, totals and payload compare in full: integers, no tolerance.
"""

import copy
import ctypes as C

import numpy as np
import pytest

from oracle import OracleLinkState
from refcases import dbs_from_json, load_cases
from test_gpu_ksp2_routes import Loaded, graph_a, holds_no_routes
from openr_amd import _native as N
from openr_amd.hiprt import read_device, synchronize
from openr_amd.link_state import LinkState
from openr_amd.lsdb import create_adj_db, create_adjacency, pack

pytestmark = pytest.mark.gpu

D, M = N.SPF_DELTA_DELETE, N.SPF_DELTA_DELETE - 1


# ---- graphs: {name: AdjacencyDatabase}, so single nodes can be pushed again --------
def dbs_from_links(links, label, drained=()):
    """links: (u, v, metric u->v, metric v->u, overloaded); label: {node: label}."""
    adjs = {n: [] for n in label}
    seen = {}
    for i, (u, v, mu, mv, ovl) in enumerate(links):
        k = seen.get((u, v), 0)
        seen[(u, v)] = k + 1
        a = create_adjacency(v, f"{u}/{v}/{k}", f"{v}/{u}/{k}", f"fe80::{i + 1:x}", f"10.0.{i % 250}.1", mu, 0)
        b = create_adjacency(u, f"{v}/{u}/{k}", f"{u}/{v}/{k}", f"fe80::1:{i + 1:x}", f"10.0.{i % 250}.2", mv, 0)
        a.isOverloaded = b.isOverloaded = ovl
        adjs[u].append(a)
        adjs[v].append(b)
    return {n: create_adj_db(n, adjs[n], label[n], overLoadBit=(n in drained)) for n in label}


def golden_dbs(name):
    case = next(c for c in load_cases() if c["name"] == name)
    return {d.thisNodeName: d for d in dbs_from_json(case["steps"][0]["update"])}


def graph_a_dbs():
    """test_gpu_ksp2_routes.graph_a's links (two components, parallel links, a
    drained node, an overloaded link) as databases."""
    links = [
        ("b1", "b2", 1, 1, False), ("b1", "b2", 1, 1, False), ("b2", "b3", 1, 1, False),
        ("b3", "b4", 1, 1, False), ("b2", "b4", 3, 3, False), ("b4", "b5", 1, 2, False),
        ("b5", "b6", 2, 2, False), ("b6", "b7", 1, 1, False), ("b7", "b8", 1, 1, False),
        ("b8", "b9", 1, 3, False), ("b9", "b1", 2, 2, False), ("b5", "b8", 2, 2, True),
        ("b4", "b7", 2, 2, False), ("b4", "b7", 5, 5, False),
        ("a1", "a2", 1, 1, False), ("a2", "c1", 1, 1, False), ("c1", "c2", 1, 1, False),
        ("c2", "a1", 2, 2, False),
    ]
    nodes = ["a1", "a2", "b1", "b2", "b3", "b4", "b5", "b6", "b7", "b8", "b9", "c1", "c2"]
    return dbs_from_links(links, {n: 100 + i for i, n in enumerate(nodes)}, drained=("b3",))


def ring6_dbs(leaf=False):
    nodes = [f"r{i}" for i in range(6)]
    links = [(nodes[i], nodes[(i + 1) % 6], 1 + i % 2, 1 + i % 2, False) for i in range(6)]
    if leaf:
        nodes.append("z")
        links.append(("z", "r2", 1, 1, False))
    return dbs_from_links(links, {n: 200 + i for i, n in enumerate(nodes)})


def hub_dbs(leaves=70):
    nodes = ["hub"] + [f"l{i:03d}" for i in range(leaves)]
    return dbs_from_links([("hub", l, 1, 1, False) for l in nodes[1:]], {n: 1 + i for i, n in enumerate(nodes)})


def random_dbs(seed=5, n=20, extra=18, more=()):
    """A connected multigraph: a ring, random chords, a quarter of them doubled;
    then the links of `more`, whose new nodes are labelled after the others."""
    rng = np.random.default_rng(seed)
    nodes = [f"n{i:02d}" for i in range(n)]
    links = [(nodes[i], nodes[(i + 1) % n], int(rng.integers(1, 5)), int(rng.integers(1, 5)), False)
             for i in range(n)]
    for _ in range(extra):
        u, v = (int(x) for x in rng.choice(n, 2, replace=False))
        m = int(rng.integers(1, 5))
        links.append((nodes[min(u, v)], nodes[max(u, v)], m, m, False))
        if rng.random() < 0.25:
            links.append((nodes[min(u, v)], nodes[max(u, v)], m, int(rng.integers(1, 5)), False))
    for link in more:
        links.append(link)
        nodes += [x for x in link[:2] if x not in nodes]
    return dbs_from_links(links, {s: 300 + i for i, s in enumerate(nodes)})


# name -> (databases, two anycast sets, two links (u, v, k) on shortest paths)
GRAPHS = {
    "graph_a": (graph_a_dbs, [["b1", "b7"], ["b9", "c1", "b4"]], [("b6", "b7", 0), ("b9", "b1", 0)]),
    "ring6": (ring6_dbs, [["r0", "r3"], ["r1", "r4", "r5"]], [("r0", "r1", 0), ("r3", "r4", 0)]),
    "parallel_ring": (lambda: golden_dbs("decision_parallel_adj_ring"), [["2", "3"], ["1", "4"]], None),
    "hub": (lambda: hub_dbs(70), [["l000", "l069"], [f"l{i:03d}" for i in range(70)]],
            [("hub", "l005", 0), ("hub", "l060", 0)]),
    "random": (random_dbs, [["n03", "n11"], ["n00", "n07", "n15", "n19"]], [("n00", "n01", 0), ("n09", "n10", 0)]),
}


def adj(dbs, u, v, k=0):
    return next(a for a in dbs[u].adjacencies if a.ifName == f"{u}/{v}/{k}")


# ---- one generation ---------------------------------------------------------------------
class Gen:
    """The routes of one allSourcesKsp2Routes read back by value."""

    def __init__(self, ls, n_sets, n_mes):
        names, _rp, _col, _met, lid, _ovl = ls.flatten()
        self.names = list(names)
        self.lid = np.array(lid)
        self.lh = np.array(ls.linkValueHashes())
        self.raw, self.order, self.routes, self.edges = {}, {}, {}, {}
        for t in range(n_mes):
            rptr, rec, lptr, lab = ls.allSourcesKsp2RouteDb(t)
            self.raw[t] = (rptr, rec, lptr, lab)
            for p in range(n_sets):
                hops = []
                for h in range(int(rptr[p]), int(rptr[p + 1])):
                    r = int(rec[h])
                    hops.append((r & 0xFFFFFFFF, r >> 32, tuple(int(x) for x in lab[int(lptr[h]): int(lptr[h + 1])])))
                self.edges[(t, p)] = [e for e, _, _ in hops]
                self.order[(t, p)] = [self.value(h) for h in hops]
                self.routes[(t, p)] = frozenset(self.order[(t, p)])
                assert len(self.routes[(t, p)]) == len(hops)  # each side is a set

    def value(self, hop):
        e, cost, stack = hop
        return (int(self.lh[int(self.lid[e])]), int(cost), tuple(stack))


def flatten_sets(sets, pre, id_of):
    """[[names]] in the order given (+ [{name: prepend}]) -> set_ptr, set_nodes, prepend."""
    ptr, nodes, out = [0], [], []
    for p, s in enumerate(sets):
        nodes += [id_of[d] for d in s]
        out += [(pre[p].get(d) if pre else None) for d in s]
        ptr.append(len(nodes))
    return np.array(ptr, np.uint32), np.array(nodes, np.uint32), (out if pre else None)


class World:
    def __init__(self, dbs, mes=None):
        self.dbs = dbs
        self.ls = LinkState(device=0)
        self.push(*sorted(dbs))
        self.names = list(self.ls.flatten()[0])
        self.id_of = {s: i for i, s in enumerate(self.names)}
        self.mes = None if mes is None else [self.id_of[m] for m in mes]
        self.n_mes = len(self.names) if mes is None else len(mes)

    def push(self, *nodes):
        for n in nodes:
            self.ls.updateAdjacencyDatabase(copy.deepcopy(self.dbs[n]))

    def build(self, sets, pre=None):
        sp, sn, prepend = flatten_sets(sets, pre, self.id_of)
        self.ls.allSourcesKsp2Routes(sp, sn, prepend, self.mes)
        return Gen(self.ls, len(sets), self.n_mes)

    def loopbacks(self, anycast):
        return [[n] for n in self.names] + [list(s) for s in anycast]

    def close(self):
        self.ls.close()


def expected(g0, g1, n_mes, n_sets):
    """calculateUpdate's rules: per source (updates, deletes), ascending."""
    out = []
    for t in range(n_mes):
        up, dele = [], []
        for p in range(n_sets):
            o, n = g0.routes[(t, p)], g1.routes[(t, p)]
            if not n:
                if o:
                    dele.append(p)
            elif o != n:
                up.append(p)
        out.append((up, dele))
    return out


def check(w, snap, g0, g1, n_sets):
    """The delta and its payload against the Python expectation, in full."""
    lists, totals, ms, payload, info = w.ls.allSourcesKsp2RouteUpdate(snap)
    want = expected(g0, g1, w.n_mes, n_sets)
    assert [(list(u), list(d)) for u, d in lists] == want
    n_up, n_del = sum(len(u) for u, _ in want), sum(len(d) for _, d in want)
    assert totals[:2] == [n_up, n_del]
    records = words = 0
    for t, (up, _dele) in enumerate(want):
        assert sorted(payload[t]) == up
        for p in up:
            got = [g1.value(h) for h in payload[t][p]]
            assert got, (t, p)  # no UPDATE carries zero records
            assert len(set(got)) == len(got) and frozenset(got) == g1.routes[(t, p)], (t, p)
            # pool order: the records as the database holds them
            assert [h[0] for h in payload[t][p]] == g1.edges[(t, p)], (t, p)
            records += len(got)
            words += sum(len(h[2]) for h in payload[t][p])
    assert info["update_totals"] == [n_up, records, words]
    assert info["pool_bytes"] == 8 * (n_up + n_del + 1) + 8 * records + 8 * (records + 1) + 4 * words
    assert ms >= 0 and len(info["phase_ms"]) == 6 and all(x >= 0 for x in info["phase_ms"])
    # the same lists without the payload, and through the per-source call
    lists2, totals2, _ = w.ls.allSourcesKsp2RouteDelta(snap)
    assert lists2 == lists and totals2 == totals
    plan = w.ls._k2r[0].plan
    for t, (up, dele) in enumerate(want):
        ent = plan.route_delta_db(t).tolist()
        assert [v & M for v in ent] == sorted(up + dele)
        assert sorted(v & M for v in ent if v & D) == dele
    return lists, totals, info


# ---- 1. identical generations ---------------------------------------------------------
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_identical_generations(graph):
    make, anycast, _ = GRAPHS[graph]
    w = World(make())
    try:
        sets = w.loopbacks(anycast)
        g0 = w.build(sets)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        assert snap.bytes() > 0
        g1 = w.build(sets)
        assert g0.routes == g1.routes and any(g0.routes.values())
        lists, totals, info = check(w, snap, g0, g1, len(sets))
        assert totals == [0, 0, 0] and all(l == ([], []) for l in lists)
        assert info["update_totals"] == [0, 0, 0] and info["pool_bytes"] == 8 + 8
        dptr, dset, uptr, urec, ulptr, ulab = w.ls._k2r[0].plan.route_update()[:6]
        assert not dptr.any() and len(dset) == 0 and uptr.tolist() == [0]
        assert len(urec) == 0 and ulptr.tolist() == [0] and len(ulab) == 0
    finally:
        w.close()


# ---- 2. a link withdrawn through the row-patch path, then re-advertised ----------------
def host_direct_path(dbs, u, v, k):
    """On the CPU (the oracle's runSpf): the link u/v/k is a shortest u -> v path."""
    orc = OracleLinkState()
    orc.update_packed(pack([dbs[n] for n in sorted(dbs)]))
    e = orc.spf(u)[v]
    return v in e["nextHops"] and e["metric"] == adj(dbs, u, v, k).metric


@pytest.mark.parametrize("graph", ["graph_a", "ring6", "hub", "random"])
def test_link_withdrawn_then_readvertised(graph):
    make, anycast, tight = GRAPHS[graph]
    moved = False
    for u, v, k in tight:
        dbs = make()
        assert host_direct_path(dbs, u, v, k), (u, v)
        w = World(dbs)
        try:
            sets = w.loopbacks(anycast)
            g0 = w.build(sets)
            snap = w.ls.allSourcesKsp2RouteSnapshot()
            with pytest.raises(N.SpfError) as e:
                w.ls.allSourcesKsp2RouteDb(0)  # the pools moved into the snapshot
            assert e.value.status == N.SPF_E_STATE
            patches = N.lib.ls_debug_row_patches(w.ls._h)
            gone = adj(dbs, u, v, k)
            dbs[u].adjacencies.remove(gone)
            w.push(u)
            g1 = w.build(sets)
            assert N.lib.ls_debug_row_patches(w.ls._h) > patches  # patched in place, not reloaded
            lists, totals, _ = check(w, snap, g0, g1, len(sets))
            assert totals[0] >= 1
            assert w.id_of[v] in lists[w.id_of[u]][0] + lists[w.id_of[u]][1]
            # back again: the same routes by value, on CSR slots that moved
            dbs[u].adjacencies.append(gone)
            w.push(u)
            g2 = w.build(sets)
            assert g2.routes == g0.routes
            lists, totals, _ = check(w, snap, g0, g2, len(sets))
            assert totals[:2] == [0, 0] and all(l == ([], []) for l in lists)
            moved |= any(g0.edges[key] != g2.edges[key] for key in g0.edges)
        finally:
            w.close()
    assert moved, "every record kept its CSR edge: the key compare was not exercised"


# ---- 3. order only ----------------------------------------------------------------------
def members_with_own_hops(g, t, p, members, loop):
    """Members of set p that give route (t, p) a next hop no other member's
    loopback route has."""
    n = 0
    for d in members:
        others = frozenset().union(*(g.routes[(t, loop[x])] for x in members if x != d))
        n += bool((g.routes[(t, p)] & g.routes[(t, loop[d])]) - others)
    return n


@pytest.mark.parametrize("graph", ["graph_a", "ring6", "parallel_ring", "random"])
def test_order_only(graph):
    make, anycast, _ = GRAPHS[graph]
    w = World(make())
    try:
        sets = w.loopbacks(anycast)
        p = len(sets) - 1
        g0 = w.build(sets)
        # a route of the anycast set with next hops of two different members
        loop = {s[0]: q for q, s in enumerate(sets) if len(s) == 1}
        mixed = [t for t in range(w.n_mes) if members_with_own_hops(g0, t, p, sets[p], loop) >= 2]
        assert mixed, "no route of the anycast set has next hops from two members"
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        g1 = w.build(sets[:p] + [sets[p][::-1]])
        assert g1.routes == g0.routes
        assert any(g0.order[(t, p)] != g1.order[(t, p)] for t in mixed)  # the pools' order did move
        lists, totals, _ = check(w, snap, g0, g1, len(sets))
        assert totals[:2] == [0, 0] and totals[2] > 0 and all(l == ([], []) for l in lists)
    finally:
        w.close()


# ---- 4. labels only -----------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["graph_a", "random"])
def test_labels_only(graph):
    make, anycast, _ = GRAPHS[graph]
    dbs = make()
    w = World(dbs)
    try:
        sets = w.loopbacks(anycast)
        p = len(sets) - 1
        pre0 = [{d: None for d in s} for s in sets]
        g0 = w.build(sets, pre0)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        node = anycast[0][1]
        dbs[node].nodeLabel = 7777
        w.push(node)
        pre1 = copy.deepcopy(pre0)
        pre1[p][sets[p][0]] = 8888
        g1 = w.build(sets, pre1)
        lists, totals, _ = check(w, snap, g0, g1, len(sets))
        mentions = sorted(key for key, r in g1.routes.items() if any(7777 in s or 8888 in s for _, _, s in r))
        assert mentions and totals[1] == 0
        assert sorted((t, q) for t, (up, _) in enumerate(lists) for q in up) == mentions
    finally:
        w.close()


# ---- 5, 6. withdrawn routes, a new route ---------------------------------------------------
def test_leaf_cut_off_then_a_new_route():
    dbs = ring6_dbs(leaf=True)
    w = World(dbs)
    try:
        sets = w.loopbacks([["r0", "z"], ["r1", "r4"]]) + [[]]
        g0 = w.build(sets)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        link = adj(dbs, "z", "r2")
        dbs["z"].adjacencies.remove(link)
        w.push("z")
        g1 = w.build(sets)
        lists, totals, _ = check(w, snap, g0, g1, len(sets))
        z = w.id_of["z"]
        for t, (up, dele) in enumerate(lists):
            if t != z:
                assert z in dele, t
        # z itself: every set it had a route to is a DELETE, nothing is an UPDATE
        assert lists[z][0] == [] and lists[z][1] == [q for q in range(len(sets)) if g0.routes[(z, q)]]
        assert len(lists[z][1]) == len(sets) - 2  # all but its own loopback and the empty set
        # 6: back up, and the empty set populated: new routes are UPDATEs
        snap1 = w.ls.allSourcesKsp2RouteSnapshot()
        dbs["z"].adjacencies.append(link)
        w.push("z")
        sets2 = sets[:-1] + [["r3", "z"]]
        g2 = w.build(sets2)
        lists, totals, _ = check(w, snap1, g1, g2, len(sets))
        assert totals[1] == 0
        for t, (up, _dele) in enumerate(lists):
            assert len(sets) - 1 in up, t  # the set that was empty
            if t != z:
                assert z in up, t
        # the first snapshot is still good: only the new set differs from it
        lists, totals, _ = check(w, snap, g0, g2, len(sets))
        assert all(l == ([len(sets) - 1], []) for l in lists)
    finally:
        w.close()


# ---- 7. a route with more than 64 next hops ----------------------------------------------
def test_hub_route_with_more_than_64_next_hops():
    dbs = hub_dbs(70)
    leaves = [f"l{i:03d}" for i in range(70)]
    w = World(dbs, mes=["hub", "l000", "l001", "l035", "l069"])
    try:
        sets = [[n] for n in w.names] + [leaves]
        p = len(sets) - 1
        g0 = w.build(sets)
        assert len(g0.routes[(0, p)]) == 70 and len(g0.routes[(1, p)]) == 69
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        # order only: 70 and 69 next hops matched as sets
        g1 = w.build(sets[:p] + [leaves[::-1]])
        lists, totals, _ = check(w, snap, g0, g1, len(sets))
        assert totals[:2] == [0, 0] and totals[2] >= w.n_mes
        # one leaf's label changes: in place (positionally) ...
        dbs["l040"].nodeLabel = 9999
        w.push("l040")
        g2 = w.build(sets)
        lists, totals, _ = check(w, snap, g0, g2, len(sets))
        for t in range(1, w.n_mes):  # (the hub's own next hops carry no labels)
            assert p in lists[t][0] and len(g2.routes[(t, p)]) == 69
        assert p not in lists[0][0]
        # ... and with the pool order reversed as well
        g3 = w.build(sets[:p] + [leaves[::-1]])
        assert g3.routes == g2.routes and g3.order[(1, p)] != g2.order[(1, p)]
        lists3, totals3, _ = check(w, snap, g0, g3, len(sets))
        assert lists3 == lists and totals3[:2] == totals[:2]
    finally:
        w.close()


# ---- 8. determinism and layout -----------------------------------------------------------
def test_determinism_and_layout():
    make, anycast, tight = GRAPHS["random"]
    dbs = make()
    w = World(dbs)
    try:
        sets = w.loopbacks(anycast)
        w.build(sets)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        u, v, k = tight[0]
        dbs[u].adjacencies.remove(adj(dbs, u, v, k))
        w.push(u)
        w.build(sets)
        plan, lh = w.ls._k2r[0].plan, w.ls.linkValueHashes()
        calls = []
        for _ in range(2):
            dptr, dset, totals, _ms = plan.route_delta(snap, lh)
            d_dptr, d_dset, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
            assert N.lib.spf_ksp2_route_delta_buffers(plan._h, C.byref(d_dptr), C.byref(d_dset),
                                                      C.byref(n)) == N.SPF_OK
            synchronize()
            calls.append((read_device(d_dptr.value, w.n_mes + 1, np.uint64), read_device(d_dset.value, n.value, np.uint32)))
            assert n.value == totals[0] + totals[1] > 0
            assert np.array_equal(calls[-1][0], dptr) and np.array_equal(calls[-1][1], dset)
        assert all(np.array_equal(a, b) for a, b in zip(*calls))
        dptr, dset = calls[0]
        assert dptr[0] == 0 and int(dptr[-1]) == len(dset) and np.all(np.diff(dptr.astype(np.int64)) >= 0)
        for t in range(w.n_mes):
            mine = (dset[int(dptr[t]): int(dptr[t + 1])] & np.uint32(M)).astype(np.int64)
            assert np.all(np.diff(mine) > 0) and (len(mine) == 0 or mine[-1] < len(sets))
        dptr2, dset2, uptr, urec, ulptr, ulab, utot, nbytes, _ms = plan.route_update()
        assert np.array_equal(dptr2, dptr) and np.array_equal(dset2, dset)
        assert uptr[0] == 0 and int(uptr[-1]) == len(urec) and np.all(np.diff(uptr.astype(np.int64)) >= 0)
        assert ulptr[0] == 0 and int(ulptr[-1]) == len(ulab) and np.all(np.diff(ulptr.astype(np.int64)) >= 0)
        is_del = (dset & np.uint32(D)) != 0
        assert np.all((np.diff(uptr.astype(np.int64)) == 0) == is_del)  # a DELETE owns none, an UPDATE some
        assert utot == [int((~is_del).sum()), len(urec), len(ulab)]
        assert nbytes == 8 * (len(dset) + 1) + 8 * len(urec) + 8 * (len(urec) + 1) + 4 * len(ulab)
        # the device pools are the read-back; the per-source call rebases them
        bufs = plan.route_update_buffers()
        assert bufs[4:] == (len(urec), len(ulab))
        assert np.array_equal(read_device(bufs[1], len(urec), np.uint64), urec)
        assert np.array_equal(read_device(bufs[3], len(ulab), np.int32), ulab)
        for t in range(w.n_mes):
            a, b = int(dptr[t]), int(dptr[t + 1])
            up, rec, lp, lab = plan.route_update_db(t)
            assert np.array_equal(up + uptr[a], uptr[a: b + 1])
            assert np.array_equal(rec, urec[int(uptr[a]): int(uptr[b])])
            assert np.array_equal(lab, ulab[int(ulptr[int(uptr[a])]): int(ulptr[int(uptr[b])])])
            assert np.array_equal(lp + ulptr[int(uptr[a])], ulptr[int(uptr[a]): int(uptr[b]) + 1])
    finally:
        w.close()


# ---- 9. state and refusals ---------------------------------------------------------------
def status_of(call, *args):
    with pytest.raises(N.SpfError) as e:
        call(*args)
    return e.value.status


def test_state_and_refusals():
    lsdb = graph_a()
    g, other = Loaded(lsdb), Loaded(lsdb)
    try:
        n = g.n
        sp, sn = np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32)
        lab = np.arange(1, n + 1, dtype=np.int32)
        lh = (np.arange(1, 64, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        routes = lambda plan, sp=sp, sn=sn: plan.routes(g.d_pairs.ptr, g.d_pool.ptr, sp, sn, lab)  # noqa: E731
        g.execute()
        plan = g.plan
        assert status_of(plan.route_snapshot, lh) == N.SPF_E_STATE  # no routes yet
        routes(plan)
        assert status_of(plan.route_snapshot, lh[:1]) == N.SPF_E_INVALID  # link_hash too short
        assert len(plan.route_db(0)[0]) == n + 1  # ... and nothing moved
        snap = plan.route_snapshot(lh)
        assert snap.bytes() > 0 and holds_no_routes(plan)
        assert status_of(plan.route_delta, snap, lh) == N.SPF_E_STATE  # the plan holds no routes
        assert status_of(plan.route_update) == N.SPF_E_STATE  # no delta
        routes(plan)
        assert plan.route_delta(snap, lh)[2] == [0, 0, 0]
        # another srcs order
        rev = g.eng.ksp2_plan(list(range(n))[::-1])
        rev.execute(g.d_pairs.ptr, g.d_pool.ptr, g.words, g.d_cnt.ptr)
        synchronize()
        routes(rev)
        assert status_of(rev.route_delta, snap, lh) == N.SPF_E_INVALID
        assert status_of(rev.route_delta_db, 0) == N.SPF_E_STATE
        rev.close()
        g.execute()
        # another n_sets: refused, and the previous lists are unreadable
        routes(plan)
        assert plan.route_delta(snap, lh)[2] == [0, 0, 0] and len(plan.route_delta_db(0)) == 0
        routes(plan, sp[:-1], sn[:-1])
        assert status_of(plan.route_delta, snap, lh) == N.SPF_E_INVALID
        assert status_of(plan.route_delta_db, 0) == N.SPF_E_STATE
        assert status_of(plan.route_update) == N.SPF_E_STATE
        assert N.lib.spf_ksp2_route_delta_buffers(plan._h, None, None, None) == N.SPF_E_STATE
        # a snapshot of another context
        other.execute()
        other.plan.routes(other.d_pairs.ptr, other.d_pool.ptr, sp, sn, lab)
        foreign = other.plan.route_snapshot(lh)
        routes(plan)
        assert status_of(plan.route_delta, foreign, lh) == N.SPF_E_INVALID
        # an update after a later spf_ksp2_routes, or after a snapshot took the routes
        plan.route_delta(snap, lh)
        plan.route_update()
        routes(plan)
        assert status_of(plan.route_update) == N.SPF_E_STATE
        assert status_of(plan.route_update_db, 0) == N.SPF_E_STATE
        plan.route_delta(snap, lh)
        later = plan.route_snapshot(lh)
        assert status_of(plan.route_update) == N.SPF_E_STATE
        later.close()
        assert later.closed
        # the snapshot outlives its plan and a reload of the graph
        plan.close()
        with LinkState(device=-1) as ls:
            ls.updateAdjacencyDatabases(lsdb)
            g.eng.load(*ls.flatten()[1:])
        plan = g.plan = g.eng.ksp2_plan(list(range(n)))
        g.execute()
        routes(plan)
        assert plan.route_delta(snap, lh)[2] == [0, 0, 0]
        lab[3] = 4242  # ... and still tells a difference
        routes(plan)
        assert plan.route_delta(snap, lh)[2][0] > 0
        # closing the engine closes its snapshots with it
        g.eng.close()
        assert snap.closed
    finally:
        g.close()
        other.close()


# ---- 10. the facade ------------------------------------------------------------------------
def test_facade_update_is_the_difference_of_the_next_hop_sets():
    make, anycast, tight = GRAPHS["random"]
    dbs = make()
    w = World(dbs)
    try:
        sets = w.loopbacks(anycast)
        sp, sn, _ = flatten_sets(sets, None, w.id_of)

        def thrift():
            w.ls.allSourcesKsp2Routes(sp, sn)
            return {(t, p): w.ls.allSourcesKsp2NextHops(t, p) for t in range(w.n_mes) for p in range(len(sets))}

        nh0 = thrift()
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        u, v, k = tight[1]
        dbs[u].adjacencies.remove(adj(dbs, u, v, k))
        w.push(u)
        nh1 = thrift()
        w.ls.allSourcesKsp2RouteUpdate(snap)
        changed = 0
        for t in range(w.n_mes):
            updates, deletes = w.ls.allSourcesKsp2DecisionRouteUpdate(t)
            for p in range(len(sets)):
                o, n = nh0[(t, p)], nh1[(t, p)]
                if not n:
                    assert (p in deletes) == bool(o) and p not in updates, (t, p)
                elif o != n:
                    assert updates[p] == n and p not in deletes, (t, p)
                else:
                    assert p not in updates and p not in deletes, (t, p)
            changed += len(updates) + len(deletes)
        assert changed > 0
    finally:
        w.close()
