"""Every node's KSP2_ED_ECMP routes (SR-MPLS label stacks) on the GPU
(spf_ksp2_routes, include/openr_spf.h): selectBestPathsKsp2,
Decision.cpp:895-1018, for every node and every destination set at once, from
the device-resident paths of a batched KSP2 pass.

Every expectation comes from the oracle's restatement of that function
(oracle.sr_nexthops(..., ksp2=True)), never from the product's host solvers;
the one exception pins the facade's decoding against SpfSolver._ksp2NextHops.
Next hops compare as sets of (ifName, metric, neighbour, action, labels), for
every route of every listed node: integers, no tolerance.
"""

import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import OracleLinkState, sr_nexthops
from refcases import dbs_from_json, load_cases
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.engine import SpfEngine
from openr_amd.hiprt import DeviceArray, read_device, synchronize
from openr_amd.link_state import LinkState
from openr_amd.lsdb import create_adj_db, create_adjacency, pack, pack_fast
from openr_amd.spf_solver import SpfSolver

pytestmark = pytest.mark.gpu


# ---- graphs ---------------------------------------------------------------------
def lsdb_from_links(links, label, drained=()):
    """links: (u, v, metric u->v, metric v->u, overloaded); label: {node: label}."""
    adjs = {n: [] for n in label}
    seen = {}
    for i, (u, v, mu, mv, ovl) in enumerate(links):
        k = seen.get((u, v), 0)
        seen[(u, v)] = k + 1
        a = create_adjacency(v, f"{u}/{v}/{k}", f"{v}/{u}/{k}", f"fe80::{i + 1:x}", f"10.0.{i}.1", mu,
                             50000 + 2 * i)
        b = create_adjacency(u, f"{v}/{u}/{k}", f"{u}/{v}/{k}", f"fe80::1:{i + 1:x}", f"10.0.{i}.2", mv,
                             50001 + 2 * i)
        a.isOverloaded = b.isOverloaded = ovl
        adjs[u].append(a)
        adjs[v].append(b)
    return pack([create_adj_db(n, adjs[n], label[n], overLoadBit=(n in drained)) for n in label])


def golden_lsdb(name):
    case = next(c for c in load_cases() if c["name"] == name)
    return pack(dbs_from_json(case["steps"][0]["update"]))


def graph_a(label=None):
    """Two components, 13 nodes: b1..b9 with parallel links (b1-b2 at equal
    metrics, b4-b7 at different ones), b3 drained, the b5-b8 link overloaded;
    a1, a2, c1, c2: a ring nobody in b* reaches."""
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
    label = label or {n: 100 + i for i, n in enumerate(nodes)}
    return lsdb_from_links(links, label, drained=("b3",))


def star(labels):
    """me -l1- x, x - y, x - z, all metric 1."""
    return lsdb_from_links([("me", "x", 1, 1, False), ("x", "y", 1, 1, False), ("x", "z", 1, 1, False)],
                           labels)


def hub(leaves, zero_labels):
    nodes = ["hub"] + [f"l{i:03d}" for i in range(leaves)]
    src, dst, ifs, oifs = [], [], [], []
    for i in range(1, leaves + 1):
        for a, b in ((0, i), (i, 0)):
            src.append(a)
            dst.append(b)
            ifs.append(f"{nodes[a]}/{nodes[b]}")
            oifs.append(f"{nodes[b]}/{nodes[a]}")
    lab = np.zeros(len(nodes), np.int32) if zero_labels else np.arange(1, len(nodes) + 1, dtype=np.int32)
    return pack_fast(nodes, np.asarray(src), np.asarray(dst), ifs, oifs, np.ones(len(src), np.int32),
                     node_label=lab), nodes


# ---- product and oracle -----------------------------------------------------------
def flat_sets(sets, prepends, id_of):
    """[[names]] (+ [{name: prepend}]) -> set_ptr, set_nodes (ascending id), prepend list."""
    ptr, nodes, pre = [0], [], []
    for p, s in enumerate(sets):
        ids = sorted(id_of[d] for d in s)
        nodes += ids
        ptr.append(len(nodes))
        by_id = {id_of[d]: (prepends[p].get(d) if prepends else None) for d in s}
        pre += [by_id[i] for i in ids]
    return np.array(ptr, np.uint32), np.array(nodes, np.uint32), (pre if prepends else None)


def product(lsdb, sets, prepends=None, me_names=None, kinds=None):
    """{(me, p): rows in rec order}, rows = (ifName, metric, neighbour, action,
    labels), and the call's totals.  `kinds`: the KSP2 plan kinds
    (Ksp2Plan.info().kind) the paths may come from."""
    with LinkState(device=0) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        names, _rp, col, _met, lid, _ovl = ls.flatten()
        id_of = {s: i for i, s in enumerate(names)}
        me_names = list(names) if me_names is None else me_names
        set_ptr, set_nodes, pre = flat_sets(sets, prepends, id_of)
        totals = ls.allSourcesKsp2Routes(set_ptr, set_nodes, pre, [id_of[m] for m in me_names])
        info = ls._k2r[0].plan.info()
        print(f"ksp2 plan: {info}")
        assert kinds is None or info.kind in kinds, (info, kinds)
        got, hops, words = {}, 0, 0
        for t, me in enumerate(me_names):
            rptr, rec, lptr, lab = ls.allSourcesKsp2RouteDb(t)
            assert len(rptr) == len(sets) + 1 and rptr[0] == 0 and int(rptr[-1]) == len(rec)
            assert len(lptr) == len(rec) + 1 and lptr[0] == 0 and int(lptr[-1]) == len(lab)
            assert np.all(np.diff(rptr.astype(np.int64)) >= 0) and np.all(np.diff(lptr.astype(np.int64)) >= 0)
            hops += len(rec)
            words += len(lab)
            for p in range(len(sets)):
                rows = []
                for h in range(int(rptr[p]), int(rptr[p + 1])):
                    e, cost = int(rec[h]) & 0xFFFFFFFF, int(rec[h]) >> 32
                    link = ls._link(int(lid[e]))
                    assert names[int(col[e])] == link.getOtherNodeName(me)
                    stack = tuple(int(x) for x in lab[int(lptr[h]): int(lptr[h + 1])])
                    rows.append((link.getIfaceFromNode(me), cost, link.getOtherNodeName(me),
                                 "PUSH" if stack else None, stack or None))
                got[(me, p)] = rows
        assert (hops, words) == totals[:2]
        assert totals[2] == 8 * hops + 8 * (len(me_names) * len(sets) + 1) + 8 * (hops + 1) + 4 * words
    return got, totals


def oracle_rows(lsdb, sets, prepends=None, me_names=None):
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    want = {}
    for me in me_names:
        for p, s in enumerate(sets):
            if not s:
                want[(me, p)] = set()
                continue
            pre = {d: (prepends[p].get(d) if prepends else None) for d in s}
            rows = sr_nexthops(orc, me, pre, lfa=False, v4=False, ksp2=True)
            want[(me, p)] = {(r[0], r[1], r[2], r[4], tuple(r[5]) if r[5] is not None else None)
                             for r in rows}
    return want


def names_of(lsdb):
    with LinkState(device=-1) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        return list(ls.flatten()[0])


def check(lsdb, sets, prepends=None, me_names=None, kinds=None):
    """Every route of every me equals the oracle's; no duplicates in a route.
    Returns (got, want)."""
    me_names = names_of(lsdb) if me_names is None else me_names
    want = oracle_rows(lsdb, sets, prepends, me_names)
    got, _ = product(lsdb, sets, prepends, me_names, kinds)
    assert set(got) == set(want)
    for k, rows in got.items():
        assert len(rows) == len(set(rows)), (k, rows)
    bad = [k for k in want if set(got[k]) != want[k]]
    assert not bad, (bad[:3], [(got[k], sorted(want[k], key=str)) for k in bad[:1]])
    return got, want


# ---- 1. reference-pinned shapes -----------------------------------------------------
def test_ring():
    lsdb = golden_lsdb("decision_ring_ksp2_routes_v6")
    nodes = names_of(lsdb)
    got, _ = check(lsdb, [[n] for n in nodes])
    # DecisionTest's expectations for node 1 (golden reference_expectations.json)
    case = next(c for c in load_cases() if c["name"] == "decision_ring_ksp2_routes_v6")
    exp = case["checks"][0]["expect"]["1"]
    for dst, rows in exp.items():
        want = {(r[0], r[1], r[2], r[4], tuple(r[5]) if r[5] is not None else None) for r in rows}
        assert set(got[("1", nodes.index(dst))]) == want, dst


def test_full_mesh_anycast_drops_k2_paths():
    """A -> B -> C contains A -> B (Decision.cpp:942-947): towards {2, 3} node
    1 keeps its two direct paths and the k = 2 paths through 4; those through
    2 and 3 vanish."""
    lsdb = golden_lsdb("decision_mesh_ksp2_routes_v6")
    nodes = names_of(lsdb)
    assert nodes == ["1", "2", "3", "4"]
    sets = [[n] for n in nodes] + [["2", "3"]]
    got, want = check(lsdb, sets)
    assert sorted((r[2], r[4]) for r in got[("1", 4)]) == [("2", None), ("3", None), ("4", (2,)), ("4", (3,))]
    # (alone, each of them also has k = 2 paths through the others)
    assert len(got[("1", 1)]) == 3 and len(got[("1", 2)]) == 3


def test_parallel_adjacency_ring():
    lsdb = golden_lsdb("decision_parallel_adj_ring")
    nodes = names_of(lsdb)
    got, _ = check(lsdb, [[n] for n in nodes] + [["2", "3"], ["1", "4"]])
    assert any(len(rows) > 2 for rows in got.values())  # parallel links give more than two paths


# ---- 2. dedup ---------------------------------------------------------------------
@pytest.mark.parametrize("ly, lz, n_hops", [(0, 0, 1), (7, 8, 2), (9, 9, 1)],
                         ids=["no_labels", "distinct", "shared"])
def test_dedup(ly, lz, n_hops):
    lsdb = star({"me": 1, "x": 2, "y": ly, "z": lz})
    got, _ = check(lsdb, [["y", "z"]])
    rows = got[("me", 0)]
    assert len(rows) == n_hops
    assert rows[0] == ("me/x/0", 2, "x", "PUSH", (ly,))
    if n_hops == 2:
        assert rows[1] == ("me/x/0", 2, "x", "PUSH", (lz,))


# ---- 3. prepend -------------------------------------------------------------------
def test_prepend():
    label = {"p1": 11, "p2": 12, "p3": 13, "p4": 14}
    lsdb = lsdb_from_links([("p1", "p2", 1, 1, False), ("p2", "p3", 1, 1, False),
                            ("p3", "p4", 1, 1, False)], label)
    sets = [["p2"], ["p2"], ["p4"], ["p2", "p4"]]
    pre = [{"p2": 900}, {"p2": None}, {"p4": 901}, {"p2": None, "p4": 902}]
    got, _ = check(lsdb, sets, pre)
    assert got[("p1", 0)] == [("p1/p2/0", 1, "p2", "PUSH", (900,))]  # one hop, a prepend
    assert got[("p1", 1)] == [("p1/p2/0", 1, "p2", None, None)]  # one hop, none: no action
    assert got[("p1", 2)] == [("p1/p2/0", 3, "p2", "PUSH", (901, 14, 13))]  # three hops
    assert got[("p1", 3)] == [("p1/p2/0", 1, "p2", None, None),
                              ("p1/p2/0", 3, "p2", "PUSH", (902, 14, 13))]


# ---- 4. set edges -------------------------------------------------------------------
def test_set_edges():
    lsdb = graph_a()
    sets = [[], ["b1"], ["b1", "b4", "b7"], ["a1"], ["b9", "c1"], ["b4"], ["b8"], ["b5"], ["b3"]]
    got, want = check(lsdb, sets)
    for me in names_of(lsdb):
        assert got[(me, 0)] == []  # the empty set
    assert got[("b1", 1)] == []  # {me}
    assert got[("b1", 2)] and all(r[2] in ("b2", "b9") for r in got[("b1", 2)])  # me and others
    assert got[("b1", 3)] == [] and got[("a2", 3)]  # another component
    assert got[("b1", 4)] and got[("c2", 4)]  # one member reachable from either side
    # behind the drained b3 the short way b1-b2-b3-b4 is closed: b2-b4 at 3 is taken
    assert min(r[1] for r in got[("b1", 5)]) == 4
    # the overloaded b5-b8 link carries nothing: b5 reaches b8 around it
    assert min(r[1] for r in got[("b5", 6)]) == 4


# ---- 5. more than 64 candidates in one route ---------------------------------------
def test_more_than_64_candidates():
    lsdb, nodes = hub(70, zero_labels=False)
    leaves = nodes[1:]
    got, _ = check(lsdb, [leaves], me_names=["hub", "l000", "l069"])
    assert len(got[("hub", 0)]) == 70 and all(r[3] is None for r in got[("hub", 0)])
    # candidate order = set order: the hub's links in leaf order
    assert [r[2] for r in got[("hub", 0)]] == leaves
    for me in ("l000", "l069"):
        rows = got[(me, 0)]
        assert len(rows) == 69 and {r[0] for r in rows} == {f"{me}/hub"}
        # first occurrences in candidate order: the other leaves' labels ascending
        assert [r[4] for r in rows] == [(i + 1,) for i, n in enumerate(nodes) if i and n != me]


def test_dedup_across_chunks():
    lsdb, nodes = hub(70, zero_labels=True)
    got, _ = check(lsdb, [nodes[1:]], me_names=["hub", "l000", "l069"])
    assert len(got[("hub", 0)]) == 70
    for me in ("l000", "l069"):
        assert got[(me, 0)] == [(f"{me}/hub", 2, "hub", "PUSH", (0,))]


# ---- 6. seeded random multigraph ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case():
    topo = T.random_graph(60, 170, 12, max_metric=6, parallel_frac=0.25, overload_frac=0.1,
                          link_overload_frac=0.05)
    rng = np.random.default_rng(77)
    n = len(topo.nodes)
    lab = 1000 + rng.permutation(n).astype(np.int32)
    lab[rng.random(n) < 0.1] = 0
    pick = rng.choice(np.nonzero(lab)[0], 10, replace=False)
    lab[pick[5:]] = lab[pick[:5]]
    topo.lsdb.dbs["node_label"] = lab
    sets, pre = [], []
    for _ in range(16):
        members = [topo.nodes[int(i)] for i in rng.choice(n, int(rng.integers(1, 5)), replace=False)]
        sets.append(members)
        pre.append({d: (int(rng.integers(60000, 60100)) if rng.random() < 0.5 else None) for d in members})
    return topo.lsdb, dict(zip(topo.nodes, lab.tolist())), sets, pre


# the paths the routes are built from: written by the staged-graph kernel (the
# default on this graph) or by ksp2_kernel (SPF_KSP2_HBM)
KSP2_KERNELS = [("staged", None, ("LDS_U16", "LDS_U32")), ("hbm", "1", ("HBM",))]


@pytest.mark.parametrize("hbm,kinds", [k[1:] for k in KSP2_KERNELS], ids=[k[0] for k in KSP2_KERNELS])
def test_random_multigraph(hbm, kinds, monkeypatch):
    if hbm:
        monkeypatch.setenv("SPF_KSP2_HBM", hbm)
    else:
        monkeypatch.delenv("SPF_KSP2_HBM", raising=False)
    lsdb, _label_of, sets, pre = random_case()
    got, _ = check(lsdb, sets, pre, kinds=kinds)
    assert sum(len(r) for r in got.values()) > 2 * len(got)  # (most routes have k = 2 paths too)


# ---- 7. weighted sparse graph ---------------------------------------------------------
def test_wan():
    topo = T.wan(200, 100, seed=1)
    nodes = sorted(topo.nodes)
    rng = np.random.default_rng(3)
    topo.lsdb.dbs["node_label"] = np.array([nodes.index(s) + 1 for s in topo.nodes], np.int32)
    mes = [nodes[int(i)] for i in rng.choice(len(nodes), 24, replace=False)]
    sets = [[n] for n in nodes]
    for _ in range(8):
        sets.append([nodes[int(i)] for i in rng.choice(len(nodes), int(rng.integers(2, 5)), replace=False)])
    check(topo.lsdb, sets, None, mes)


# ---- 8, 9: the engine's calls -------------------------------------------------------
class Loaded:
    """An engine with the LSDB's graph, an executed all-sources KSP2 plan."""

    def __init__(self, lsdb=None, csr=None):
        if csr is None:
            with LinkState(device=-1) as ls:
                ls.updateAdjacencyDatabases(lsdb)
                csr = ls.flatten()[1:]
        self.n = len(csr[0]) - 1
        self.eng = SpfEngine(0)
        self.eng.load(*csr)
        self.plan = self.eng.ksp2_plan(list(range(self.n)))
        self.d_pairs = DeviceArray(4 * self.n * self.n, np.uint32)
        self.words = 1 << 20
        self.d_pool = DeviceArray(self.words, np.uint32)
        self.d_cnt = DeviceArray(4, np.uint64)

    def execute(self):
        self.plan.execute(self.d_pairs.ptr, self.d_pool.ptr, self.words, self.d_cnt.ptr)
        synchronize()
        assert not int(self.d_cnt.numpy()[2]) & 1

    def close(self):
        self.eng.close()
        for b in (self.d_pairs, self.d_pool, self.d_cnt):
            b.free()


def test_layout_and_determinism():
    lsdb, _label_of, sets, pre = random_case()
    names = names_of(lsdb)
    id_of = {s: i for i, s in enumerate(names)}
    set_ptr, set_nodes, prepend = flat_sets(sets, pre, id_of)
    prepend = [-1 if v is None else v for v in prepend]
    lab = np.arange(1, len(names) + 1, dtype=np.int32)
    g = Loaded(lsdb)
    try:
        g.execute()
        calls = []
        for _ in range(2):
            hops, words, nbytes, ms = g.plan.routes(g.d_pairs.ptr, g.d_pool.ptr, set_ptr, set_nodes, lab,
                                                    prepend)
            parts = g.plan.routes_timing()
            assert ms > 0 and all(x >= 0 for x in parts)
            assert abs(sum(parts) - ms) <= 1e-6 * max(1.0, ms)
            d_rptr, d_rec, d_lptr, d_lab, h2, w2 = g.plan.route_buffers()
            assert (h2, w2) == (hops, words) and hops > 0 and words > 0
            n_routes = g.n * len(sets)
            assert nbytes == 8 * hops + 8 * (n_routes + 1) + 8 * (hops + 1) + 4 * words
            synchronize()
            arrs = (read_device(d_rptr, n_routes + 1, np.uint64), read_device(d_rec, hops, np.uint64),
                    read_device(d_lptr, hops + 1, np.uint64), read_device(d_lab, words, np.int32))
            calls.append(arrs)
        rptr, rec, lptr, lab_words = calls[0]
        assert all(np.array_equal(x, y) for x, y in zip(*calls))  # a second call: identical arrays
        assert np.all(np.diff(rptr.astype(np.int64)) >= 0) and np.all(np.diff(lptr.astype(np.int64)) >= 0)
        assert rptr[0] == 0 and int(rptr[-1]) == hops == len(rec)
        assert lptr[0] == 0 and int(lptr[-1]) == words
        # route_db(i) of every i concatenates to the device arrays
        S = len(sets)
        dbs = [g.plan.route_db(i) for i in range(g.n)]
        for i, (rp, rc, lp, lb) in enumerate(dbs):
            assert np.array_equal(rp + rptr[i * S], rptr[i * S: (i + 1) * S + 1])
        assert np.array_equal(np.concatenate([d[1] for d in dbs]), rec)
        assert np.array_equal(np.concatenate([d[3] for d in dbs]), lab_words)
        off = np.cumsum([0] + [len(d[3]) for d in dbs])
        assert np.array_equal(np.concatenate([d[2][:-1] + off[i] for i, d in enumerate(dbs)] +
                                             [[words]]).astype(np.uint64), lptr)
    finally:
        g.close()


def raw_routes(plan, d_pairs, d_pool, set_ptr, set_nodes, label):
    """spf_ksp2_routes itself (no wrapper checks); set_ptr / label None: a NULL pointer."""
    sp = None if set_ptr is None else np.asarray(set_ptr, np.uint32)
    sn = np.asarray(set_nodes, np.uint32)
    lab = None if label is None else np.asarray(label, np.int32)
    return N.lib.spf_ksp2_routes(plan._h, C.c_void_p(d_pairs), C.c_void_p(d_pool),
                                 None if sp is None else N.ptr(sp), N.ptr(sn),
                                 1 if sp is None else len(sp) - 1, None,
                                 None if lab is None else N.ptr(lab, C.c_int32), None, None, None, None)


def holds_no_routes(plan):
    with pytest.raises(N.SpfError) as e1:
        plan.route_db(0)
    with pytest.raises(N.SpfError) as e2:
        plan.route_buffers()
    with pytest.raises(N.SpfError) as e3:
        plan.routes_timing()
    return {e.value.status for e in (e1, e2, e3)} == {N.SPF_E_STATE}


def test_refusals():
    g = Loaded(star({"me": 1, "x": 2, "y": 3, "z": 4}))
    try:
        g.execute()
        plan, pairs, pool = g.plan, g.d_pairs.ptr, g.d_pool.ptr
        lab = [1, 2, 3, 4]
        assert holds_no_routes(plan)  # before the first call
        assert raw_routes(plan, pairs, pool, [0, 1], [2], lab) == N.SPF_OK
        plan._rt_sets = 1
        assert len(plan.route_db(0)[0]) == 2
        for args in ((0, pool, [0, 1], [2], lab), (pairs, 0, [0, 1], [2], lab),
                     (pairs, pool, None, [2], lab), (pairs, pool, [0, 1], [2], None),
                     (pairs, pool, [0, 1], [4], lab),  # a set node >= n_nodes
                     (pairs, pool, [0, 2, 1], [1, 2], lab)):  # a non-monotone set_ptr
            st = raw_routes(plan, *args)
            assert st == N.SPF_E_INVALID, args
            assert holds_no_routes(plan)  # after a refused call
            assert raw_routes(plan, pairs, pool, [0, 1], [2], lab) == N.SPF_OK
    finally:
        g.close()


def test_cost_bound_is_refused():
    """max metric x (n_nodes - 1) >= 2^32: a cost might not fit the record."""
    big = 1500000000  # x 3 links >= 2^32
    # a 4-node ring as CSR: link k joins k and (k + 1) % 4; link 0 carries the big metric
    row_ptr = [0, 2, 4, 6, 8]
    col = [1, 3, 0, 2, 1, 3, 2, 0]
    link = [0, 3, 0, 1, 1, 2, 2, 3]
    metric = [big if k == 0 else 1 for k in link]
    g = Loaded(csr=(row_ptr, col, metric, link, [0, 0, 0, 0]))
    try:
        assert raw_routes(g.plan, g.d_pairs.ptr, g.d_pool.ptr, [0, 1], [2], [1, 2, 3, 4]) == N.SPF_E_UNSUPPORTED
        assert holds_no_routes(g.plan)
    finally:
        g.close()


# ---- 10. the facade -------------------------------------------------------------------
def facade_case(lsdb, sets, pre):
    with LinkState(device=0) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        names = list(ls.flatten()[0])
        id_of = {s: i for i, s in enumerate(names)}
        set_ptr, set_nodes, prepend = flat_sets(sets, pre, id_of)
        ls.allSourcesKsp2Routes(set_ptr, set_nodes, prepend)
        labels = ls.getAdjacencyDatabaseLabels()
        area = ls.getArea()
        routes = 0
        for t, me in enumerate(names):
            ls.prefetchKthPaths(me)
            solver = SpfSolver(me, False, False)
            for p, s in enumerate(sets):
                ents = {(d, area): SimpleNamespace(prependLabel=(pre[p].get(d) if pre else None)) for d in s}
                want = solver._ksp2NextHops(ls, me, area, [(d, area) for d in s], ents, False, labels)
                got = ls.allSourcesKsp2NextHops(t, p)
                assert got == want, (me, p)
                routes += len(got)
        return routes


def test_facade_equals_host_solver_dedup_graph():
    for ly, lz in ((0, 0), (7, 8), (9, 9)):
        assert facade_case(star({"me": 1, "x": 2, "y": ly, "z": lz}), [["y", "z"], ["x"]], None) > 0


def test_facade_equals_host_solver_random_graph():
    lsdb, label_of, sets, pre = random_case()
    keep = [p for p, s in enumerate(sets) if len({label_of[d] for d in s}) == len(s)]
    assert len(keep) >= 8
    assert facade_case(lsdb, [sets[p] for p in keep], [pre[p] for p in keep]) > 0
