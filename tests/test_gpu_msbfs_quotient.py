"""msbfs_kernel's sweep over the twin-class quotient graph (nodes with equal
neighbour sets share a frontier slot: a pod's rack switches, a plane's spines)
against the CPU oracle, bit-exact: every source's distance row and next-hop
bitmaps, once with the quotient sweep and once with SPF_QUOTIENT=0 (the plain
sweep).  Graphs without twins must keep the plain sweep."""

import ctypes as C

import numpy as np
import pytest

from oracle import OracleLinkState
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.engine import SpfEngine, graph_from_lsdb
from openr_amd.lsdb import PackedLsdb

pytestmark = pytest.mark.gpu

U32_INF = np.uint32(0xFFFFFFFF)


def small_fabric():
    """3 pods, 2 planes x 2 spines, 2 fabric and 3 rack switches per pod: 19 nodes."""
    return T.fabric(2 * 2 + 3 * (2 + 3), ssw_per_plane=2, fsw_per_pod=2, rsw_per_pod=3)


def mid_fabric():
    """24 pods of 4 + 20, 4 planes x 4 spines: 592 nodes = 9 slices + 16 (three
    sources per workgroup; the 20-member classes straddle slices and waves)."""
    return T.fabric(4 * 4 + 24 * (4 + 20), ssw_per_plane=4, fsw_per_pod=4, rsw_per_pod=20)


def db_names(lsdb):
    return [bytes(lsdb.blob[o: o + n]).decode()
            for o, n in zip(lsdb.dbs["name_off"], lsdb.dbs["name_len"])]


def adjacencies(lsdb):
    """(advertising node, other node) of every packed adjacency, in lsdb.adjs order."""
    out = []
    for name, b, k in zip(db_names(lsdb), lsdb.dbs["adj_begin"], lsdb.dbs["adj_count"]):
        for a in lsdb.adjs[int(b): int(b) + int(k)]:
            o, n = int(a["other_off"]), int(a["other_len"])
            out.append((name, bytes(lsdb.blob[o: o + n]).decode()))
    return out


def with_changes(lsdb, drain=(), links_down=(), metric=None):
    """Nodes (by name) drained, adjacencies (by index) overloaded = their link
    down in both directions, metrics replaced."""
    dbs, adjs = lsdb.dbs.copy(), lsdb.adjs.copy()
    names = db_names(lsdb)
    for n in drain:
        dbs["is_overloaded"][names.index(n)] = 1
    for k in links_down:
        adjs["is_overloaded"][k] = 1
    if metric is not None:
        adjs["metric"] = metric
    return PackedLsdb(lsdb.blob, dbs, adjs)


def quotient(eng):
    n_cls, n_edge, used = C.c_uint32(), C.c_uint64(), C.c_uint32()
    eng._err(N.lib.spf_graph_quotient(eng._h, C.byref(n_cls), C.byref(n_edge), C.byref(used)))
    return n_cls.value, n_edge.value, bool(used.value)


def expected(names, lsdb, hop):
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    dist, mats = orc.dense(names, list(range(len(names))), ulm=not hop)
    return np.where(dist == np.iinfo(np.uint64).max, U32_INF, dist).astype(np.uint32), mats


def same(names, eng, exp, mats, hop):
    res = eng.solve(list(range(len(names))), hop=hop)
    assert np.array_equal(res.dist, exp), "distance mismatch"
    for s in range(len(names)):
        k = len(eng.neighbors(s))
        assert int(res.words[s]) == k
        assert not mats[s][k:].any()
        assert np.array_equal(res.nh_matrix(s), mats[s][:k]), f"next hops of {names[s]}"


def both_sweeps(monkeypatch, lsdb, hop=False, twins=True):
    """A fresh load of lsdb solved with the quotient sweep and with the plain
    one; returns the engine of the first."""
    monkeypatch.setenv("SPF_MSBFS", "masks")   # msbfs_kernel, not the register-plane BFS
    monkeypatch.setenv("SPF_MSBFS_TEAM", "0")  # nor the team kernel
    names, rp, col, met, lid, ovl = graph_from_lsdb(lsdb)
    exp, mats = expected(names, lsdb, hop)
    kept = None
    for knob in (None, "0"):
        if knob is None:
            monkeypatch.delenv("SPF_QUOTIENT", raising=False)
        else:
            monkeypatch.setenv("SPF_QUOTIENT", knob)
        eng = SpfEngine(0)
        eng.load(rp, col, met, lid, ovl)
        assert eng.plan([0], hop=hop).kernels()[0] == "msbfs_kernel"
        assert quotient(eng)[2] == (twins and knob is None)
        same(names, eng, exp, mats, hop)
        if kept is None:
            kept = eng
        else:
            eng.close()
    return names, kept


def test_small_fabric_all_sources(monkeypatch):
    """A twin as source; the source's twins are found at level 2."""
    names, eng = both_sweeps(monkeypatch, small_fabric().lsdb)
    n_cls, n_edge, used = quotient(eng)
    assert n_cls == 3 * 2 + 3 + 2  # fabric switches, rack classes, spine classes
    assert n_edge == 2 * (3 * 2 + 3 * 2)  # fabric switch -- its plane's spines, its pod's racks
    eng.close()


@pytest.mark.parametrize("drain", [["3-1-2"], ["1-0-1"], ["3-1-2", "3-1-0", "1-0-1", "2-2-0"]],
                         ids=["rack", "spine", "several"])
def test_small_fabric_drained_members(monkeypatch, drain):
    """A drained class member, a drained source, a drained source with twins."""
    names, eng = both_sweeps(monkeypatch, with_changes(small_fabric().lsdb, drain=drain))
    eng.close()


def test_mid_fabric_classes_straddle_slices_and_waves(monkeypatch):
    """N no multiple of 64, 20-member classes across slice and wave borders,
    several sources (twins among them, some drained) per workgroup."""
    lsdb = mid_fabric().lsdb
    names = db_names(lsdb)
    drain = [n for n in names if n.startswith("3-5-")][:3] + ["1-2-1", "2-7-3", "3-11-19"]
    _, eng = both_sweeps(monkeypatch, with_changes(lsdb, drain=drain))
    assert len(names) % 64 and quotient(eng)[0] == 24 * 4 + 24 + 4
    eng.close()


@pytest.mark.parametrize("batch", ["20", "64"])
def test_full_batches_share_class_slots(monkeypatch, batch):
    """SPF_MSBFS_BATCH sources per workgroup whatever the device: whole twin
    classes (20 rack switches, some drained, and their drained fabric switch)
    are sources of one workgroup, their bits meeting in one class slot."""
    monkeypatch.setenv("SPF_MSBFS_BATCH", batch)
    lsdb = mid_fabric().lsdb
    names = db_names(lsdb)
    drain = [n for n in names if n.startswith("3-5-")][:3] + ["1-2-1", "1-2-2", "2-5-0", "2-7-3", "3-11-19"]
    _, eng = both_sweeps(monkeypatch, with_changes(lsdb, drain=drain))
    eng.close()


def test_pod_cut_off_is_unreachable(monkeypatch):
    """Every uplink of pod 1 down: the unreachable epilogue with class members."""
    topo = small_fabric()
    down = [k for k, (a, b) in enumerate(adjacencies(topo.lsdb)) if a.startswith("2-1-") and b.startswith("1-")]
    assert len(down) == 2 * 2
    lsdb = with_changes(topo.lsdb, links_down=down)
    names, eng = both_sweeps(monkeypatch, lsdb)
    d = eng.solve([names.index("3-1-0")]).dist[0]
    assert d[names.index("3-0-0")] == U32_INF and d[names.index("3-1-2")] == 2
    eng.close()


def test_hop_count_on_a_weighted_fabric(monkeypatch):
    """SPF_FLAG_HOP_COUNT plans of a weighted graph run the same kernel."""
    topo = small_fabric()
    rng = np.random.default_rng(2)
    lsdb = with_changes(topo.lsdb, metric=rng.integers(1, 9, len(topo.lsdb.adjs)).astype(np.int32))
    _, eng = both_sweeps(monkeypatch, lsdb, hop=True)
    eng.close()


@pytest.mark.parametrize("name,make,hop", [("grid10", lambda: T.grid(10), False),
                                           ("ring", lambda: T.wan(70, 0, seed=1), True)],  # (weighted: hop counts)
                         ids=["grid10", "ring"])
def test_graphs_without_twins_keep_the_plain_sweep(monkeypatch, name, make, hop):
    topo = make()
    names, eng = both_sweeps(monkeypatch, topo.lsdb, hop=hop, twins=False)
    n_cls, n_edge, used = quotient(eng)
    assert n_cls == len(names) and not used
    eng.close()


def test_row_patch_splits_a_class_and_joins_it_again(monkeypatch):
    """One rack-switch link down through spf_graph_patch_rows: the rack leaves
    its class (and its fabric switch's row changes); results follow the oracle.
    Up again: the class is whole again."""
    monkeypatch.setenv("SPF_MSBFS", "masks")
    monkeypatch.setenv("SPF_MSBFS_TEAM", "0")
    topo = small_fabric()
    names, rp, col, met, lid, ovl = graph_from_lsdb(topo.lsdb)
    u, v = names.index("3-1-2"), names.index("2-1-0")
    e = [q for q in range(int(rp[u]), int(rp[u + 1])) if col[q] == v][0]
    r = [q for q in range(int(rp[v]), int(rp[v + 1])) if lid[q] == lid[e]][0]
    k_adj = [k for k, ab in enumerate(adjacencies(topo.lsdb)) if ab == ("3-1-2", "2-1-0")]
    assert len(k_adj) == 1
    states = {False: expected(names, with_changes(topo.lsdb, links_down=k_adj), False),
              True: expected(names, topo.lsdb, False)}

    def patch(eng, up):
        nodes = np.array([u, v], np.uint32)
        cc, mm, ll = [], [], []
        for x in (u, v):
            for q in range(int(rp[x]), int(rp[x + 1])):
                dead = (q in (e, r)) and not up
                cc.append(x if dead else int(col[q]))
                mm.append(1 if dead else int(met[q]))
                ll.append(int(lid[q]))
        cc, mm, ll = np.array(cc, np.uint32), np.array(mm, np.int32), np.array(ll, np.uint32)
        eng._err(N.lib.spf_graph_patch_rows(eng._h, N.ptr(nodes), 2, N.ptr(cc), N.ptr(mm, C.c_int32),
                                            N.ptr(ll)))

    for knob in (None, "0"):
        if knob is None:
            monkeypatch.delenv("SPF_QUOTIENT", raising=False)
        else:
            monkeypatch.setenv("SPF_QUOTIENT", knob)
        eng = SpfEngine(0)
        eng.load(rp, col, met, lid, ovl)
        same(names, eng, *states[True], False)
        whole = quotient(eng)[0]
        for up in (False, True):
            patch(eng, up)
            # down: {3-1-2} alone, {3-1-0, 3-1-1} still twins
            assert quotient(eng)[0] == whole + (0 if up else 1)
            assert quotient(eng)[2] == (knob is None)
            same(names, eng, *states[up], False)
        eng.close()
