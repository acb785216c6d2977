"""Class rows (class_bfs_kernel + expand_rows_kernel: one BFS row per twin class
among a plan's closure rows, the node rows, bit planes and u8 rows expanded
from those) against the CPU oracle, bit for bit: distance rows and next-hop
matrices, once on the class path (SPF_CLASS_ROWS=1; spf_plan_class_rows reports
it in use) and once with SPF_CLASS_ROWS=0 (msbfs_kernel's rows).  Every case runs with
SPF_MSBFS=masks and SPF_MSBFS_TEAM=0.

The depth case: a K(4,20) with a tail past 254 levels cannot have its quotient
in use (the tail's nodes are classes of their own: 4 + 2t quotient edges
against 160 + 2t neighbour entries, and the sweep wants half: t <= 76), so the
deep case hangs its tail off a K(4,160); the tails of 5, 6 and 7 use K(4,20)."""

import ctypes as C

import numpy as np
import pytest

from oracle import NameTable, OracleLinkState, route_digests
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.engine import SpfEngine, graph_from_lsdb
from openr_amd.link_state import LinkState

from test_gpu_msbfs_quotient import (adjacencies, db_names, expected, mid_fabric, quotient, same,
                                     small_fabric, with_changes)

pytestmark = pytest.mark.gpu


def class_rows(plan):
    k, used = C.c_uint32(), C.c_uint32()
    assert N.lib.spf_plan_class_rows(plan._h, C.byref(k), C.byref(used)) == 0
    return k.value, bool(used.value)


def knobs(monkeypatch, class_knob, narrow="2"):
    """narrow "2": u8 rows and bit planes whatever the graph's degrees (small
    fabrics would take the u32 next-hop pass: no planes written); None: the
    plan's own choice."""
    monkeypatch.setenv("SPF_MSBFS", "masks")
    monkeypatch.setenv("SPF_MSBFS_TEAM", "0")
    if narrow is None:
        monkeypatch.delenv("SPF_NARROW", raising=False)
    else:
        monkeypatch.setenv("SPF_NARROW", narrow)
    monkeypatch.setenv("SPF_CLASS_ROWS", class_knob)


def check_sources(names, eng, srcs, exp, mats, hop):
    res = eng.solve(srcs, hop=hop)
    assert np.array_equal(res.dist, exp[srcs]), "distance mismatch"
    for i, s in enumerate(srcs):
        k = len(eng.neighbors(s))
        assert int(res.words[i]) == k
        assert np.array_equal(res.nh_matrix(i), mats[s][:k]), f"next hops of {names[s]}"


def both_paths(monkeypatch, lsdb, hop=False, srcs=None, narrow="2"):
    """lsdb solved on the class path and with SPF_CLASS_ROWS=0; the oracle's
    rows are computed once.  Returns (names, class sources of the class plan)."""
    names, rp, col, met, lid, ovl = graph_from_lsdb(lsdb)
    exp, mats = expected(names, lsdb, hop)
    k_used = 0
    for knob in ("1", "0"):
        knobs(monkeypatch, knob, narrow)
        eng = SpfEngine(0)
        eng.load(rp, col, met, lid, ovl)
        plan = eng.plan(list(range(len(names))) if srcs is None else srcs, hop=hop)
        assert plan.kernels()[0] == "msbfs_kernel"
        assert plan.row_mode() == ("sliced" if narrow else "u32")
        k, used = class_rows(plan)
        assert used == (knob == "1") and quotient(eng)[2]
        if used:
            k_used = k
        if srcs is None:
            same(names, eng, exp, mats, hop)
        else:
            check_sources(names, eng, srcs, exp, mats, hop)
        eng.close()
    return names, k_used


@pytest.mark.parametrize("narrow", ["2", None], ids=["sliced", "u32"])
def test_small_fabric_every_source(monkeypatch, narrow):
    names, k = both_paths(monkeypatch, small_fabric().lsdb, narrow=narrow)
    assert k == 3 * 2 + 3 + 2  # every class is a class source


@pytest.mark.parametrize("batch", ["1", "64"])
def test_mid_fabric_every_source(monkeypatch, batch):
    monkeypatch.setenv("SPF_MSBFS_BATCH", batch)
    names, k = both_paths(monkeypatch, mid_fabric().lsdb)
    assert k == 24 * 4 + 24 + 4


DRAINS = {
    "twin": ["3-1-2"],                                # a rack switch whose twins are not drained
    "class": ["3-1-0", "3-1-1", "3-1-2"],             # a class drained as a whole
    "neighbours": ["2-1-0", "2-1-1"],                 # every neighbour of pod 1's racks: t_C is not 2
    "representative": ["3-0-0", "1-0-0"],             # drained sources, the first of their classes
    "not_representative": ["3-2-1", "1-1-1"],         # drained sources, not the first
}


@pytest.mark.parametrize("state", list(DRAINS), ids=list(DRAINS))
def test_small_fabric_drained(monkeypatch, state):
    both_paths(monkeypatch, with_changes(small_fabric().lsdb, drain=DRAINS[state]))


def test_mid_fabric_drained(monkeypatch):
    lsdb = mid_fabric().lsdb
    names = db_names(lsdb)
    drain = [n for n in names if n.startswith("3-5-")] + ["3-7-0", "3-7-3", "1-2-1", "2-9-0", "2-9-1", "2-9-2", "2-9-3"]
    both_paths(monkeypatch, with_changes(lsdb, drain=drain))


@pytest.mark.parametrize("srcs", [list(range(300, 500)), [3, 1, 3, 0]], ids=["300..499", "3,1,3,0"])
def test_partial_plans(monkeypatch, srcs):
    both_paths(monkeypatch, T.fabric(1000, full=True).lsdb, srcs=srcs)


def test_hop_count_on_a_weighted_fabric(monkeypatch):
    topo = small_fabric()
    rng = np.random.default_rng(2)
    lsdb = with_changes(topo.lsdb, metric=rng.integers(2, 9, len(topo.lsdb.adjs)).astype(np.int32))
    both_paths(monkeypatch, lsdb, hop=True)


def bipartite_with_tail(b, tail):
    """K(4, b), a path of `tail` nodes hanging off the first of the four."""
    nodes = [f"a{i}" for i in range(4)] + [f"b{i:03d}" for i in range(b)] + [f"t{i:03d}" for i in range(tail)]
    links = [(i, 4 + j) for i in range(4) for j in range(b)]
    links += [(0 if t == 0 else 4 + b + t - 1, 4 + b + t) for t in range(tail)]
    ones = np.ones(len(links), np.int64)
    return T._undirected_to_adj(nodes, links, ones, ones, f"k4_{b}_tail{tail}")


@pytest.mark.parametrize("tail", [5, 6, 7])
def test_planes_change_at_depth_7(monkeypatch, tail):
    """Deepest level tail + 2 (a b node to the tail's end): 7, 8, 9, so the
    planes go from 3 to 4 bits."""
    both_paths(monkeypatch, bipartite_with_tail(20, tail).lsdb)


def test_depth_past_the_planes(monkeypatch):
    """Distances up to 262: exact u32 rows, no planes, next hops on the u32 rows."""
    lsdb = bipartite_with_tail(160, 260).lsdb
    names, _ = both_paths(monkeypatch, lsdb)
    exp, _ = expected(names, lsdb, False)
    assert int(exp[exp != 0xFFFFFFFF].max()) > 254


def test_copy_narrow_rows_on_demand_and_in_pass(monkeypatch):
    """The u8 rows after an execute on the class path: min(d, 254), 255 for
    unreachable and the padding, over the whole pitch; filled on the first call
    from the last execute's class rows, and by the expansion pass after that."""
    from openr_amd.hiprt import DeviceArray, synchronize

    knobs(monkeypatch, "1")
    topo = small_fabric()
    down = [k for k, (a, b) in enumerate(adjacencies(topo.lsdb)) if a.startswith("2-1-") and b.startswith("1-")]
    lsdb = with_changes(topo.lsdb, links_down=down, drain=["3-0-1"])  # pod 1 cut off: unreachable entries
    names, rp, col, met, lid, ovl = graph_from_lsdb(lsdb)
    exp, _ = expected(names, lsdb, False)
    eng = SpfEngine(0)
    eng.load(rp, col, met, lid, ovl)
    n, pitch = len(names), eng.pitch
    plan = eng.plan(list(range(n)))
    assert class_rows(plan)[1]
    dist = DeviceArray(n * pitch, np.uint32)
    nh = DeviceArray(max(1, plan.nh_words), np.uint32)
    out = DeviceArray(n * pitch, np.uint8)
    want = np.full((n, pitch), 255, np.uint8)
    want[:, :n] = np.where(exp == 0xFFFFFFFF, 255, np.minimum(exp, 254)).astype(np.uint8)
    try:
        for _ in range(2):  # the on-demand fill, then the in-pass one
            plan.execute(dist.ptr, nh.ptr)
            out.zero()
            plan.copy_narrow_rows(out.ptr)
            synchronize()
            assert np.array_equal(out.numpy().reshape(n, pitch), want)
    finally:
        for a in (dist, nh, out):
            a.free()
        eng.close()


def test_row_patch_splits_a_class(monkeypatch):
    """One link of a rack switch down through spf_graph_patch_rows: its class
    splits, the quotient is rebuilt, and the same plan object follows the oracle;
    up again, it follows it again."""
    knobs(monkeypatch, "1")
    topo = small_fabric()
    names, rp, col, met, lid, ovl = graph_from_lsdb(topo.lsdb)
    u, v = names.index("3-1-2"), names.index("2-1-0")
    e = [q for q in range(int(rp[u]), int(rp[u + 1])) if col[q] == v][0]
    r = [q for q in range(int(rp[v]), int(rp[v + 1])) if lid[q] == lid[e]][0]
    k_adj = [k for k, ab in enumerate(adjacencies(topo.lsdb)) if ab == ("3-1-2", "2-1-0")]
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
        eng._err(N.lib.spf_graph_patch_rows(eng._h, N.ptr(nodes), 2, N.ptr(cc), N.ptr(mm, C.c_int32), N.ptr(ll)))

    eng = SpfEngine(0)
    eng.load(rp, col, met, lid, ovl)
    # sources whose neighbour counts the patch leaves alone (the plan's layout holds)
    srcs = [s for s in range(len(names)) if s not in (u, v)]
    plan = eng.plan(srcs)
    k_whole = class_rows(plan)[0]

    def run_same_plan(up):
        res = plan.execute_host()
        exp, mats = states[up]
        assert np.array_equal(res.dist, exp[srcs])
        for i, s in enumerate(srcs):
            k = len(eng.neighbors(s))
            assert np.array_equal(res.nh_matrix(i), mats[s][:k]), f"next hops of {names[s]}"

    run_same_plan(True)
    for up in (False, True):
        patch(eng, up)
        run_same_plan(up)
        k, used = class_rows(plan)
        assert used and k == k_whole + (0 if up else 1)
    eng.close()


def test_two_member_route_digests_with_lfa(monkeypatch):
    """route_prepare's u8 rows filled on demand: every node's route digests
    with LFA of a two-member context equal those of SPF_CLASS_ROWS=0, and the
    oracle's."""
    topo = mid_fabric()
    out = {}
    for knob in ("1", "0"):
        knobs(monkeypatch, knob)
        with LinkState(devices=[0, 0]) as ls:
            ls.updateAdjacencyDatabases(topo.lsdb)
            ls.prefetchAllSources()
            names = list(ls.flatten()[0])
            sets = [[v] for v in range(len(names))]
            ptr = np.arange(len(sets) + 1, dtype=np.uint32)
            nodes = np.arange(len(names), dtype=np.uint32)
            out[knob], _ = ls.allSourcesRouteDigests(ptr, nodes, True)
    assert np.array_equal(out["1"], out["0"])
    orc = OracleLinkState()
    orc.update_packed(topo.lsdb)
    want = route_digests(orc, NameTable(names), np.arange(len(names)), ptr, nodes, True)
    assert np.array_equal(out["1"], want)
