"""expand_rows_kernel past one node chunk and below one row group, against the
CPU oracle, bit for bit, on the class path and with SPF_CLASS_ROWS=0.

T.fabric(2200, full=True) has 2,192 nodes: three 1,024-node chunks, the last
holding 144 nodes; 39 rack classes of 48 twins and 8 spine classes of 36 keep
the quotient in use (checked on the CPU below).  The default pitch is 3,072
for u32 and u8 rows alike; SPF_PITCH_ALIGN=64 gives 2,240 against 3,072.
The oracle solves only the sources a case asks for, once per graph state.

Every source of fabric(2200) by digest is left out: the oracle's 2,192 rows
and next-hop matrices alone take longer than a test here may."""

import functools

import numpy as np
import pytest

from openr_amd import topology as T
from openr_amd.engine import SpfEngine, graph_from_lsdb

from oracle import OracleLinkState
from test_gpu_class_rows import class_rows, knobs
from test_gpu_msbfs_quotient import U32_INF, db_names, mid_fabric, quotient, with_changes
from test_twin_classes import classes, neighbour_lists

gpu = pytest.mark.gpu

DRAIN = {
    "none": (),
    # a rack class as a whole, one twin of another class, a class source
    # (3-0-0: the first member of its class, and a source below)
    "drained": tuple(f"3-5-{k}" for k in range(48)) + ("3-7-0", "3-0-0"),
}


@functools.lru_cache(maxsize=None)
def fabric2200(state):
    lsdb = with_changes(T.fabric(2200, full=True).lsdb, drain=DRAIN[state])
    return (lsdb,) + tuple(graph_from_lsdb(lsdb))


@functools.lru_cache(maxsize=None)
def sources2200():
    """About 200 sources with self entries in every chunk: node 0, both sides of
    the chunk borders, the last node, a repeat, the drained nodes' three kinds."""
    names = fabric2200("none")[1]
    n = len(names)
    srcs = [0, 1023, 1024, 2047, 2048, n - 1] + list(range(5, n, 11))
    srcs += [names.index("3-5-3"), names.index("3-7-0"), names.index("3-0-0"), 1023]
    assert len(srcs) % 8 and len(set(srcs)) < len(srcs)
    assert all(any(lo <= s < hi for s in srcs) for lo, hi in ((0, 1024), (1024, 2048), (2048, n)))
    return tuple(srcs)


@functools.lru_cache(maxsize=None)
def oracle_rows(key, srcs):
    """(dist [len(srcs), n] u32, next-hop matrices) of the oracle; key names the graph."""
    lsdb, names = (fabric2200(key[1])[:2] if key[0] == "f2200"
                   else (mid_fabric().lsdb, tuple(graph_from_lsdb(mid_fabric().lsdb)[0])))
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    dist, mats = orc.dense(list(names), list(srcs), ulm=True)
    dist = np.where(dist == np.iinfo(np.uint64).max, U32_INF, dist).astype(np.uint32)
    dist.setflags(write=False)
    return dist, mats


def both_paths(monkeypatch, graph, key, srcs, narrow, align=None):
    names, rp, col, met, lid, ovl = graph
    exp, mats = oracle_rows(key, tuple(srcs))
    if align is None:
        monkeypatch.delenv("SPF_PITCH_ALIGN", raising=False)
    else:
        monkeypatch.setenv("SPF_PITCH_ALIGN", align)
    for knob in ("1", "0"):
        knobs(monkeypatch, knob, narrow)
        eng = SpfEngine(0)
        try:
            eng.load(rp, col, met, lid, ovl)
            plan = eng.plan(list(srcs))
            assert plan.kernels()[0] == "msbfs_kernel"
            assert narrow is None or plan.row_mode() == "sliced"
            assert class_rows(plan)[1] == (knob == "1") and quotient(eng)[2]
            res = eng.solve(list(srcs))
            assert np.array_equal(res.dist, exp), "distance mismatch"
            for i, s in enumerate(srcs):
                k = len(eng.neighbors(s))
                assert int(res.words[i]) == k
                assert np.array_equal(res.nh_matrix(i), mats[i][:k]), f"next hops of {names[s]}"
        finally:
            eng.close()


def test_quotient_in_use_on_fabric_2200():
    """Host only: the sweep wants at most half as many quotient edges as
    neighbour entries (use_quotient)."""
    topo = T.fabric(2200, full=True)
    assert topo.n_nodes == 2192
    ptr, ids = neighbour_lists(topo.n_nodes, topo.adj_src.tolist(), topo.adj_dst.tolist())
    cls, k = classes(ptr, ids)
    assert np.bincount(cls).max() == 48 and k < topo.n_nodes // 4  # the racks of a pod are twins
    edges = {(int(cls[v]), int(cls[u])) for v in range(topo.n_nodes) for u in ids[ptr[v]: ptr[v + 1]]}
    assert 2 * len(edges) <= len(ids)


@gpu
@pytest.mark.parametrize("align", [None, "64"], ids=["pitch3072", "pitch2240"])
@pytest.mark.parametrize("narrow", ["2", None], ids=["sliced", "u32"])
@pytest.mark.parametrize("state", list(DRAIN))
def test_fabric_2200_partial_plan(monkeypatch, state, narrow, align):
    g = fabric2200(state)
    both_paths(monkeypatch, g[1:], ("f2200", state), sources2200(), narrow, align)


@gpu
@pytest.mark.parametrize("count", [1, 7, 8, 9])
def test_mid_fabric_few_sources(monkeypatch, count):
    """Fewer rows than a group, a full group, one over (the closure adds the
    sources' neighbours: the u32 path keeps the rows to the sources)."""
    graph = graph_from_lsdb(mid_fabric().lsdb)
    srcs = [591, 0, 300, 17, 100, 590, 41, 299, 16][:count]
    for narrow in ("2", None):
        both_paths(monkeypatch, graph, ("mid",), srcs, narrow)


@gpu
def test_fabric_2200_narrow_rows_on_demand_and_in_pass(monkeypatch):
    """The Dn-only expansion (plan_ensure_narrow), then the in-pass one writing
    all three outputs: min(d, 254), 255 for unreachable and the padding."""
    from openr_amd.hiprt import DeviceArray, synchronize

    monkeypatch.delenv("SPF_PITCH_ALIGN", raising=False)
    knobs(monkeypatch, "1")
    names, rp, col, met, lid, ovl = fabric2200("drained")[1:]
    srcs = list(dict.fromkeys(sources2200()))
    exp, _ = oracle_rows(("f2200", "drained"), tuple(srcs))
    eng = SpfEngine(0)
    eng.load(rp, col, met, lid, ovl)
    n, pitch, ns = len(names), eng.pitch, len(srcs)
    plan = eng.plan(srcs)
    assert class_rows(plan)[1]
    dist = DeviceArray(ns * pitch, np.uint32)
    nh = DeviceArray(max(1, plan.nh_words), np.uint32)
    out = DeviceArray(ns * pitch, np.uint8)
    want = np.full((ns, pitch), 255, np.uint8)
    want[:, :n] = np.where(exp == U32_INF, 255, np.minimum(exp, 254)).astype(np.uint8)
    try:
        for _ in range(2):
            plan.execute(dist.ptr, nh.ptr)
            out.zero()
            plan.copy_narrow_rows(out.ptr)
            synchronize()
            assert np.array_equal(out.numpy().reshape(ns, pitch), want)
    finally:
        for a in (dist, nh, out):
            a.free()
        eng.close()
