"""Every node's IP route database in an exactly sized pool
(spf_mplan_route_records with SPF_ROUTE_COMPACT, include/openr_spf.h;
LinkState.allSourcesRouteRecords(compact=True); routes.hip kRsCount / kRsFill).

* the databases equal the tiled layout's, header by header and record by
  record, and the oracle's digests (oracle/spf_oracle.cpp
  orc_ls_route_digests), on a random multigraph, a WAN and a fabric, members of
  1 and 3, SP and LFA;
* the device layout read through spf_mplan_route_record_buffers: stride 1,
  base + offset = the exclusive scan of the counts, a pool of exactly the
  records, and what spf_mplan_route_record_pool reports for either layout;
* the shapes at which the count / scan / fill passes take another path;
* snapshot, delta and update with a tiled or a compact database on either
  side give the lists and the payload two tiled ones give.
"""

import copy
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import route_db_digest
from oracle import NameTable, OracleLinkState, route_digests
from openr_amd import _native as N
from openr_amd import hiprt
from openr_amd import topology as T
from openr_amd.link_state import LinkState
from openr_amd.lsdb import pack_fast
from openr_amd.wire import unpack
from test_gpu_label_routes import hub_graph
from test_gpu_route_delta import single_sets
from test_gpu_routes_edges import DOWN_NODE, PAR_NBR, PAR_NODE, rand_par_with_labels, wide_chain
from test_gpu_routes_resident import GRAPHS, sets_for

pytestmark = pytest.mark.gpu

GRAPH = {g[0]: g[1] for g in GRAPHS}
LFA = pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
TILE = 1024  # sets per block of the four-sets-per-thread kernels (256 with SPF_ROUTE_SETS1)


# ---- reading the device arrays ----------------------------------------------------
def plan(ls):
    return C.c_void_p(N.lib.ls_all_sources_plan(ls._h))


def d2h(ptr, n):
    out = np.zeros(max(1, n), np.uint64)
    if n:
        hiprt._check(hiprt._lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), 8 * n, 2),
                     "hipMemcpy D2H")
    return out[:n]


def member_buffers(ls, members, n_sets):
    """Per member (slots, hdr [k * n_sets], base [k], records) through
    spf_mplan_route_record_buffers; the pool is copied by the caller, who knows
    how long it is in the layout at hand."""
    out = []
    for r in range(members):
        k, nrec = C.c_uint32(), C.c_uint64()
        ph, pb, pp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        N.raise_for(N.lib.spf_mplan_route_record_buffers(plan(ls), r, C.byref(ph), C.byref(pb), C.byref(pp),
                                                         C.byref(nrec), None, 0, C.byref(k)),
                    N.global_error())
        slots = np.zeros(max(1, k.value), np.uint32)
        N.raise_for(N.lib.spf_mplan_route_record_buffers(plan(ls), r, None, None, None, None, N.ptr(slots),
                                                         k.value, None), N.global_error())
        assert bool(ph.value) == bool(pb.value) == bool(pp.value) == bool(k.value)
        hiprt.synchronize()
        out.append((slots[: k.value].tolist(), d2h(ph.value, k.value * n_sets), d2h(pb.value, k.value),
                    int(nrec.value), pp.value))
    return out


def fields(hdr):
    return ((hdr & np.uint64(0xFFFFFFFF)).astype(np.int64), ((hdr >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64),
            (hdr >> np.uint64(48)).astype(np.int64))


def check_compact_layout(ls, members, n_sets, total, dbs):
    """The device arrays of a compact call: stride 1 everywhere, base[k] +
    offset over (k, p) = the exclusive cumsum of the counts, the pool exactly
    the records -- each me's slice of it its read-back database -- and the
    sizes spf_mplan_route_record_pool reports.  Returns the raw arrays."""
    raw, want_pool, seen = [], 0, 0
    for slots, hdr, base, nrec, ppool in member_buffers(ls, members, n_sets):
        if not slots:
            raw.append(None)
            continue
        off, cnt, stride = fields(hdr)
        assert np.all(stride == 1)
        start = np.repeat(base.astype(np.int64), n_sets) + off
        excl = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if len(cnt) else np.zeros(0, np.int64)
        assert np.array_equal(start, excl)
        assert int(cnt.sum()) == nrec
        pool = d2h(ppool, nrec)
        for k, t in enumerate(slots):
            h, rec = dbs[t]
            lo = int(base[k])
            assert np.array_equal(pool[lo: lo + len(rec)], rec), t
            assert np.array_equal((h >> np.uint64(32)).astype(np.int64), cnt[k * n_sets: (k + 1) * n_sets])
        want_pool += 8 * max(nrec, 1)
        seen += nrec
        raw.append((slots, hdr, base, pool))
    assert seen == total
    assert ls.allSourcesRouteRecordPool() == (1, want_pool, 8 * total)
    return raw


def check_tiled_pool(ls, members, n_sets, total, rp, mes, tile=TILE):
    """After a tiled call: layout 0, the pool ceil(n_sets / tile) * tile * deg(me)
    slots per me."""
    tiles = (n_sets + tile - 1) // tile * tile
    want = 0
    for slots, _hdr, _base, _nrec, _pp in member_buffers(ls, members, n_sets):
        if slots:
            want += 8 * max(1, sum(tiles * int(rp[mes[t] + 1] - rp[mes[t]]) for t in slots))
    assert ls.allSourcesRouteRecordPool() == (0, want, 8 * total)
    return want


def read_all(ls, n_me):
    return [ls.allSourcesRouteDb(t) for t in range(n_me)]


def assert_same(a, b):
    assert len(a) == len(b)
    for t, ((h0, r0), (h1, r1)) in enumerate(zip(a, b)):
        assert np.array_equal(h0, h1) and np.array_equal(r0, r1), t


def both_layouts(ls, members, ptr, nodes, lfa, mes=None, tile=TILE):
    """A compact call (its device layout checked) and a tiled call on the same
    inputs: the read-back databases are equal.  Returns (dbs, total, raw)."""
    n_sets = len(ptr) - 1
    rp = ls.flatten()[1]
    ids = list(range(len(rp) - 1)) if mes is None else [int(v) for v in mes]
    total, ms = ls.allSourcesRouteRecords(ptr, nodes, lfa, mes, compact=True)
    assert ms >= 0
    dbs = read_all(ls, len(ids))
    assert sum(len(r) for _h, r in dbs) == total
    raw = check_compact_layout(ls, members, n_sets, total, dbs)
    total_t, _ = ls.allSourcesRouteRecords(ptr, nodes, lfa, mes)
    assert total_t == total
    assert_same(dbs, read_all(ls, len(ids)))
    tiled_bytes = check_tiled_pool(ls, members, n_sets, total, rp, ids, tile)
    assert tiled_bytes >= 8 * max(total, 1)
    return dbs, total, raw


# ---- 1 / 2. equal to the tiled path and the oracle; size and layout ----------------
@functools.lru_cache(maxsize=None)
def oracle_digests(name, lfa):
    topo = GRAPH[name]()
    orc = OracleLinkState()
    orc.update_packed(topo.lsdb)
    names = sorted(topo.nodes)
    ptr, nodes = sets_for(len(names), np.random.default_rng(len(names)))
    return route_digests(orc, NameTable(names), np.arange(len(names)), ptr, nodes, lfa, kept_min=True)


@pytest.mark.parametrize("name", ["rand0", "wan120", "fabric1000"])
@pytest.mark.parametrize("members", [1, 3])
@LFA
def test_compact_equals_tiled_and_oracle(name, members, lfa):
    topo = GRAPH[name]()
    with LinkState(devices=[0] * members) as ls:
        ls.updateAdjacencyDatabases(topo.lsdb)
        ls.prefetchAllSources()
        names, _rp, _col, _met, lid = ls.flatten()[:5]
        names = list(names)
        assert names == sorted(topo.nodes)
        lh = ls.linkValueHashes()
        ptr, nodes = sets_for(len(names), np.random.default_rng(len(names)))
        dbs, total, raw = both_layouts(ls, members, ptr, nodes, lfa)
        got = np.array([route_db_digest(h, r, lid, lh) for h, r in dbs], np.uint64)
        # a second compact call (after the tiled one: the pool sized afresh)
        total2, _ = ls.allSourcesRouteRecords(ptr, nodes, lfa, compact=True)
        assert total2 == total
        raw2 = check_compact_layout(ls, members, len(ptr) - 1, total, dbs)
        for a, b in zip(raw, raw2):
            assert (a is None) == (b is None)
            if a is not None:
                assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    want = oracle_digests(name, lfa)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} nodes differ, first {[names[i] for i in bad[:5]]}"
    assert np.count_nonzero(want) > len(names) // 2 and total > 0


# ---- 3. shapes ----------------------------------------------------------------------
def repeated_sets(n, n_sets, rng):
    """n_sets sets over n nodes: single nodes in id order (runs of four aligned
    ones take the 16-byte path) with every seventh set an anycast one (its
    quad takes the per-set path)."""
    sets = []
    for i in range(n_sets):
        if i % 7 == 3:
            sets.append(sorted(int(x) for x in rng.choice(n, int(rng.integers(2, 5)), replace=False)))
        else:
            sets.append([i % n])
    ptr = np.zeros(n_sets + 1, np.uint32)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    return ptr, np.concatenate([np.asarray(s, np.uint32) for s in sets])


@pytest.mark.parametrize("n_sets", [1, 3, 1023, 1024, 1025, 2049])
@LFA
def test_set_counts_around_a_block(n_sets, lfa):
    """A partial quad, one set short of a block, an exact block, one set into
    a second block, a third block: 60 me, on two members."""
    topo = GRAPH["rand0"]()
    with LinkState(devices=[0, 0]) as ls:
        ls.updateAdjacencyDatabases(topo.lsdb)
        ls.prefetchAllSources()
        n = len(ls.flatten()[0])
        ptr, nodes = repeated_sets(n, n_sets, np.random.default_rng(n_sets))
        _dbs, total, _raw = both_layouts(ls, 2, ptr, nodes, lfa)
        assert total > 0


def test_sets1_kernel_and_unstaged_fill_give_the_same_arrays(monkeypatch):
    """One set per thread (SPF_ROUTE_SETS1=1: 256-set blocks, five of them for
    1,025 sets) and a fill that stages nothing (SPF_ROUTE_STAGE=0) write what
    the default kernels write."""
    topo = GRAPH["rand0"]()
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(topo.lsdb)
        ls.prefetchAllSources()
        n = len(ls.flatten()[0])
        ptr, nodes = repeated_sets(n, 1025, np.random.default_rng(5))
        for lfa in (False, True):
            dbs, total, raw = both_layouts(ls, 1, ptr, nodes, lfa)
            monkeypatch.setenv("SPF_ROUTE_SETS1", "1")
            dbs1, total1, raw1 = both_layouts(ls, 1, ptr, nodes, lfa, tile=256)
            monkeypatch.delenv("SPF_ROUTE_SETS1")
            monkeypatch.setenv("SPF_ROUTE_STAGE", "0")
            assert N.lib.spf_route_compact_stage() == 0
            dbs0, total0, raw0 = both_layouts(ls, 1, ptr, nodes, lfa)
            monkeypatch.delenv("SPF_ROUTE_STAGE")
            assert total == total1 == total0
            assert_same(dbs, dbs1)
            assert_same(dbs, dbs0)
            for other in (raw1, raw0):
                assert all(np.array_equal(x, y) for x, y in zip(raw[0][1:], other[0][1:]))


def isolated_graph():
    """a - b, and c with no link at all."""
    return pack_fast(["a", "b", "c"], np.array([0, 1]), np.array([1, 0]), ["a/b/0", "b/a/0"],
                     ["b/a/0", "a/b/0"], np.array([3, 4], np.int32))


@LFA
def test_me_without_links_and_an_empty_database(lfa):
    """A me with no link slot at all has an empty region between its
    neighbours'; a call whose every route is unreachable holds no record and
    a pool of one word."""
    ptr = np.array([0, 1, 2, 3, 5], np.uint32)
    sets = np.array([0, 1, 2, 0, 1], np.uint32)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(isolated_graph())
        ls.prefetchAllSources()
        rp = ls.flatten()[1]
        assert int(rp[3] - rp[2]) == 0
        dbs, total, raw = both_layouts(ls, 1, ptr, sets, lfa, mes=[0, 2, 1])
        la, lc, lb = (len(r) for _h, r in dbs)
        assert la > 0 and lb > 0 and lc == 0 and total == la + lb
        assert raw[0][2].tolist() == [0, la, la]  # c's region is empty, b's follows a's
        assert np.all(fields(raw[0][1])[0][4:8] == 0) and np.all(fields(raw[0][1])[1][4:8] == 0)
        # c alone towards a, b and a again: nothing reachable
        none = np.array([0, 1, 0], np.uint32)
        dbs, total, raw = both_layouts(ls, 1, ptr[:4], none, lfa, mes=[2])
        assert total == 0 and len(dbs[0][1]) == 0
        assert ls.allSourcesRouteRecords(ptr[:4], none, lfa, mes=[2], compact=True)[0] == 0
        assert ls.allSourcesRouteRecordPool() == (1, 8, 0)


@pytest.mark.parametrize("members", [1, 3])
def test_me_whose_links_are_all_dead_slots(members):
    """Every adjacency of one node overloaded by a publication that patches
    the rows in place: its row holds dead slots only, its count is 0 and its
    region empty, in both layouts and as the oracle has it."""
    lsdb = rand_par_with_labels()
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    dbs_in = {d.thisNodeName: d for d in unpack(lsdb)}
    names = sorted(dbs_in)
    with LinkState(devices=[0] * members) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        db = dbs_in[DOWN_NODE]
        for a in db.adjacencies:
            a.isOverloaded = True
        orc.update([copy.deepcopy(db)])
        ls.updateAdjacencyDatabase(copy.deepcopy(db))
        ls.prefetchAllSources()
        _names, rp, col, _met, lid = ls.flatten()[:5]
        me = names.index(DOWN_NODE)
        row = col[int(rp[me]): int(rp[me + 1])]
        assert len(row) and np.all(row == me)  # dead slots only
        lh = ls.linkValueHashes()
        ptr, nodes = sets_for(len(names), np.random.default_rng(len(names)))
        for lfa in (False, True):
            dbs, total, _raw = both_layouts(ls, members, ptr, nodes, lfa)
            assert len(dbs[me][1]) == 0 and total > 0
            got = np.array([route_db_digest(h, r, lid, lh) for h, r in dbs], np.uint64)
            want = route_digests(orc, NameTable(names), np.arange(len(names)), ptr, nodes, lfa, kept_min=True)
            assert np.array_equal(got, want)


@LFA
def test_hub_with_more_links_than_one_staging_pass(lfa):
    """The hub of a 300-leaf star has 320 link slots: two passes of the
    256-link staging; its routes and eight leaves' against the tiled layout and
    the oracle."""
    lsdb, label_of, me_names = hub_graph(300)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        names, rp, _col, _met, lid = ls.flatten()[:5]
        names = list(names)
        mes = np.array([names.index(s) for s in me_names], np.uint32)
        assert int(rp[mes[0] + 1] - rp[mes[0]]) == 320
        lh = ls.linkValueHashes()
        ptr, nodes = sets_for(len(names), np.random.default_rng(7))
        dbs, total, _raw = both_layouts(ls, 1, ptr, nodes, lfa, mes=mes)
        got = np.array([route_db_digest(h, r, lid, lh) for h, r in dbs], np.uint64)
    want = route_digests(orc, NameTable(names), mes, ptr, nodes, lfa, kept_min=True)
    assert np.array_equal(got, want) and total > 300


def test_a_span_longer_than_the_staging_is_stored_directly():
    """Two nodes joined by 64 parallel links, LFA, 1,024 copies of the set
    {b}: a's one block holds 1,024 x 64 = 65,536 records, more than a block
    stages, so the fill stores them as the walk finds them."""
    par, copies = 64, 1024
    src = np.concatenate([np.zeros(par, np.int64), np.ones(par, np.int64)])
    dst = 1 - src
    ifs = [f"a/b/{i}" for i in range(par)] + [f"b/a/{i}" for i in range(par)]
    oifs = ifs[par:] + ifs[:par]
    lsdb = pack_fast(["a", "b"], src, dst, ifs, oifs, np.ones(2 * par, np.int32))
    stage = int(N.lib.spf_route_compact_stage())
    assert 0 < stage < par * copies
    ptr = np.arange(copies + 1, dtype=np.uint32)
    nodes = np.ones(copies, np.uint32)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        rp = ls.flatten()[1]
        assert int(rp[1] - rp[0]) == par
        dbs, total, raw = both_layouts(ls, 1, ptr, nodes, True, mes=[0])
        assert total == par * copies  # one block's span, past the staging
        hdr, rec = dbs[0]
        assert np.all(hdr >> np.uint64(32) == par)
        edges = np.arange(int(rp[0]), int(rp[0]) + par, dtype=np.uint64) | np.uint64(1 << 32)
        assert np.array_equal(rec, np.tile(edges, copies))
        # both nodes: b's block (the same size) follows a's
        dbs, total, raw = both_layouts(ls, 1, ptr[:4], np.array([1, 0, 1], np.uint32), True)
        assert total == 3 * par and raw[0][2].tolist() == [0, 2 * par]


@LFA
def test_largest_admitted_metrics(lfa):
    """A next-hop metric past 2^32 - 1 sets the kernels' refusal flag in either
    layout, but no graph that gets a resident pass has one (max metric x N <
    2^32 - 1 bounds every w + via): the 50-node chain at the largest admitted
    metric, records up to 49 x that metric (past 2^31), is equal in both."""
    lsdb, _label_of = wide_chain()
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        n = len(ls.flatten()[0])
        ptr, nodes = single_sets(n)
        dbs, total, _raw = both_layouts(ls, 1, ptr, nodes, lfa)
        assert max(int(r.max() >> np.uint64(32)) for _h, r in dbs if len(r)) >= 1 << 31


def test_compact_refuses_a_65536_slot_me():
    """The count field is 16 bits in the compact headers too: a me with 65,536
    link slots is refused, the node named, before anything is launched."""
    par = 1 << 16
    src = np.concatenate([np.zeros(par, np.int64), np.ones(par, np.int64), [1, 2]])
    dst = np.concatenate([np.ones(par, np.int64), np.zeros(par, np.int64), [2, 1]])
    ab = [f"a/b/{i}" for i in range(par)]
    ba = [f"b/a/{i}" for i in range(par)]
    lsdb = pack_fast(["a", "b", "c"], src, dst, ab + ba + ["b/c/0", "c/b/0"], ba + ab + ["c/b/0", "b/c/0"],
                     np.ones(len(src), np.int32))
    ptr = np.array([0, 1, 2, 3, 5], np.uint32)
    sets = np.array([0, 1, 2, 0, 1], np.uint32)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        for lfa in (False, True):
            total, _ = ls.allSourcesRouteRecords(ptr, sets, lfa, mes=[2], compact=True)
            assert total == 3 and ls.allSourcesRouteRecordPool() == (1, 24, 24)
            for mes in ([0], [2, 0]):
                with pytest.raises(N.UnsupportedInput, match="node 0") as ei:
                    ls.allSourcesRouteRecords(ptr, sets, lfa, mes=mes, compact=True)
                assert ei.value.status == N.SPF_E_UNSUPPORTED


# ---- 4. snapshot, delta and update across layouts -----------------------------------
def raw_update(ls, members):
    """Per member the update's arrays as spf_mplan_route_update_read copies
    them: (counts, IP dptr / dset / uptr / urec, label dptr / dset / uowner /
    uptr / urec)."""
    mp, out = plan(ls), []
    for r in range(members):
        n = np.zeros(5, np.uint64)
        N.raise_for(N.lib.spf_mplan_route_update_read(mp, r, N.ptr(n, C.c_uint64), *([None] * 9)),
                    N.global_error())
        k, ei, ri, el, rl = (int(v) for v in n)
        dp = [np.zeros(k + 1, np.uint64) for _ in range(2)]
        ds = [np.zeros(max(1, e), np.uint32) for e in (ei, el)]
        up = [np.zeros(e + 1, np.uint64) for e in (ei, el)]
        ur = [np.zeros(max(1, c), np.uint64) for c in (ri, rl)]
        uo = np.zeros(max(1, el), np.uint32)
        if k:
            N.raise_for(N.lib.spf_mplan_route_update_read(
                mp, r, None, N.ptr(dp[0], C.c_uint64), N.ptr(ds[0]), N.ptr(up[0], C.c_uint64),
                N.ptr(ur[0], C.c_uint64), N.ptr(dp[1], C.c_uint64), N.ptr(ds[1]), N.ptr(uo),
                N.ptr(up[1], C.c_uint64), N.ptr(ur[1], C.c_uint64)), N.global_error())
        out.append([n.tolist(), dp[0].tolist(), ds[0][:ei].tolist(), up[0].tolist(), ur[0][:ri].tolist(),
                    dp[1].tolist(), ds[1][:el].tolist(), uo[:el].tolist(), up[1].tolist(), ur[1][:rl].tolist()])
    return out


def publications(dbs):
    """Three publications on rand_par, in order: a node's metrics changed (rows
    untouched), one of two parallel links withdrawn (a dead slot in the row),
    every link of a node down (deletes)."""
    def metric():  # every link of one node: each of its routes' next-hop metrics moves
        db = dbs[PAR_NODE]
        for a in db.adjacencies:
            a.metric += 1
        return db

    def withdraw():
        db = dbs[PAR_NODE]
        idx = [i for i, a in enumerate(db.adjacencies) if a.otherNodeName == PAR_NBR]
        assert len(idx) == 2
        db.adjacencies.pop(idx[0])
        return db

    def down():
        db = dbs[DOWN_NODE]
        for a in db.adjacencies:
            a.isOverloaded = True
        return db

    return [metric, withdraw, down]


def generations(members, lfa, old_compact, new_compact):
    """Per publication: the old generation materialised in one layout and
    snapshotted, the new one in the other, the delta and its payload."""
    lsdb = rand_par_with_labels()
    dbs = {d.thisNodeName: d for d in unpack(lsdb)}
    out, info = [], []
    with LinkState(devices=[0] * members) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        n = len(dbs)
        ptr, nodes = single_sets(n)
        for change in publications(dbs):
            ls.prefetchAllSources()
            ls.allSourcesRouteRecords(ptr, nodes, lfa, compact=old_compact)
            ls.allSourcesLabelRoutes(lfa)
            layout, pool_bytes, record_bytes = ls.allSourcesRouteRecordPool()
            assert layout == int(old_compact)
            if old_compact:
                assert pool_bytes == record_bytes
            used = sum(1 for m in member_buffers(ls, members, n) if m[0])
            snap = ls.allSourcesRouteSnapshot()
            info.append((snap.deviceBytes, pool_bytes, used))
            # the snapshot took the database, whatever its layout
            cnt = C.c_uint64()
            assert N.lib.spf_mplan_route_db(plan(ls), 0, None, None, 0, C.byref(cnt)) == N.SPF_E_STATE
            assert N.lib.spf_mplan_route_record_pool(plan(ls), None, None, None) == N.SPF_E_STATE
            ls.updateAdjacencyDatabase(copy.deepcopy(change()))
            ls.prefetchAllSources()
            ls.allSourcesRouteRecords(ptr, nodes, lfa, compact=new_compact)
            ls.allSourcesLabelRoutes(lfa)
            lists, dtot, _ms, payload, upd = ls.allSourcesRouteUpdate(snap)
            flat = [({v: r.tolist() for v, r in ip.items()}, {v: (o, r.tolist()) for v, (o, r) in lb.items()})
                    for ip, lb in payload]
            out.append((lists, dtot, flat, upd["totals"], raw_update(ls, members)))
            snap.close()
    return out, info


@functools.lru_cache(maxsize=None)
def tiled_generations(members, lfa):
    return generations(members, lfa, False, False)


@pytest.mark.parametrize("members", [1, 3])
@LFA
@pytest.mark.parametrize("old_compact,new_compact", [(False, True), (True, False), (True, True)],
                         ids=["tiled_compact", "compact_tiled", "compact_compact"])
def test_delta_and_update_across_layouts(members, lfa, old_compact, new_compact):
    want, want_info = tiled_generations(members, lfa)
    got, info = generations(members, lfa, old_compact, new_compact)
    assert len(got) == len(want) == 3
    for step, (g, w) in enumerate(zip(got, want)):
        for what, a, b in zip(("lists", "delta totals", "payload", "update totals", "arrays"), g, w):
            assert a == b, (step, what)
    # the publications reach what they are for: updates of both kinds, then
    # deletes of both kinds (the withdrawn parallel link changes routes only
    # where it was a next hop: with LFA)
    assert want[0][1][0] > 0 and want[0][1][2] > 0 and want[2][1][1] > 0 and want[2][1][3] > 0
    if lfa:
        assert want[1][1][0] > 0
    if old_compact:
        # a compact snapshot holds the exact pool (and one more header word per
        # member, the scan's total) where the tiled one holds the tiles
        for (b_c, pool_c, used), (b_t, pool_t, used_t) in zip(info, want_info):
            assert used == used_t and pool_c < pool_t
            assert b_t - b_c == (pool_t - pool_c) - 8 * used
