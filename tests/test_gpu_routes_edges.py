"""The every-node route kernels (route_quads_kernel / route_sets_kernel,
csrc/routes.hip) and the label-route kernels (label_routes_kernel and its
u64 scan, csrc/label_routes.hip) at the edges the other modules do not reach:

* graphs patched in place after link flaps: dead slots (col[e] == tail,
  edge_nb[e] == kInf), rewritten edge_nb and re-indexed next-hop bitmaps;
* the scan's top level carrying across more than 256 tiles, cell counts on
  a tile boundary, one cell;
* metrics near the largest a resident pass admits (next-hop metrics past
  2^31, shortest + d(x, me) past 2^32);
* the plain-store fill (SPF_LABEL_NT=0);
* the 16-bit count of the materialised route database's headers.

Every expectation comes from the oracle (OracleLinkState, nexthops,
route_digests), compared for equality; every test asserts on the oracle's
side that its inputs reach the case it is for.
"""

import copy

import numpy as np
import pytest

from helpers import route_db_digest
from oracle import NameTable, OracleLinkState, nexthops, route_digests
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.engine import SpfEngine
from openr_amd.link_state import LinkState
from openr_amd.lsdb import pack_fast
from openr_amd.wire import unpack
from test_gpu_label_routes import expand, expected_from, hub_graph, label_candidates, member_pools
from test_gpu_routes_resident import sets_for

pytestmark = pytest.mark.gpu

U64 = np.iinfo(np.uint64).max


# ---- shared checks ----------------------------------------------------------------
def label_dbs(ls, lfa, mes):
    """allSourcesLabelRoutes(lfa, mes) and every me's (owner, ptr, rec), with
    the CSR invariants of each: ptr[0] == 0, ptr non-decreasing, ptr[G] ==
    len(rec), the lengths' sum == n_records."""
    labels, n_records, pool_bytes, ms = ls.allSourcesLabelRoutes(lfa, mes)
    assert ms >= 0
    G = len(labels)
    dbs = [ls.allSourcesLabelRouteDb(t) for t in range(len(mes))]
    seen = 0
    for owner, ptr, rec in dbs:
        assert len(owner) == G and len(ptr) == G + 1
        assert ptr[0] == 0 and np.all(np.diff(ptr.astype(np.int64)) >= 0)
        assert int(ptr[G]) == len(rec)
        seen += len(rec)
    assert seen == n_records
    return labels, n_records, pool_bytes, dbs


def assert_label_routes(ls, flat, me_names, labels, dbs, want):
    """Owners, next hops (interface, metric, neighbour, PHP / SWAP, swap
    label) and link order of the listed me equal the oracle's `want`
    (expected_from over exactly these me)."""
    got = {}
    for me, (owner, ptr, rec) in zip(me_names, dbs):
        for lab, val in expand(ls, flat, me, labels, owner, ptr, rec).items():
            got[(me, lab)] = val
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (bad[:3], [(got[k], want[k]) for k in bad[:1]])


def check_label_graph(lsdb, label_of, me_names, lfa, members=1):
    """One graph, the listed me (names; None: every node): the label routes
    against the oracle.  Returns (labels, n_records, pool_bytes, dbs, want)."""
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    me_names = sorted(label_of) if me_names is None else me_names
    want = expected_from(orc, label_of, me_names, lfa)
    with LinkState(devices=[0] * members) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        flat = ls.flatten()
        names = list(flat[0])
        assert names == sorted(label_of)
        mes = np.array([names.index(s) for s in me_names], np.uint32)
        labels, n_records, pool_bytes, dbs = label_dbs(ls, lfa, mes)
        assert labels.tolist() == list(label_candidates(label_of))
        assert_label_routes(ls, flat, me_names, labels, dbs, want)
    return labels, n_records, pool_bytes, dbs, want


# ---- A. patched graphs ------------------------------------------------------------
def rand_par_with_labels():
    """test_gpu_patch's rand_par with test_gpu_label_routes.graph_b's seeded
    labels: about 10 % zeros, five labels advertised by two nodes each."""
    topo = T.random_graph(40, 120, 17, max_metric=5, parallel_frac=0.35, overload_frac=0.1,
                          link_overload_frac=0.05)
    rng = np.random.default_rng(2024)
    n = len(topo.nodes)
    lab = 1000 + rng.permutation(n).astype(np.int32)
    lab[rng.random(n) < 0.1] = 0
    pick = rng.choice(np.nonzero(lab)[0], 10, replace=False)
    lab[pick[5:]] = lab[pick[:5]]
    topo.lsdb.dbs["node_label"] = lab
    return topo.lsdb


# the five publications, in order (nodes chosen on the oracle so that at
# least half of the (me, label) pairs keep a route after each, which
# expected_from asserts)
PAR_NODE, PAR_NBR = "0", "18"  # two parallel links 0 - 18
LONE_NODE = "36"               # 36 has one link per neighbour (the first, to n017, is withdrawn)
OVL_NODE = "9"                 # one adjacency of 9 (to n014) gets isOverloaded
DOWN_NODE = "n028"             # every link of n028 goes down


@pytest.mark.parametrize("members", [1, 3])
def test_route_and_label_kernels_on_patched_graphs(members):
    """After each of five publications that patch the engine's rows in place
    (no reload) -- one of two parallel links withdrawn (a dead slot, the
    neighbour set unchanged), a node's only link to a neighbour withdrawn
    (its neighbour list shrinks, its bitmaps re-index), an adjacency's
    overload bit, every link of a node down (a row of dead slots only), the
    first link advertised again -- a fresh resident pass gives, for every
    node as me, SP and LFA: allSourcesRouteDigests and the materialised
    route databases equal to the oracle's digests, and allSourcesLabelRoutes
    equal to the oracle's owners, next hops and link order."""
    lsdb = rand_par_with_labels()
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    dbs = {d.thisNodeName: d for d in unpack(lsdb)}
    names = sorted(dbs)
    label_of = {s: dbs[s].nodeLabel for s in names}
    cands = label_candidates(label_of)
    assert len(cands) < sum(1 for v in label_of.values() if v)  # shared labels
    assert label_of[DOWN_NODE] and len(cands[label_of[DOWN_NODE]]) == 1
    held = []

    def publish(step):
        if step == 0:
            db = dbs[PAR_NODE]
            idx = [i for i, a in enumerate(db.adjacencies) if a.otherNodeName == PAR_NBR]
            assert len(idx) == 2 and not any(db.adjacencies[i].isOverloaded for i in idx)
            held.append(db.adjacencies.pop(idx[0]))
        elif step == 1:
            db = dbs[LONE_NODE]
            nbrs = [a.otherNodeName for a in db.adjacencies]
            assert len(set(nbrs)) == len(nbrs) and not db.adjacencies[0].isOverloaded
            db.adjacencies.pop(0)
        elif step == 2:
            db = dbs[OVL_NODE]
            a = next(a for a in db.adjacencies if not a.isOverloaded)
            a.isOverloaded = True
        elif step == 3:
            db = dbs[DOWN_NODE]
            assert db.adjacencies
            for a in db.adjacencies:
                a.isOverloaded = True
        else:
            db = dbs[PAR_NODE]
            db.adjacencies.append(held.pop())
        orc.update([copy.deepcopy(db)])
        ls.updateAdjacencyDatabase(copy.deepcopy(db))
        return db.thisNodeName

    with LinkState(devices=[0] * members) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        assert list(ls.flatten()[0]) == names
        eng = SpfEngine(handle=ls.engine_handle())
        loads0 = eng.loads
        table = NameTable(names)
        every = np.arange(len(names), dtype=np.uint32)
        ptr, nodes = sets_for(len(names), np.random.default_rng(len(names)))
        for step in range(5):
            patches0 = int(N.lib.ls_debug_row_patches(ls._h))
            node = publish(step)
            ls.prefetchAllSources()
            flat = ls.flatten()
            assert list(flat[0]) == names
            # the publication patched rows in place: no reload
            assert eng.loads == loads0, step
            assert int(N.lib.ls_debug_row_patches(ls._h)) > patches0, step
            _names, rp, col, _met, lid, _ovl = flat
            me_id = names.index(node)
            row = col[int(rp[me_id]): int(rp[me_id + 1])]
            if step < 4:  # a dead slot in the row of a me that is checked
                assert np.any(row == me_id), (step, node)
            if step == 3:
                assert np.all(row == me_id)
            lh = ls.linkValueHashes()
            for lfa in (False, True):
                # route digests and materialised databases
                got, _ = ls.allSourcesRouteDigests(ptr, nodes, lfa)
                want = route_digests(orc, table, every, ptr, nodes, lfa)
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, (step, lfa, [names[i] for i in bad[:5]])
                assert np.count_nonzero(want) > len(names) // 2
                total, _ = ls.allSourcesRouteRecords(ptr, nodes, lfa)
                got = np.zeros(len(names), np.uint64)
                seen = 0
                for t in range(len(names)):
                    hdr, rec = ls.allSourcesRouteDb(t)
                    assert int((hdr >> np.uint64(32)).sum()) == len(rec)
                    seen += len(rec)
                    got[t] = route_db_digest(hdr, rec, lid, lh)
                assert seen == total
                want = route_digests(orc, table, every, ptr, nodes, lfa, kept_min=True)
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, (step, lfa, [names[i] for i in bad[:5]])
                # label routes (expected_from keeps the share of routed pairs)
                want_l = expected_from(orc, label_of, names, lfa)
                labels, _n, _b, ldbs = label_dbs(ls, lfa, every)
                assert labels.tolist() == list(cands)
                assert_label_routes(ls, flat, names, labels, ldbs, want_l)
                if step == 3:  # the isolated node: its own POP_AND_LOOKUP alone
                    mine = {k: v for k, v in want_l.items() if k[0] == DOWN_NODE}
                    assert mine == {(DOWN_NODE, label_of[DOWN_NODE]): (DOWN_NODE, set())}
                    owner = ldbs[me_id][0]
                    assert np.count_nonzero(owner != N.SPF_UNREACHABLE) == 1 and len(ldbs[me_id][2]) == 0


# ---- B. scan and grid shapes ------------------------------------------------------
@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_label_scan_carries_across_the_top_level(lfa):
    """Every node of fabric1000 as me on ONE member: 960 x 960 = 921,600 cells
    = 450 scan tiles, so scan_top_kernel takes a second round of 256 tiles
    and the carry reaches every me from slot 546 on (cell 524,288 lies in
    slot 546's run).  Also the only case with more than 32 me slots (a second
    XCD round of kLrGroup groups) together with more than one 256-label
    chunk (960 labels: 4 chunks).  All 960 me: the CSR invariants, the
    exact pool size, owner == me exactly at me's own label; 16 seeded me
    (slot 0, slot 546, 8 or more beyond it, the last) in full against the
    oracle -- a wrong base offset makes those me read other routes' records."""
    topo = T.fabric(1000, full=True)
    rank = {s: i for i, s in enumerate(sorted(topo.nodes))}
    lab = np.array([rank[s] + 1 for s in topo.nodes], np.int32)
    topo.lsdb.dbs["node_label"] = lab
    label_of = dict(zip(topo.nodes, lab.tolist()))
    n = len(label_of)
    assert n * n > 256 * 2048  # more cells than one round of the top level scans
    straddle = (256 * 2048) // n
    assert straddle * n < 256 * 2048 < (straddle + 1) * n and straddle == 546
    rng = np.random.default_rng(21)
    sample = sorted({0, straddle, n - 1}
                    | {int(x) for x in rng.choice(np.arange(straddle + 1, n - 1), 9, replace=False)}
                    | {int(x) for x in rng.choice(np.arange(1, straddle), 4, replace=False)})
    assert len(sample) == 16 and sum(1 for t in sample if t > straddle) >= 8
    orc = OracleLinkState()
    orc.update_packed(topo.lsdb)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(topo.lsdb)
        ls.prefetchAllSources()
        flat = ls.flatten()
        names = list(flat[0])
        assert names == sorted(label_of)
        every = np.arange(n, dtype=np.uint32)
        labels, n_records, pool_bytes, dbs = label_dbs(ls, lfa, every)
        pools = member_pools(N.lib.ls_all_sources_plan(ls._h), 1)
        G = len(labels)
        assert G == n and labels.tolist() == list(range(1, n + 1))
        assert pools == [(list(range(n)), n_records)]
        assert pool_bytes == 8 * n_records + 8 * (n * G + 1) + 4 * n * G
        owner = np.stack([d[0] for d in dbs])
        # label g + 1 is node g's: me owns exactly its own, every other label's
        # owner is its one advertiser (the fabric is connected)
        assert np.array_equal(owner, np.broadcast_to(np.arange(n, dtype=np.uint32), (n, n)))
        ptr = np.stack([d[1] for d in dbs]).astype(np.int64)
        cnt = np.diff(ptr, axis=1)
        assert np.all(cnt[np.eye(n, dtype=bool)] == 0) and np.all(cnt[~np.eye(n, dtype=bool)] > 0)
        me_names = [names[t] for t in sample]
        want = expected_from(orc, label_of, me_names, lfa)
        assert_label_routes(ls, flat, me_names, labels, [dbs[t] for t in sample], want)


@pytest.fixture(scope="module")
def hub255():
    """A hub with 255 leaves: 256 nodes, 256 labels, so k me are k x 256 cells."""
    lsdb, label_of, mes = hub_graph(255, n_me=8)
    assert len(label_of) == 256 and len(mes) == 9
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    return lsdb, label_of, mes, {lfa: expected_from(orc, label_of, mes, lfa) for lfa in (False, True)}


@pytest.mark.parametrize("n_me", [1, 8, 9])
@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_label_scan_tile_boundaries(hub255, n_me, lfa):
    """256, 2048 (exactly one scan tile) and 2304 cells on one member."""
    lsdb, label_of, mes, want = hub255
    me_names = mes[:n_me]
    want = {k: v for k, v in want[lfa].items() if k[0] in me_names}
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        flat = ls.flatten()
        names = list(flat[0])
        ids = np.array([names.index(s) for s in me_names], np.uint32)
        labels, n_records, pool_bytes, dbs = label_dbs(ls, lfa, ids)
        assert len(labels) * n_me == {1: 256, 8: 2048, 9: 2304}[n_me]
        assert pool_bytes == 8 * n_records + 8 * (n_me * 256 + 1) + 4 * n_me * 256
        assert_label_routes(ls, flat, me_names, labels, dbs, want)
    assert len(want) == n_me * 256  # every pair has a route


@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_label_routes_of_one_cell(lfa):
    """Two nodes, one label, one me: cells == 1 (one thread live, a scan of
    one entry), the route one record."""
    lsdb = pack_fast(["a", "b"], np.array([0, 1]), np.array([1, 0]), ["a/b/0", "b/a/0"],
                     ["b/a/0", "a/b/0"], np.array([3, 4], np.int32), node_label=np.array([77, 0], np.int32))
    label_of = {"a": 77, "b": 0}
    labels, n_records, pool_bytes, dbs, want = check_label_graph(lsdb, label_of, ["b"], lfa)
    assert labels.tolist() == [77] and n_records == 1 and pool_bytes == 8 + 16 + 4
    assert want == {("b", 77): ("a", {("b/a/0", 4, "a", "PHP", None)})}


# ---- C. large metrics in the label kernel -----------------------------------------
def wide_random():
    """test_route_sums_u32_and_u64_paths_agree's 2^26-metric graph, labelled."""
    topo = T.random_graph(50, 140, 9, max_metric=1 << 26, parallel_frac=0.2, overload_frac=0.1)
    lab = np.arange(1, len(topo.nodes) + 1, dtype=np.int32)
    topo.lsdb.dbs["node_label"] = lab
    return topo.lsdb, dict(zip(topo.nodes, lab.tolist()))


# The largest metric a 50-node graph may carry and still get a resident pass:
# max metric x N < 2^32 - 1 (needs64, graph_host.cpp metric_flags).
WIDE_N = 50
WIDE_M = (2**32 - 2) // WIDE_N


def chain(nodes, m, length, extra=()):
    """nodes[0] - nodes[1] - ... - nodes[length - 1] at metric m both ways, plus
    the extra (a, b) links."""
    pairs = [(i, i + 1) for i in range(length - 1)] + list(extra)
    src, dst, ifs, oifs = [], [], [], []
    for k, (a, b) in enumerate(pairs):
        for u, v in ((a, b), (b, a)):
            src.append(u)
            dst.append(v)
            ifs.append(f"{nodes[u]}/{nodes[v]}/{k}")
            oifs.append(f"{nodes[v]}/{nodes[u]}/{k}")
    lab = np.arange(1, len(nodes) + 1, dtype=np.int32)
    lsdb = pack_fast(nodes, np.asarray(src), np.asarray(dst), ifs, oifs,
                     np.full(len(src), m, np.int32), node_label=lab)
    return lsdb, dict(zip(nodes, lab.tolist()))


def wide_chain():
    """c00 - c01 - ... - c49 at WIDE_M per link: d(c00, c49) = 49 WIDE_M (past
    2^31), and shortest + d(c01, c00) = 50 WIDE_M = 2^32 - 46, the largest
    sum an admitted 50-node graph can show."""
    return chain([f"c{i:02d}" for i in range(WIDE_N)], WIDE_M, WIDE_N)


def wide_triangle():
    """c00 - ... - c48 and y joined to c00 and c01, all at WIDE_M: from c00 the
    link to y is a loop-free alternate only (d_y(c48) = 48 WIDE_M < 48 WIDE_M +
    WIDE_M), its metric WIDE_M + 48 WIDE_M -- a record past 2^31 that only
    the LFA branch (via = d_x(owner), over = w + via) produces."""
    nodes = [f"c{i:02d}" for i in range(WIDE_N - 1)] + ["y"]
    return chain(nodes, WIDE_M, WIDE_N - 1, extra=[(WIDE_N - 1, 0), (WIDE_N - 1, 1)])


WIDE = {"rand26": wide_random, "chain": wide_chain, "triangle": wide_triangle}


@pytest.mark.parametrize("key", sorted(WIDE))
@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_label_routes_with_large_metrics(key, lfa):
    """label_routes_kernel's own u64 arithmetic (shortest + back, w + via,
    over << 32) against the oracle, every node as me.

    rand26 is the 2^26-metric graph of test_route_sums_u32_and_u64_paths_agree.
    No seed of that generator reaches 2^31: 140 links over 50 nodes give
    paths of a few links, so distances stay below 2^30 (asserted below, so
    that the case is not mistaken for more than it is).  A metric past 2^31
    needs a path of nearly N - 1 links at nearly the largest admitted
    metric, which `chain` and `triangle` build: asserted on the oracle's
    rows, a next-hop metric >= 2^31 (in `triangle` under LFA on a next hop
    that is a loop-free alternate only).

    shortest + d(x, me) cannot pass 2^32 on a graph that gets a resident
    pass: shortest <= max metric x (N - 1), d(x, me) <= max metric for a
    neighbour x, and the pass needs max metric x N < 2^32 - 1.  (With the
    earlier bound, max metric x (N - 1), a 50-node chain reached 2^32 + 87
    million -- and showed the u32 SPF kernels wrapping, see
    test_a_graph_whose_relaxations_would_wrap_u32_takes_u64.)  `chain`
    asserts the largest sum there is, 50 WIDE_M = 2^32 - 46."""
    lsdb, label_of = WIDE[key]()
    _labels, _n, _b, _dbs, want = check_label_graph(lsdb, label_of, None, lfa)
    # (the oracle reports metrics as the reference's i32: >= 2^31 is negative)
    top = max((m + (1 << 32) if m < 0 else m) for _o, rows in want.values() for (_i, m, _x, _a, _s) in rows)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    names = sorted(label_of)
    dist, _mats = orc.dense(names, list(range(len(names))))
    d = {(a, b): int(dist[i, j]) for i, a in enumerate(names) for j, b in enumerate(names)
         if dist[i, j] != U64}
    # shortest + d(x, me) over the (me, owner, next-hop neighbour x) of the oracle's rows
    sums = max(d[(me, o)] + d[(x, me)] for (me, _lab), (o, rows) in want.items()
               for (_i, _m, x, _a, _s) in rows if (x, me) in d)
    if key == "rand26":
        assert top < 1 << 30 and sums < 1 << 31
        return
    assert 1 << 31 <= top < 1 << 32, top
    if key == "chain":
        assert top == (WIDE_N - 1) * WIDE_M and sums == WIDE_N * WIDE_M == (1 << 32) - 46
    if key == "triangle" and lfa:
        sp = expected_from(orc, label_of, ["c00"], False)
        far = ("c00", label_of["c48"])
        alt = set(want[far][1]) - set(sp[far][1])
        assert [(r[2], r[1] + (1 << 32)) for r in alt] == [("y", 49 * WIDE_M)] and 49 * WIDE_M >= 1 << 31


def test_a_graph_whose_relaxations_would_wrap_u32_takes_u64():
    """A 50-node chain at (2^32 - 2) // 49 per link: every distance fits u32
    (the far end is at 2^32 - 39) but the relaxation back from the far end,
    d + w = 2^32 + 87,652,354, does not -- in u32 it wrapped to a distance
    "shorter" than the true one of the 24 nodes before it.  Such a graph now
    counts as needing u64 distances (max metric x N >= 2^32 - 1): no
    resident pass, and getSpfResult (the exact kernel) equals the oracle."""
    from helpers import spf_canonical

    m = (2**32 - 2) // (WIDE_N - 1)
    assert m * (WIDE_N - 1) < 2**32 - 1 <= m * WIDE_N
    lsdb, _label_of = chain([f"c{i:02d}" for i in range(WIDE_N)], m, WIDE_N)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        assert SpfEngine(handle=ls.engine_handle()).needs_dist64
        assert not N.lib.ls_all_sources_plan(ls._h)
        with pytest.raises(RuntimeError):
            ls.allSourcesLabelRoutes(False)
        for me in ("c00", "c24", "c49"):
            want = orc.spf(me)
            assert spf_canonical(ls.getSpfResult(me)) == want, me
        assert want["c00"]["metric"] == 49 * m == 2**32 - 39


# ---- D. SPF_LABEL_NT=0 ------------------------------------------------------------
@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_label_fill_plain_stores_equal_streaming_stores(lfa, monkeypatch):
    """The fill pass with plain stores (SPF_LABEL_NT=0) writes the same arrays
    as with streaming stores (unset), and both equal the oracle's: the hub
    of graph C (320 links at the hub, 301 labels)."""
    lsdb, label_of, me_names = hub_graph(300)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    want = expected_from(orc, label_of, me_names, lfa)
    out = []
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        flat = ls.flatten()
        names = list(flat[0])
        ids = np.array([names.index(s) for s in me_names], np.uint32)
        for nt in (None, "0"):
            if nt is None:
                monkeypatch.delenv("SPF_LABEL_NT", raising=False)
            else:
                monkeypatch.setenv("SPF_LABEL_NT", nt)
            labels, n_records, pool_bytes, dbs = label_dbs(ls, lfa, ids)
            assert_label_routes(ls, flat, me_names, labels, dbs, want)
            out.append((labels, n_records, pool_bytes, dbs))
    (l0, n0, b0, d0), (l1, n1, b1, d1) = out
    assert np.array_equal(l0, l1) and n0 == n1 and b0 == b1
    for x, y in zip(d0, d1):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))


# ---- E. the 16-bit count of the route-database headers ----------------------------
PAR = 1 << 16


@pytest.fixture(scope="module")
def fat_pair():
    """a = b joined by 65,536 parallel links of metric 1, b - c by one link."""
    nodes = ["a", "b", "c"]
    k = np.arange(PAR)
    src = np.concatenate([np.zeros(PAR, np.int64), np.ones(PAR, np.int64), [1, 2]])
    dst = np.concatenate([np.ones(PAR, np.int64), np.zeros(PAR, np.int64), [2, 1]])
    ab = [f"a/b/{i}" for i in k]
    ba = [f"b/a/{i}" for i in k]
    ifs = ab + ba + ["b/c/0", "c/b/0"]
    oifs = ba + ab + ["c/b/0", "b/c/0"]
    lab = np.array([1, 2, 3], np.int32)
    lsdb = pack_fast(nodes, src, dst, ifs, oifs, np.ones(len(src), np.int32), node_label=lab)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    return lsdb, orc, nodes


def test_route_records_refuse_a_65536_slot_me(fat_pair):
    """A materialised route database's header holds its next-hop count in 16
    bits: a me whose row has 65,536 slots is refused (SPF_E_UNSUPPORTED, the
    node named) instead of being misread; a me with one link on the same
    graph gets the oracle's records."""
    lsdb, orc, nodes = fat_pair
    ptr = np.array([0, 1, 2, 3, 5], np.uint32)
    sets = np.array([0, 1, 2, 0, 1], np.uint32)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        names, rp, _col, _met, lid = ls.flatten()[:5]
        assert list(names) == nodes
        assert int(rp[1] - rp[0]) == PAR and int(rp[3] - rp[2]) == 1
        lh = ls.linkValueHashes()
        for lfa in (False, True):
            total, _ = ls.allSourcesRouteRecords(ptr, sets, lfa, mes=[2])
            hdr, rec = ls.allSourcesRouteDb(0)
            assert total == len(rec) == 3  # c: one next hop towards a, b and {a, b}
            got = route_db_digest(hdr, rec, lid, lh)
            want = route_digests(orc, NameTable(nodes), [2], ptr, sets, lfa, kept_min=True)
            assert got == int(want[0]) and got != 0
            for mes in ([0], [2, 0]):
                with pytest.raises(N.UnsupportedInput, match="node 0") as ei:
                    ls.allSourcesRouteRecords(ptr, sets, lfa, mes=mes)
                assert ei.value.status == N.SPF_E_UNSUPPORTED


@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_label_routes_keep_65536_next_hops(fat_pair, lfa):
    """The label path has 64-bit offsets and no packed count: a's route to b's
    label is 65,536 records, edge | 1 << 32 each, in link order -- the
    oracle's 65,536 next hops."""
    lsdb, orc, nodes = fat_pair
    rows = nexthops(orc, "a", ["b"], lfa, swap_label=2)["nh"]
    assert len(rows) == PAR and {(r[1], r[2], r[4], r[5]) for r in rows} == {(1, "b", "PHP", None)}
    want_if = sorted(r[0] for r in rows)
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        names, rp, col, _met, lid, _ovl = ls.flatten()
        labels, n_records, _bytes, dbs = label_dbs(ls, lfa, np.array([0], np.uint32))
        owner, ptr, rec = dbs[0]
        assert labels.tolist() == [1, 2, 3] and owner.tolist() == [0, 1, 2]
        assert ptr.tolist() == [0, 0, PAR, 2 * PAR] and n_records == 2 * PAR
        e0 = int(rp[0])
        edges = np.arange(e0, e0 + PAR, dtype=np.uint64)
        assert np.all(col[e0: e0 + PAR] == 1)
        far = nexthops(orc, "a", ["c"], lfa, swap_label=3)["nh"]
        assert len(far) == PAR and {(r[1], r[2], r[4], r[5]) for r in far} == {(2, "b", "SWAP", 3)}
        for g in (1, 2):  # towards b (PHP) and towards c through b (SWAP): metric 1 and 2
            assert np.array_equal(rec[g * PAR - PAR: g * PAR], edges | np.uint64(g << 32))
        got_if = sorted(ls._link(int(l)).getIfaceFromNode("a") for l in lid[e0: e0 + PAR].tolist())
        assert got_if == want_if
