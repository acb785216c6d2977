"""The prefix-routes kernels (openr_amd/csrc/prefix_routes.hip) and their plan
stage at the smallest shapes at which they can go wrong: the block's thread
count and the scan's tile on either side, a me with one more link than the
LDS staging chunk (dead slots and parallel links among them), prefixes of
every node / of no node / no prefixes at all, advertisers half the nodes
cannot reach, min_nexthop at the count and one past it, and the refusals.
Expectations come from the oracle (tests/prefix_routes.py)."""

import copy
import ctypes as C
import functools

import numpy as np
import pytest

import prefix_routes as PR
from oracle import OracleLinkState, nexthops
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.link_state import LinkState
from openr_amd.lsdb import pack_fast
from openr_amd.wire import unpack
from test_gpu_label_routes import graph_a

pytestmark = pytest.mark.gpu

THREADS = int(N.lib.spf_prefix_routes_threads())
LINKS = int(N.lib.spf_prefix_routes_links())
TILE = int(N.lib.spf_prefix_routes_scan_tile())


@functools.lru_cache(maxsize=None)
def rand1():
    topo = T.random_graph(45, 90, 7, max_metric=3, parallel_frac=0.1, overload_frac=0.2)
    orc = OracleLinkState()
    orc.update_packed(topo.lsdb)
    return topo.lsdb, sorted(topo.nodes), orc


def prefixes_of(n, P, seed):
    """P prefixes: the loopbacks first (all of them when P allows), the rest
    multi-advertiser."""
    rng = np.random.default_rng(seed)
    return PR.random_prefixes(n, rng, n_multi=max(P - n, 0))[:P]


def check(ls, lsdb_names, orc, prefixes, mes, lfa, all_best=False):
    """One call over `mes` (ids, any order) against the oracle; returns the
    expectation."""
    flat = ls.flatten()
    assert list(flat[0]) == lsdb_names
    n_records, _bytes, _ms = ls.allSourcesPrefixRoutes(PR.make_table(prefixes), lfa,
                                                       np.asarray(mes, np.uint32), allBest=all_best)
    got, seen = PR.got_db(ls, flat, [int(v) for v in mes])
    assert seen == n_records
    exp = PR.expected(orc, lsdb_names, prefixes, [int(v) for v in mes], lfa, all_best)
    assert set(got) == set(exp)
    bad = [k for k in exp if got[k] != exp[k]]
    assert not bad, (len(bad), [(k, prefixes[k[1]], got[k], exp[k]) for k in bad[:3]])
    return exp


def test_constants_are_the_units():
    assert THREADS == 256 and LINKS == 256 and TILE == 2048


@pytest.mark.parametrize("P", [THREADS - 1, THREADS, THREADS + 1])
@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_prefix_count_at_the_block_size(P, lfa):
    """One block short of full, full, and a second block of one thread."""
    lsdb, names, orc = rand1()
    mes = np.random.default_rng(P).permutation(len(names))[:6]
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        exp = check(ls, names, orc, prefixes_of(len(names), P, P), mes, lfa)
    assert {v[0] for v in exp.values()} >= {PR.SELF, PR.MIN_NEXTHOP, PR.ROUTE}


@pytest.mark.parametrize("n_me,P", [(23, 89), (32, 64), (3, 683)],
                         ids=["tile-1", "tile", "tile+1"])
def test_cells_at_the_scan_tile(n_me, P):
    """n_me x P = the scan tile - 1, the tile, the tile + 1 on one member
    (members = 2 splits them: both partial tiles), mes a seeded unsorted
    subset."""
    assert n_me * P == TILE + {"23x89": -1, "32x64": 0, "3x683": 1}[f"{n_me}x{P}"]
    lsdb, names, orc = rand1()
    mes = np.random.default_rng(n_me).permutation(len(names))[:n_me]
    assert list(mes) != sorted(mes)
    for members in (1, 2):
        with LinkState(devices=[0] * members) as ls:
            ls.updateAdjacencyDatabases(lsdb)
            ls.prefetchAllSources()
            check(ls, names, orc, prefixes_of(len(names), P, 5), mes, True)


def hub_lsdb():
    """A hub with LINKS - 6 leaves and a second, parallel link to 7 of them (4
    at the same metric, 3 at a larger one): LINKS + 1 links at the hub, one
    more than the staging chunk; a ring over the first 12 leaves gives the
    leaves alternates."""
    leaves = LINKS - 6
    nodes = ["hub"] + [f"l{i:03d}" for i in range(leaves)]
    src, dst, met, ifs, oifs = [], [], [], [], []

    def link(a, b, k, m):
        for u, v in ((a, b), (b, a)):
            src.append(u)
            dst.append(v)
            met.append(m)
            ifs.append(f"{nodes[u]}/{nodes[v]}/{k}")
            oifs.append(f"{nodes[v]}/{nodes[u]}/{k}")

    for i in range(1, leaves + 1):
        link(0, i, 0, 1)
        if i <= 7:
            link(0, i, 1, 1 if i <= 4 else 2)
    for i in range(1, 13):
        link(i, i % 12 + 1, 0, 1)
    return pack_fast(nodes, np.asarray(src), np.asarray(dst), ifs, oifs, np.asarray(met, np.int32))


@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_hub_with_one_more_link_than_the_staging_chunk(lfa):
    """The hub as me walks its links in two staged chunks (LINKS and 1);
    after one of two parallel links is withdrawn its row keeps a dead slot."""
    lsdb = hub_lsdb()
    dbs = {d.thisNodeName: d for d in unpack(lsdb)}
    names = sorted(dbs)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    hub = names.index("hub")
    n = len(names)
    prefixes = prefixes_of(n, n + 24, 3)
    mes = [hub] + [int(v) for v in np.random.default_rng(4).choice(n, 5, replace=False) if v != hub]
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        rp = ls.flatten()[1]
        assert int(rp[hub + 1] - rp[hub]) == LINKS + 1
        check(ls, names, orc, prefixes, mes, lfa)
        # a link-down row patch: one of the two hub - l002 links withdrawn
        db = dbs["hub"]
        idx = [i for i, a in enumerate(db.adjacencies) if a.otherNodeName == "l002"]
        assert len(idx) == 2
        db.adjacencies.pop(idx[0])
        patches0 = int(N.lib.ls_debug_row_patches(ls._h))
        orc.update([copy.deepcopy(db)])
        ls.updateAdjacencyDatabase(copy.deepcopy(db))
        ls.prefetchAllSources()
        assert int(N.lib.ls_debug_row_patches(ls._h)) > patches0
        _names, rp, col = ls.flatten()[:3]
        row = col[int(rp[hub]): int(rp[hub + 1])]
        assert len(row) == LINKS + 1 and np.count_nonzero(row == hub) == 1  # the dead slot
        check(ls, names, orc, prefixes, mes, lfa)


@pytest.mark.parametrize("all_best", [False, True], ids=["best", "allbest"])
def test_prefix_of_every_node_of_no_node_and_no_prefixes(all_best):
    lsdb, names, orc = rand1()
    n = len(names)
    rng = np.random.default_rng(6)
    everyone = [(v, int(rng.integers(0, 2)), 0, int(rng.integers(0, 2)), int(rng.integers(0, 3)))
                for v in range(n)]
    prefixes = [everyone, [], [(3, 0, 0, 0, 0)], []]
    with LinkState(devices=[0, 0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        exp = check(ls, names, orc, prefixes, list(range(n)), False, all_best)
        assert all(exp[(me, 1)][0] == PR.NONE and exp[(me, 3)][0] == PR.NONE for me in range(n))
        assert PR.SELF in {exp[(me, 0)][0] for me in range(n)}
        assert {exp[(me, 0)][0] for me in range(n)} & {PR.ROUTE, PR.MIN_NEXTHOP}
        # a table without prefixes: a database of nothing
        n_records, nbytes, _ms = ls.allSourcesPrefixRoutes(PR.make_table([]), False)
        assert n_records == 0 and nbytes == 2 * 8  # two members with a me: their totals
        info, ptr, rec = ls.allSourcesPrefixRouteDb(n - 1)
        assert len(info) == 0 and ptr.tolist() == [0] and len(rec) == 0
        # ... and no me
        assert ls.allSourcesPrefixRoutes(PR.make_table(prefixes), False, np.zeros(0, np.uint32))[0] == 0


@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_advertisers_half_the_nodes_cannot_reach(lfa):
    """graph_a's b* component advertises; a1, a2, c1, c2 reach none of it."""
    lsdb = graph_a()[0]
    names = sorted(d.thisNodeName for d in unpack(lsdb))
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    b = [i for i, s in enumerate(names) if s.startswith("b")]
    prefixes = [[(b[0], 0, 0, 0, 0), (b[4], 0, 0, 0, 0)], [(b[2], 2, 0, 0, 1)],
                [(v, 0, 1, 0, 0) for v in b], [(names.index("a1"), 0, 0, 0, 0), (b[6], 0, 0, 0, 0)]]
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        exp = check(ls, names, orc, prefixes, list(range(len(names))), lfa)
    for me, s in enumerate(names):
        assert (exp[(me, 0)][0] == PR.NONE) == (not s.startswith("b")), s
        assert exp[(me, 3)][0] != PR.NONE  # either component has one of its advertisers


def test_min_nexthop_at_the_count_and_one_past_it():
    lsdb, names, orc = rand1()
    # a (me, advertiser) pair with at least two next hops, found on the oracle
    me, d, c = next((me, d, len(r)) for me in range(len(names)) for d in range(len(names)) if me != d
                    for r in [nexthops(orc, names[me], [names[d]], False)["nh"]] if len(r) >= 2)
    prefixes = [[(d, 0, 0, 0, c)], [(d, 0, 0, 0, c + 1)], [(d, 0, 0, 0, c - 1)], [(d, 0, 0, 0, 1 << 40)]]
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        exp = check(ls, names, orc, prefixes, [me], False)
    assert [exp[(me, p)][0] for p in range(4)] == [PR.ROUTE, PR.MIN_NEXTHOP, PR.ROUTE, PR.MIN_NEXTHOP]
    assert len(exp[(me, 0)][3]) == c


def no_prefix_db(ls):
    """The plan holds no prefix database: the reader refuses, no member holds a share."""
    mp = C.c_void_p(N.lib.ls_all_sources_plan(ls._h))
    n = C.c_uint64()
    assert N.lib.spf_mplan_prefix_route_db(mp, 0, None, None, None, 0, C.byref(n)) == N.SPF_E_INVALID
    k = C.c_uint32(7)
    pi = C.c_void_p(1)
    assert N.lib.spf_mplan_prefix_route_buffers(mp, 0, C.byref(pi), None, None, None, None, 0,
                                                C.byref(k)) == N.SPF_OK
    assert k.value == 0 and not pi.value
    ms3 = (C.c_double * 3)()
    assert N.lib.spf_mplan_prefix_routes_timing(mp, ms3) == N.SPF_E_STATE
    with pytest.raises(RuntimeError):
        ls.allSourcesPrefixRouteDb(0)
    return True


def test_refusals_leave_no_prefix_database_and_the_others_intact():
    lsdb, names, orc = rand1()
    n = len(names)
    good = prefixes_of(n, n + 10, 1)
    bad = {
        "pfx_ptr decreases": lambda t: t.pfx_ptr.__setitem__(5, 3),
        "pfx_ptr does not start at 0": lambda t: t.pfx_ptr.__setitem__(0, 1),
        "out of range": lambda t: t.node.__setitem__(7, n),
        "twice": lambda t: t.node.__setitem__(int(t.pfx_ptr[n]) + 1, t.node[int(t.pfx_ptr[n])]),
        "INT32_MIN": lambda t: t.distance.__setitem__(2, -(1 << 31)),
    }
    with LinkState(devices=[0, 0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        ids = np.arange(n, dtype=np.uint32)
        ls.allSourcesRouteRecords(np.arange(n + 1, dtype=np.uint32), ids, False, compact=True)
        ls.allSourcesLabelRoutes(False)
        before = [ls.allSourcesRouteDb(t) for t in range(n)], [ls.allSourcesLabelRouteDb(t) for t in range(n)]
        for what, spoil in bad.items():
            ls.allSourcesPrefixRoutes(PR.make_table(good), False)  # a database to lose
            ls.allSourcesPrefixRouteDb(0)
            table = PR.make_table(good)
            spoil(table)
            with pytest.raises(N.SpfError) as ei:
                ls.allSourcesPrefixRoutes(table, False)
            assert ei.value.status == N.SPF_E_INVALID, what
            assert what in str(ei.value) and "prefix " in str(ei.value), (what, str(ei.value))
            assert no_prefix_db(ls)
        after = [ls.allSourcesRouteDb(t) for t in range(n)], [ls.allSourcesLabelRouteDb(t) for t in range(n)]
        for x, y in zip(before, after):
            assert all(np.array_equal(p, q) for a, b in zip(x, y) for p, q in zip(a, b))
        # the next good call works
        check(ls, names, orc, good, [0, 1, 2], False)
    with LinkState(devices=[0]) as ls:  # a hop-count plan
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources(useLinkMetric=False)
        with pytest.raises(N.UnsupportedInput) as ei:
            ls.allSourcesPrefixRoutes(PR.make_table(good), False)
        assert ei.value.status == N.SPF_E_UNSUPPORTED
        assert no_prefix_db(ls)
