"""Every node's unicast route decision from prefix entries, from a resident
all-sources pass (spf_mplan_prefix_routes, include/openr_spf.h): what
createRouteForPrefix (Decision.cpp:390-554) decides for every node -- the
advertisers it reaches, the best of them by PrefixMetrics, the drained filter,
no route to oneself, minNexthop -- with no SPF and no prefix walk per node.

The expectation comes from the oracle only (tests/prefix_routes.py): B, best
and the status are restated there over OracleLinkState.spf / is_overloaded,
the records come from oracle.nexthops for the set B.  A second, independent
check holds 8 seeded me against the Python restatement of SpfSolver
(native = False).

NO_NEXTHOP is the one status no consistent pass can produce: every member of
B has a finite distance from me, so the first link of a shortest path to the
nearest member is a next hop, and (without LFA) the cheapest parallel link to
that neighbour passes over == shortest.  The cases are asserted to hold the
other four on the oracle's side, and NO_NEXTHOP never, there and on the GPU.
"""

import ctypes as C
import functools
from collections import Counter

import numpy as np
import pytest

import prefix_routes as PR
from oracle import OracleLinkState
from openr_amd import _native as N
from openr_amd.link_state import LinkState
from openr_amd.spf_solver import PrefixEntry, PrefixMetrics, PrefixState, SpfSolver, prefixTable
from test_gpu_label_routes import graph_a
from test_gpu_routes_resident import GRAPHS as RESIDENT_GRAPHS

pytestmark = pytest.mark.gpu

# rand0, rand1, wan120 (overload fractions > 0 in the random ones) and a
# two-component graph (reachability changes B per me; b3 is drained)
MAKERS = {name: (lambda make=make: make().lsdb) for name, make in RESIDENT_GRAPHS[:3]}
MAKERS["twocomp"] = lambda: graph_a()[0]
SEEDS = {"rand0": 3, "rand1": 3, "wan120": 1, "twocomp": 2}


@functools.lru_cache(maxsize=None)
def case(name):
    """(lsdb, names in id order, prefixes, oracle): every node's loopback, ~60
    multi-advertiser prefixes with random metrics, and per drained node (three
    at the most) one prefix it advertises beside two undrained nodes at equal
    metrics."""
    from openr_amd.wire import unpack

    lsdb = MAKERS[name]()
    names = sorted(d.thisNodeName for d in unpack(lsdb))
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    rng = np.random.default_rng(SEEDS[name])
    prefixes = PR.random_prefixes(len(names), rng)
    drained = [i for i, s in enumerate(names) if orc.is_overloaded(s)]
    free = [i for i in range(len(names)) if i not in drained]
    for d in drained[:3]:
        reach = set(orc.spf(names[d]))
        peers = [v for v in free if names[v] in reach][:2]
        prefixes.append([(d, 1, 0, 0, 0)] + [(v, 1, 0, 0, 0) for v in peers])
    return lsdb, names, prefixes, orc


@functools.lru_cache(maxsize=None)
def want(name, lfa, all_best=False):
    """Computed once per (graph, lfa) and shared by the member counts."""
    _lsdb, names, prefixes, orc = case(name)
    return PR.expected(orc, names, prefixes, list(range(len(names))), lfa, all_best)


def member_pools(mp, n_members):
    """[(me slots, records)] of every member (spf_mplan_prefix_route_buffers)."""
    out = []
    for r in range(n_members):
        k, nrec = C.c_uint32(), C.c_uint64()
        pi, pp, pr = C.c_void_p(), C.c_void_p(), C.c_void_p()
        N.raise_for(N.lib.spf_mplan_prefix_route_buffers(C.c_void_p(mp), r, C.byref(pi), C.byref(pp),
                                                         C.byref(pr), C.byref(nrec), None, 0, C.byref(k)),
                    N.global_error())
        slots = np.zeros(max(1, k.value), np.uint32)
        N.raise_for(N.lib.spf_mplan_prefix_route_buffers(C.c_void_p(mp), r, None, None, None, None,
                                                         N.ptr(slots), k.value, None), N.global_error())
        assert bool(pi.value) == bool(k.value) == bool(pp.value) == bool(pr.value)
        out.append((slots[: k.value].tolist(), int(nrec.value)))
    return out


def other_dbs(ls, n):
    """A records database and a label database of the first ten me, read back."""
    return ([ls.allSourcesRouteDb(t) for t in range(min(n, 10))],
            [ls.allSourcesLabelRouteDb(t) for t in range(min(n, 10))])


def same_arrays(a, b):
    return all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


@pytest.mark.parametrize("name", sorted(MAKERS))
@pytest.mark.parametrize("members", [1, 2, 3])
@pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])
def test_prefix_routes_match_oracle(name, members, lfa):
    lsdb, names, prefixes, _orc = case(name)
    exp = want(name, lfa)
    table = PR.make_table(prefixes)
    n, P = len(names), len(prefixes)
    with LinkState(devices=[0] * members) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        flat = ls.flatten()
        assert list(flat[0]) == names
        # a records database and a label database made before the call ...
        ids = np.arange(n, dtype=np.uint32)
        ls.allSourcesRouteRecords(np.arange(n + 1, dtype=np.uint32), ids, lfa, compact=True)
        ls.allSourcesLabelRoutes(lfa)
        before = other_dbs(ls, n)
        calls = []
        for _ in range(2):
            n_records, pool_bytes, ms = ls.allSourcesPrefixRoutes(table, lfa)
            assert ms >= 0
            got, seen = PR.got_db(ls, flat, list(range(n)))
            assert seen == n_records  # n_records equals the sum of the counts
            calls.append((n_records, pool_bytes, got))
        pools = member_pools(N.lib.ls_all_sources_plan(ls._h), members)
        ms3 = (C.c_double * 3)()
        N.raise_for(N.lib.spf_mplan_prefix_routes_timing(C.c_void_p(N.lib.ls_all_sources_plan(ls._h)), ms3),
                    N.global_error())
        assert all(x >= 0 for x in ms3) and sum(ms3) > 0
        # ... read back identical after it
        after = other_dbs(ls, n)
    assert same_arrays(before[0], after[0]) and same_arrays(before[1], after[1])
    # the exactly sized pools: per member with a me, 8 records + 8 (n P + 1) + 8 n P
    assert sorted(t for slots, _ in pools for t in slots) == list(range(n))
    assert sum(r for _, r in pools) == n_records
    assert pool_bytes == sum(8 * r + 8 * (len(s) * P + 1) + 8 * len(s) * P for s, r in pools if s)
    # a second call gives identical output
    assert calls[0] == calls[1]
    # status, best, |B| and next hops equal the oracle's
    assert set(got) == set(exp)
    bad = [k for k in exp if got[k] != exp[k]]
    assert not bad, (len(bad), [(k, names[k[0]], prefixes[k[1]], got[k], exp[k]) for k in bad[:3]])


def test_cases_cover_every_status():
    """What the generated cases are for, checked on the oracle's expectation:
    NONE, SELF, MIN_NEXTHOP and ROUTE occur on every graph that can hold them,
    NO_NEXTHOP on none (module docstring), and a drained me that advertises
    beside undrained peers gets a route to them with best = me."""
    seen = Counter()
    drained_me_routes = 0
    for name in sorted(MAKERS):
        _lsdb, names, prefixes, orc = case(name)
        for lfa in (False, True):
            exp = want(name, lfa)
            here = Counter(v[0] for v in exp.values())
            seen.update(here)
            assert here[PR.SELF] and here[PR.MIN_NEXTHOP] and here[PR.ROUTE], (name, here)
            assert here[PR.NO_NEXTHOP] == 0
            hits = [k for k, v in exp.items() if v[0] == PR.ROUTE and v[1] == k[0]]
            assert all(orc.is_overloaded(names[me]) for me, _p in hits)
            if any(orc.is_overloaded(s) for s in names):
                assert hits, name
            drained_me_routes += len(hits)
    assert seen[PR.NONE] and drained_me_routes
    # reachability changes B per me: the same prefix, different sets
    exp = want("twocomp", False)
    P = len(case("twocomp")[2])
    assert any(len({(exp[(me, p)][0] == PR.NONE) for me in range(13)}) == 2 for p in range(P))


def prefix_state(names, prefixes):
    ps = PrefixState()
    name_of = []
    for p, prefix in enumerate(prefixes):
        name_of.append(f"fd00:{p:x}::/64")
        for v, pp, sp, dist, mn in prefix:
            ps.updatePrefix(names[v], "0", PrefixEntry(name_of[p], metrics=PrefixMetrics(pp, sp, dist),
                                                       minNexthop=mn if mn > 0 else None))
    return ps, name_of


@pytest.mark.parametrize("lfa,brs", [(False, True), (True, True), (False, False)],
                         ids=["sp", "lfa", "sp_allbest"])
def test_prefix_routes_equal_python_solver(lfa, brs):
    """8 seeded me of rand1 against the Python restatement of SpfSolver
    (native = False), best-route selection on (and once off, against
    allBest=True): the prefixes with a unicast route, each route's (ifName,
    metric, neighbour) set and its best node equal the ROUTE entries' records
    and info.  The table comes from spf_solver.prefixTable."""
    lsdb, names, prefixes, _orc = case("rand1")
    ps, name_of = prefix_state(names, prefixes)
    # prefixes the helper leaves to the host solver
    ps.updatePrefix(names[0], "0", PrefixEntry("fd09::/64", type="BGP"))
    ps.updatePrefix(names[1], "0", PrefixEntry("fd0a::/64", prependLabel=70001))
    ps.updatePrefix(names[2], "0", PrefixEntry("fd0b::/64", forwardingType="SR_MPLS"))
    ps.updatePrefix(names[3], "0", PrefixEntry("fd0c::/64", forwardingType="SR_MPLS",
                                               forwardingAlgorithm="KSP2_ED_ECMP"))
    table, left = prefixTable(ps, "0", names)
    assert sorted(left) == ["fd09::/64", "fd0a::/64", "fd0b::/64", "fd0c::/64"]
    assert table.prefixes == name_of
    other = PrefixState()  # (an entry in another area: its prefix is left too)
    other.updatePrefix(names[4], "1", PrefixEntry("fd0d::/64"))
    other.updatePrefix(names[5], "0", PrefixEntry("fd0d::/64"))
    empty, left1 = prefixTable(other, "0", names)
    assert left1 == ["fd0d::/64"] and empty.prefixes == [] and empty.pfx_ptr.tolist() == [0]
    mes = np.random.default_rng(8).choice(len(names), 8, replace=False).astype(np.uint32)
    with LinkState(devices=[0, 0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        ls.prefetchAllSources()
        flat = ls.flatten()
        ls.allSourcesPrefixRoutes(table, lfa, mes, allBest=not brs)
        got, _ = PR.got_db(ls, flat, [int(v) for v in mes])
        routes = 0
        for me in (int(v) for v in mes):
            sol = SpfSolver(names[me], False, lfa, enableBestRouteSelection=brs)
            sol.native = False
            db = sol.buildRouteDb(names[me], {"0": ls}, ps)
            cache = sol.getBestRoutesCache()
            mine = {name_of[p]: got[(me, p)] for p in range(len(name_of)) if got[(me, p)][0] == PR.ROUTE}
            theirs = {p: r for p, r in db.unicastRoutes.items() if p in set(name_of)}
            assert set(mine) == set(theirs), names[me]
            for p, r in theirs.items():
                assert {(h.ifName, h.metric, h.neighborNodeName) for h in r.nexthops} == mine[p][3], (names[me], p)
                assert cache[p].bestNodeArea[0] == names[mine[p][1]], (names[me], p)
            routes += len(mine)
    assert routes > 8 * len(names) // 2


def test_prefix_routes_need_a_resident_pass():
    lsdb, _names, prefixes, _orc = case("twocomp")
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(lsdb)
        with pytest.raises(RuntimeError):
            ls.allSourcesPrefixRoutes(PR.make_table(prefixes), False)
        with pytest.raises(RuntimeError):
            ls.allSourcesPrefixRouteDb(0)
