"""Shared by the prefix-routes tests (spf_mplan_prefix_routes): seeded prefix
tables, the expectation restated over the oracle alone, and the expansion of a
node's records into the oracle's rows.  TEST INFRASTRUCTURE.

The expectation never touches the code under test: reachability comes from
OracleLinkState.spf(me), drained nodes from OracleLinkState.is_overloaded, the
next hops from oracle.nexthops (getNextHopsWithMetric + getNextHopsThrift) for
the selected set B; the selection itself (createRouteForPrefix,
Decision.cpp:390-554) is restated here in a dozen lines.
"""

import numpy as np

from oracle import nexthops
from openr_amd import _native as N
from openr_amd.link_state import PrefixTable

NONE, SELF, NO_NEXTHOP, MIN_NEXTHOP, ROUTE = range(5)


def make_table(prefixes):
    """[[(node id, path_preference, source_preference, distance, min_nexthop)]] -> PrefixTable."""
    ptr = np.zeros(len(prefixes) + 1, np.uint32)
    ptr[1:] = np.cumsum([len(p) for p in prefixes])
    flat = [e for p in prefixes for e in p]
    col = lambda k, dt: np.asarray([e[k] for e in flat], dt)  # noqa: E731
    return PrefixTable(ptr, col(0, np.uint32), col(1, np.int32), col(2, np.int32), col(3, np.int32),
                       col(4, np.int64))


def random_prefixes(n, rng, n_multi=60):
    """Every node's loopback (one entry, zero metrics, no min_nexthop), then
    n_multi prefixes of 2-5 advertisers with preferences and distances in {0,
    1, 2} and min_nexthop in {none, 1, 2, 3}."""
    out = [[(v, 0, 0, 0, 0)] for v in range(n)]
    for _ in range(n_multi):
        k = int(rng.integers(2, 6))
        out.append([(int(v), int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3)),
                     int(rng.integers(0, 4))) for v in rng.choice(n, k, replace=False)])
    return out


def select(prefix, me, reach, drained, all_best):
    """Steps 1-5 up to the walk: (B sorted, best, need) -- B empty: NONE.
    reach: the node ids with a path from me (me included); drained: a set."""
    r = [e for e in prefix if e[0] == me or e[0] in reach]
    if all_best:
        b0 = r
    else:
        key = lambda e: (e[1], e[2], -e[3])  # noqa: E731
        r = [e for e in r if key(e) >= (0, 0, 0)]
        top = max(map(key, r), default=None)
        b0 = [e for e in r if key(e) == top]
    if not b0:
        return [], N.SPF_UNREACHABLE, 0
    ids = sorted(e[0] for e in b0)
    best = me if (me in ids and not all_best) else ids[0]
    b = [e for e in b0 if e[0] not in drained] or b0
    need = max([e[4] for e in b if e[4] > 0], default=0)
    return sorted(e[0] for e in b), best, need


def expected(orc, names, prefixes, mes, lfa, all_best=False):
    """{(me id, p): (status, best, |B|, rows)} over the oracle alone; rows = the
    set of (ifName, metric, neighbour) of a ROUTE, else empty."""
    id_of = {s: i for i, s in enumerate(names)}
    drained = {i for i, s in enumerate(names) if orc.is_overloaded(s)}
    out = {}
    for me in mes:
        reach = {id_of[s] for s in orc.spf(names[me])} | {me}
        memo = {}
        for p, prefix in enumerate(prefixes):
            b, best, need = select(prefix, me, reach, drained, all_best)
            if not b:
                out[(me, p)] = (NONE, best, 0, set())
            elif me in b:
                out[(me, p)] = (SELF, best, len(b), set())
            else:
                key = tuple(b)
                if key not in memo:
                    memo[key] = {(r[0], r[1], r[2])
                                 for r in nexthops(orc, names[me], [names[v] for v in b], lfa)["nh"]}
                rows = memo[key]
                status = NO_NEXTHOP if not rows else MIN_NEXTHOP if need > len(rows) else ROUTE
                out[(me, p)] = (status, best, len(b), rows if status == ROUTE else set())
    return out


def unpack(info):
    """info words -> (status, best, |B|) lists."""
    info = np.asarray(info, np.uint64)
    return ((info >> np.uint64(56)).astype(np.int64).tolist(),
            (info & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist(),
            ((info >> np.uint64(32)) & np.uint64(0xFFFFFF)).astype(np.int64).tolist())


def rows_of(ls, flat, me_name, rec, cache):
    """One route's records -> {(ifName, metric, neighbour)}; they must be in
    me's link order, one per link.  cache: {CSR edge: (ifName, neighbour)}."""
    names, rp, col, _met, lid, _ovl = flat
    edges = (rec & np.uint64(0xFFFFFFFF)).astype(np.int64).tolist()
    assert edges == sorted(set(edges)), "records not in me's link order"
    out = set()
    for e, m in zip(edges, (rec >> np.uint64(32)).astype(np.int64).tolist()):
        if e not in cache:
            link = ls._link(int(lid[e]))
            assert rp[names.index(me_name)] <= e < rp[names.index(me_name) + 1], "not a link of me"
            assert names[int(col[e])] == link.getOtherNodeName(me_name)
            cache[e] = (link.getIfaceFromNode(me_name), names[int(col[e])])
        out.add((cache[e][0], m, cache[e][1]))
    assert len(out) == len(edges)
    return out


def got_db(ls, flat, mes):
    """{(me id, p): (status, best, |B|, rows)} of the last allSourcesPrefixRoutes,
    plus the records seen; every structural property of a database is asserted
    on the way."""
    names = flat[0]
    out, seen, cache = {}, 0, {}
    for t, me in enumerate(mes):
        info, ptr, rec = ls.allSourcesPrefixRouteDb(t)
        P = len(info)
        assert len(ptr) == P + 1 and ptr[0] == 0 and int(ptr[P]) == len(rec)
        cnt = np.diff(ptr.astype(np.int64))
        assert np.all(cnt >= 0)
        seen += len(rec)
        st, best, nb = unpack(info)
        for p in range(P):
            assert (cnt[p] > 0) == (st[p] == ROUTE), (me, p, st[p], cnt[p])  # only ROUTE has records
            rows = rows_of(ls, flat, names[me], rec[int(ptr[p]): int(ptr[p + 1])], cache) if cnt[p] else set()
            out[(int(me), p)] = (st[p], best[p], nb[p], rows)
    return out, seen
