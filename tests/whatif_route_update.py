"""Checker of what-if route updates (spf_whatif_route_update), in numpy.

The semantics restated from four inputs -- the base result, a failure's change
list, the source's CSR row and the failure's description.  A failure is a
tuple: ("link", l), ("down", x), ("drain", x), ("set", [links]) or
("metric", l, m_lo, m_hi) with 0 keeping a direction.  The route of a set
under the failure is the reference's selection over the patched result
(whatif_routes.routes); slot q of the row, with head x, is a next hop of it
iff it is live, survives the failure, x's bit is set in the route's words and
w'(q) == d'(x).  A record is q | min << 32; the update list of a failure holds
the sets whose record sequence differs from the base's.

Also here: the graphs of the tests (as LSDBs, so the CPU tests can put the
oracle beside the checker and the GPU tests load the same CSR), the failed
LSDB of any failure, and the oracle's link-level next hops as records.
"""

import numpy as np

import whatif_lists as L
import whatif_routes as R
from openr_amd import topology as T
from openr_amd.link_state import LinkState
from openr_amd.lsdb import PackedLsdb

U64_MAX = L.U64_MAX
KEEP = 0


class Row:
    """The source's CSR row: per slot the edge index, head, metric, link id and
    the head's neighbour bit (-1 for a dead slot, a self-loop)."""

    def __init__(self, rp, col, met, lid, s):
        self.s = int(s)
        self.q = np.arange(int(rp[s]), int(rp[s + 1]), dtype=np.int64)
        self.head = np.asarray(col, np.int64)[self.q]
        self.w = np.asarray(met, np.int64)[self.q]
        self.lid = np.asarray(lid, np.int64)[self.q]
        nbrs = L.neighbours(rp, col, s)
        bit = {v: j for j, v in enumerate(nbrs)}
        self.bit = np.array([bit.get(int(x), -1) if int(x) != self.s else -1 for x in self.head], np.int64)

    def weights(self, fail):
        """w' per slot under `fail` (None: no failure); 0 where the slot is dead
        or does not survive."""
        w = np.where(self.bit >= 0, self.w, 0)
        if fail is None or fail[0] == "drain":
            return w
        if fail[0] == "link":
            return np.where(self.lid == int(fail[1]), 0, w)
        if fail[0] == "down":
            return np.where(self.head == int(fail[1]), 0, w)
        if fail[0] == "set":
            return np.where(np.isin(self.lid, np.asarray(list(fail[1]), np.int64)), 0, w)
        if fail[0] == "metric":
            _, l, m_lo, m_hi = fail
            # the direction src -> x is the link's "lo" direction when src has the smaller id
            new = np.where(self.s < self.head, int(m_lo), int(m_hi))
            hit = (self.lid == int(l)) & (new != KEEP) & (self.bit >= 0)
            return np.where(hit, new, w)
        raise ValueError(fail)

    def touches(self, fail):
        return bool((self.weights(fail) != self.weights(None)).any())


def qualifying(row, fail, dist, metrics, words):
    """[n_sets, slots] bool: slot is a next hop of the set's route (metrics,
    words) on the result with node metrics `dist` under `fail`."""
    w = row.weights(fail)
    ok = (w > 0) & (dist[row.head].astype(np.uint64) == w.astype(np.uint64))
    bit = np.maximum(row.bit, 0)
    wanted = ((words[:, bit >> 5] >> (bit & 31).astype(np.uint32)) & 1).astype(bool)
    return wanted & ok[None, :] & (metrics != U64_MAX)[:, None]


def records_of(row, q_row, metric):
    return (row.q[q_row].astype(np.uint64) | (np.uint64(metric) << np.uint64(32))).astype(np.uint64)


def base_records(row, base_dist, base_nh, sets, base=None):
    bm, bw = base if base is not None else R.routes(base_dist, base_nh, sets, row.s)
    Q = qualifying(row, None, base_dist, bm, bw)
    return [records_of(row, Q[k], bm[k]) for k in range(len(bm))]


def expected(row, fail, base_dist, base_nh, node, dist, nh, sets, base=None):
    """The failure's update list: (set ids ascending, min metrics, [records])."""
    bm, bw = base if base is not None else R.routes(base_dist, base_nh, sets, row.s)
    d, n = L.patched(base_dist, base_nh, np.asarray(node, np.int64), dist, nh)
    m, w = R.routes(d, n, sets, row.s)
    Qb = qualifying(row, None, base_dist, bm, bw)
    Q = qualifying(row, fail, d, m, w)
    differs = (Q != Qb).any(axis=1) | (Q.any(axis=1) & (m != bm))
    ids = np.nonzero(differs)[0]
    return ids.astype(np.uint32), m[ids], [records_of(row, Q[k], m[k]) for k in ids]


def same_lists(got, want):
    (gi, gm, gr), (wi, wm, wr) = got, want
    return (np.array_equal(gi, wi) and np.array_equal(gm, wm) and len(gr) == len(wr)
            and all(np.array_equal(a, b) for a, b in zip(gr, wr)))


# ---- graphs ---------------------------------------------------------------------------


def topology(name, n, links, fwd, rev):
    """An LSDB of nodes n0 .. n<n-1> and `links` [(a, b)] (parallel links
    allowed) with per-direction metrics."""
    width = len(str(n - 1))
    nodes = [f"n{i:0{width}d}" for i in range(n)]
    links = np.asarray(links, np.int64)
    counter, ifs, oifs = {}, [], []
    for a, b in links.tolist():
        key = (min(a, b), max(a, b))
        c = counter.get(key, 0)
        counter[key] = c + 1
        ifs.append(f"{nodes[a]}/{nodes[b]}/{c}")
        oifs.append(f"{nodes[b]}/{nodes[a]}/{c}")
    src = np.concatenate([links[:, 0], links[:, 1]])
    dst = np.concatenate([links[:, 1], links[:, 0]])
    met = np.concatenate([np.asarray(fwd), np.asarray(rev)]).astype(np.int32)
    return T._build(name, nodes, src, dst, met, ifs=ifs + oifs, oifs=oifs + ifs)


class Graph:
    """A topology flattened: the CSR the engine loads, and the LinkState that
    names its links."""

    def __init__(self, topo):
        self.topo = topo
        self.ls = LinkState(device=-1)
        self.ls.updateAdjacencyDatabases(topo.lsdb)
        self.names, self.rp, self.col, self.met, self.lid, self.ovl = self.ls.flatten()
        assert list(self.names) == list(topo.nodes)

    def links_between(self, u, v):
        return [int(self.lid[e]) for e in range(int(self.rp[u]), int(self.rp[u + 1])) if self.col[e] == v]

    def up_links(self):
        rows = np.repeat(np.arange(len(self.rp) - 1), np.diff(self.rp))
        return sorted(set(int(l) for l in np.asarray(self.lid)[rows != self.col]))


def bundle_graph():
    """Seven nodes; the source n0 has two equal links (metric 1) and a heavier
    one (metric 3) to n1, and one link to n2.  n3 is behind both neighbours,
    n5 behind n1 only, n6 behind n2 only, n4 behind n3."""
    links = [(0, 1), (0, 1), (0, 1), (0, 2), (1, 3), (2, 3), (3, 4), (1, 5), (2, 6)]
    w = [1, 1, 3, 1, 1, 1, 1, 1, 1]
    return Graph(topology("bundle7", 7, links, w, w))


def wide_graph():
    """A source with 40 distinct neighbours (W = 2), four of them over bundles of
    two equal links -- the neighbours with bits 0, 17, 31 and 32 -- and a second
    ring of 40 nodes behind them, each behind two neighbours."""
    links, w = [], []
    for j in range(40):
        links.append((0, 1 + j))
        w.append(2)
        if j in (0, 17, 31, 32):
            links.append((0, 1 + j))
            w.append(2)
    for j in range(40):
        links += [(1 + j, 41 + j), (1 + (j + 1) % 40, 41 + j)]
        w += [1, 1 + j % 2]
    return Graph(topology("wide81", 81, links, w, w))


class Hub:
    """Where hub_graph put things: the source `hub`, its distinct neighbours
    `nbrs` in bit order (the first `n_lower` of them have smaller ids than the
    hub), the ring node behind nbrs[j] and nbrs[(j + 1) % k], and the two
    bundled neighbours, one on each side of the hub."""

    def __init__(self, hub, nbrs, n_lower, ring):
        self.hub, self.nbrs, self.n_lower, self.ring = hub, nbrs, n_lower, ring
        self.lower_bundle, self.upper_bundle = nbrs[n_lower - 1], nbrs[n_lower]


def hub_graph(slots, nbrs=None):
    """A source in the middle of the id range with exactly `slots` slots in its
    row: `nbrs` distinct neighbours (metric 2), half with smaller ids than the
    source and half with larger ones, and parallel links for the rest of the
    row -- a bundle of two equal members and a heavier one (metric 4) to the
    nearest neighbour on each side, then further equal members dealt out from
    the last neighbour downwards.  Behind the neighbours a ring of as many
    nodes, ring node j behind neighbours j (metric 1) and j + 1 (metric 1 or
    2), so every second one has ECMP across two neighbours; half of the ring
    has smaller ids than every neighbour, half larger ones.  Returns (Graph,
    Hub); graph.rp[hub] > 0."""
    k = max(4, slots - 4 - slots // 40) if nbrs is None else nbrs
    assert k >= 4 and slots >= k + 4
    a = k // 2
    hub = 2 * a
    nb = list(range(a, 2 * a)) + list(range(hub + 1, hub + 1 + k - a))
    ring = list(range(a)) + list(range(hub + 1 + k - a, 2 * k + 1))
    links, w = [], []
    for x in nb:
        links.append((hub, x))
        w.append(2)
    for x in (nb[a - 1], nb[a]):
        links += [(hub, x), (hub, x)]
        w += [2, 4]
    for e in range(slots - k - 4):
        links.append((hub, nb[k - 1 - e % k]))
        w.append(2)
    for j in range(k):
        links += [(nb[j], ring[j]), (nb[(j + 1) % k], ring[j])]
        w += [1, 1 + j % 2]
    g = Graph(topology(f"hub{slots}_{k}", 2 * k + 1, links, w, w))
    assert int(g.rp[hub + 1] - g.rp[hub]) == slots and int(g.rp[hub]) > 0
    return g, Hub(hub, nb, a, ring)


def hub_sets(g, h):
    """Every node alone (the source's own prefix among them), anycast sets over
    the ring and over the bundled neighbours on both sides, and an empty set."""
    return [[v] for v in range(len(g.names))] + [
        [h.ring[0], h.ring[2]], [h.nbrs[0], h.ring[-1]], [h.lower_bundle, h.upper_bundle],
        [h.ring[1], h.hub], []]


def hub_failures(g, h):
    """Of the small hub graph: every up link failed and re-weighed in either
    direction and in both, above and below its metric, and every other node
    down and drained."""
    w = {int(l): int(m) for l, m in zip(g.lid, g.met)}  # (the same in both directions)
    fails = []
    for l in g.up_links():
        fails.append(("link", l))
        for m in (1, 2, 3, 5):
            if m != w[l]:
                fails += [("metric", l, m, KEEP), ("metric", l, KEEP, m), ("metric", l, m, m)]
    fails += [(kind, x) for kind in ("down", "drain") for x in range(len(g.names)) if x != h.hub]
    return fails


def one_direction_moves(g, h, fails, lists):
    """The direction facts of a source that is the higher end of some of its
    links: of the one-direction metric changes on the source's own links, the
    one out of the source -- m_hi towards a neighbour of smaller id, m_lo
    towards a larger one -- changes some set's records for some link on either
    side, and the matching change of the direction into the source never does.
    `lists[i]` is the update list of fails[i]."""
    at = {f: i for i, f in enumerate(fails)}
    moved = {True: 0, False: 0}
    for e in range(int(g.rp[h.hub]), int(g.rp[h.hub + 1])):
        x, l = int(g.col[e]), int(g.lid[e])
        for f, i in at.items():
            if f[0] != "metric" or f[1] != l or (f[2] == KEEP) == (f[3] == KEEP):
                continue
            outward = (f[3] != KEEP) if x < h.hub else (f[2] != KEEP)
            if outward:
                moved[x < h.hub] += len(lists[i][0]) > 0
            else:
                assert len(lists[i][0]) == 0, (f, lists[i])
    assert moved[True] and moved[False], moved


def seeded_graph(n=200, n_links=420, seed=3):
    """A seeded multigraph, metrics 1 to 4 (the same in both directions, so
    ties abound), a quarter of the links doubled; the source n000 gets three
    bundles by construction."""
    rng = np.random.default_rng(seed)
    links = [(i, int(rng.integers(0, i))) for i in range(1, n)]  # connected
    while len(links) < n_links:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            links.append((a, b))
    w = [int(x) for x in rng.integers(1, 5, len(links))]
    for k in range(len(links)):
        if rng.random() < 0.25:
            links.append(links[k])
            w.append(w[k] if rng.random() < 0.6 else int(rng.integers(1, 5)))
    for x, extra in ((1, (0, 0)), (2, (0, 1)), (3, (1,))):  # bundles at the source: equal and heavier members
        base = next((wk for (a, b), wk in zip(links, w) if {a, b} == {0, x}), None)
        if base is None:
            links.append((0, x))
            w.append(1)
            base = 1
        for up in extra:
            links.append((0, x))
            w.append(base + up)
    return Graph(topology(f"multi{n}_{seed}", n, links, w, w))


# ---- the oracle on a failed LSDB --------------------------------------------------------


def failed_oracle(g, fail):
    """A fresh oracle LinkState of g's topology with `fail` applied."""
    import whatif_sets as WS
    import whatif_nodes as WN
    from oracle import OracleLinkState

    lsdb = g.topo.lsdb
    orc = OracleLinkState()
    if fail is None:
        orc.update_packed(lsdb)
        return orc
    if fail[0] in ("down", "drain"):
        return WN.failed_oracle(lsdb, g.names[int(fail[1])], fail[0])
    adj = WS.adjacency_records(lsdb)
    adjs = lsdb.adjs.copy()
    if fail[0] in ("link", "set"):
        for l in ([fail[1]] if fail[0] == "link" else fail[1]):
            lk = g.ls._link(int(l))
            adjs["is_overloaded"][adj[(lk._n1, lk._if1)]] = 1
    else:
        _, l, m_lo, m_hi = fail
        lk = g.ls._link(int(l))
        index = {n: i for i, n in enumerate(g.names)}
        ends = sorted([(index[lk._n1], adj[(lk._n1, lk._if1)]), (index[lk._n2], adj[(lk._n2, lk._if2)])])
        for (_, r), m in zip(ends, (m_lo, m_hi)):
            if m != KEEP:
                adjs["metric"][r] = m
    orc.update_packed(PackedLsdb(lsdb.blob, lsdb.dbs.copy(), adjs))
    return orc


def oracle_result(g, s, orc):
    return L.base_from_oracle(orc, g.names, g.rp, g.col, s)


def oracle_records(g, s, orc, members):
    """The oracle's link-level next hops of `s` towards the set `members`
    (getNextHopsThrift through orc_ls_nexthops_json) as records in slot order."""
    from oracle import nexthops

    slot = {}
    for q in range(int(g.rp[s]), int(g.rp[s + 1])):
        if int(g.col[q]) == s:
            continue
        lk = g.ls._link(int(g.lid[q]))
        slot[lk._if1 if lk._n1 == g.names[s] else lk._if2] = q
    r = nexthops(orc, g.names[s], [g.names[int(v)] for v in members])
    if r["min"] is None or not r["nh"]:
        return np.zeros(0, np.uint64)
    qs = sorted(slot[row[0]] for row in r["nh"])
    assert all(int(row[1]) == int(r["min"]) for row in r["nh"])
    return np.array([q | (int(r["min"]) << 32) for q in qs], np.uint64)
