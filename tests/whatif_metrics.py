"""Expected values of link-metric what-if batches
(spf_whatif_plan_create_metrics), in numpy beside whatif_sets.py, and a numpy
restatement of the device's classify rule and slack-bounded growth of D.

The pin for a change (link, m_lo, m_hi) is a full oracle re-run on a changed
LSDB, from a fresh OracleLinkState each time: a copy of the packed LSDB whose
two adjacency records of that link carry the new metrics -- m_lo in the record
of the endpoint with the smaller CSR id, m_hi in the other's, 0 leaving a
record as it is.  ``orc.spf(names[src])`` is rendered with
whatif_lists.base_from_oracle over the unchanged CSR and reduced with
whatif_nodes.digest_of.

The restatement (classify / grow) reads the base render and the CSR only:
  * a direction a -> b whose weight goes from w to w' is hot when a is reached
    and expanded (not drained unless it is the source) and either w' > w with
    dist[a] + w == dist[b], or w' < w with dist[a] + w' <= dist[b]; delta is 0
    for a raise and dist[b] - dist[a] - w' for a lower;
  * D grows from b over edges x -> c (x expanded) with
    dist[x] + w(x, c) <= dist[c] + delta under the new weights, c reached and
    not the source.
"""

import numpy as np

import whatif_lists as L
import whatif_nodes as WN
import whatif_sets as WS
from oracle import OracleLinkState
from openr_amd.lsdb import PackedLsdb

KEEP = 0


class Expected(WS.Expected):
    """whatif_sets.Expected plus the expected result of any metric change."""

    def __init__(self, lsdb, ls, names, rp, col, s: int) -> None:
        super().__init__(lsdb, ls, names, rp, col, s)
        self._index = {n: i for i, n in enumerate(names)}
        self._metric_memo = {}

    def sides(self, link: int):
        """[(csr id, adjacency record)] of the link's two ends, smaller id first."""
        lk = self.ls._link(int(link))
        ends = [(self._index[lk._n1], self._adj[(lk._n1, lk._if1)]),
                (self._index[lk._n2], self._adj[(lk._n2, lk._if2)])]
        return sorted(ends)

    def current(self, link: int):
        """(metric lo -> hi, metric hi -> lo) as advertised."""
        (_, r_lo), (_, r_hi) = self.sides(link)
        return int(self.lsdb.adjs["metric"][r_lo]), int(self.lsdb.adjs["metric"][r_hi])

    def resolved(self, link: int, m_lo: int, m_hi: int):
        w_lo, w_hi = self.current(link)
        return (int(m_lo) if m_lo != KEEP else w_lo, int(m_hi) if m_hi != KEEP else w_hi)

    def metric_result(self, link: int, m_lo: int, m_hi: int):
        new = self.resolved(link, m_lo, m_hi)
        if new == self.current(link):
            return self.base  # the LSDB is the unchanged one
        key = (int(link),) + new
        if key not in self._metric_memo:
            (_, r_lo), (_, r_hi) = self.sides(link)
            adjs = self.lsdb.adjs.copy()
            adjs["metric"][r_lo], adjs["metric"][r_hi] = new
            orc = OracleLinkState()
            orc.update_packed(PackedLsdb(self.lsdb.blob, self.lsdb.dbs.copy(), adjs))
            self._metric_memo[key] = L.base_from_oracle(orc, self.names, self.rp, self.col, self.s)
        return self._metric_memo[key]

    def metric_digest(self, link: int, m_lo: int, m_hi: int):
        return WN.digest_of(self.base, self.metric_result(link, m_lo, m_hi))


def link_edges(rp, col, lid):
    """{link id: (edge lo -> hi, edge hi -> lo)} of the up links (a link that
    is not up is a self-loop in the CSR)."""
    out = {}
    for a in range(len(rp) - 1):
        for e in range(int(rp[a]), int(rp[a + 1])):
            b = int(col[e])
            if a != b:
                pair = out.setdefault(int(lid[e]), [None, None])
                pair[0 if a < b else 1] = e
    return {l: tuple(p) for l, p in out.items()}


def tail_of(rp, e: int) -> int:
    return int(np.searchsorted(rp, e, side="right")) - 1


def classify(rp, col, met, ovl, dist, s, edges, new):
    """The hot direction of a change: (root edge, delta), or (None, 0) when
    cold.  `edges` = (e_lo, e_hi) of the link, `new` = its resolved weights."""
    hot = []
    for e, w1 in zip(edges, new):
        a, b, w0 = tail_of(rp, e), int(col[e]), int(met[e])
        if w1 == w0 or (ovl[a] and a != s) or dist[a] == L.U64_MAX:
            continue
        da, db = int(dist[a]), int(dist[b])
        if w1 > w0 and da + w0 == db:
            hot.append((e, 0))
        elif w1 < w0 and da + w1 <= db:
            hot.append((e, db - da - w1))
    assert len(hot) <= 1, "positive metrics: one direction at most is hot"
    return hot[0] if hot else (None, 0)


def grow(rp, col, met, ovl, dist, s, edges, new, root_edge, delta):
    """D of a hot change: the nodes reached from the root edge's head over
    edges of slack <= delta (new weights), heads reached and not the source."""
    w = {edges[0]: new[0], edges[1]: new[1]}
    v = int(col[root_edge])
    seen, todo = {v}, [v]
    while todo:
        x = todo.pop()
        if ovl[x]:  # drained (never the source: it is not in D): no children
            continue
        for e in range(int(rp[x]), int(rp[x + 1])):
            c = int(col[e])
            if c in seen or c == s or dist[c] == L.U64_MAX:
                continue
            if int(dist[x]) + w.get(e, int(met[e])) <= int(dist[c]) + delta:
                seen.add(c)
                todo.append(c)
    return seen


def changed_nodes(base, res):
    """Nodes whose metric or next-hop row differs between two renders."""
    (bd, bn), (d, n) = base, res
    return set(int(v) for v in np.nonzero((d != bd) | (n != bn).any(axis=1))[0])


def variants(w_lo: int, w_hi: int, link: int):
    """The six changes the GPU test applies to every up link, by name."""
    one = link & 1  # the single-direction changes alternate between the directions
    return {
        "raise_x2": (2 * w_lo, 2 * w_hi),
        "raise_one": (KEEP, w_hi + 1) if one else (w_lo + 1, KEEP),
        "lower_to_1": (1, 1),
        "lower_one": (max(1, w_lo - 1), KEEP) if one else (KEEP, max(1, w_hi - 1)),
        "keep": (KEEP, KEEP),
        "current": (w_lo, w_hi),
    }
