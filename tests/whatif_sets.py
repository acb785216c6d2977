"""Expected values of link-set what-if batches (spf_whatif_plan_create_sets),
in numpy beside whatif_nodes.py, and the set families the tests use.

The oracle's what-if entry point takes one link, so the pin for a set is a
full re-run on a changed LSDB, from a fresh OracleLinkState each time: a copy
of the packed LSDB in which one adjacency record of every member link has
is_overloaded = 1.  The oracle skips a link that is not up exactly where it
skips an ignored one, so the SPF result is that of linksToIgnore = the set.

``orc.spf(names[src])`` is rendered with whatif_lists.base_from_oracle over the
UNFAILED CSR (a failed neighbour's bit is simply never set) and reduced with
whatif_nodes.digest_of.

The families are built from the base render alone (distances and the CSR):
an edge a -> b is tight when a is reached, a is not drained unless it is the
source, and dist[a] + metric == dist[b].
"""

import numpy as np

import whatif_lists as L
import whatif_nodes as WN
from oracle import OracleLinkState
from openr_amd.lsdb import PackedLsdb


def adjacency_records(lsdb):
    """{(node name, interface name): index of the packed adjacency record}."""
    out = {}
    blob = lsdb.blob
    for r in lsdb.dbs:
        node = bytes(blob[int(r["name_off"]): int(r["name_off"]) + int(r["name_len"])]).decode()
        for k in range(int(r["adj_begin"]), int(r["adj_begin"]) + int(r["adj_count"])):
            a = lsdb.adjs[k]
            ifn = bytes(blob[int(a["if_off"]): int(a["if_off"]) + int(a["if_len"])]).decode()
            out[(node, ifn)] = k
    return out


class Expected:
    """The unfailed render of one (topology, source), computed once, and the
    expected digest / full result of any link set against it."""

    def __init__(self, lsdb, ls, names, rp, col, s: int) -> None:
        self.lsdb, self.ls, self.names, self.rp, self.col, self.s = lsdb, ls, names, rp, col, int(s)
        orc = OracleLinkState()
        orc.update_packed(lsdb)
        self.base = L.base_from_oracle(orc, names, rp, col, self.s)
        self.base_digest = (0, 0, L.result_hash(*self.base))
        self._adj = adjacency_records(lsdb)
        self._memo = {}

    def record(self, link: int) -> int:
        lk = self.ls._link(int(link))
        return self._adj[(lk._n1, lk._if1)]

    def result(self, links):
        key = tuple(sorted(set(int(l) for l in links)))
        if key not in self._memo:
            adjs = self.lsdb.adjs.copy()
            for l in key:
                adjs["is_overloaded"][self.record(l)] = 1
            orc = OracleLinkState()
            orc.update_packed(PackedLsdb(self.lsdb.blob, self.lsdb.dbs.copy(), adjs))
            self._memo[key] = L.base_from_oracle(orc, self.names, self.rp, self.col, self.s)
        return self._memo[key]

    def digest(self, links):
        return WN.digest_of(self.base, self.result(links))


class Dag:
    """The unfailed shortest-path DAG of a base render over the CSR."""

    def __init__(self, rp, col, met, lid, ovl, dist, s: int) -> None:
        self.rp, self.col, self.lid, self.s = rp, col, lid, int(s)
        n = len(rp) - 1
        self.n = n
        self.tight = {}      # link id -> (tail, head) of its tight direction
        self.into = [[] for _ in range(n)]   # head -> tight links into it
        self.kids = [set() for _ in range(n)]
        self.pair = {}       # (min node, max node) -> link ids between them
        for a in range(n):
            for e in range(int(rp[a]), int(rp[a + 1])):
                b, l = int(col[e]), int(lid[e])
                if a == b:
                    continue
                self.pair.setdefault((min(a, b), max(a, b)), set()).add(l)
                if dist[a] == L.U64_MAX or (ovl[a] and a != self.s):
                    continue
                if int(dist[a]) + int(met[e]) == int(dist[b]) and dist[b] != L.U64_MAX:
                    self.tight[l] = (a, b)
                    self.into[b].append(l)
                    self.kids[a].add(b)
        # (the CSR keeps a link that is not up as a self-loop carrying its id)
        self.up = sorted(set().union(*self.pair.values())) if self.pair else []
        self.ids = sorted(set(int(l) for l in lid))
        self.loose = [l for l in self.up if l not in self.tight]
        self._desc = {}

    def desc(self, v: int):
        """v and its DAG descendants."""
        if v not in self._desc:
            seen, todo = {v}, [v]
            while todo:
                for c in self.kids[todo.pop()]:
                    if c not in seen:
                        seen.add(c)
                        todo.append(c)
            self._desc[v] = seen
        return self._desc[v]

    def heads(self, links):
        return {self.tight[int(l)][1] for l in links if int(l) in self.tight}


def not_up_links(ls, dag):
    """Link ids of the graph that are not up (here: a side is overloaded), so
    no CSR edge between two nodes carries them."""
    out = []
    up = set(dag.up)
    for l in range(max(dag.ids) + 1):
        if l in up:
            continue
        try:
            lk = ls._link(l)
        except Exception:
            continue
        if not lk.isUp():
            out.append(l)
    return out


def families(ls, dag, seed: int, per_family: int = 3):
    """{family: [set, ...]} over one graph; at most `per_family` sets of each
    constructed family (the first found in node / link order)."""
    rng = np.random.default_rng(seed)
    fam = {k: [] for k in ("ecmp_cut", "parallel", "nested", "same_head", "disjoint", "mixed",
                           "cold", "empty", "random")}
    tight = sorted(dag.tight)
    for b in range(dag.n):
        if len(dag.into[b]) >= 2 and len(fam["ecmp_cut"]) < per_family:
            fam["ecmp_cut"].append(sorted(dag.into[b]))
        if len(dag.into[b]) >= 2 and len(fam["same_head"]) < per_family:
            fam["same_head"].append(sorted(dag.into[b])[:2])
    for ids in dag.pair.values():
        if len(ids) >= 2 and len(fam["parallel"]) < per_family:
            fam["parallel"].append(sorted(ids))
    for l in tight:
        b = dag.tight[l][1]
        inner = [m for m in tight if m != l and dag.tight[m][0] in dag.desc(b)]
        if inner and len(fam["nested"]) < per_family:
            fam["nested"].append([l, inner[-1]])
        apart = [m for m in tight if not (dag.desc(dag.tight[m][1]) & dag.desc(b))]
        if apart and len(fam["disjoint"]) < per_family:
            fam["disjoint"].append([l, apart[len(apart) // 2]])
    dead = not_up_links(ls, dag)
    if tight and dag.loose and dead:
        fam["mixed"].append([tight[len(tight) // 2], dag.loose[0], dead[0], dag.loose[-1]])
        fam["mixed"].append([dead[-1], tight[0], dag.loose[len(dag.loose) // 2]])
    if len(dag.loose) >= 3:
        fam["cold"].append(dag.loose[:3])
    if dead and dag.loose:
        fam["cold"].append([dead[0], dag.loose[-1]])
    fam["empty"].append([])
    up = np.array(dag.up)
    for k in (2, 3, 5, 8):
        for _ in range(2):
            fam["random"].append(sorted(int(l) for l in rng.choice(up, k, replace=False)))
    return fam
