"""Every node's route-database delta between two passes on the GPU
(spf_mplan_route_snapshot / spf_mplan_route_delta, include/openr_spf.h;
LinkState.allSourcesRouteSnapshot / allSourcesRouteDelta): what
DecisionRouteDb::calculateUpdate (Decision.cpp:111-146) gives for every node.

Two expectations, neither from the code under test:
  primary    DecisionRouteDb.calculateUpdate (the restatement next to the
             solver) over SpfSolver.buildRouteDb(me) taken before and after the
             change, prefix i = the loopback of node i = destination set i (a
             mapping fixed across the two passes), shared labels included
             (777 on a0 and b0, 778 on r25 and w0);
  secondary  the two full read-backs (allSourcesRouteDb / allSourcesLabelRouteDb
             of every me, taken before the snapshot and after the second
             pass), translated to {(link by value, metric)} sets and compared
             on the host.
Both are compared by equality, for every me.
"""

import copy
import ctypes as C

import numpy as np
import pytest

from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.link_state import LinkState
from openr_amd.lsdb import create_adj_db, create_adjacency
from openr_amd.spf_solver import DecisionRouteDb, PrefixEntry, PrefixState, SpfSolver

pytestmark = pytest.mark.gpu

RING = 33
SHARED = 777


def world():
    """40 nodes: a ring r00..r32 with chords and mixed metrics, and
      me0   two parallel links to x0 (equal metrics) and one link to y0;
            x0 and y0 hang off the ring;
      z0    a leaf of r05 (cut off when that link goes down);
      a0,b0 leaves of r10 at equal metrics sharing label 777: from anywhere
            else the next hops towards either are the same;
      w0    a leaf of r20, sharing label 778 with r25 (the smaller name,
            reachable: it owns the label from everywhere, w0 included).
    Returns {name: AdjacencyDatabase} (no adjacency labels: the MPLS routes
    are the node-label ones)."""
    ring = [f"r{i:02d}" for i in range(RING)]
    links = []
    for i in range(RING):
        links.append((ring[i], ring[(i + 1) % RING], 1 + i % 3, 1 + (i + 1) % 3))
    for i in range(0, RING, 5):
        links.append((ring[i], ring[(i + 11) % RING], 4, 4))
    links += [("me0", "x0", 2, 2), ("me0", "x0", 2, 2), ("me0", "y0", 3, 3), ("x0", "r02", 1, 1),
              ("y0", "r03", 1, 1), ("z0", "r05", 2, 2), ("a0", "r10", 1, 1), ("b0", "r10", 1, 1),
              ("w0", "r20", 1, 1)]
    names = sorted({u for u, _, _, _ in links} | {v for _, v, _, _ in links})
    adjs = {n: [] for n in names}
    seen = {}
    for i, (u, v, mu, mv) in enumerate(links):
        k = seen.get((u, v), 0)
        seen[(u, v)] = k + 1
        adjs[u].append(create_adjacency(v, f"{u}/{v}/{k}", f"{v}/{u}/{k}", f"fe80::{i + 1:x}",
                                        f"10.0.{i}.1", mu, 0))
        adjs[v].append(create_adjacency(u, f"{v}/{u}/{k}", f"{u}/{v}/{k}", f"fe80::1:{i + 1:x}",
                                        f"10.0.{i}.2", mv, 0))
    label = {n: 100 + i for i, n in enumerate(names)}
    label["a0"] = label["b0"] = SHARED
    label["r25"] = label["w0"] = SHARED + 1
    return {n: create_adj_db(n, adjs[n], label[n]) for n in names}


def adj(dbs, u, v, k=0):
    return next(a for a in dbs[u].adjacencies if a.ifName == f"{u}/{v}/{k}")


def push(ls, dbs, *nodes):
    for n in nodes:
        ls.updateAdjacencyDatabase(copy.deepcopy(dbs[n]))


def single_sets(n):
    return np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32)


class Gen:
    """One generation: the pass, both materialising calls, the full read-back
    by value (secondary) and, when asked, every me's buildRouteDb (primary)."""

    def __init__(self, ls, sets, lfa, mes=None, solver_ps=None, sample=None, solver_mes=None):
        sp, sn = sets
        ls.prefetchAllSources()
        self.n_records, _ = ls.allSourcesRouteRecords(sp, sn, lfa, mes)
        self.labels = ls.allSourcesLabelRoutes(lfa, mes)[0]
        names, rp, _col, _met, lid, _ovl = ls.flatten()
        self.names = list(names)
        self.lid, self.rp = np.array(lid), np.array(rp)
        mes = list(range(len(names))) if mes is None else [int(v) for v in mes]
        self.mes = mes
        self.link_names = {int(l): ls._link(int(l)).orderedNames for l in np.unique(lid)
                           if self._up(ls, int(l))}
        self.ip, self.lb, self.raw = {}, {}, {}
        for t in (range(len(mes)) if sample is None else sample):
            hdr, rec = ls.allSourcesRouteDb(t)
            owner, ptr, lrec = ls.allSourcesLabelRouteDb(t)
            self.raw[t] = (hdr, rec, owner, ptr, lrec)
            off, cnt = (hdr & np.uint64(0xFFFFFFFF)).astype(np.int64), (hdr >> np.uint64(32)).astype(np.int64)
            self.ip[t] = {int(p): self._nhs(rec[off[p]: off[p] + cnt[p]]) for p in np.nonzero(cnt)[0]}
            self.lb[t] = {int(lab): (int(owner[g]), self._nhs(lrec[int(ptr[g]): int(ptr[g + 1])]))
                          for g, lab in enumerate(self.labels.tolist()) if owner[g] != N.SPF_UNREACHABLE}
        self.dbs = None
        if solver_ps is not None:
            self.dbs = {}
            for t in (range(len(mes)) if solver_mes is None else solver_mes):
                me = self.names[mes[t]]
                db = SpfSolver(me, False, lfa).buildRouteDb(me, {ls.getArea(): ls}, solver_ps)
                self.dbs[t] = DecisionRouteDb() if db is None else db

    @staticmethod
    def _up(ls, l):
        try:
            ls._link(l)
            return True
        except N.SpfError:  # a withdrawn link's dead slots
            return False

    def _nhs(self, rec):
        out = frozenset((self.link_names[int(self.lid[r & 0xFFFFFFFF])], r >> 32) for r in rec.tolist())
        assert len(out) == len(rec)
        return out


def secondary(g0, g1):
    """Per me (updated sets, deleted sets, updated labels, deleted labels)."""
    out = {}
    for t in g1.ip:
        a, b, la, lb = g0.ip[t], g1.ip[t], g0.lb[t], g1.lb[t]
        out[t] = ([p for p in sorted(b) if a.get(p) != b[p]], [p for p in sorted(a) if p not in b],
                  [l for l in sorted(lb) if la.get(l) != lb[l]], [l for l in sorted(la) if l not in lb])
    return out


def primary(g0, g1, prefix_set):
    """The same from calculateUpdate over buildRouteDb before / after."""
    out = {}
    for t, old in g0.dbs.items():
        new = g1.dbs[t]
        d = old.calculateUpdate(new)
        applied = copy.deepcopy(old)
        applied.update(d)
        assert applied == new
        out[t] = (sorted(prefix_set[p] for p in d.unicastRoutesToUpdate),
                  sorted(prefix_set[p] for p in d.unicastRoutesToDelete),
                  sorted(r.label for r in d.mplsRoutesToUpdate), sorted(d.mplsRoutesToDelete))
    return out


def loopbacks(ls, names, sets=None):
    """Prefix p = destination set p, advertised by every node of the set (one
    node: its loopback; several: an anycast prefix).  The mapping is fixed
    across the passes."""
    ps, prefix_set = PrefixState(), {}
    sets = [[i] for i in range(len(names))] if sets is None else sets
    for p, members in enumerate(sets):
        for v in members:
            ps.updatePrefix(names[v], ls.getArea(), PrefixEntry(f"fd00::{p:x}/128"))
        prefix_set[f"fd00::{p:x}/128"] = p
    return ps, prefix_set


def moved_only(g0, g1, t):
    """Labels of me t whose owner changed while the next hops stayed the same
    (a shared label's owner moving between two nodes behind the same links):
    the GPU's delta lists them, its record carrying the owner; a RibMplsEntry
    does not hold the owner, so calculateUpdate does not."""
    return [l for l in sorted(g1.lb[t]) if l in g0.lb[t] and g0.lb[t][l][0] != g1.lb[t][l][0]
            and g0.lb[t][l][1] == g1.lb[t][l][1]]


def check(delta, want, owner_moves=None):
    """owner_moves: {me: moved_only(...)} when `want` is calculateUpdate's --
    exactly those labels are listed on top of its updates."""
    lists, totals, ms = delta
    assert ms >= 0
    for t, w in want.items():
        got = lists[t]
        if owner_moves is not None:
            assert not set(owner_moves[t]) & set(w[2]), (t, owner_moves[t], w[2])
            w = (w[0], w[1], sorted(list(w[2]) + owner_moves[t]), w[3])
        assert tuple(got) == tuple(w), (t, got, w)
    if len(want) == len(lists) and owner_moves is None:
        assert totals[:4] == [sum(len(w[k]) for w in want.values()) for k in range(4)]


def step(ls, dbs, change, lfa, with_primary=True, sets=None, set_lists=None, solver_mes=None):
    """generation 0, snapshot, `change`, generation 1, delta -> (g0, g1, delta),
    checked against both expectations (the primary one for the me of
    solver_mes; None: every me)."""
    names = sorted(dbs)
    sets = single_sets(len(names)) if sets is None else sets
    ps, prefix_set = loopbacks(ls, names, set_lists) if with_primary else (None, None)
    g0 = Gen(ls, sets, lfa, solver_ps=ps, solver_mes=solver_mes)
    snap = ls.allSourcesRouteSnapshot()
    assert snap.deviceBytes > 0
    change()
    g1 = Gen(ls, sets, lfa, solver_ps=ps, solver_mes=solver_mes)
    assert g1.names == g0.names == names
    delta = ls.allSourcesRouteDelta(snap)
    check(delta, secondary(g0, g1))
    if with_primary:
        want = primary(g0, g1, prefix_set)
        check(delta, want, {t: moved_only(g0, g1, t) for t in want})
    again = ls.allSourcesRouteDelta(snap)  # the snapshot is only read
    assert again[0] == delta[0] and again[1] == delta[1]
    snap.close()
    return g0, g1, delta


MEMBERS = pytest.mark.parametrize("members", [1, 3])
LFA = pytest.mark.parametrize("lfa", [False, True], ids=["sp", "lfa"])


@MEMBERS
@LFA
def test_nothing_changed(members, lfa):
    """Every list is empty, and the materialising calls after a snapshot give
    the pools a fresh run gives."""
    dbs = world()
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *sorted(dbs))
        g0, g1, (lists, totals, _) = step(ls, dbs, lambda: None, lfa)
        assert all(l == ([], [], [], []) for l in lists) and totals == [0, 0, 0, 0, 0]
        assert g0.n_records == g1.n_records and g0.ip == g1.ip and g0.lb == g1.lb
        for t in g0.raw:
            assert all(np.array_equal(x, y) for x, y in zip(g0.raw[t], g1.raw[t]))


@MEMBERS
@LFA
def test_metric_change_takes_the_fast_path(members, lfa):
    """One link's metric changed, rows untouched: updates only, exactly the
    routes whose sets moved, every me compared position by position."""
    dbs = world()
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *sorted(dbs))

        def change():
            adj(dbs, "r00", "r01").metric = 7
            adj(dbs, "r01", "r00").metric = 7
            push(ls, dbs, "r00", "r01")

        ls.flatten()
        patches, loads = N.lib.ls_debug_row_patches(ls._h), N.lib.spf_graph_loads(N.lib.ls_engine(ls._h))
        _g0, g1, (lists, totals, _) = step(ls, dbs, change, lfa)
        assert totals[0] > 0 and totals[2] > 0 and totals[1] == 0 and totals[3] == 0
        assert totals[4] == 0, "a me left the positional compare"
        # (with LFA every neighbour is kept, so more routes carry the link's metric)
        assert any(l[0] for l in lists) and totals[0] < sum(len(r) for r in g1.ip.values())
        # rows untouched: neither patched in place nor reloaded
        assert N.lib.ls_debug_row_patches(ls._h) == patches
        assert N.lib.spf_graph_loads(N.lib.ls_engine(ls._h)) == loads


@MEMBERS
def test_parallel_link_withdrawn_takes_the_set_path(members):
    """One of me0's two parallel links to x0 withdrawn: me0's row is reordered
    (the dead slot moves), so its records' edge indices move; the route to y0
    is not reported, the route to x0 is."""
    moved = False
    for k in (0, 1):
        dbs = world()
        names = sorted(dbs)
        me, x, y = names.index("me0"), names.index("x0"), names.index("y0")
        with LinkState(devices=[0] * members) as ls:
            push(ls, dbs, *names)

            def change():
                dbs["me0"].adjacencies.remove(adj(dbs, "me0", "x0", k))
                push(ls, dbs, "me0")

            g0, g1, (lists, totals, _) = step(ls, dbs, change, False)
            assert totals[4] >= 1, "no me took the set path"
            assert x in lists[me][0] and y not in lists[me][0] and lists[me][1] == []
            assert g0.ip[me][y] == g1.ip[me][y] and g0.ip[me][x] != g1.ip[me][x]
            # the route to y0 has one next hop; its slot within me0's row, before and after
            e0 = (int(g0.raw[me][1][int(g0.raw[me][0][y]) & 0xFFFFFFFF]) & 0xFFFFFFFF) - int(g0.rp[me])
            e1 = (int(g1.raw[me][1][int(g1.raw[me][0][y]) & 0xFFFFFFFF]) & 0xFFFFFFFF) - int(g1.rp[me])
            moved |= e0 != e1
            # the label routes follow the same compare
            assert 100 + x in lists[me][2] and 100 + y not in lists[me][2]
    assert moved, "me0's record of the route to y0 kept its edge index in both variants"


@MEMBERS
@LFA
def test_link_down_cuts_a_node_off_then_back(members, lfa):
    """z0's only link down: a DELETE of its route (and label) at every me, and
    of every route at z0; back up: an UPDATE (new route).  r04 is drained: with
    LFA it is an overloaded LFA neighbour of r05's."""
    dbs = world()
    dbs["r04"].isOverloaded = True
    names = sorted(dbs)
    z = names.index("z0")
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)

        def down():
            adj(dbs, "z0", "r05").isOverloaded = True
            push(ls, dbs, "z0")

        def up():
            adj(dbs, "z0", "r05").isOverloaded = False
            push(ls, dbs, "z0")

        _g0, _g1, (lists, totals, _) = step(ls, dbs, down, lfa)
        for t, l in enumerate(lists):
            if t != z:
                assert z in l[1] and 100 + z in l[3], t
        assert len(lists[z][1]) == len(names) - 1 and lists[z][0] == []
        assert totals[1] >= 2 * (len(names) - 1)
        _g0, _g1, (lists, totals, _) = step(ls, dbs, up, lfa)
        for t, l in enumerate(lists):
            if t != z:
                assert z in l[0] and 100 + z in l[2], t
        assert len(lists[z][0]) == len(names) - 1 and totals[1] == 0 and totals[3] == 0


@MEMBERS
def test_new_adjacency_reloads_and_reissues_a_link_id(members):
    """A link withdrawn (its id stays with its dead slots), then a new
    adjacency between two existing nodes: a full reload, which frees that id
    for another link.  The compare is by link value."""
    dbs = world()
    names = sorted(dbs)
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)
        lid = ls.flatten()[4]  # (flattened: the withdrawal below patches me0's and x0's rows)
        gone = (("me0", "me0/x0/1"), ("x0", "x0/me0/1"))
        (ghost,) = [int(l) for l in np.unique(lid) if ls._link(int(l)).orderedNames == gone]
        dbs["me0"].adjacencies.remove(adj(dbs, "me0", "x0", 1))
        push(ls, dbs, "me0")
        ls.prefetchAllSources()
        eng = N.lib.ls_engine(ls._h)
        loads = N.lib.spf_graph_loads(eng)

        def add(u, v, i):
            dbs[u].adjacencies.append(create_adjacency(v, f"{u}/{v}/0", f"{v}/{u}/0", f"fe80::{i:x}",
                                                       "10.1.0.1", 2, 0))
            dbs[v].adjacencies.append(create_adjacency(u, f"{v}/{u}/0", f"{u}/{v}/0", f"fe80::1:{i:x}",
                                                       "10.1.0.2", 2, 0))
            push(ls, dbs, u, v)

        def change():
            add("r07", "r25", 200)
            ls.flatten()  # the reload: the withdrawn link's id is free again
            add("r08", "r26", 201)

        g0, g1, (_lists, totals, _) = step(ls, dbs, change, False)
        assert N.lib.spf_graph_loads(N.lib.ls_engine(ls._h)) > loads
        # an id of generation 0 (the withdrawn link's, kept with its dead slots)
        # names another link in generation 1
        assert ghost in g0.lid.tolist(), "the withdrawn link kept no dead slots"
        assert g1.link_names.get(ghost, gone) != gone, "no link id was re-issued"
        assert totals[0] > 0


def tile_sets(names):
    """1,100 sets over the 40 nodes: sets 0..39 = the nodes (aligned quads of
    single nodes: the quads kernel's fast case), then pairs and triples; z0
    alone in sets 1023, 1024 (both sides of the 1,024-set tile boundary) and
    1099 (the last), and first in name order among... set 0 is names[0] = a0."""
    n = len(names)
    z = names.index("z0")
    sets = [[i] for i in range(n)]
    k = 0
    while len(sets) < 1100:
        a, b, c = k % n, (3 * k + 1) % n, (7 * k + 2) % n
        sets.append(sorted({a, b}) if k % 2 else sorted({a, b, c}))
        k += 1
    for p in (1023, 1024, 1099):
        sets[p] = [z]
    sp = np.zeros(len(sets) + 1, np.uint32)
    sp[1:] = np.cumsum([len(s) for s in sets])
    return sp, np.array([v for s in sets for v in s], np.uint32), sets


@MEMBERS
@LFA
def test_tile_and_word_edges(members, lfa):
    """1,100 sets (two 1,024-set tiles, five 256-route blocks per me, not a
    multiple of 4 or 32), single-node quads and multi-node sets; changes in the
    first set (a0 comes up), at both sides of the tile boundary and in the last
    set (z0 goes down); w0's whole row is dead in both generations."""
    dbs = world()
    names = sorted(dbs)
    sp, sn, sets = tile_sets(names)
    a0, z, w = names.index("a0"), names.index("z0"), names.index("w0")
    assert sets[0] == [a0]
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)
        adj(dbs, "w0", "r20").isOverloaded = True
        adj(dbs, "a0", "r10").isOverloaded = True
        push(ls, dbs, "w0", "a0")

        def change():
            adj(dbs, "a0", "r10").isOverloaded = False
            adj(dbs, "z0", "r05").isOverloaded = True
            push(ls, dbs, "a0", "z0")

        # The primary expectation too, set p = an anycast prefix of its nodes,
        # for six me (1,100 prefixes each).  Shortest paths only: the sets are
        # handed over as buildRouteDb would filter them for one me, and a shared
        # list cannot drop me from its own anycast sets -- without LFA such a set
        # has no next hop either way (distance 0), with LFA the engine's
        # selection would add backups towards the other members.
        some = [names.index(s) for s in ("a0", "me0", "r10", "r15", "w0", "z0")]
        g0, g1, (lists, totals, _) = step(ls, dbs, change, lfa, with_primary=not lfa, sets=(sp, sn),
                                          set_lists=sets, solver_mes=some)
        assert g0.ip[w] == {} and g1.ip[w] == {} and lists[w] == ([], [], [], [])
        me = names.index("r15")
        assert 0 in lists[me][0] and all(p in lists[me][1] for p in (1023, 1024, 1099))
        assert lists[z][0] == [] and len(lists[z][1]) > 1000


@MEMBERS
@LFA
def test_labels(members, lfa):
    """777 is advertised by a0 and b0.  a0 (the smaller name) comes up: the
    owner changes from b0 to a0 with identical next hops -- an UPDATE; r12's
    label is withdrawn -- a DELETE; r13 gets a new one -- an UPDATE of the new
    and a DELETE of the old; a label its me owns on both sides is not
    reported."""
    dbs = world()
    names = sorted(dbs)
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)
        adj(dbs, "a0", "r10").isOverloaded = True
        push(ls, dbs, "a0")
        old12, old13 = dbs["r12"].nodeLabel, dbs["r13"].nodeLabel

        def change():
            adj(dbs, "a0", "r10").isOverloaded = False
            dbs["r12"].nodeLabel = 0
            dbs["r13"].nodeLabel = 5000
            push(ls, dbs, "a0", "r12", "r13")

        g0, g1, (lists, _totals, _) = step(ls, dbs, change, lfa)
        me = names.index("me0")
        assert g0.lb[me][SHARED][0] == names.index("b0") and g1.lb[me][SHARED][0] == names.index("a0")
        assert g0.lb[me][SHARED][1] == g1.lb[me][SHARED][1], "the next hops were meant to be identical"
        assert SHARED in lists[me][2]
        assert old12 in lists[me][3] and old13 in lists[me][3] and 5000 in lists[me][2]
        for t, n in enumerate(names):
            own = 100 + t
            if n not in ("a0", "b0", "r12", "r13"):
                assert own not in lists[t][2] and own not in lists[t][3]
        r13 = names.index("r13")
        assert 5000 in lists[r13][2] and old13 in lists[r13][3]


def test_scan_crosses_a_tile():
    """fabric1000 (960 nodes), every node a me, its loopback and its label:
    960 me x 4 blocks = 3,840 block counts, past one 2,048-entry scan tile.
    One rack switch's uplink metric changes; a sample of me around the tile
    boundary and across the list is compared in full, the totals for all."""
    topo = T.fabric(1000, full=True)
    rank = {s: i for i, s in enumerate(sorted(topo.nodes))}
    topo.lsdb.dbs["node_label"] = np.array([rank[s] + 1 for s in topo.nodes], np.int32)
    from openr_amd.wire import unpack

    dbs = {d.thisNodeName: d for d in unpack(topo.lsdb)}
    names = sorted(dbs)
    n = len(names)
    sample = sorted(set(range(0, n, 61)) | set(range(508, 516)) | {n - 1})
    with LinkState(devices=[0, 0]) as ls:
        ls.updateAdjacencyDatabases(topo.lsdb)
        sets = single_sets(n)
        g0 = Gen(ls, sets, False, sample=sample)
        snap = ls.allSourcesRouteSnapshot()
        node = names[n // 3]
        for a in dbs[node].adjacencies[:1]:
            a.metric += 3
        push(ls, dbs, node)
        g1 = Gen(ls, sets, False, sample=sample)
        lists, totals, _ = ls.allSourcesRouteDelta(snap)
        want = secondary(g0, g1)
        for t in sample:
            assert tuple(lists[t]) == tuple(want[t]), t
        assert totals[:4] == [sum(len(l[k]) for l in lists) for k in range(4)]
        assert totals[0] > 0 and any(lists[t][0] for t in sample if t > 512)


def test_contract():
    dbs = world()
    names = sorted(dbs)
    n = len(names)
    sets = single_sets(n)

    def status(fn):
        with pytest.raises(N.SpfError) as ei:
            fn()
        return ei.value.status

    with LinkState(devices=[0, 0]) as ls:
        push(ls, dbs, *names)
        ls.prefetchAllSources()
        assert status(ls.allSourcesRouteSnapshot) == N.SPF_E_STATE  # no route records yet
        Gen(ls, sets, False)
        snap = ls.allSourcesRouteSnapshot()
        # the plan holds no database now
        assert status(lambda: ls.allSourcesRouteDb(0)) == N.SPF_E_STATE
        assert status(lambda: ls.allSourcesLabelRouteDb(0)) == N.SPF_E_STATE
        assert status(ls.allSourcesRouteSnapshot) == N.SPF_E_STATE
        assert status(lambda: ls.allSourcesRouteDelta(snap)) == N.SPF_E_STATE
        # another me list, another n_sets, another LFA choice
        Gen(ls, sets, False, mes=np.arange(n - 1, dtype=np.uint32))
        assert status(lambda: ls.allSourcesRouteDelta(snap)) == N.SPF_E_INVALID
        Gen(ls, single_sets(n - 1), False)
        assert status(lambda: ls.allSourcesRouteDelta(snap)) == N.SPF_E_INVALID
        Gen(ls, sets, True)
        assert status(lambda: ls.allSourcesRouteDelta(snap)) == N.SPF_E_INVALID
        # label routes of another me list than the route records': no snapshot, and nothing has moved
        ls.allSourcesLabelRoutes(True, np.arange(n - 1, dtype=np.uint32))
        assert status(ls.allSourcesRouteSnapshot) == N.SPF_E_INVALID
        ls.allSourcesRouteDb(0)
        ls.allSourcesLabelRouteDb(0)
        # a row patch drops the LinkState's plan; the snapshot is still good
        adj(dbs, "z0", "r05").isOverloaded = True
        push(ls, dbs, "z0")
        assert not N.lib.ls_all_sources_plan(ls._h)
        Gen(ls, sets, False)
        lists, totals, _ = ls.allSourcesRouteDelta(snap)
        assert totals[1] >= n - 1 and names.index("z0") in lists[0][1]
        # device-side consumers: every me slot of every member is listed once
        mp = N.lib.ls_all_sources_plan(ls._h)
        seen = []
        for r in range(2):
            k = C.c_uint32()
            p = [C.c_void_p() for _ in range(4)]
            N.raise_for(N.lib.spf_mplan_route_delta_buffers(C.c_void_p(mp), r, *[C.byref(x) for x in p], None,
                                                            0, C.byref(k)), N.global_error())
            slots = np.zeros(max(1, k.value), np.uint32)
            N.raise_for(N.lib.spf_mplan_route_delta_buffers(C.c_void_p(mp), r, None, None, None, None,
                                                            N.ptr(slots), k.value, None), N.global_error())
            assert all(bool(x.value) == bool(k.value) for x in p)
            seen += slots[: k.value].tolist()
        assert sorted(seen) == list(range(n))
        assert not snap.closed
    assert snap.closed  # closed with its LinkState, before the context
