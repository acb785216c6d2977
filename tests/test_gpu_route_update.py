"""The payload of every node's route-database delta on the GPU
(spf_mplan_route_update, include/openr_spf.h; LinkState.allSourcesRouteUpdate /
allSourcesDecisionRouteUpdate): the next hops -- for a label route the owner
too -- of the routes the delta lists, what a DecisionRouteUpdate carries
(Decision.cpp:111-146), gathered into one exactly sized pool per member.

Two expectations, neither from the code under test, both compared by equality:
  by value   the full read-back of generation 1 (allSourcesRouteDb /
             allSourcesLabelRouteDb): an UPDATE entry's records are that route's
             rec[off : off + cnt] -- same order, same u64s --, its owner is
             owner[g]; a DELETE entry has no records and owner SPF_UNREACHABLE;
             uptr is non-decreasing and ends at the reported total; pool_bytes
             is the header's formula;
  reference  old.calculateUpdate(new) over SpfSolver.buildRouteDb(me) before and
             after: the updated unicast routes' next hops and the updated
             RibMplsEntry's, the shared labels' included, and old.update(delta)
             rebuilt from the GPU's payload gives new.
"""

import copy
import ctypes as C

import numpy as np
import pytest

from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.link_state import LinkState
from openr_amd.lsdb import create_adj_db, create_adjacency
from openr_amd.spf_solver import DecisionRouteUpdate, PrefixEntry, RibUnicastEntry
from test_gpu_route_delta import (LFA, MEMBERS, SHARED, Gen, adj, loopbacks, moved_only, push, single_sets,
                                  tile_sets, world)

pytestmark = pytest.mark.gpu

DEL, VAL = N.SPF_DELTA_DELETE, N.SPF_DELTA_DELETE - 1


def plan(ls):
    return C.c_void_p(N.lib.ls_all_sources_plan(ls._h))


def raw_update(ls, t):
    """me t's arrays as the C-ABI hands them over: (ip entries, ip_ptr, ip_rec,
    label entries, label_owner, label_ptr, label_rec)."""
    mp = plan(ls)
    ni, nl, ri, rl = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    N.raise_for(N.lib.spf_mplan_route_delta_db(mp, t, None, 0, C.byref(ni), None, 0, C.byref(nl)),
                N.global_error())
    ip, lb = np.zeros(max(1, ni.value), np.uint32), np.zeros(max(1, nl.value), np.uint32)
    N.raise_for(N.lib.spf_mplan_route_delta_db(mp, t, N.ptr(ip), ni.value, None, N.ptr(lb), nl.value, None),
                N.global_error())
    iptr, lptr = np.full(ni.value + 1, 7, np.uint64), np.full(nl.value + 1, 7, np.uint64)
    owner = np.zeros(max(1, nl.value), np.uint32)
    N.raise_for(N.lib.spf_mplan_route_update_db(mp, t, N.ptr(iptr, C.c_uint64), None, 0, C.byref(ri),
                                                N.ptr(owner), N.ptr(lptr, C.c_uint64), None, 0, C.byref(rl)),
                N.global_error())
    irec, lrec = np.zeros(max(1, ri.value), np.uint64), np.zeros(max(1, rl.value), np.uint64)
    N.raise_for(N.lib.spf_mplan_route_update_db(mp, t, None, N.ptr(irec, C.c_uint64), ri.value, None, None,
                                                None, N.ptr(lrec, C.c_uint64), rl.value, None),
                N.global_error())
    return (ip[: ni.value], iptr, irec[: ri.value], lb[: nl.value], owner[: nl.value], lptr,
            lrec[: rl.value])


def members_with_me(ls, members):
    n = 0
    for r in range(members):
        k = C.c_uint32()
        N.raise_for(N.lib.spf_mplan_route_delta_buffers(plan(ls), r, None, None, None, None, None, 0,
                                                        C.byref(k)), N.global_error())
        n += k.value > 0
    return n


def by_value(ls, g1, upd, members, every=True):
    """The payload of every me of g1.raw against generation 1's full read-back;
    with every=True the totals and pool_bytes too (g1 holds every me)."""
    lists, _totals, _ms, payload, info = upd
    n_ip = n_lb = r_ip = r_lb = u_ip = u_lb = 0
    for t, (hdr, rec, owner, ptr, lrec) in g1.raw.items():
        ip, iptr, irec, lb, uowner, lptr, ulrec = raw_update(ls, t)
        up, dele, lup, ldel = lists[t]
        assert [int(v & VAL) for v in ip if not v & DEL] == up and [int(v & VAL) for v in ip if v & DEL] == dele
        assert [int(v & VAL) for v in lb if not v & DEL] == lup and [int(v & VAL) for v in lb if v & DEL] == ldel
        for p_, r_ in ((iptr, irec), (lptr, ulrec)):
            assert p_[0] == 0 and np.all(p_[1:] >= p_[:-1]) and int(p_[-1]) == len(r_), t
        off, cnt = (hdr & np.uint64(0xFFFFFFFF)).astype(np.int64), (hdr >> np.uint64(32)).astype(np.int64)
        for j, v in enumerate(ip.tolist()):
            got = irec[int(iptr[j]): int(iptr[j + 1])]
            if v & DEL:
                assert len(got) == 0, (t, v & VAL)
                continue
            assert cnt[v] > 0 and np.array_equal(got, rec[off[v]: off[v] + cnt[v]]), (t, v)
            assert np.array_equal(payload[t][0][v], got)
        group = {int(lab): g for g, lab in enumerate(g1.labels.tolist())}
        for j, v in enumerate(lb.tolist()):
            got = ulrec[int(lptr[j]): int(lptr[j + 1])]
            if v & DEL:
                assert len(got) == 0 and uowner[j] == N.SPF_UNREACHABLE, (t, v & VAL)
                continue
            g = group[v]
            assert owner[g] != N.SPF_UNREACHABLE and uowner[j] == owner[g], (t, v)
            assert np.array_equal(got, lrec[int(ptr[g]): int(ptr[g + 1])]), (t, v)
            assert payload[t][1][v][0] == int(owner[g]) and np.array_equal(payload[t][1][v][1], got)
        assert sorted(payload[t][0]) == up and sorted(payload[t][1]) == lup
        n_ip, n_lb, r_ip, r_lb = n_ip + len(ip), n_lb + len(lb), r_ip + len(irec), r_lb + len(ulrec)
        u_ip, u_lb = u_ip + len(up), u_lb + len(lup)
    if every:
        assert len(g1.raw) == len(lists)
        assert info["totals"] == [u_ip, r_ip, u_lb, r_lb]
        k = members_with_me(ls, members)
        assert info["pool_bytes"] == 8 * r_ip + 8 * (n_ip + k) + 8 * r_lb + 8 * (n_lb + k) + 4 * n_lb
    assert info["kernel_ms"] >= 0 and len(info["phase_ms"]) == 3
    return n_ip, r_ip, n_lb, r_lb


def reference(ls, g0, g1, prefix_set, owner_moves=None):
    """calculateUpdate over buildRouteDb before / after against the expanded
    payload, for every me the generations hold solver databases of."""
    prefix_of = {p: s for s, p in prefix_set.items()}
    for t, old in g0.dbs.items():
        new = g1.dbs[t]
        d = old.calculateUpdate(new)
        uni, dele, mpls, ldel = ls.allSourcesDecisionRouteUpdate(t)
        assert {prefix_set[p]: e.nexthops for p, e in d.unicastRoutesToUpdate.items()} == uni, t
        assert sorted(prefix_set[p] for p in d.unicastRoutesToDelete) == dele
        # (a label whose owner moved behind unchanged next hops is in the GPU's
        # update, the owner being part of its record, and not in calculateUpdate's:
        # its entry is the one the old database holds)
        moved = moved_only(g0, g1, t) if owner_moves is None else owner_moves[t]
        got = {r.label: r for r in mpls}
        assert len(got) == len(mpls)
        assert all(got[l] == old.mplsRoutes[l] == new.mplsRoutes[l] for l in moved), t
        assert {r.label: r for r in d.mplsRoutesToUpdate} == {l: r for l, r in got.items() if l not in moved}, t
        assert list(d.mplsRoutesToDelete) == list(ldel)
        # old.update(the GPU's delta) gives new
        gpu = DecisionRouteUpdate()
        for p, nhs in uni.items():
            gpu.unicastRoutesToUpdate[prefix_of[p]] = RibUnicastEntry(prefix_of[p], nhs, PrefixEntry(prefix_of[p]),
                                                                      ls.getArea())
        gpu.unicastRoutesToDelete = [prefix_of[p] for p in dele]
        gpu.mplsRoutesToUpdate, gpu.mplsRoutesToDelete = mpls, ldel
        applied = copy.deepcopy(old)
        applied.update(gpu)
        assert {p: e.nexthops for p, e in applied.unicastRoutes.items()} == \
            {p: e.nexthops for p, e in new.unicastRoutes.items()}, t
        assert applied.mplsRoutes == new.mplsRoutes, t


def step(ls, dbs, change, lfa, members, with_primary=True, sets=None, set_lists=None, solver_mes=None):
    """generation 0, snapshot, `change`, generation 1, delta + update, checked
    against both expectations -> (g0, g1, the update)."""
    names = sorted(dbs)
    sets = single_sets(len(names)) if sets is None else sets
    ps, prefix_set = loopbacks(ls, names, set_lists) if with_primary else (None, None)
    g0 = Gen(ls, sets, lfa, solver_ps=ps, solver_mes=solver_mes)
    snap = ls.allSourcesRouteSnapshot()
    change()
    g1 = Gen(ls, sets, lfa, solver_ps=ps, solver_mes=solver_mes)
    upd = ls.allSourcesRouteUpdate(snap)
    by_value(ls, g1, upd, members)
    if with_primary:
        reference(ls, g0, g1, prefix_set)
    snap.close()
    return g0, g1, upd


@MEMBERS
@LFA
def test_nothing_changed(members, lfa):
    dbs = world()
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *sorted(dbs))
        _g0, _g1, (lists, _tot, _ms, payload, info) = step(ls, dbs, lambda: None, lfa, members)
        assert info["totals"] == [0, 0, 0, 0] and all(p == ({}, {}) for p in payload)
        for r in range(members):
            nr = [C.c_uint64(5), C.c_uint64(5)]
            N.raise_for(N.lib.spf_mplan_route_update_buffers(plan(ls), r, None, None, None, None, None,
                                                             C.byref(nr[0]), C.byref(nr[1])), N.global_error())
            assert nr[0].value == 0 and nr[1].value == 0


@MEMBERS
@LFA
def test_metric_change_updates_only(members, lfa):
    dbs = world()
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *sorted(dbs))

        def change():
            adj(dbs, "r00", "r01").metric = 7
            adj(dbs, "r01", "r00").metric = 7
            push(ls, dbs, "r00", "r01")

        _g0, _g1, (lists, totals, _ms, _payload, info) = step(ls, dbs, change, lfa, members)
        assert totals[0] > 0 and totals[2] > 0 and totals[1] == 0 and totals[3] == 0
        assert info["totals"][1] >= totals[0] and info["totals"][3] > 0


@MEMBERS
def test_parallel_link_withdrawn_names_the_new_edges(members):
    """me0's first parallel link to x0 withdrawn: its row is reordered, the
    payload's records are edges of the NEW row."""
    dbs = world()
    names = sorted(dbs)
    me, x = names.index("me0"), names.index("x0")
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)

        def change():
            dbs["me0"].adjacencies.remove(adj(dbs, "me0", "x0", 0))
            push(ls, dbs, "me0")

        _g0, g1, (lists, totals, _ms, payload, _info) = step(ls, dbs, change, False, members)
        assert totals[4] >= 1 and x in lists[me][0]
        rec = payload[me][0][x]
        assert len(rec) == 1
        e = int(rec[0]) & 0xFFFFFFFF
        assert g1.rp[me] <= e < g1.rp[me + 1]
        assert g1.link_names[int(g1.lid[e])] == (("me0", "me0/x0/1"), ("x0", "x0/me0/1"))


@MEMBERS
@LFA
def test_deletes_between_updates(members, lfa):
    """z0 cut off while r00-r01 changes its metric: at most me a DELETE (no
    records) sits between UPDATEs in one list; then z0 back: updates only."""
    dbs = world()
    names = sorted(dbs)
    z = names.index("z0")
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)

        def down():
            adj(dbs, "z0", "r05").isOverloaded = True
            adj(dbs, "r00", "r01").metric = 7
            adj(dbs, "r01", "r00").metric = 7
            push(ls, dbs, "z0", "r00", "r01")

        def up():
            adj(dbs, "z0", "r05").isOverloaded = False
            push(ls, dbs, "z0")

        _g0, _g1, (lists, _tot, _ms, _payload, _info) = step(ls, dbs, down, lfa, members)
        mixed = 0
        for t in range(len(names)):
            ip = raw_update(ls, t)[0]
            kinds = [bool(v & DEL) for v in ip.tolist()]
            mixed += False in kinds and True in kinds[kinds.index(False):]
        assert mixed > 0, "no list has a delete behind an update"
        assert len(lists[z][1]) == len(names) - 1
        _g0, _g1, (lists, totals, _ms, payload, _info) = step(ls, dbs, up, lfa, members)
        assert totals[1] == 0 and totals[3] == 0 and len(payload[z][0]) == len(names) - 1


@MEMBERS
@LFA
def test_labels(members, lfa):
    """777's owner changes from b0 to a0 (a0 comes up); r12's label is
    withdrawn; r13 advertises a new one: at r13 itself an UPDATE with owner ==
    me and no records (POP_AND_LOOKUP)."""
    dbs = world()
    names = sorted(dbs)
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)
        adj(dbs, "a0", "r10").isOverloaded = True
        push(ls, dbs, "a0")
        old12 = dbs["r12"].nodeLabel

        def change():
            adj(dbs, "a0", "r10").isOverloaded = False
            dbs["r12"].nodeLabel = 0
            dbs["r13"].nodeLabel = 5000
            push(ls, dbs, "a0", "r12", "r13")

        _g0, _g1, (lists, _tot, _ms, payload, _info) = step(ls, dbs, change, lfa, members)
        me, r13 = names.index("me0"), names.index("r13")
        assert payload[me][1][SHARED][0] == names.index("a0") and len(payload[me][1][SHARED][1]) > 0
        assert old12 in lists[me][3] and payload[me][1][5000][0] == r13
        own, rec = payload[r13][1][5000]
        assert own == r13 and len(rec) == 0
        (entry,) = [e for e in ls.allSourcesDecisionRouteUpdate(r13)[2] if e.label == 5000]
        assert [nh.mplsAction.action for nh in entry.nexthops] == ["POP_AND_LOOKUP"]


@MEMBERS
def test_two_tiles(members):
    """1,100 sets: updates on both sides of set 1,024 (z0 alone in sets 1023,
    1024 and 1099 comes up), the second tile's offsets and the header's stride."""
    dbs = world()
    names = sorted(dbs)
    sp, sn, sets = tile_sets(names)
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)
        adj(dbs, "z0", "r05").isOverloaded = True
        push(ls, dbs, "z0")

        def change():
            adj(dbs, "z0", "r05").isOverloaded = False
            adj(dbs, "r00", "r01").metric = 7
            adj(dbs, "r01", "r00").metric = 7
            push(ls, dbs, "z0", "r00", "r01")

        some = [names.index(s) for s in ("a0", "me0", "r10", "r15", "w0", "z0")]
        _g0, _g1, (lists, _tot, _ms, payload, _info) = step(ls, dbs, change, False, members, sets=(sp, sn),
                                                          set_lists=sets, solver_mes=some)
        me = names.index("r15")
        assert all(p in lists[me][0] and len(payload[me][0][p]) > 0 for p in (1023, 1024, 1099))
        assert any(p < 1023 for p in lists[me][0])


def many_next_hops():
    """a / b / c hold 300 / 64 / 65 equal-metric parallel links to x; d1 and d2
    hang off x."""
    links = [("a", "x")] * 300 + [("b", "x")] * 64 + [("c", "x")] * 65 + [("x", "d1"), ("x", "d2")]
    names = sorted({u for u, _ in links} | {v for _, v in links})
    adjs = {n: [] for n in names}
    seen = {}
    for i, (u, v) in enumerate(links):
        k = seen.get((u, v), 0)
        seen[(u, v)] = k + 1
        adjs[u].append(create_adjacency(v, f"{u}/{v}/{k}", f"{v}/{u}/{k}", f"fe80::{i + 1:x}",
                                        f"10.{i >> 8}.{i & 255}.1", 2, 0))
        adjs[v].append(create_adjacency(u, f"{v}/{u}/{k}", f"{u}/{v}/{k}", f"fe80::1:{i + 1:x}",
                                        f"10.{i >> 8}.{i & 255}.2", 2, 0))
    return {n: create_adj_db(n, adjs[n], 100 + i) for i, n in enumerate(names)}


@MEMBERS
def test_many_next_hops(members):
    """Routes of 300 / 64 / 65 records: past a lane group, a wave and beyond,
    past a 256-thread block.  x's link to d1 changes its metric."""
    dbs = many_next_hops()
    names = sorted(dbs)
    d1 = names.index("d1")
    with LinkState(devices=[0] * members) as ls:
        push(ls, dbs, *names)

        def change():
            adj(dbs, "x", "d1").metric = 5
            adj(dbs, "d1", "x").metric = 5
            push(ls, dbs, "x", "d1")

        _g0, _g1, (lists, _tot, _ms, payload, _info) = step(ls, dbs, change, False, members)
        for node, want in (("a", 300), ("b", 64), ("c", 65)):
            t = names.index(node)
            assert lists[t][0] == [d1] and len(payload[t][0][d1]) == want
            assert len(payload[t][1][100 + d1][1]) == want
            assert len(ls.allSourcesDecisionRouteUpdate(t)[0][d1]) == want


def test_scan_crosses_a_tile():
    """fabric1000 (960 nodes, one member), one spine switch overloaded: more
    than one 2,048-entry scan tile of IP entries, not a multiple of 256; 16
    seeded me in full, the totals over every me against the headers' counts of
    the listed routes."""
    topo = T.fabric(1000, full=True)
    rank = {s: i for i, s in enumerate(sorted(topo.nodes))}
    topo.lsdb.dbs["node_label"] = np.array([rank[s] + 1 for s in topo.nodes], np.int32)
    from openr_amd.wire import unpack

    dbs = {d.thisNodeName: d for d in unpack(topo.lsdb)}
    names = sorted(dbs)
    n = len(names)
    spine = next(s for s in names if s.startswith("1-"))
    rng = np.random.default_rng(5)
    fsw = [t for t, s in enumerate(names) if s.startswith("2-")]
    sample = sorted(set(rng.choice(n, 12, replace=False).tolist()) | set(fsw[:4]))[:16]
    with LinkState(devices=[0]) as ls:
        ls.updateAdjacencyDatabases(topo.lsdb)
        sets = single_sets(n)
        Gen(ls, sets, False, sample=[])
        snap = ls.allSourcesRouteSnapshot()
        dbs[spine].isOverloaded = True
        push(ls, dbs, spine)
        g1 = Gen(ls, sets, False, sample=sample)
        upd = ls.allSourcesRouteUpdate(snap)
        lists, totals, _ms, _payload, info = upd
        entries = totals[0] + totals[1]
        assert entries > 2048 and entries % 256 != 0, entries
        by_value(ls, g1, upd, 1, every=False)
        assert any(lists[t][0] for t in sample)
        # every me: the records its listed routes hold in generation 1
        mp, want_ip, want_lb = plan(ls), 0, 0
        group = {int(lab): g for g, lab in enumerate(g1.labels.tolist())}
        for t, (up, _dele, lup, _ldel) in enumerate(lists):
            if up:
                hdr = np.zeros(n, np.uint64)
                N.raise_for(N.lib.spf_mplan_route_db(mp, t, N.ptr(hdr, C.c_uint64), None, 0, None),
                            N.global_error())
                want_ip += int(((hdr[up] >> np.uint64(32)) & np.uint64(0xFFFF)).sum())
            if lup:
                ptr = np.zeros(len(group) + 1, np.uint64)
                N.raise_for(N.lib.spf_mplan_label_route_db(mp, t, None, N.ptr(ptr, C.c_uint64), None, 0, None),
                            N.global_error())
                want_lb += sum(int(ptr[group[l] + 1] - ptr[group[l]]) for l in lup)
        assert info["totals"] == [totals[0], want_ip, totals[2], want_lb]
        snap.close()


def test_contract():
    dbs = world()
    names = sorted(dbs)
    n = len(names)
    sets = single_sets(n)

    def status(fn):
        with pytest.raises(N.SpfError) as ei:
            fn()
        return ei.value.status

    def update(ls):
        N.raise_for(N.lib.spf_mplan_route_update(plan(ls), None, None, None), N.global_error())

    with LinkState(devices=[0, 0]) as ls:
        push(ls, dbs, *names)
        Gen(ls, sets, False, sample=[])
        assert status(lambda: update(ls)) == N.SPF_E_STATE  # no delta yet
        snap = ls.allSourcesRouteSnapshot()
        adj(dbs, "r00", "r01").metric = 7
        adj(dbs, "r01", "r00").metric = 7
        push(ls, dbs, "r00", "r01")
        Gen(ls, sets, False, sample=[])
        ls.allSourcesRouteDelta(snap)
        assert status(lambda: raw_update(ls, 0)) == N.SPF_E_STATE  # a delta, no update of it
        update(ls)
        first = [raw_update(ls, t) for t in range(n)]
        assert sum(len(f[2]) for f in first) > 0 and sum(len(f[6]) for f in first) > 0
        update(ls)  # a second call: identical arrays
        for t in range(n):
            assert all(np.array_equal(a, b) for a, b in zip(first[t], raw_update(ls, t)))
        # a cap one short
        t = next(t for t in range(n) if len(first[t][2]) and len(first[t][6]))
        rec = np.zeros(len(first[t][2]), np.uint64)
        lrec = np.zeros(len(first[t][6]), np.uint64)
        assert status(lambda: N.raise_for(N.lib.spf_mplan_route_update_db(
            plan(ls), t, None, N.ptr(rec, C.c_uint64), len(rec) - 1, None, None, None, None, 0, None),
            N.global_error())) == N.SPF_E_NOMEM
        assert status(lambda: N.raise_for(N.lib.spf_mplan_route_update_db(
            plan(ls), t, None, None, 0, None, None, None, N.ptr(lrec, C.c_uint64), len(lrec) - 1, None),
            N.global_error())) == N.SPF_E_NOMEM
        # the databases replaced behind the delta's back
        ls.allSourcesRouteRecords(*sets, False)
        assert status(lambda: update(ls)) == N.SPF_E_STATE
        ls.allSourcesRouteDelta(snap)
        update(ls)
        ls.allSourcesLabelRoutes(False)
        assert status(lambda: update(ls)) == N.SPF_E_STATE
        ls.allSourcesRouteDelta(snap)
        update(ls)
        # ... or moved away by a snapshot
        ls.allSourcesRouteDelta(snap)
        snap2 = ls.allSourcesRouteSnapshot()
        assert status(lambda: update(ls)) == N.SPF_E_STATE
        snap2.close()
        # device-side consumers: a member with a me has every buffer
        Gen(ls, sets, False, sample=[])
        ls.allSourcesRouteUpdate(snap)
        for r in range(2):
            p = [C.c_void_p() for _ in range(5)]
            nr = [C.c_uint64(), C.c_uint64()]
            N.raise_for(N.lib.spf_mplan_route_update_buffers(plan(ls), r, *[C.byref(x) for x in p],
                                                             C.byref(nr[0]), C.byref(nr[1])), N.global_error())
            assert all(bool(x.value) for x in p)
        snap.close()
        # one me: the other member holds nothing of the delta; records only (the
        # label routes went with a snapshot): empty label outputs
        one = np.array([3], np.uint32)
        Gen(ls, sets, False, mes=one, sample=[])
        ls.allSourcesRouteSnapshot().close()
        ls.allSourcesRouteRecords(*sets, False, one)
        snap3 = ls.allSourcesRouteSnapshot()
        adj(dbs, "r00", "r01").metric = 9
        adj(dbs, "r01", "r00").metric = 9
        push(ls, dbs, "r00", "r01")
        ls.prefetchAllSources()
        ls.allSourcesRouteRecords(*sets, False, one)
        lists, totals, _ms, payload, info = ls.allSourcesRouteUpdate(snap3)
        assert len(lists) == 1 and totals[0] > 0 and info["totals"][2:] == [0, 0] and payload[0][1] == {}
        assert len(raw_update(ls, 0)[2]) == info["totals"][1] and len(raw_update(ls, 0)[6]) == 0
        held = []
        for r in range(2):
            p = [C.c_void_p() for _ in range(5)]
            N.raise_for(N.lib.spf_mplan_route_update_buffers(plan(ls), r, *[C.byref(x) for x in p], None, None),
                        N.global_error())
            assert len({bool(x.value) for x in p}) == 1
            held.append(bool(p[0].value))
        assert sorted(held) == [False, True]
        snap3.close()
