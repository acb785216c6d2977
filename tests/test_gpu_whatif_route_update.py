"""spf_whatif_route_update on the device: every failure's update list equals
the numpy checker (tests/whatif_route_update.py, pinned to the oracle by
test_whatif_route_update_host.py) fed with that failure's own change list, and
for the failures that touch the source's row and a hundred seeded others per
kind also ground truth that passes through no what-if code: a second engine
loaded with the same arrays and the failure applied in place (a removed link
becomes dead self-loop slots of metric 1, so CSR slots keep their positions),
spf_routes there against spf_routes on the unfailed engine.

Every case here has source 0, a row of at most 44 live slots and no overloaded
node; test_gpu_whatif_route_update_edges.py takes the same Bench to the other
sources, rows and graphs."""

import ctypes as C

import numpy as np
import pytest

import whatif_route_update as U
import whatif_routes as R
from openr_amd import _native as N
from openr_amd.engine import SpfEngine

pytestmark = pytest.mark.gpu

KINDS = ("link", "down", "drain", "set", "metric")


def make_plan(eng, s, kind, fails):
    if kind == "link":
        return eng.whatif_plan(s, [f[1] for f in fails])
    if kind in ("down", "drain"):
        return eng.whatif_node_plan(s, [f[1] for f in fails], kind)
    if kind == "set":
        return eng.whatif_set_plan(s, [list(f[1]) for f in fails])
    return eng.whatif_metric_plan(s, [list(f[1:]) for f in fails])


def link_slots(g):
    out = {}
    for a in range(len(g.rp) - 1):
        for e in range(int(g.rp[a]), int(g.rp[a + 1])):
            if int(g.col[e]) != a:
                out.setdefault(int(g.lid[e]), {})[a] = e
    return out


def failed_arrays(g, fail, slots):
    """The CSR with `fail` applied in place."""
    rows = np.repeat(np.arange(len(g.rp) - 1), np.diff(g.rp))
    col, met, ovl = np.array(g.col).copy(), np.array(g.met).copy(), np.array(g.ovl).copy()
    dead = np.zeros(len(col), bool)
    if fail[0] == "link":
        dead = np.asarray(g.lid) == fail[1]
    elif fail[0] == "set":
        dead = np.isin(np.asarray(g.lid), np.asarray(list(fail[1]), np.int64))
    elif fail[0] == "down":
        dead = (rows == fail[1]) | (col == fail[1])
    elif fail[0] == "drain":
        ovl[fail[1]] = 1
    else:
        _, l, m_lo, m_hi = fail
        ends = slots.get(int(l), {})  # a link that is not up has no slot
        for a, m in zip(sorted(ends), (m_lo, m_hi)):
            if m != U.KEEP:
                met[ends[a]] = m
    dead &= rows != col
    col[dead] = rows[dead]
    met[dead] = 1
    return g.rp, col, met, g.lid, ovl


def native_routes(eng, s, flat, deg):
    """spf_routes(s, sets): (min_metric[n], [records of each set] in slot order)."""
    ptr, nodes = (np.ascontiguousarray(x, np.uint32) for x in flat)
    n = len(ptr) - 1
    mm, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    edge, met = np.zeros(max(1, n * deg), np.uint32), np.zeros(max(1, n * deg), np.uint64)
    eng._err(N.lib.spf_routes(eng._h, s, N.ptr(ptr), N.ptr(nodes), n, 0, N.ptr(mm, C.c_uint64),
                              N.ptr(cnt), N.ptr(edge), N.ptr(met, C.c_uint64)))
    recs = []
    for k in range(n):
        e, m = edge[k * deg: k * deg + int(cnt[k])], met[k * deg: k * deg + int(cnt[k])]
        assert (m == mm[k]).all()
        recs.append(np.sort(e.astype(np.uint64) | (m << np.uint64(32))))
    return mm, recs


class Bench:
    """One graph on an engine, its sets, and a second engine for ground truth."""

    def __init__(self, g, s, sets):
        self.g, self.s, self.sets, self.flat = g, s, sets, R.flatten(sets)
        self.row = U.Row(g.rp, g.col, g.met, g.lid, s)
        self.deg = int(g.rp[s + 1] - g.rp[s])
        self.slots = link_slots(g)
        self.eng, self.truth = SpfEngine(0), SpfEngine(0)
        self.eng.load(g.rp, g.col, g.met, g.lid, g.ovl)
        self.truth_base = native_routes(self.eng, s, self.flat, self.deg)

    def close(self):
        self.eng.close()
        self.truth.close()

    def ground_truth(self, fail):
        self.truth.load(*failed_arrays(self.g, fail, self.slots))
        mm, recs = native_routes(self.truth, self.s, self.flat, self.deg)
        bm, brecs = self.truth_base
        ids = [k for k in range(len(mm)) if mm[k] != bm[k] or not np.array_equal(recs[k], brecs[k])]
        return np.array(ids, np.uint32), mm[ids], [recs[k] for k in ids]

    def run(self, kind, fails, truth_for):
        """The plan of `fails`: every failure against the checker, the failures
        `truth_for` against ground truth.  Returns (changes, routes, update,
        the update lists by failure)."""
        plan = make_plan(self.eng, self.s, kind, fails)
        ch = plan.changes()
        rt = ch.routes(self.sets)
        up = rt.update()
        base_d, base_nh, _ = plan.base()
        routes = R.routes(base_d, base_nh, self.flat, self.s)
        base_recs = U.base_records(self.row, base_d, base_nh, self.flat, routes)
        got_base = up.base()
        assert len(got_base) == len(base_recs)
        assert all(np.array_equal(a, b) for a, b in zip(got_base, base_recs))
        assert int(up.ptr[0]) == 0 and int(up.ptr[-1]) == up.n_entries == len(up.set)
        assert int(up.rec_ptr[0]) == 0 and int(up.rec_ptr[-1]) == up.n_records == len(up.rec)
        assert (np.diff(up.ptr.astype(np.int64)) >= 0).all()
        assert (np.diff(up.rec_ptr.astype(np.int64)) >= 0).all()
        assert up.pool_bytes == 8 * (len(fails) + 1) + 12 * up.n_entries + 8 * (up.n_entries + 1) + 8 * up.n_records
        lists = []
        for i, fail in enumerate(fails):
            a, b = int(ch.ptr[i]), int(ch.ptr[i + 1])
            want = U.expected(self.row, fail, base_d, base_nh, ch.node[a:b], ch.dist[a:b], ch.nh[a:b],
                              self.flat, routes)
            a, b = int(up.ptr[i]), int(up.ptr[i + 1])
            order = a + np.argsort(up.set[a:b], kind="stable")
            got = (up.set[order], up.min_metric[order],
                   [up.rec[int(up.rec_ptr[e]): int(up.rec_ptr[e + 1])] for e in order])
            assert U.same_lists(got, want), (kind, i, fail, got, want)
            lists.append(got)
        for i in truth_for:
            assert U.same_lists(lists[i], self.ground_truth(fails[i])), (kind, i, fails[i])
        assert up.n_touched == sum(self.row.touches(f) for f in fails)
        return ch, rt, up, lists


@pytest.fixture(scope="module")
def bundle():
    g = U.bundle_graph()
    b = Bench(g, 0, [[1], [2], [3], [4], [5], [6], [3, 5], [2, 6], [0, 3], []])
    yield b
    b.close()


def test_a_bundle_member_failure_is_seen_at_link_level_only(bundle):
    b, g = bundle, bundle.g
    links = g.up_links()
    fails = [("link", l) for l in links]
    ch, rt, up, lists = b.run("link", fails, range(len(fails)))
    w = {int(g.lid[e]): int(g.met[e]) for e in range(int(g.rp[0]), int(g.rp[1]))}
    members = [l for l in g.links_between(0, 1) if w[l] == 1]
    assert len(members) == 2
    via_n1 = [0, 2, 3, 4, 6]
    base = up.base()
    for l in members:
        i = links.index(l)
        assert ch.ptr[i] == ch.ptr[i + 1] and rt.ptr[i] == rt.ptr[i + 1]  # cold at node level
        ids, metric, recs = lists[i]
        assert list(ids) == via_n1
        assert list(metric) == [int(rt.base_metric[k]) for k in via_n1]
        for k, rec in zip(via_n1, recs):
            assert len(rec) == len(base[k]) - 1 and set(rec.tolist()) < set(base[k].tolist())
    # the calls of one failure: sorted by set id, the offsets from zero
    ids, metric, recs = up.of(links.index(members[0]))
    assert U.same_lists((ids, metric, recs), lists[links.index(members[0])])


def test_bundle_metric_changes_and_both_members(bundle):
    b, g = bundle, bundle.g
    w = {int(g.lid[e]): int(g.met[e]) for e in range(int(g.rp[0]), int(g.rp[1]))}
    eq = [l for l in g.links_between(0, 1) if w[l] == 1]
    heavy = next(l for l in g.links_between(0, 1) if w[l] == 3)
    fails = [("metric", eq[0], 2, 2), ("metric", heavy, 1, U.KEEP), ("metric", heavy, U.KEEP, 1),
             ("metric", eq[1], U.KEEP, U.KEEP), ("metric", eq[1], 1, 1), ("metric", heavy, 2, 2)]
    _, _, up, lists = b.run("metric", fails, range(len(fails)))
    base = up.base()
    assert [len(r) for r in lists[0][2]] == [len(base[k]) - 1 for k in lists[0][0]]
    assert [len(r) for r in lists[1][2]] == [len(base[k]) + 1 for k in lists[1][0]]
    assert all(len(lists[i][0]) == 0 for i in (2, 3, 4, 5))
    fails = [("set", eq), ("set", [eq[0]]), ("set", []), ("set", g.links_between(0, 1)),
             ("set", [int(g.lid[e]) for e in range(int(g.rp[0]), int(g.rp[1]))])]
    _, _, _, lists = b.run("set", fails, range(len(fails)))
    assert {int(k): (int(m), len(r)) for k, m, r in zip(*lists[0])} == {
        0: (3, 2), 2: (2, 1), 3: (3, 1), 4: (4, 2), 6: (2, 1)}
    assert (lists[4][1] == U.U64_MAX).all() and not any(len(r) for r in lists[4][2])


@pytest.mark.parametrize("kind", KINDS)
def test_forty_neighbours_two_words(kind):
    g = U.wide_graph()
    n = len(g.names)
    sweep = int(N.lib.spf_whatif_route_update_sweep_sets())
    # one set more than a workgroup of the sweep takes, the last one behind a bundle
    sets = [[1 + k % (n - 1)] for k in range(sweep - 2)] + [[32], [1, 33]] + [[1]]
    assert len(sets) == sweep + 1
    b = Bench(g, 0, sets)
    try:
        assert b.row.bit.max() == 39 and b.deg == 44
        links = g.up_links()
        bundles = [g.links_between(0, x) for x in (1, 18, 32, 33)]
        assert all(len(x) == 2 for x in bundles)
        fails = {
            "link": [("link", l) for l in links],
            "down": [("down", x) for x in range(1, n)],
            "drain": [("drain", x) for x in range(1, n)],
            "set": [("set", x) for x in bundles] + [("set", [x[0]]) for x in bundles] + [
                ("set", bundles[2] + bundles[3]), ("set", [bundles[2][1], bundles[3][0]]), ("set", [])],
            "metric": [("metric", x[k], lo, hi) for x in bundles for k in (0, 1)
                       for lo, hi in ((3, U.KEEP), (U.KEEP, 3), (1, 1), (2, 2))],
        }[kind]
        touching = [i for i, f in enumerate(fails) if b.row.touches(f)]
        rng = np.random.default_rng(2)
        some = set(touching) | set(int(i) for i in rng.choice(len(fails), min(30, len(fails)), replace=False))
        _, rt, up, lists = b.run(kind, fails, sorted(some))
        if kind in ("link", "set", "metric"):  # the last set is listed by the sweep's second round
            assert any(sweep in ids and sweep not in rt.of(i)[0]
                       for i, (ids, _, _) in enumerate(lists))
    finally:
        b.close()


@pytest.fixture(scope="module")
def multi():
    g = U.seeded_graph()
    sets, _ = R.case_sets(len(g.names), 0)
    b = Bench(g, 0, sets)
    yield b
    b.close()


def multi_failures(b, kind):
    g, rng = b.g, np.random.default_rng(7)
    links, n = g.up_links(), len(g.names)
    own = [int(g.lid[e]) for e in range(int(g.rp[0]), int(g.rp[1])) if int(g.col[e]) != 0]
    if kind == "link":
        return [("link", l) for l in links]
    if kind in ("down", "drain"):
        return [(kind, x) for x in range(1, n)]
    bundle = g.links_between(0, 2)  # two equal members and a heavier one
    assert len(bundle) >= 3
    if kind == "set":
        fails = [("set", bundle), ("set", bundle[: len(bundle) // 2]), ("set", own), ("set", [])]
        while len(fails) < 64:
            k = int(rng.integers(1, 6))
            pool = own if len(fails) % 3 == 0 else links
            fails.append(("set", sorted(int(l) for l in rng.choice(pool, min(k, len(pool)), replace=False))))
        return fails
    w = {int(g.lid[e]): int(g.met[e]) for e in range(int(g.rp[0]), int(g.rp[1]))}
    lightest = min(w[l] for l in bundle)
    tight = next(l for l in bundle if w[l] == lightest)
    heavier = next(l for l in bundle if w[l] > lightest)
    fails = [("metric", tight, U.KEEP, lightest + 1), ("metric", tight, lightest + 1, U.KEEP),
             ("metric", tight, lightest + 1, lightest + 1), ("metric", heavier, lightest, lightest),
             ("metric", heavier, 1, 9), ("metric", heavier, 2, U.KEEP), ("metric", heavier, 4, 4)]
    for l in own:
        fails += [("metric", l, m, m) for m in (1, 2, 5)]
    for l in rng.choice(links, 120, replace=False):
        fails.append(("metric", int(l), int(rng.integers(1, 6)), int(rng.integers(0, 6))))
    return fails


@pytest.mark.parametrize("kind", KINDS)
def test_seeded_multigraph(multi, kind):
    b = multi
    fails = multi_failures(b, kind)
    touching = [i for i, f in enumerate(fails) if b.row.touches(f)]
    rng = np.random.default_rng(5)
    others = rng.choice(len(fails), min(100, len(fails)), replace=False)
    ch, rt, up, lists = b.run(kind, fails, sorted(set(touching) | set(int(i) for i in others)))
    if kind != "drain":
        assert touching
    if kind == "link":
        extra = sum(len(set(ids.tolist()) - set(rt.of(i)[0].tolist())) for i, (ids, _, _) in enumerate(lists)
                    if i in touching)
        assert extra >= 20
        assert any(ch.ptr[i + 1] > ch.ptr[i] for i in touching)


def ring(n):
    links = [(i, (i + 1) % n) for i in range(n)]
    w = [1 + (i % 3 == 0) for i in range(n)]
    return U.Graph(U.topology(f"ring{n}", n, links, w, w))


def test_offsets_past_one_scan_tile():
    tile = int(N.lib.spf_whatif_scan_tile())
    g = ring(tile + 1)  # one link more than the scan takes per round
    n = len(g.names)
    sets = [[int(v)] for v in np.linspace(1, n - 1, 24).astype(int)] + [[n // 3, 2 * n // 3]]
    b = Bench(g, 0, sets)
    try:
        links = g.up_links()
        assert len(links) == tile + 1
        fails = [("link", l) for l in links]
        edge = {0, 1, tile - 1, tile}
        _, _, up, _ = b.run("link", fails, sorted(edge | set(range(0, tile, 997))))
        assert len(up.ptr) == tile + 2 and len(up.rec_ptr) > tile + 1  # both cross a tile
        size = np.diff(up.ptr.astype(np.int64))
        assert size[:tile].any() and size[tile:].any()
    finally:
        b.close()


def update_call(plan):
    n = C.c_uint64(0xAB)
    st = N.lib.spf_whatif_route_update(plan._h, C.byref(n), None, None, None, None)
    return st, n.value


def test_states(bundle):
    b, g = bundle, bundle.g
    sets = b.sets
    plan = b.eng.whatif_plan(0)
    assert update_call(plan) == (N.SPF_E_STATE, 0xAB)  # no lists at all
    ch = plan.changes()
    assert update_call(plan) == (N.SPF_E_STATE, 0xAB)  # no route lists
    rt = ch.routes(sets)
    by_set = rt.by_set()
    a, c = rt.update(), rt.update()
    assert a.n_entries == c.n_entries > 0 and a.pool_bytes == c.pool_bytes  # the pools did not grow
    for x, y in ((a.ptr, c.ptr), (a.rec_ptr, c.rec_ptr)):
        assert np.array_equal(x, y)
    for i in range(a.n_fail):
        assert U.same_lists(a.of(i), c.of(i))
    assert len(by_set.of(0)[0]) >= 0  # the transposition outlives an update
    assert len(c.timing()) == 7
    plan.changes()  # fresh change lists: the route lists and the updates are gone
    assert update_call(plan) == (N.SPF_E_STATE, 0xAB)
    assert N.lib.spf_whatif_route_update_read(plan._h, None, None, None, None, None) == N.SPF_E_STATE
    with pytest.raises(N.SpfError) as e:
        c.of(0)
    assert e.value.status == N.SPF_E_STATE
    # no sets
    empty = plan.changes().routes([]).update()
    assert empty.n_entries == 0 and empty.n_records == 0 and empty.base() == []
    assert not empty.ptr.any()
    # every failure cold: the links beyond n4 and n5 lead nowhere else; a drain of a leaf
    leaves = b.eng.whatif_node_plan(0, [4, 5, 6], "drain")
    cold = leaves.changes().routes(sets).update()
    assert cold.n_entries == 0 and cold.n_touched == 0 and len(cold.ptr) == 4
    # zero failures
    none = b.eng.whatif_set_plan(0, []).changes().routes(sets).update()
    assert none.n_entries == 0 and list(none.ptr) == [0]


def test_exact_path_plans_are_refused():
    g = U.bundle_graph()
    met = np.array(g.met).copy()
    met[int(g.rp[3])] = 0  # one zero metric: the exact path
    with SpfEngine(0) as eng:
        eng.load(g.rp, g.col, met, g.lid, g.ovl)
        plan = eng.whatif_plan(0)
        rt = plan.changes().routes([[1], [3]])
        assert rt.n_fail > 0
        assert update_call(plan) == (N.SPF_E_UNSUPPORTED, 0xAB)
        assert len(rt.of(0)) == 3  # the route lists stand
