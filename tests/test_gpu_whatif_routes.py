"""What-if route impact on the MI355X (spf_whatif_routes): per failure the
destination sets of the source whose route (min metric over the members, OR of
the next hops of the members at the min) changes, with the new route.

Every change list is pinned to the CPU oracle first, by the checkers the list
tests use (whatif_lists.check_failure and the node / set / metric helpers);
the expected route lists are then tests/whatif_routes.py's restatement of the
selection over the base patched with those lists, compared entry for entry.
"""

import ctypes as C

import numpy as np
import pytest

import whatif_lists as L
import whatif_routes as R
from openr_amd import _native as N
from openr_amd import topology as T
from test_gpu_whatif import SMALL, setup
from test_gpu_whatif_lists import check as check_lists

pytestmark = pytest.mark.gpu


def small(name):
    return next(make for n, make, _ in SMALL if n == name)()


def check_routes(plan, ch, rt, sets, s, idx=None):
    """Failures idx (default: all) of a route list against the checker; the
    change lists are taken as right (the caller has pinned them).  Returns
    (base routes, {i: (ids, metric, words)})."""
    idx = range(plan.n_fail) if idx is None else [int(i) for i in idx]
    base_d, base_nh, W = plan.base()
    flat = R.flatten(sets)
    base = R.routes(base_d, base_nh, flat, s)
    assert rt.W == W and rt.n_sets == len(sets) and rt.n_fail == plan.n_fail
    assert np.array_equal(rt.base_metric, base[0]) and np.array_equal(rt.base_nh, base[1])
    assert int(rt.ptr[0]) == 0 and int(rt.ptr[-1]) == rt.n_entries == len(rt.set)
    assert (np.diff(rt.ptr.astype(np.int64)) >= 0).all()
    assert rt.pool_bytes == 8 * (rt.n_fail + 1) + rt.n_entries * (12 + 4 * W)
    seen = {}
    for i in idx:
        node, dist, nh = ch.of(i)
        want = R.expected(base_d, base_nh, node, dist, nh, flat, s, base)
        got = rt.of(i)
        assert len(got[0]) == int(rt.ptr[i + 1]) - int(rt.ptr[i])
        assert (np.diff(got[0].astype(np.int64)) > 0).all()  # ascending
        for g, w, what in zip(got, want, ("sets", "metrics", "words")):
            assert np.array_equal(g, w), (i, what)
        gone = got[1] == L.U64_MAX
        assert not got[2][gone].any()  # withdrawn: no words
        lo, hi = int(rt.ptr[i]), int(rt.ptr[i + 1])  # the device order holds the same entries
        assert sorted(rt.set[lo:hi]) == list(got[0])
        seen[i] = got
    return base, seen


EVERY = [f"rand{k}" for k in range(4)] + ["wan200", "grid12"]


@pytest.mark.parametrize("name", EVERY)
def test_every_failure_of_a_link_plan(name):
    ls, names, eng, orc, _ = setup(small(name))
    n = len(names)
    sets, at = R.case_sets(n, 0)
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        rt = ch.routes(sets)
        base, seen = check_routes(ch.plan, ch, rt, sets, 0)
        nh_only = metric = listed_c = False
        for i, (ids, m, w) in seen.items():
            # sets (a), one per node: the route list is the change list, relabelled
            node, dist, nh = ch.of(i)
            own = ids < n
            assert np.array_equal(ids[own], node) and np.array_equal(m[own], dist)
            assert np.array_equal(w[own], nh)
            assert at["e"] not in ids and at["h"] not in ids and 0 not in ids
            assert (at["f"] in ids) == (at["f"] + 1 in ids) == (at["b"] in ids)  # identical sets
            nh_only |= bool((m == base[0][ids]).any())
            metric |= bool((m != base[0][ids]).any())
            listed_c |= at["c"] in ids
        assert rt.n_entries >= ch.n_entries > 0
        if name == "rand0":  # (the oracle agrees: test_whatif_routes_host.py)
            assert nh_only  # a route whose metric stays and whose next hops change
            assert metric and listed_c
        assert len(rt.timing()) == 4 and rt.kernel_ms == pytest.approx(sum(rt.timing()))


def test_more_than_one_word():
    """ba1500 from its hub, node "3" (6 words): 400 seeded failures plus the
    12 longest lists -- the multi-word OR of both walks."""
    ls, names, eng, orc, _ = setup(small("ba1500"))
    s = names.index("3")
    sets, at = R.case_sets(len(names), s)
    with eng.whatif_changes(s) as ch:
        assert ch.W >= 2
        rng = np.random.default_rng(1)
        pick = rng.choice(ch.n_fail, min(ch.n_fail, 400), replace=False)
        longest = np.argsort(-np.diff(ch.ptr.astype(np.int64)))[:12]
        idx = list(pick) + list(longest)
        check_lists(ls, names, orc, s, ch.plan, ch, idx)
        rt = eng.whatif_routes(ch, sets)
        base, seen = check_routes(ch.plan, ch, rt, sets, s, idx)
        assert any((w[:, 1:] != base[1][ids][:, 1:]).any() for ids, m, w in seen.values())


@pytest.mark.parametrize("kind", ["down", "drain"])
def test_node_plans(kind):
    import test_gpu_whatif_nodes as TN

    eng, names, exp, s, _ = TN.prepare(small("rand0"))
    sets, at = R.case_sets(len(names), s)
    with eng.whatif_node_changes(s, kind=kind) as ch:
        TN.check(exp, ch.plan, ch)
        rt = ch.routes(sets)
        base, seen = check_routes(ch.plan, ch, rt, sets, s)
        assert rt.n_entries > 0
        if kind == "down":  # the failed node's own route is withdrawn
            assert any((m == L.U64_MAX).any() for ids, m, w in seen.values())


def test_set_plan():
    import test_gpu_whatif_sets as TS

    eng, ls, names, exp, dag, s, _ = TS.prepare(small("rand0"))
    sets, at = R.case_sets(len(names), s)
    srlgs = [dag.up[k: k + 3] for k in range(0, len(dag.up), 2)] + [[]]
    with eng.whatif_set_changes(s, srlgs) as ch:
        TS.check(exp, ch.plan, ch)
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, s)
        assert rt.n_entries > 0 and rt.ptr[-1] == rt.ptr[-2]  # the empty SRLG moves nothing


def test_metric_plan_with_lowered_links():
    import test_gpu_whatif_metrics as TM
    import whatif_metrics as WM

    eng, names, exp, s, (rp, col, met, lid, ovl) = TM.prepare(small("rand0"))
    sets, at = R.case_sets(len(names), s)
    var = TM.all_variants(exp, WM.link_edges(rp, col, lid))[::2]  # raise_x2, lower_to_1 and keep of every link
    changes = [(l, a, b) for _, l, a, b in var]
    assert any(k.startswith("lower") for k, _, _, _ in var)
    with eng.whatif_metric_changes(s, changes) as ch:
        TM.check(exp, ch, changes)
        rt = ch.routes(sets)
        base, seen = check_routes(ch.plan, ch, rt, sets, s)
        # metrics fall under a lowered link, so a set's min can fall
        assert any((m < base[0][ids]).any() for ids, m, w in seen.values())
        assert not (rt.min_metric == L.U64_MAX).any()  # a metric change withdraws nothing


def test_link_plan_on_the_exact_path():
    from test_gpu_exact import with_metrics, zero_frac

    topo = with_metrics(T.random_graph(40, 100, 75, max_metric=3, parallel_frac=0.2,
                                       overload_frac=0.1, link_overload_frac=0.05),
                        zero_frac(0.35), 2)
    ls, names, eng, orc, _ = setup(topo)
    sets, at = R.case_sets(len(names), 0)
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, 0)
        assert rt.n_entries > 0


def test_line6_withdraws_exactly_the_tails():
    nodes = [f"n{i}" for i in range(6)]
    topo = T._undirected_to_adj(nodes, [(i, i + 1) for i in range(5)], np.ones(5), np.ones(5),
                                "line6")
    ls, names, eng, orc, (rp, col, met, lid, ovl) = setup(topo)
    assert names == nodes
    sets = [[a] for a in range(6)] + [[a, b] for a in range(1, 6) for b in range(a + 1, 6)]
    sets += [[5, 4, 3, 2, 1, 5, 4, 3, 2, 1], []]
    plan = eng.whatif_plan(0)
    ch = plan.changes()
    check_lists(ls, names, orc, 0, plan, ch)
    rt = eng.whatif_routes(ch, sets)
    base, seen = check_routes(plan, ch, rt, sets, 0)
    for i, l in enumerate(plan.links):
        ends = sorted(u for u in range(6) for e in range(rp[u], rp[u + 1]) if lid[e] == l)
        ids, m, w = seen[i]
        assert list(ids) == [k for k, mem in enumerate(sets) if mem and min(mem) >= ends[1]]
        assert len(ids) > 0 and (m == L.U64_MAX).all() and not w.any()


def routes_call(plan, ptr, nodes, n_sets):
    ptr, nodes = np.asarray(ptr, np.uint32), np.asarray(nodes, np.uint32)
    n = C.c_uint64(0xAB)
    st = N.lib.spf_whatif_routes(plan._h, N.ptr(ptr), N.ptr(nodes) if len(nodes) else None, n_sets,
                                 C.byref(n), None, None, None)
    return st, n.value


def holds_routes(plan):
    n = C.c_uint64()
    return N.lib.spf_whatif_routes_db(plan._h, 0, None, None, None, 0, C.byref(n)) == N.SPF_OK


def test_errors_and_lifecycle():
    ls, names, eng, orc, _ = setup(small("rand1"))
    n_nodes = len(names)
    plan = eng.whatif_plan(0)
    assert routes_call(plan, [0, 1], [1], 1) == (N.SPF_E_STATE, 0xAB)  # no lists yet
    ch = plan.changes()
    assert not holds_routes(plan)  # _db before a successful call
    assert N.lib.spf_whatif_routes_read(plan._h, None, None, None, None) == N.SPF_E_STATE
    assert N.lib.spf_whatif_routes_base(plan._h, None, None) == N.SPF_E_STATE
    w = C.c_uint32()
    assert N.lib.spf_whatif_routes_buffers(plan._h, None, None, None, None, C.byref(w),
                                           None) == N.SPF_E_STATE
    sets, at = R.case_sets(n_nodes, 0)
    a, b = ch.routes(sets), ch.routes(sets)
    assert a.n_entries == b.n_entries > 0 and np.array_equal(a.ptr, b.ptr)
    for i in range(plan.n_fail):
        for x, y in zip(a.of(i), b.of(i)):
            assert np.array_equal(x, y)
    # the device arrays
    bufs = [C.c_void_p() for _ in range(4)]
    tot = C.c_uint64()
    assert N.lib.spf_whatif_routes_buffers(plan._h, *[C.byref(x) for x in bufs], C.byref(w),
                                           C.byref(tot)) == N.SPF_OK
    assert all(x.value for x in bufs) and w.value == a.W and tot.value == a.n_entries
    # a failure's entries do not fit: the count comes back all the same
    i = int(np.argmax(np.diff(a.ptr.astype(np.int64))))
    m = int(a.ptr[i + 1] - a.ptr[i])
    got, n = np.zeros(m, np.uint32), C.c_uint64()
    st = N.lib.spf_whatif_routes_db(plan._h, i, N.ptr(got), None, None, m - 1, C.byref(n))
    assert st == N.SPF_E_NOMEM and n.value == m
    assert N.lib.spf_whatif_routes_db(plan._h, plan.n_fail, None, None, None, 0,
                                      C.byref(n)) == N.SPF_E_INVALID
    # a second call with other sets replaces the first
    other = [[v for v in range(1, n_nodes)][::3], [2, 1], [5]]
    rt = ch.routes(other)
    assert rt.n_sets == 3 and len(rt.base_metric) == 3
    check_routes(plan, ch, rt, other, 0)
    assert N.lib.spf_whatif_routes_buffers(plan._h, None, None, None, None, None,
                                           C.byref(tot)) == N.SPF_OK
    assert tot.value == rt.n_entries
    # no sets: no entries
    none = ch.routes([])
    assert none.n_entries == 0 and not none.ptr.any() and len(none.ptr) == plan.n_fail + 1
    assert none.pool_bytes == 8 * (plan.n_fail + 1) and none.base_metric.shape == (0,)
    assert holds_routes(plan)
    # refused sets leave no route lists behind
    for ptr, nodes, k in (([1, 2], [1, 2], 1), ([0, 2, 1], [1, 2], 2), ([0, 1], [n_nodes], 1)):
        assert holds_routes(ch.routes([[1]]).plan)
        assert routes_call(plan, ptr, nodes, k) == (N.SPF_E_INVALID, 0xAB)
        assert not holds_routes(plan)
    assert N.lib.spf_whatif_routes(plan._h, None, None, 1, None, None, None, None) == N.SPF_E_INVALID
    # new change lists invalidate the route lists
    assert holds_routes(ch.routes(sets).plan)
    ch2 = plan.changes()
    assert not holds_routes(plan)
    rt = ch2.routes(sets)
    assert np.array_equal(rt.ptr, a.ptr)
    # the graph moves on: the plan's lists describe another graph
    eng.set_metric([0], [7])
    with pytest.raises(N.SpfError) as e:
        ch2.routes(sets)
    assert e.value.status == N.SPF_E_STATE
    assert not holds_routes(plan)
