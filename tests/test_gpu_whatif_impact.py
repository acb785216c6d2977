"""What-if impact by destination on the MI355X (spf_whatif_by_node /
spf_whatif_by_set): the change and route lists transposed to key-major on the
device, and a summary per node / set.

In every case the change or route lists are pinned to the CPU oracle first, by
the checkers the list and route tests use; the GPU output is then compared
field for field with tests/whatif_impact.py's restatement over those lists.
"""

import ctypes as C

import numpy as np
import pytest

import whatif_impact as I
import whatif_lists as L
import whatif_routes as R
from openr_amd import _native as N
from openr_amd import topology as T
from test_gpu_whatif import SMALL, setup
from test_gpu_whatif_lists import check as check_lists
from test_gpu_whatif_routes import check_routes
from test_whatif_impact_host import line, ring

pytestmark = pytest.mark.gpu
NONE = I.NONE


def small(name):
    return next(make for n, make, _ in SMALL if n == name)()


def check_impact(imp, ptr, key, dist, nh, base_dist, base_nh):
    """A WhatIfImpact against the restatement over the lists it was built
    from; returns the expected summaries."""
    want, tptr, tfail, tent = I.impact(ptr, key, dist, nh, base_dist, base_nh)
    n_keys, total = len(base_dist), len(key)
    assert imp.n_keys == n_keys == len(imp.impact) and imp.n_entries == total == int(ptr[-1])
    for f in I.DTYPE.names:
        assert np.array_equal(imp.impact[f], want[f]), f
    assert not imp.impact["reserved"].any()
    assert int(imp.impact["n_changed"].astype(np.int64).sum()) == imp.n_entries
    assert imp.pool_bytes == 8 * (n_keys + 1) + 12 * total + 32 * n_keys
    assert np.array_equal(imp.ptr, tptr) and len(imp.fail) == len(imp.ent) == total
    # the device order of each key holds the restatement's pairs
    sf, se = I.in_key_order(imp.ptr, imp.fail, imp.ent)
    assert np.array_equal(sf, tfail) and np.array_equal(se, tent)
    # ent points at an entry of failure fail whose key is the key
    e, f, p = imp.ent.astype(np.int64), imp.fail.astype(np.int64), np.asarray(ptr).astype(np.int64)
    assert np.array_equal(np.asarray(key).astype(np.int64)[e], I.owners(imp.ptr))
    assert ((p[f] <= e) & (e < p[f + 1])).all()
    # of(key): sorted by failure, the same pairs as the device order
    rng = np.random.default_rng(3)
    busiest = np.argsort(-want["n_changed"].astype(np.int64))[:24]
    keys = np.unique(np.concatenate([busiest, rng.choice(n_keys, min(n_keys, 40), replace=False)])) \
        if n_keys else []
    for k in keys:
        lo, hi = int(tptr[k]), int(tptr[k + 1])
        gf, ge = imp.of(int(k))
        assert np.array_equal(gf, tfail[lo:hi]) and np.array_equal(ge, tent[lo:hi])
        assert sorted(zip(imp.fail[lo:hi].tolist(), imp.ent[lo:hi].tolist())) == list(zip(gf.tolist(), ge.tolist()))
    assert len(imp.timing()) == 3 and imp.kernel_ms == pytest.approx(sum(imp.timing()))
    return want


def by_node(ch):
    base_d, base_nh, W = ch.plan.base()
    imp = ch.by_node()
    assert imp.flavour == "node" and imp.n_keys == len(base_d)
    return imp, check_impact(imp, ch.ptr, ch.node, ch.dist, ch.nh, base_d, base_nh), (base_d, base_nh)


def by_set(rt):
    imp = rt.by_set()
    assert imp.flavour == "set" and imp.n_keys == rt.n_sets
    return imp, check_impact(imp, rt.ptr, rt.set, rt.min_metric, rt.nh, rt.base_metric, rt.base_nh)


EVERY = [f"rand{k}" for k in range(4)] + ["wan200", "grid12"]


@pytest.mark.parametrize("name", EVERY)
def test_every_failure_of_a_link_plan(name):
    ls, names, eng, orc, _ = setup(small(name))
    sets, at = R.case_sets(len(names), 0)
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, 0)
        imp, want, _ = by_node(ch)
        assert imp.n_entries == ch.n_entries > 0
        assert want["n_changed"][0] == 0  # the source is never listed
        simp, swant = by_set(rt)
        assert simp.n_entries == rt.n_entries > 0
        # never listed: the empty set, the set that holds the source; the loopback sets are the nodes
        assert swant["n_changed"][at["e"]] == swant["n_changed"][at["h"]] == 0
        assert swant["max_metric"][at["e"]] == I.U64_MAX and swant["max_metric"][at["h"]] == 0
        n = len(names)
        for f in I.DTYPE.names:
            assert np.array_equal(simp.impact[f][:n], imp.impact[f]), f
        # the engine's entry point takes either kind of list
        again = eng.whatif_impact(ch)
        assert again.flavour == "node" and np.array_equal(again.impact, imp.impact)
        assert eng.whatif_impact(rt).flavour == "set"


def links_of(plan, csr, pairs):
    """Plan indices of the links between the node pairs."""
    rp, col, lid = csr[0], csr[1], csr[3]
    ids = [next(int(lid[e]) for e in range(rp[u], rp[u + 1]) if col[e] == v) for u, v in pairs]
    where = {int(l): i for i, l in enumerate(plan.links)}
    return [where[l] for l in ids]


def test_line6_counts_the_links_before_a_node():
    ls, names, eng, orc, csr = setup(line(6))
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        imp, want, _ = by_node(ch)
        for k in range(6):
            x = imp.impact[k]
            assert x["n_changed"] == x["n_unreachable"] == x["n_metric"] == k
            assert x["max_metric"] == k and x["max_fail"] == NONE  # cut off never wins max_metric
            assert x["min_width"] == (1 if k else 0)
            assert sorted(imp.of(k)[0]) == sorted(links_of(ch.plan, csr, [(j, j + 1) for j in range(k)]))
        rt = ch.routes([[k] for k in range(6)] + [[4, 5], []])
        check_routes(ch.plan, ch, rt, [[k] for k in range(6)] + [[4, 5], []], 0)
        simp, swant = by_set(rt)
        assert list(simp.impact["n_unreachable"]) == [0, 1, 2, 3, 4, 5, 4, 0]


def test_ring7_detours_and_their_ties():
    ls, names, eng, orc, csr = setup(ring(7))
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        sizes = np.diff(ch.ptr.astype(np.int64))
        cold = links_of(ch.plan, csr, [(3, 4)])[0]
        assert sizes[cold] == 0 and (np.delete(sizes, cold) > 0).all()  # one cold failure inside
        imp, want, _ = by_node(ch)
        for k in range(1, 7):
            arc = [(j, j + 1) for j in range(k)] if k <= 3 else [((j + 1) % 7, j) for j in range(k, 7)]
            x = imp.impact[k]
            assert x["n_changed"] == x["n_metric"] == len(arc) and x["n_unreachable"] == 0
            assert x["max_metric"] == max(k, 7 - k) and x["min_width"] == 1
            assert x["max_fail"] == min(links_of(ch.plan, csr, arc))  # a tie of len(arc) failures


def test_ring8_far_node_only_narrows():
    ls, names, eng, orc, csr = setup(ring(8))
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        imp, want, (base_d, base_nh) = by_node(ch)
        x = imp.impact[4]
        assert I.popcount(base_nh)[4] == 2
        assert x["n_changed"] == 8 and x["n_metric"] == 0 and x["min_width"] == 1
        assert x["max_metric"] == base_d[4] == 4 and x["max_fail"] == NONE


def test_repeated_links_and_cold_failures_at_both_ends():
    """[cold, l, l, cold, cold, m, l, cold]: the binary search steps over runs
    of cold failures at the start, in the middle and at the end of the plan,
    and of the equal failures 1, 2 and 6 the first is named."""
    ls, names, eng, orc, _ = setup(small("rand0"))
    with eng.whatif_changes(0) as full:
        base_d, _, _ = full.plan.base()
        sizes = np.diff(full.ptr.astype(np.int64))
        cold = [int(l) for l, n in zip(full.plan.links, sizes) if n == 0]
        # l sends node v a longer way round; m is a failure that leaves v alone
        i, v = next((i, int(v)) for i in range(full.n_fail) for v, d in zip(*full.of(i)[:2])
                    if d != L.U64_MAX and d > base_d[v])
        j = next(j for j in range(full.n_fail) if j != i and sizes[j] and v not in full.of(j)[0])
        l, m = int(full.plan.links[i]), int(full.plan.links[j])
    assert len(cold) >= 4
    links = [cold[0], l, l, cold[1], cold[2], m, l, cold[3]]
    sets, at = R.case_sets(len(names), 0)
    with eng.whatif_changes(0, links) as ch:
        assert list(ch.plan.links) == links
        assert [bool(x) for x in np.diff(ch.ptr.astype(np.int64))] == [0, 1, 1, 0, 0, 1, 1, 0]
        check_lists(ls, names, orc, 0, ch.plan, ch)
        imp, want, _ = by_node(ch)
        named = imp.impact["max_fail"][imp.impact["max_fail"] != NONE]
        assert imp.impact["max_fail"][v] == 1 and 2 not in named and 6 not in named
        assert set(imp.fail.tolist()) == {1, 2, 5, 6}
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, 0)
        simp, swant = by_set(rt)
        assert set(simp.fail.tolist()) == {1, 2, 5, 6}


def test_more_than_one_word():
    """ba1500 from its hub, node "3" (6 words): the popcount runs over every
    word of a row, and the rows of a workgroup's 256 entries are read as one
    run of words."""
    ls, names, eng, orc, _ = setup(small("ba1500"))
    s = names.index("3")
    sets, at = R.case_sets(len(names), s)
    with eng.whatif_changes(s) as ch:
        assert ch.W >= 2 and ch.n_entries > 256
        rng = np.random.default_rng(1)
        pick = rng.choice(ch.n_fail, min(ch.n_fail, 400), replace=False)
        longest = np.argsort(-np.diff(ch.ptr.astype(np.int64)))[:12]
        idx = list(pick) + list(longest)
        check_lists(ls, names, orc, s, ch.plan, ch, idx)
        imp, want, (base_d, base_nh) = by_node(ch)
        # the words past the first decide some key's min_width: on them alone a key's
        # narrowest entry differs from its base, and word 0 alone gives another answer
        high = I.impact(ch.ptr, ch.node, ch.dist, ch.nh[:, 1:], base_d, base_nh[:, 1:])[0]
        assert (high["min_width"] != I.popcount(base_nh[:, 1:])).any()
        low = I.impact(ch.ptr, ch.node, ch.dist, ch.nh[:, :1], base_d, base_nh[:, :1])[0]
        assert (low["min_width"] != imp.impact["min_width"]).any()
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, s, idx)
        by_set(rt)


@pytest.mark.parametrize("kind", ["down", "drain"])
def test_node_plans(kind):
    import test_gpu_whatif_nodes as TN

    eng, names, exp, s, _ = TN.prepare(small("rand0"))
    sets, at = R.case_sets(len(names), s)
    with eng.whatif_node_changes(s, kind=kind) as ch:
        TN.check(exp, ch.plan, ch)
        imp, want, _ = by_node(ch)
        assert imp.n_entries > 0
        if kind == "down":  # a node that is down is cut off, and so is what hangs on it
            assert (imp.impact["n_unreachable"] > 0).any()
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, s)
        by_set(rt)


def test_set_plan_ending_in_the_empty_srlg():
    import test_gpu_whatif_sets as TS

    eng, ls, names, exp, dag, s, _ = TS.prepare(small("rand0"))
    sets, at = R.case_sets(len(names), s)
    srlgs = [dag.up[k: k + 3] for k in range(0, len(dag.up), 2)] + [[]]
    with eng.whatif_set_changes(s, srlgs) as ch:
        TS.check(exp, ch.plan, ch)
        assert ch.ptr[-1] == ch.ptr[-2]  # the empty SRLG moves nothing: a cold failure at the end
        imp, want, _ = by_node(ch)
        assert imp.n_entries > 0 and ch.n_fail - 1 not in imp.fail
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, s)
        by_set(rt)


def test_metric_plan_with_lowered_links():
    import test_gpu_whatif_metrics as TM
    import whatif_metrics as WM

    eng, names, exp, s, (rp, col, met, lid, ovl) = TM.prepare(small("rand0"))
    sets, at = R.case_sets(len(names), s)
    var = TM.all_variants(exp, WM.link_edges(rp, col, lid))[::2]
    changes = [(l, a, b) for _, l, a, b in var]
    assert any(k.startswith("lower") for k, _, _, _ in var)
    with eng.whatif_metric_changes(s, changes) as ch:
        TM.check(exp, ch, changes)
        imp, want, (base_d, _) = by_node(ch)
        # a node that only ever gets nearer: its metric moves, nobody makes it worse than the base
        x = imp.impact
        assert ((x["n_metric"] > 0) & (x["max_fail"] == NONE) & (x["max_metric"] == base_d)).any()
        assert not x["n_unreachable"].any()  # a metric change cuts nothing off
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, s)
        by_set(rt)


def test_link_plan_on_the_exact_path_zero_metrics():
    from test_gpu_exact import with_metrics, zero_frac

    topo = with_metrics(T.random_graph(40, 100, 75, max_metric=3, parallel_frac=0.2,
                                       overload_frac=0.1, link_overload_frac=0.05),
                        zero_frac(0.35), 2)
    ls, names, eng, orc, _ = setup(topo)
    sets, at = R.case_sets(len(names), 0)
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        imp, want, _ = by_node(ch)
        assert imp.n_entries > 0
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, 0)
        by_set(rt)


def test_link_plan_on_the_exact_path_u64_metrics():
    """Metrics of 2^30 .. 2^31: distances beyond 32 bits, so the 64-bit max is
    decided in its high word."""
    from test_gpu_exact import with_metrics

    topo = with_metrics(T.wan(30, 10, seed=4),
                        lambda m, rng: rng.integers(2 ** 30, 2 ** 31 - 1, len(m)), 5)
    ls, names, eng, orc, _ = setup(topo)
    assert eng.needs_dist64
    sets, at = R.case_sets(len(names), 0)
    with eng.whatif_changes(0) as ch:
        check_lists(ls, names, orc, 0, ch.plan, ch)
        imp, want, (base_d, _) = by_node(ch)
        x = imp.impact
        assert ((x["max_metric"] >= 2 ** 32) & (x["max_metric"] != I.U64_MAX) & (x["max_fail"] != NONE)).any()
        rt = ch.routes(sets)
        check_routes(ch.plan, ch, rt, sets, 0)
        by_set(rt)


def holds(plan, flavour):
    n = C.c_uint64()
    call = getattr(N.lib, f"spf_whatif_by_{flavour}_db")
    return call(plan._h, 0, None, None, 0, C.byref(n)) == N.SPF_OK


def call_of(plan, flavour):
    n = C.c_uint64(0xAB)
    st = getattr(N.lib, f"spf_whatif_by_{flavour}")(plan._h, C.byref(n), None, None, None)
    return st, n.value


def test_errors_and_lifecycle():
    ls, names, eng, orc, _ = setup(small("rand1"))
    n_nodes = len(names)
    plan = eng.whatif_plan(0)
    for flavour in ("node", "set"):
        assert call_of(plan, flavour) == (N.SPF_E_STATE, 0xAB)  # no lists yet
        assert not holds(plan, flavour)
    ch = plan.changes()
    assert call_of(plan, "set") == (N.SPF_E_STATE, 0xAB)  # by set before the routes
    k, tot, ms = C.c_uint32(), C.c_uint64(), (C.c_double * 3)()
    for flavour, which in (("node", 0), ("set", 1)):
        call = lambda name: getattr(N.lib, f"spf_whatif_by_{flavour}{name}")
        assert call("_read")(plan._h, None, None, None, None) == N.SPF_E_STATE
        assert call("_impact")(plan._h, None) == N.SPF_E_STATE
        assert call("_buffers")(plan._h, None, None, None, None, C.byref(k), None) == N.SPF_E_STATE
        assert N.lib.spf_whatif_impact_timing(plan._h, which, ms) == N.SPF_E_STATE
    assert N.lib.spf_whatif_impact_timing(plan._h, 2, ms) == N.SPF_E_INVALID
    sets, at = R.case_sets(n_nodes, 0)
    rt = ch.routes(sets)
    # the two calls are repeatable with equal results
    for make, flavour in ((ch.by_node, "node"), (rt.by_set, "set")):
        a, b = make(), make()
        assert a.n_entries == b.n_entries > 0 and np.array_equal(a.ptr, b.ptr)
        assert np.array_equal(a.impact, b.impact)
        for key in range(a.n_keys):
            for x, y in zip(a.of(key), b.of(key)):
                assert np.array_equal(x, y)
        # the device arrays
        bufs = [C.c_void_p() for _ in range(4)]
        call = lambda name: getattr(N.lib, f"spf_whatif_by_{flavour}{name}")
        assert call("_buffers")(plan._h, *[C.byref(x) for x in bufs], C.byref(k), C.byref(tot)) == N.SPF_OK
        assert all(x.value for x in bufs) and k.value == a.n_keys and tot.value == a.n_entries
        got = np.zeros(a.n_keys, I.DTYPE)
        assert call("_impact")(plan._h, C.c_void_p(got.ctypes.data)) == N.SPF_OK
        assert np.array_equal(got, a.impact)
        # a key's entries do not fit: the count comes back all the same
        key = int(np.argmax(a.impact["n_changed"]))
        m = int(a.impact["n_changed"][key])
        fails, n = np.zeros(m, np.uint32), C.c_uint64()
        assert call("_db")(plan._h, key, N.ptr(fails), None, m - 1, C.byref(n)) == N.SPF_E_NOMEM
        assert n.value == m
        assert call("_db")(plan._h, key, N.ptr(fails), None, m, C.byref(n)) == N.SPF_OK
        assert np.array_equal(fails, a.of(key)[0])
        assert call("_db")(plan._h, a.n_keys, None, None, 0, C.byref(n)) == N.SPF_E_INVALID
        assert holds(plan, flavour)
    # new route lists invalidate by set only
    rt = ch.routes(sets)
    assert holds(plan, "node") and not holds(plan, "set")
    assert holds(rt.by_set().plan, "set")
    # no sets: no entries and no keys
    none = ch.routes([]).by_set()
    assert none.n_entries == 0 and none.n_keys == 0 and list(none.ptr) == [0]
    assert none.pool_bytes == 8 and holds(plan, "node")
    with pytest.raises(N.SpfError) as e:
        none.of(0)
    assert e.value.status == N.SPF_E_INVALID
    # new change lists invalidate both
    assert holds(ch.routes(sets).by_set().plan, "set") and holds(plan, "node")
    ch2 = plan.changes()
    assert not holds(plan, "node") and not holds(plan, "set")
    assert np.array_equal(ch2.by_node().impact, a_node_impact(ch2))
    # lists without an entry: every summary is the base's
    cold = [int(l) for l, n in zip(plan.links, np.diff(ch2.ptr.astype(np.int64))) if n == 0]
    assert cold
    with eng.whatif_changes(0, cold[:3]) as quiet:
        assert quiet.n_entries == 0
        imp, want, (base_d, base_nh) = by_node(quiet)
        assert not imp.ptr.any() and np.array_equal(imp.impact["max_metric"], base_d)
        assert np.array_equal(imp.impact["min_width"], I.popcount(base_nh))
        assert (imp.impact["max_fail"] == NONE).all() and not imp.impact["n_changed"].any()
    # the graph moves on: the plan's lists describe another graph
    eng.set_metric([0], [7])
    for flavour in ("node", "set"):
        assert call_of(plan, flavour)[0] == N.SPF_E_STATE
        assert not holds(plan, flavour)
    with pytest.raises(N.SpfError) as e:
        ch2.by_node()
    assert e.value.status == N.SPF_E_STATE


def a_node_impact(ch):
    base_d, base_nh, _ = ch.plan.base()
    return I.impact(ch.ptr, ch.node, ch.dist, ch.nh, base_d, base_nh)[0]
