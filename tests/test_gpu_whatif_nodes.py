"""What-if batches for node failures on the MI355X
(spf_whatif_plan_create_nodes): for every node x of a list, the SPF of one
source with x down (every link of x ignored) or drained (x overloaded), as
digests and as change lists.

The expected values come from tests/whatif_nodes.py: a full oracle re-run on
the changed LSDB per node, reduced against the unfailed run.  Lists are
checked with whatif_lists.check_failure: the plan's unfailed result patched
with a node's list must have that digest.
"""

import ctypes as C

import numpy as np
import pytest

import whatif_lists as L
import whatif_nodes as WN
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.link_state import LinkState
from test_gpu_whatif import SMALL, as_tuple, setup

pytestmark = pytest.mark.gpu


def small(name):
    return next(make for n, make, _ in SMALL if n == name)()


def prepare(topo, src=None):
    """src: a node name, or a function (names, rp, col, ovl) -> id; node 0
    when None."""
    ls, names, eng, orc, (rp, col, met, lid, ovl) = setup(topo)
    s = names.index(src) if isinstance(src, str) else int(src(names, rp, col, ovl) if src else 0)
    return eng, names, WN.Expected(topo.lsdb, names, rp, col, s), s, (rp, col, lid, ovl)


def check(exp, plan, ch, idx=None):
    """Failures idx (default: all) of a node plan's lists and digests against
    the helper; returns the expected digests."""
    idx = range(plan.n_fail) if idx is None else [int(i) for i in idx]
    base_d, base_nh, W = plan.base()
    assert W == ch.W == base_nh.shape[1]
    assert np.array_equal(base_d, exp.base[0]) and np.array_equal(base_nh, exp.base[1])
    assert as_tuple(ch.base_digest) == exp.base_digest
    assert int(ch.ptr[0]) == 0 and int(ch.ptr[-1]) == ch.n_entries
    want = {}
    for i in idx:
        x = int(plan.nodes[i])
        w = want[i] = exp.digest(x, plan.kind)
        node, dist, nh = ch.of(i)
        assert len(node) == int(ch.ptr[i + 1]) - int(ch.ptr[i])
        assert (np.diff(node.astype(np.int64)) > 0).all()  # ascending
        L.check_failure(base_d, base_nh, node, dist, nh, w, where=f"{plan.kind} node {x}")
        assert as_tuple(ch.digests[i]) == w, (plan.kind, x)
        if plan.kind == "drain":
            assert x not in node  # a drained node keeps its metric and next hops
        elif base_d[x] != L.U64_MAX:
            k = int(np.searchsorted(node, x))
            assert node[k] == x and dist[k] == L.U64_MAX and not nh[k].any()
    return want


WAVE = [f"rand{s}" for s in range(4)] + ["wan200"]


@pytest.mark.parametrize("kind", WN.KINDS)
@pytest.mark.parametrize("name", WAVE)
def test_wave_teams_every_node(name, kind):
    eng, names, exp, s, _ = prepare(small(name))
    nodes, digests, base = eng.whatif_nodes(s, kind=kind)
    assert list(nodes) == [v for v in range(len(names)) if v != s]
    assert as_tuple(base) == exp.base_digest
    with eng.whatif_node_changes(s, kind=kind) as ch:
        assert ch.plan.kind == kind and len(ch.plan.links) == 0
        assert list(ch.plan.nodes) == list(nodes) and ch.n_fail == len(nodes)
        want = check(exp, ch.plan, ch)
        assert [as_tuple(d) for d in digests] == [want[i] for i in range(len(nodes))]
        assert [as_tuple(d) for d in ch.digests] == [as_tuple(d) for d in digests]
        assert ch.pool_bytes == 8 * (ch.n_fail + 1) + ch.n_entries * (12 + 4 * ch.W)


def test_line6_tails():
    nodes = [f"n{i}" for i in range(6)]
    topo = T._undirected_to_adj(nodes, [(i, i + 1) for i in range(5)], np.ones(5), np.ones(5),
                                "line6")
    eng, names, exp, s, _ = prepare(topo)
    assert names == nodes
    with eng.whatif_node_changes(0, kind="down") as ch:
        assert list(ch.plan.nodes) == [1, 2, 3, 4, 5]
        check(exp, ch.plan, ch)
        for k, i in enumerate(ch.plan.nodes):
            node, dist, nh = ch.of(k)
            assert list(node) == list(range(int(i), 6))  # the node and its tail
            assert (dist == L.U64_MAX).all() and not nh.any()
    with eng.whatif_node_changes(0, kind="drain") as ch:
        check(exp, ch.plan, ch)
        for k, i in enumerate(ch.plan.nodes):
            node, dist, nh = ch.of(k)
            assert list(node) == list(range(int(i) + 1, 6))  # nothing for the last node
            assert (dist == L.U64_MAX).all() and not nh.any()


TEAMS = [("wavecap64", {"SPF_WHATIF_WAVECAP": "64"}),
         ("classify16", {"SPF_WHATIF_CLASSIFY": "16"}),
         ("classify16_one_workgroup", {"SPF_WHATIF_CLASSIFY": "16", "SPF_WHATIF_GROUP": "1"})]


@pytest.mark.parametrize("kind", WN.KINDS)
@pytest.mark.parametrize("env", [t[1] for t in TEAMS], ids=[t[0] for t in TEAMS])
def test_workgroup_and_group_teams(monkeypatch, env, kind):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng, names, exp, s, _ = prepare(small("grid12"))  # node 0: a corner
    plan = eng.whatif_node_plan(0, kind=kind)
    ch = plan.changes()
    assert plan.stats()[1] > 0  # big repairs
    check(exp, plan, ch)


@pytest.mark.parametrize("kind", WN.KINDS)
def test_more_than_one_word_and_wide_fans(kind):
    """ba1500 from the hub "3" (167 neighbours, W = 6): the 12 highest-degree
    nodes, the 12 longest lists and 150 seeded nodes."""
    eng, names, exp, s, (rp, col, lid, ovl) = prepare(small("ba1500"), "3")
    with eng.whatif_node_changes(s, kind=kind) as ch:
        assert ch.W == L.words_of(len(L.neighbours(rp, col, s))) == 6
        nodes = ch.plan.nodes.astype(np.int64)
        deg = np.diff(rp.astype(np.int64))[nodes]
        rng = np.random.default_rng(1)
        pick = list(np.argsort(-deg)[:12]) + \
            list(np.argsort(-np.diff(ch.ptr.astype(np.int64)))[:12]) + \
            list(rng.choice(ch.n_fail, 150, replace=False))
        nbrs = set(L.neighbours(rp, col, s))
        assert any(int(nodes[i]) in nbrs for i in pick)  # a failed neighbour of the source
        check(exp, ch.plan, ch, pick)


def edge_topo():
    return T.random_graph(50, 120, 17, max_metric=4, overload_frac=0.2)


@pytest.mark.parametrize("kind", WN.KINDS)
def test_drained_source(kind):
    first_drained = lambda names, rp, col, ovl: np.nonzero(ovl)[0][0]  # noqa: E731
    eng, names, exp, s, (rp, col, lid, ovl) = prepare(edge_topo(), first_drained)
    assert ovl[s]  # a drained node still expands as the source
    with eng.whatif_node_changes(s, kind=kind) as ch:
        check(exp, ch.plan, ch)
        assert ch.n_entries > 0


def test_node_drained_in_the_base():
    first_up = lambda names, rp, col, ovl: np.nonzero(ovl == 0)[0][0]  # noqa: E731
    eng, names, exp, s, (rp, col, lid, ovl) = prepare(edge_topo(), first_up)
    assert not ovl[s]
    xs = [int(v) for v in np.nonzero(ovl)[0] if exp.base[0][v] != L.U64_MAX]
    assert xs
    with eng.whatif_node_changes(s, xs, kind="down") as ch:
        check(exp, ch.plan, ch)
        assert ch.plan.stats()[0] == len(xs)  # every one hot
        for k, x in enumerate(xs):
            node, dist, nh = ch.of(k)
            assert list(node) == [x]  # a drained node has no DAG children: D = {x}
    with eng.whatif_node_changes(s, xs, kind="drain") as ch:
        check(exp, ch.plan, ch)
        assert ch.plan.stats() == (0, 0) and ch.n_entries == 0  # cold
        assert all(as_tuple(d) == exp.base_digest for d in ch.digests)


@pytest.mark.parametrize("kind", WN.KINDS)
def test_node_unreachable_in_the_base(kind):
    """Every neighbour of v drained (none of them the source): v is recorded
    by nobody, and failing it is cold."""
    topo = edge_topo()
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names0, rp, col, met, lid, ovl = ls.flatten()
    s = int(np.nonzero(ovl == 0)[0][0])
    v = next(v for v in range(len(names0)) if v != s and rp[v + 1] > rp[v]
             and s not in col[rp[v]: rp[v + 1]])
    for u in set(int(c) for c in col[rp[v]: rp[v + 1]]):
        topo.lsdb.dbs["is_overloaded"][WN.db_index(topo.lsdb, names0[u])] = 1
    eng, names, exp, s, _ = prepare(topo, names0[s])
    v = names.index(names0[v])
    assert exp.base[0][v] == L.U64_MAX
    with eng.whatif_node_changes(s, [v], kind=kind) as ch:
        check(exp, ch.plan, ch)
        assert ch.plan.stats() == (0, 0) and ch.n_entries == 0
        assert as_tuple(ch.digests[0]) == exp.base_digest
    with eng.whatif_node_changes(s, kind=kind) as ch:  # and every node of that graph
        check(exp, ch.plan, ch)


def test_lollipop_only_neighbour_down():
    nodes = [f"p{i}" for i in range(6)]
    links = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 2)]
    topo = T._undirected_to_adj(nodes, links, np.arange(1, 7), np.arange(2, 8), "lollipop")
    eng, names, exp, s, _ = prepare(topo)
    with eng.whatif_node_changes(0, [1], kind="down") as ch:
        check(exp, ch.plan, ch)
        node, dist, nh = ch.of(0)
        assert list(node) == [1, 2, 3, 4, 5] and (dist == L.U64_MAX).all()
        assert as_tuple(ch.digests[0])[:2] == (5, 5)
    for kind in WN.KINDS:
        with eng.whatif_node_changes(0, kind=kind) as ch:
            check(exp, ch.plan, ch)


def test_patched_distances_equal_single_source_runs():
    """Round the oracle: x down = every link of x's CSR row ignored."""
    eng, names, exp, s, (rp, col, lid, ovl) = prepare(small("rand0"))
    with eng.whatif_node_changes(0, kind="down") as ch:
        base_d, base_nh, _ = ch.plan.base()
        for i, x in enumerate(ch.plan.nodes):
            node, dist, nh = ch.of(i)
            d, _ = L.patched(base_d, base_nh, node, dist, nh)
            ign = sorted(set(int(l) for l in lid[rp[x]: rp[x + 1]]))
            want = eng.sssp(0, ignore_links=ign).astype(np.uint64)
            want[want == 0xFFFFFFFF] = L.U64_MAX
            assert np.array_equal(d, want), (i, int(x))


@pytest.mark.parametrize("kind", WN.KINDS)
def test_explicit_lists_keep_their_order(kind):
    eng, names, exp, s, _ = prepare(small("rand0"))
    nodes, digests, base = eng.whatif_nodes(0, kind=kind)
    cold = [int(x) for x, d in zip(nodes, digests) if as_tuple(d) == as_tuple(base)]
    hot = [int(x) for x, d in zip(nodes, digests) if as_tuple(d) != as_tuple(base)]
    assert len(hot) >= 3
    if kind == "drain":
        assert len(cold) >= 3  # leaves and drained nodes
    mixed = [hot[2]] + cold[:1] + [hot[0]] + cold[1:3] + [hot[1], hot[2]]  # scrambled, one repeat
    with eng.whatif_node_changes(0, mixed, kind=kind) as ch:
        assert list(ch.plan.nodes) == mixed  # the order is kept
        sizes = np.diff(ch.ptr.astype(np.int64))
        assert [bool(n) for n in sizes] == [x in hot for x in mixed]  # empty exactly on cold
        check(exp, ch.plan, ch)
        for a, b in zip(ch.of(0), ch.of(len(mixed) - 1)):
            assert np.array_equal(a, b)  # the repeat
        assert as_tuple(ch.digests[0]) == as_tuple(ch.digests[-1])


def test_wide_metrics_sweep_fallback():
    """U[1, 1000] metrics on a 3000-node WAN: the largest repairs hold more
    than kDialLevels (1024) distinct distances and leave the Dial loop for the
    label-correcting sweeps and the level sort."""
    eng, names, exp, s, _ = prepare(T.wan(3000, 1500, seed=2))
    with eng.whatif_node_changes(0, kind="down") as ch:
        size = ch.digests["n_dist_changed"].astype(np.int64)
        assert size.max() > 1024
        rng = np.random.default_rng(3)
        pick = list(np.argsort(-size)[:12]) + list(rng.choice(ch.n_fail, 30, replace=False))
        check(exp, ch.plan, ch, pick)


def test_errors():
    from test_gpu_exact import with_metrics, zero_frac

    eng, names, exp, s, _ = prepare(small("rand1"))
    n = len(names)

    def create(kind, ids, src=0):
        h = C.c_void_p()
        a = np.ascontiguousarray(ids, np.uint32)
        st = N.lib.spf_whatif_plan_create_nodes(eng._h, src, kind, N.ptr(a), len(a), C.byref(h))
        assert (st == N.SPF_OK) == bool(h.value)
        if h.value:
            N.lib.spf_whatif_plan_destroy(h)
        return st

    assert create(N.SPF_WHATIF_NODE_DOWN, [1, 2]) == N.SPF_OK
    assert create(N.SPF_WHATIF_NODE_DOWN, [1, 0, 2]) == N.SPF_E_INVALID  # the source
    assert create(N.SPF_WHATIF_NODE_DRAIN, [1, n]) == N.SPF_E_INVALID  # not a node
    assert create(7, [1, 2]) == N.SPF_E_INVALID  # not a kind
    assert create(0, [1, 2]) == N.SPF_E_INVALID
    assert create(N.SPF_WHATIF_NODE_DOWN, [1], src=n) == N.SPF_E_INVALID
    ids = np.zeros(n, np.uint32)
    k = C.c_uint32()
    node_plan, link_plan = eng.whatif_node_plan(0, kind="drain"), eng.whatif_plan(0)
    assert N.lib.spf_whatif_plan_links(node_plan._h, N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_nodes(link_plan._h, N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_kind(node_plan._h, C.byref(k)) == N.SPF_OK
    assert k.value == N.SPF_WHATIF_NODE_DRAIN
    assert N.lib.spf_whatif_plan_kind(link_plan._h, C.byref(k)) == N.SPF_OK and k.value == 0
    with pytest.raises(ValueError):
        eng.whatif_node_plan(0, kind="link")
    eng.close()

    topo = with_metrics(T.random_graph(40, 100, 75, max_metric=3, parallel_frac=0.2,
                                       overload_frac=0.1, link_overload_frac=0.05),
                        zero_frac(0.35), 2)
    ls, names, eng, orc, _ = setup(topo)
    for kind in WN.KINDS:
        with pytest.raises(N.SpfError) as e:
            eng.whatif_node_plan(0, kind=kind)
        assert e.value.status == N.SPF_E_UNSUPPORTED
        assert "exact" in str(e.value)


@pytest.mark.parametrize("kind", WN.KINDS)
def test_stability(kind):
    from openr_amd.engine import DIGEST_DTYPE
    from openr_amd.hiprt import DeviceArray

    eng, names, exp, s, _ = prepare(small("rand1"))
    _, alone_nodes, _ = eng.whatif_nodes(0, kind=kind)
    _, alone_links, _ = eng.whatif(0)
    plan, lplan = eng.whatif_node_plan(0, kind=kind), eng.whatif_plan(0)
    a, b = plan.changes(), plan.changes()
    assert np.array_equal(a.ptr, b.ptr)
    for i in range(plan.n_fail):
        for x, y in zip(a.of(i), b.of(i)):
            assert np.array_equal(x, y)
    assert np.array_equal(a.digests, alone_nodes)
    d_node, d_link = DeviceArray(plan.n_fail, DIGEST_DTYPE), DeviceArray(lplan.n_fail, DIGEST_DTYPE)
    for _ in range(2):  # a digest-only execute after changes(); the two plans in turn
        plan.execute(d_node.ptr)
        plan.stats()
        assert np.array_equal(d_node.numpy(), alone_nodes)
        lplan.execute(d_link.ptr)
        lplan.stats()
        assert np.array_equal(d_link.numpy(), alone_links)
    lch = lplan.changes()
    assert np.array_equal(lch.digests, alone_links)
    assert np.array_equal(plan.changes().ptr, a.ptr)
    eng.set_metric([0], [7])
    with pytest.raises(N.SpfError) as e1:
        plan.changes()
    with pytest.raises(N.SpfError) as e2:
        plan.execute(d_node.ptr)
    d_node.free()
    d_link.free()
    assert e1.value.status == e2.value.status == N.SPF_E_STATE
