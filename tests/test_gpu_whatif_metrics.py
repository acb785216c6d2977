"""What-if batches for link metric changes on the MI355X
(spf_whatif_plan_create_metrics): for every change (link, m_lo, m_hi) of a
list, the SPF of one source on the graph with those metrics, as digests and as
change lists.

Everything is pinned by tests/whatif_metrics.py: a full oracle re-run on the
changed LSDB per change, reduced against the unchanged run.  A hot change's
list must be the oracle's changed nodes with their new metrics and next-hop
words, entry for entry.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import whatif_lists as L
import whatif_metrics as WM
from openr_amd import _native as N
from openr_amd import topology as T
from test_gpu_whatif import SMALL, as_tuple, setup
from test_gpu_whatif_sets import TEAMS, WAVE

pytestmark = pytest.mark.gpu

# The seed of the 40-node multigraph (metrics 1-3, 20 % parallel links) was
# picked on the CPU with the oracle (tests/whatif_metrics.py: variants over
# every up link) so that a lowered change is a new tie (delta = 0: no metric
# moves, next hops grow) and another moves metrics; 75 gives 23 and 37 of them.
M40_SEED = 75
FAMILIES = WAVE + ["m40"]


def make(name):
    if name == "m40":
        return T.random_graph(40, 100, M40_SEED, max_metric=3, parallel_frac=0.2)
    if name == "team300":  # ~300 nodes: a lowered core link's D passes a 64-node wave cap
        return T.random_graph(300, 450, 5, max_metric=5, parallel_frac=0.1, overload_frac=0.03)
    return next(mk for n, mk, _ in SMALL if n == name)()


def prepare(topo, src=None):
    ls, names, eng, orc, (rp, col, met, lid, ovl) = setup(topo)
    s = names.index(src) if isinstance(src, str) else (0 if src is None else int(src))
    exp = WM.Expected(topo.lsdb, ls, names, rp, col, s)
    return eng, names, exp, s, (rp, col, met, lid, ovl)


def all_variants(exp, edges):
    """[(variant, link, m_lo, m_hi)] over every up link, in link order."""
    out = []
    for l in sorted(edges):
        for k, (a, b) in WM.variants(*exp.current(l), l).items():
            out.append((k, l, a, b))
    return out


def check(exp, ch, changes, idx=None):
    """Changes idx (default: all) of a metric plan: digests against the oracle
    and, entry for entry, the lists.  Returns the expected digests."""
    plan = ch.plan
    idx = range(plan.n_fail) if idx is None else [int(i) for i in idx]
    base_d, base_nh, W = plan.base()
    assert W == ch.W == base_nh.shape[1]
    assert np.array_equal(base_d, exp.base[0]) and np.array_equal(base_nh, exp.base[1])
    assert as_tuple(ch.base_digest) == exp.base_digest
    assert int(ch.ptr[0]) == 0 and int(ch.ptr[-1]) == ch.n_entries
    assert ch.pool_bytes == 8 * (ch.n_fail + 1) + ch.n_entries * (12 + 4 * ch.W)
    assert not (ch.dist == L.U64_MAX).any()  # a metric change cuts nobody off
    want = {}
    for i in idx:
        l, a, b = changes[i]
        res = exp.metric_result(l, a, b)
        w = want[i] = exp.metric_digest(l, a, b)
        assert as_tuple(ch.digests[i]) == w, (i, changes[i])
        lo, hi = int(ch.ptr[i]), int(ch.ptr[i + 1])
        order = np.argsort(ch.node[lo:hi], kind="stable")
        node = ch.node[lo:hi][order].astype(np.int64)
        moved = sorted(WM.changed_nodes(exp.base, res))
        assert list(node) == moved, (i, changes[i])
        assert np.array_equal(ch.dist[lo:hi][order], res[0][node]), (i, changes[i])
        assert np.array_equal(ch.nh[lo:hi][order], res[1][node]), (i, changes[i])
    return want


@pytest.mark.parametrize("name", FAMILIES)
def test_families_against_the_oracle(name):
    eng, names, exp, s, (rp, col, met, lid, ovl) = prepare(make(name))
    edges = WM.link_edges(rp, col, lid)
    var = all_variants(exp, edges)
    changes = [(l, a, b) for _, l, a, b in var]
    with eng.whatif_metric_changes(s, changes) as ch:
        plan = ch.plan
        assert plan.kind == "metric" and plan.n_fail == len(changes) == 6 * len(edges)
        assert np.array_equal(plan.metric_changes, np.array(changes, np.uint32))
        assert list(plan.links) == [c[0] for c in changes] and len(plan.nodes) == 0
        want = check(exp, ch, changes)
        digests, base = eng.whatif_metrics(s, changes)
        assert as_tuple(base) == exp.base_digest
        assert [as_tuple(d) for d in digests] == [want[i] for i in range(len(changes))]
        n_hot = 0
        tie = moves = False
        for i, (k, l, a, b) in enumerate(var):
            root, delta = WM.classify(rp, col, met, ovl, exp.base[0], s, edges[l],
                                      exp.resolved(l, a, b))
            n_hot += root is not None
            if k in ("keep", "current"):
                assert root is None
            if root is None:
                assert want[i] == exp.base_digest and ch.ptr[i] == ch.ptr[i + 1]
            if k.startswith("lower") and root is not None:
                tie |= delta == 0 and want[i][0] == 0 and want[i][1] > 0
                moves |= want[i][0] > 0
        assert tie and moves  # a new equal-cost tie, and a lower that moves metrics
        assert plan.stats()[0] == n_hot  # hot exactly where the rule says so


@pytest.mark.parametrize("name", ["rand0", "rand2", "m40"])
def test_a_costed_out_link_changes_what_its_failure_changes(name):
    """Both directions of a link that is no bridge raised past every simple
    path's length ((N - 1) x the largest metric, above the largest base
    distance): the link plan's counts and changed nodes.  (Not the hash: the
    link remains, as a very long path nobody takes.)"""
    eng, names, exp, s, (rp, col, met, lid, ovl) = prepare(make(name))
    far = (len(names) - 1) * int(met.max()) + 1
    assert far > int(exp.base[0][exp.base[0] != L.U64_MAX].max())
    with eng.whatif_changes(s) as lch:
        links = [int(l) for l in lch.plan.links]
        with eng.whatif_metric_changes(s, [(l, far, far) for l in links]) as ch:
            n = 0
            for i, l in enumerate(links):
                ln, ld, _ = lch.of(i)
                if (ld == L.U64_MAX).any():
                    continue  # a bridge: its failure cuts nodes off, its cost-out does not
                n += 1
                node, dist, nh = ch.of(i)
                assert np.array_equal(node, ln), l
                assert (int(ch.digests[i]["n_dist_changed"]), int(ch.digests[i]["n_nh_changed"])) == \
                    (int(lch.digests[i]["n_dist_changed"]), int(lch.digests[i]["n_nh_changed"])), l
            assert n > len(links) // 2


def test_one_link_swept_over_eight_metrics():
    eng, names, exp, s, (rp, col, met, lid, ovl) = prepare(make("rand1"))
    edges = WM.link_edges(rp, col, lid)
    # a link into a node with several tight predecessors' worth of choice: the
    # first link whose lowering to 1 moves metrics
    l = next(l for l in sorted(edges) if exp.metric_digest(l, 1, 1)[0] > 0)
    sweep = [(l, m, m) for m in (1, 2, 3, 4, 5, 7, 11, 200)]
    sweep[2] = (l, 3, WM.KEEP)
    with eng.whatif_metric_changes(s, sweep) as ch:
        assert [tuple(int(x) for x in r) for r in ch.plan.metric_changes] == sweep
        want = check(exp, ch, sweep)
        assert len(set(want.values())) > 3  # the sweep is not one answer eight times
        for i, c in enumerate(sweep):
            with eng.whatif_metric_changes(s, [c]) as one:
                assert as_tuple(one.digests[0]) == want[i]
                for x, y in zip(one.of(0), ch.of(i)):
                    assert np.array_equal(x, y), c


@functools.lru_cache(maxsize=None)
def team_case():
    """The team test's topology, its oracle pins and its changes, made once."""
    topo = make("team300")
    eng, names, exp, s, (rp, col, met, lid, ovl) = prepare(topo)
    eng.close()
    edges = WM.link_edges(rp, col, lid)
    changes = [(l, a, b) for _, l, a, b in all_variants(exp, edges)]
    lowers, big_d = [], 0  # the changes with delta > 0, the largest D among them
    for i, (l, a, b) in enumerate(changes):
        new = exp.resolved(l, a, b)
        root, delta = WM.classify(rp, col, met, ovl, exp.base[0], s, edges[l], new)
        if delta > 0:
            lowers.append(i)
            big_d = max(big_d, len(WM.grow(rp, col, met, ovl, exp.base[0], s, edges[l], new, root, delta)))
    return topo, exp, changes, lowers, big_d


@pytest.mark.parametrize("env", [t[1] for t in TEAMS], ids=[t[0] for t in TEAMS])
def test_workgroup_and_group_teams(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    topo, exp, changes, lowers, big_d = team_case()
    ls, names, eng, orc, _ = setup(topo)
    s = exp.s
    assert big_d > 64  # a lowered link whose D passes a 64-node wave team
    plan = eng.whatif_metric_plan(s, changes)
    ch = plan.changes()
    assert plan.stats()[1] > 0  # big repairs: classified (raises, ties) or overflowed (lowers)
    check(exp, ch, changes)
    if "SPF_WHATIF_WAVECAP" in env:
        # lowers with delta > 0 only: none is classified big, so a big repair
        # here is a wave team's overflow, re-done by a workgroup
        only = [changes[i] for i in lowers]
        lplan = eng.whatif_metric_plan(s, only)
        lch = lplan.changes()
        assert lplan.stats()[1] > 0
        check(exp, lch, only)
    eng.close()


def test_more_than_one_word():
    """ba1500 from the hub "3" (167 neighbours, W = 6): the hub's links cost
    out and halved, 100 seeded changes elsewhere."""
    eng, names, exp, s, (rp, col, met, lid, ovl) = prepare(make("ba1500"), "3")
    edges = WM.link_edges(rp, col, lid)
    hub = sorted(set(int(l) for l in lid[rp[s]: rp[s + 1]]))
    rng = np.random.default_rng(2)
    changes = [(l, 9, 9) for l in hub[::4]] + [(l, 3, 3) for l in hub[1::8]]
    for l in rng.choice(sorted(edges), 100, replace=False):
        changes.append((int(l), int(rng.integers(1, 4)), int(rng.integers(0, 4))))
    with eng.whatif_metric_changes(s, changes) as ch:
        assert ch.W == L.words_of(len(L.neighbours(rp, col, s))) == 6
        want = check(exp, ch, changes)
        assert sum(w != exp.base_digest for w in want.values()) > 40


def test_overloaded_endpoints():
    topo = T.random_graph(50, 120, 17, max_metric=4, overload_frac=0.2)
    eng, names, exp, s, (rp, col, met, lid, ovl) = prepare(topo, 1)  # (node 0 is drained)
    edges = WM.link_edges(rp, col, lid)
    drained = [int(x) for x in np.nonzero(ovl)[0]]
    assert drained and s not in drained
    # lowering u -> v with u drained (not the source): cold
    cold = []
    for l, pair in sorted(edges.items()):
        for k, e in enumerate(pair):
            if WM.tail_of(rp, e) in drained and int(met[e]) > 1:
                cold.append((l, 1, WM.KEEP) if k == 0 else (l, WM.KEEP, 1))
    # a drained node inside D, reached at a new metric and not expanded: the
    # lowers to 1 that move a drained node in the oracle's re-run
    inside = []
    for l, pair in sorted(edges.items()):
        c = (l, 1, 1)
        root, delta = WM.classify(rp, col, met, ovl, exp.base[0], s, pair, exp.resolved(*c))
        if root is not None and delta > 0:
            D = WM.grow(rp, col, met, ovl, exp.base[0], s, pair, exp.resolved(*c), root, delta)
            if WM.changed_nodes(exp.base, exp.metric_result(*c)) & D & set(drained):
                inside.append(c)
    assert cold and inside
    changes = cold + inside
    with eng.whatif_metric_changes(s, changes) as ch:
        want = check(exp, ch, changes)
        for i in range(len(cold)):
            assert want[i] == exp.base_digest and ch.ptr[i] == ch.ptr[i + 1]
        moved = set()
        for i in range(len(cold), len(changes)):
            moved |= set(int(v) for v in ch.of(i)[0])
        assert moved & set(drained)  # a drained node is reached at a new metric
        assert ch.plan.stats()[0] == len(inside)
    eng.close()
    # the source itself drained: its links are expanded, lowering one is hot
    s2 = drained[0]
    eng, names, exp, s2, (rp, col, met, lid, ovl) = prepare(topo, s2)
    mine = []
    for e in range(int(rp[s2]), int(rp[s2 + 1])):
        b = int(col[e])
        if b != s2 and int(met[e]) > 1:
            mine.append((int(lid[e]), 1, WM.KEEP) if s2 < b else (int(lid[e]), WM.KEEP, 1))
    assert mine
    with eng.whatif_metric_changes(s2, mine) as ch:
        want = check(exp, ch, mine)
        assert ch.plan.stats()[0] == len(mine)
        assert any(w[0] > 0 for w in want.values())


def test_refusals():
    from test_gpu_exact import with_metrics, zero_frac

    eng, names, exp, s, (rp, col, met, lid, ovl) = prepare(make("rand1"))
    top = int(lid.max())
    n_nodes = len(names)
    ok_metric = (0xFFFFFFFF - 1) // n_nodes  # the largest with metric x N < 2^32 - 1
    assert ok_metric * n_nodes < 0xFFFFFFFF <= (ok_metric + 1) * n_nodes

    def create(links, lo, hi, n=None, src=0):
        h = C.c_void_p()
        arrs = [None if x is None else np.ascontiguousarray(x, np.uint32) for x in (links, lo, hi)]
        n = len(arrs[0]) if n is None else n
        st = N.lib.spf_whatif_plan_create_metrics(eng._h, src, *[None if x is None else N.ptr(x)
                                                                 for x in arrs], n, C.byref(h))
        assert (st == N.SPF_OK) == bool(h.value)
        if h.value:
            N.lib.spf_whatif_plan_destroy(h)
        return st

    assert create([1, 2, 1], [3, 0, 4], [0, 0, 9]) == N.SPF_OK
    assert create(None, None, None, n=0) == N.SPF_OK  # no changes at all
    assert create([top], [ok_metric], [1]) == N.SPF_OK
    assert create([top + 1], [1], [1]) == N.SPF_E_INVALID  # not a link id
    assert create([1], [ok_metric + 1], [1]) == N.SPF_E_INVALID  # past the 32-bit envelope
    assert create([1], [1], [0xFFFFFFFF]) == N.SPF_E_INVALID
    assert create(None, [1], [1], n=1) == N.SPF_E_INVALID
    assert create([1], None, [1]) == N.SPF_E_INVALID
    assert create([1], [1], None) == N.SPF_E_INVALID
    assert create([1], [1], [1], src=n_nodes) == N.SPF_E_INVALID
    # a link that is not up is a link id of the graph: allowed, and cold
    dead = sorted(set(range(top + 1)) - set(WM.link_edges(rp, col, lid)))
    if dead:
        digests, base = eng.whatif_metrics(0, [(dead[0], 1, 1)])
        assert as_tuple(digests[0]) == as_tuple(base) == exp.base_digest
    ids, ptr = np.zeros(n_nodes + 400, np.uint32), np.zeros(8, np.uint32)
    k = C.c_uint32()
    metric_plan = eng.whatif_metric_plan(0, [(3, 2, 0), (1, 0, 7), (3, 5, 5)])
    link_plan, node_plan = eng.whatif_plan(0), eng.whatif_node_plan(0)
    set_plan = eng.whatif_set_plan(0, [[3, 1], [2]])
    assert N.lib.spf_whatif_plan_links(metric_plan._h, N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_nodes(metric_plan._h, N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_sets(metric_plan._h, N.ptr(ptr), N.ptr(ids)) == N.SPF_E_STATE
    lo, hi = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    for other in (link_plan, node_plan, set_plan):
        assert N.lib.spf_whatif_plan_metrics(other._h, N.ptr(ids), N.ptr(lo), N.ptr(hi)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_metrics(metric_plan._h, N.ptr(ids), N.ptr(lo), N.ptr(hi)) == N.SPF_OK
    assert list(ids[:3]) == [3, 1, 3] and list(lo[:3]) == [2, 0, 5] and list(hi[:3]) == [0, 7, 5]
    assert N.lib.spf_whatif_plan_metrics(metric_plan._h, None, None, None) == N.SPF_OK
    assert N.lib.spf_whatif_plan_kind(metric_plan._h, C.byref(k)) == N.SPF_OK
    assert k.value == N.SPF_WHATIF_LINK_METRIC == 4
    assert N.lib.spf_whatif_plan_failures(metric_plan._h) == 3
    metric_plan.changes()
    eng.set_overload([int(np.nonzero(ovl == 0)[0][-1])], [1])  # a node that was not drained
    from openr_amd.engine import DIGEST_DTYPE
    from openr_amd.hiprt import DeviceArray
    d = DeviceArray(3, DIGEST_DTYPE)
    with pytest.raises(N.SpfError) as e1:
        metric_plan.execute(d.ptr)
    with pytest.raises(N.SpfError) as e2:
        metric_plan.changes()
    d.free()
    assert e1.value.status == e2.value.status == N.SPF_E_STATE
    eng.close()

    topo = with_metrics(T.random_graph(40, 100, 75, max_metric=3, parallel_frac=0.2,
                                       overload_frac=0.1, link_overload_frac=0.05),
                        zero_frac(0.35), 2)
    ls, names, eng, orc, _ = setup(topo)
    with pytest.raises(N.SpfError) as e:
        eng.whatif_metric_plan(0, [(0, 1, 1)])
    assert e.value.status == N.SPF_E_UNSUPPORTED and "exact" in str(e.value)
