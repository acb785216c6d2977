"""What-if batches for link-set failures on the MI355X
(spf_whatif_plan_create_sets): for every set of a list, the SPF of one source
with every link of the set ignored, as digests and as change lists.

A one-member set must equal the link plan and linksFromNode(x) the node-down
plan, entry for entry.  Everything else is pinned by tests/whatif_sets.py: a
full oracle re-run on the changed LSDB per set, reduced against the unfailed
run.  Lists are checked with whatif_lists.check_failure: the plan's unfailed
result patched with a set's list must have that digest.
"""

import ctypes as C

import numpy as np
import pytest

import whatif_lists as L
import whatif_sets as WS
from openr_amd import _native as N
from openr_amd import topology as T
from test_gpu_whatif import SMALL, as_tuple, setup
from test_whatif_sets_host import SEED

pytestmark = pytest.mark.gpu

WAVE = [f"rand{s}" for s in range(4)] + ["wan200"]
TEAMS = [("wavecap64", {"SPF_WHATIF_WAVECAP": "64"}),
         ("classify16", {"SPF_WHATIF_CLASSIFY": "16"}),
         ("classify16_one_workgroup", {"SPF_WHATIF_CLASSIFY": "16", "SPF_WHATIF_GROUP": "1"})]


def small(name):
    return next(make for n, make, _ in SMALL if n == name)()


def prepare(topo, src=None):
    ls, names, eng, orc, (rp, col, met, lid, ovl) = setup(topo)
    s = names.index(src) if isinstance(src, str) else 0
    exp = WS.Expected(topo.lsdb, ls, names, rp, col, s)
    dag = WS.Dag(rp, col, met, lid, ovl, exp.base[0], s)
    return eng, ls, names, exp, dag, s, (rp, col, lid, ovl)


def check(exp, plan, ch, idx=None):
    """Failures idx (default: all) of a set plan's lists and digests against
    the helper; returns the expected digests."""
    idx = range(plan.n_fail) if idx is None else [int(i) for i in idx]
    base_d, base_nh, W = plan.base()
    assert W == ch.W == base_nh.shape[1]
    assert np.array_equal(base_d, exp.base[0]) and np.array_equal(base_nh, exp.base[1])
    assert as_tuple(ch.base_digest) == exp.base_digest
    assert int(ch.ptr[0]) == 0 and int(ch.ptr[-1]) == ch.n_entries
    assert ch.pool_bytes == 8 * (ch.n_fail + 1) + ch.n_entries * (12 + 4 * ch.W)
    want = {}
    for i in idx:
        links = [int(l) for l in plan.sets[i]]
        w = want[i] = exp.digest(links)
        node, dist, nh = ch.of(i)
        assert len(node) == int(ch.ptr[i + 1]) - int(ch.ptr[i])
        assert (np.diff(node.astype(np.int64)) > 0).all()  # ascending
        L.check_failure(base_d, base_nh, node, dist, nh, w, where=f"set {links}")
        assert as_tuple(ch.digests[i]) == w, links
    return want


def same_lists(a, i, b, j):
    for x, y in zip(a.of(i), b.of(j)):
        assert np.array_equal(x, y), (i, j)
    assert as_tuple(a.digests[i]) == as_tuple(b.digests[j]), (i, j)


@pytest.mark.parametrize("name", WAVE)
def test_one_member_sets_equal_the_link_plan(name):
    eng, ls, names, exp, dag, s, _ = prepare(small(name))
    with eng.whatif_changes(s) as lch:
        links = [int(l) for l in lch.plan.links]
        assert links == dag.up
        digests, base = eng.whatif_sets(s, [[l] for l in links])
        assert as_tuple(base) == as_tuple(lch.base_digest) == exp.base_digest
        assert np.array_equal(digests, lch.digests)
        with eng.whatif_set_changes(s, [[l] for l in links]) as ch:
            assert ch.plan.kind == "sets" and len(ch.plan.links) == 0 and len(ch.plan.nodes) == 0
            assert [list(x) for x in ch.plan.sets] == [[l] for l in links]
            assert np.array_equal(ch.ptr, lch.ptr) and ch.pool_bytes == lch.pool_bytes
            for i in range(len(links)):
                same_lists(ch, i, lch, i)


@pytest.mark.parametrize("name", WAVE)
def test_links_from_node_equals_the_node_down_plan(name):
    eng, ls, names, exp, dag, s, (rp, col, lid, ovl) = prepare(small(name))
    with eng.whatif_node_changes(s, kind="down") as nch:
        sets = [sorted(set(int(l) for l in lid[rp[x]: rp[x + 1]])) for x in nch.plan.nodes]
        with eng.whatif_set_changes(s, sets) as ch:
            assert np.array_equal(ch.ptr, nch.ptr) and np.array_equal(ch.digests, nch.digests)
            base_d = ch.plan.base()[0]
            for i, x in enumerate(nch.plan.nodes):
                same_lists(ch, i, nch, i)
                if base_d[x] != L.U64_MAX:
                    node, dist, nh = ch.of(i)
                    k = int(np.searchsorted(node, x))
                    assert node[k] == x and dist[k] == L.U64_MAX and not nh[k].any()


@pytest.mark.parametrize("name", WAVE)
def test_families_against_the_oracle(name):
    eng, ls, names, exp, dag, s, _ = prepare(small(name))
    fam = WS.families(ls, dag, SEED)
    rand = name.startswith("rand")
    count = {k: len(v) for k, v in fam.items()}
    assert count["nested"] and count["disjoint"] and count["cold"] and count["random"] == 8
    assert count["empty"] == 1
    if rand:
        assert count["ecmp_cut"] and count["same_head"] and count["parallel"]
        assert count["mixed"] == 2 and count["cold"] == 2
    assert any(len(dag.heads(x)) >= 2 and exp.digest(x) != exp.base_digest for x in fam["random"])
    sets, where = [], {}
    for k, v in fam.items():
        where[k] = range(len(sets), len(sets) + len(v))
        sets += v
    twice = fam["nested"][0]
    scrambled = list(reversed(fam["random"][-1])) + [fam["random"][-1][2]]  # unsorted, one repeat
    sets += [twice, scrambled, twice]
    with eng.whatif_set_changes(s, sets) as ch:
        plan = ch.plan
        assert plan.n_fail == len(sets) and int(plan.set_ptr[-1]) == len(plan.set_links)
        assert [list(x) for x in plan.sets] == [sorted(set(x)) for x in sets]
        assert list(plan.sets[-2]) == fam["random"][-1]
        want = check(exp, plan, ch)
        digests, base = eng.whatif_sets(s, sets)
        assert [as_tuple(d) for d in digests] == [want[i] for i in range(len(sets))]
        for i in list(where["cold"]) + list(where["empty"]):
            assert want[i] == exp.base_digest and ch.ptr[i] == ch.ptr[i + 1]
        for i in where["ecmp_cut"]:
            (b,) = dag.heads(sets[i])
            assert b in ch.of(i)[0]
        same_lists(ch, len(sets) - 1, ch, len(sets) - 3)  # the same set twice
        same_lists(ch, len(sets) - 2, ch, where["random"][-1])
        n_hot = sum(bool(dag.heads(x)) for x in sets)
        assert plan.stats()[0] == n_hot  # hot exactly when a member is tight


def test_source_cut_off():
    nodes = [f"n{i}" for i in range(6)]
    topo = T._undirected_to_adj(nodes, [(i, i + 1) for i in range(5)], np.ones(5), np.ones(5),
                                "line6")
    eng, ls, names, exp, dag, s, (rp, col, lid, ovl) = prepare(topo)
    assert names == nodes
    first, far = int(lid[rp[0]]), int(lid[rp[5]])
    with eng.whatif_set_changes(0, [[first, far], [far, first, far]]) as ch:
        check(exp, ch.plan, ch)
        for i in range(2):
            node, dist, nh = ch.of(i)
            assert list(node) == [1, 2, 3, 4, 5] and (dist == L.U64_MAX).all() and not nh.any()
    eng, ls, names, exp, dag, s, (rp, col, lid, ovl) = prepare(small("rand2"))
    mine = sorted(set(int(l) for l in lid[rp[0]: rp[1]]))
    with eng.whatif_set_changes(0, [mine]) as ch:
        check(exp, ch.plan, ch)
        node, dist, nh = ch.of(0)
        base_d = ch.plan.base()[0]
        assert list(node) == [v for v in range(1, len(names)) if base_d[v] != L.U64_MAX]
        assert len(node) > 10 and (dist == L.U64_MAX).all() and not nh.any()


@pytest.mark.parametrize("env", [t[1] for t in TEAMS], ids=[t[0] for t in TEAMS])
def test_workgroup_and_group_teams(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng, ls, names, exp, dag, s, (rp, col, lid, ovl) = prepare(small("grid12"))  # node 0: a corner
    bd = exp.base[0]
    corner = sorted(set(int(l) for l in lid[rp[0]: rp[1]]))
    assert len(corner) == 2
    depth = {d: [l for l in sorted(dag.tight) if int(bd[dag.tight[l][1]]) == d] for d in (1, 2)}
    sets = [corner, depth[1][:2], depth[2][:2], depth[2][:3], depth[1][:1] + depth[2][-2:]]
    sets += [[l] for l in depth[1] + depth[2]]
    plan = eng.whatif_set_plan(0, sets)
    ch = plan.changes()
    assert plan.stats()[1] > 0  # big repairs
    check(exp, plan, ch)
    node, dist, nh = ch.of(0)
    assert len(node) == 143 and (dist == L.U64_MAX).all()


def test_more_than_one_word():
    """ba1500 from the hub "3" (167 neighbours, W = 6): the hub's links in
    runs of 5, 100 seeded 4-link sets, the 12 sets with the longest lists."""
    eng, ls, names, exp, dag, s, (rp, col, lid, ovl) = prepare(small("ba1500"), "3")
    hub = sorted(set(int(l) for l in lid[rp[s]: rp[s + 1]]))
    rng = np.random.default_rng(2)
    sets = [hub[i: i + 5] for i in range(0, len(hub), 5)]
    sets += [sorted(int(l) for l in rng.choice(dag.up, 4, replace=False)) for _ in range(100)]
    with eng.whatif_set_changes(s, sets) as ch:
        assert ch.W == L.words_of(len(L.neighbours(rp, col, s))) == 6
        longest = list(np.argsort(-np.diff(ch.ptr.astype(np.int64)))[:12])
        assert int(ch.ptr[longest[0] + 1] - ch.ptr[longest[0]]) > 5
        check(exp, ch.plan, ch)


def test_a_set_larger_than_a_wave():
    """Root seeding in more than one 64-lane chunk, the membership search on a
    long run: all 167 links of the ba1500 hub, and 200 seeded links."""
    eng, ls, names, exp, dag, s, (rp, col, lid, ovl) = prepare(small("ba1500"), "3")
    hub = sorted(set(int(l) for l in lid[rp[s]: rp[s + 1]]))
    assert len(hub) == 167
    rng = np.random.default_rng(4)
    wide = sorted(int(l) for l in rng.choice(dag.up, 200, replace=False))
    assert len(dag.heads(wide)) > 64  # more than a chunk of roots
    with eng.whatif_set_changes(s, [hub, wide, wide[:70]]) as ch:
        check(exp, ch.plan, ch)
        node, dist, nh = ch.of(0)
        assert len(node) == int((exp.base[0] != L.U64_MAX).sum()) - 1 and (dist == L.U64_MAX).all()


def test_refusals():
    from test_gpu_exact import with_metrics, zero_frac

    eng, ls, names, exp, dag, s, (rp, col, lid, ovl) = prepare(small("rand1"))
    top = max(dag.ids)

    def create(ptr, links, n=None, src=0):
        h = C.c_void_p()
        p = None if ptr is None else np.ascontiguousarray(ptr, np.uint32)
        a = None if links is None else np.ascontiguousarray(links, np.uint32)
        n = (len(p) - 1 if p is not None else 0) if n is None else n
        st = N.lib.spf_whatif_plan_create_sets(eng._h, src, None if p is None else N.ptr(p),
                                               None if a is None else N.ptr(a), n, C.byref(h))
        assert (st == N.SPF_OK) == bool(h.value)
        if h.value:
            N.lib.spf_whatif_plan_destroy(h)
        return st

    assert create([0, 2, 3], [1, 2, 3]) == N.SPF_OK
    assert create([0, 0, 0], None) == N.SPF_OK  # empty sets need no members
    assert create([0], None) == N.SPF_OK  # no sets at all
    assert create([0, 1], [top]) == N.SPF_OK
    assert create([1, 2, 3], [1, 2, 3]) == N.SPF_E_INVALID  # set_ptr[0] != 0
    assert create([0, 2, 1], [1, 2, 3]) == N.SPF_E_INVALID  # decreasing
    assert create([0, 2, 3], [1, top + 1, 3]) == N.SPF_E_INVALID  # not a link id
    assert create(None, [1, 2], n=1) == N.SPF_E_INVALID
    assert create([0, 2], None) == N.SPF_E_INVALID
    assert create([0, 1], [1], src=len(names)) == N.SPF_E_INVALID
    ids, ptr = np.zeros(len(names) + 400, np.uint32), np.zeros(8, np.uint32)
    k = C.c_uint32()
    set_plan, link_plan = eng.whatif_set_plan(0, [[3, 1], [2]]), eng.whatif_plan(0)
    node_plan = eng.whatif_node_plan(0)
    assert N.lib.spf_whatif_plan_links(set_plan._h, N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_nodes(set_plan._h, N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_sets(link_plan._h, N.ptr(ptr), N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_sets(node_plan._h, N.ptr(ptr), N.ptr(ids)) == N.SPF_E_STATE
    assert N.lib.spf_whatif_plan_sets(set_plan._h, N.ptr(ptr), N.ptr(ids)) == N.SPF_OK
    assert list(ptr[:3]) == [0, 2, 3] and list(ids[:3]) == [1, 3, 2]
    assert N.lib.spf_whatif_plan_kind(set_plan._h, C.byref(k)) == N.SPF_OK
    assert k.value == N.SPF_WHATIF_LINK_SET == 3
    set_plan.changes()
    eng.set_overload([int(np.nonzero(ovl == 0)[0][-1])], [1])  # a node that was not drained
    from openr_amd.engine import DIGEST_DTYPE
    from openr_amd.hiprt import DeviceArray
    d = DeviceArray(2, DIGEST_DTYPE)
    with pytest.raises(N.SpfError) as e1:
        set_plan.execute(d.ptr)
    with pytest.raises(N.SpfError) as e2:
        set_plan.changes()
    d.free()
    assert e1.value.status == e2.value.status == N.SPF_E_STATE
    eng.close()

    topo = with_metrics(T.random_graph(40, 100, 75, max_metric=3, parallel_frac=0.2,
                                       overload_frac=0.1, link_overload_frac=0.05),
                        zero_frac(0.35), 2)
    ls, names, eng, orc, _ = setup(topo)
    with pytest.raises(N.SpfError) as e:
        eng.whatif_set_plan(0, [[0, 1]])
    assert e.value.status == N.SPF_E_UNSUPPORTED and "exact" in str(e.value)
