"""What-if change lists on the MI355X (spf_whatif_changes): per failure the
nodes whose metric or next hops change under runSpf(src, true, {l}), with
their new values.

Every list is pinned to the CPU oracle through tests/whatif_lists.py: the
plan's unfailed result patched with the list must have the oracle's digest
for that failure (hash over every node, the two counts recounted from the
entries).  One test goes round the digest: patched distances against
single-source runs with the link ignored.
"""

import numpy as np
import pytest

import whatif_lists as L
from oracle import NameTable, whatif_digests
from openr_amd import _native as N
from openr_amd import topology as T
from test_gpu_whatif import SMALL, as_tuple, fail_of, setup

pytestmark = pytest.mark.gpu


def small(name):
    return next(make for n, make, _ in SMALL if n == name)()


def check(ls, names, orc, s, plan, ch, idx=None):
    """Failures idx (default: all) of the plan against the oracle."""
    idx = range(plan.n_fail) if idx is None else [int(i) for i in idx]
    base_d, base_nh, W = plan.base()
    assert W == ch.W == base_nh.shape[1]
    obase, want = whatif_digests(orc, NameTable(names), names[s],
                                 [fail_of(ls, plan.links[i]) for i in idx])
    assert as_tuple(ch.base_digest) == obase
    assert L.result_hash(base_d, base_nh) == obase[2]
    assert int(ch.ptr[0]) == 0 and int(ch.ptr[-1]) == ch.n_entries
    for i, w in zip(idx, want):
        node, dist, nh = ch.of(i)
        assert len(node) == int(ch.ptr[i + 1]) - int(ch.ptr[i])
        assert (np.diff(node.astype(np.int64)) > 0).all()  # ascending
        L.check_failure(base_d, base_nh, node, dist, nh, w, where=f"failure {i}")
        assert as_tuple(ch.digests[i]) == w
    return base_d, base_nh


WAVE = [f"rand{s}" for s in range(4)] + ["wan200"]


@pytest.mark.parametrize("name", WAVE)
def test_wave_teams_every_failure(name):
    ls, names, eng, orc, _ = setup(small(name))
    _, digests, base = eng.whatif(0)
    with eng.whatif_changes(0) as ch:
        assert ch.n_fail == len(digests)
        check(ls, names, orc, 0, ch.plan, ch)
        assert [as_tuple(d) for d in ch.digests] == [as_tuple(d) for d in digests]
        assert as_tuple(ch.base_digest) == as_tuple(base)
        assert ch.pool_bytes == 8 * (ch.n_fail + 1) + ch.n_entries * (12 + 4 * ch.W)


@pytest.mark.parametrize("src", ["0", "3"])
def test_more_than_one_word(src):
    """ba1500: 400 seeded failures plus the 12 longest lists.  Node "0", the
    source test_whatif_matches_oracle uses, has 23 distinct neighbours in this
    graph (one word), so W >= 2 is asserted from the hub, node "3" (167
    neighbours, 6 words: the wave-wide row copy); source "0" is checked all
    the same."""
    ls, names, eng, orc, (rp, col, _, _, _) = setup(small("ba1500"))
    s = names.index(src)
    with eng.whatif_changes(s) as ch:
        assert ch.W == L.words_of(len(L.neighbours(rp, col, s)))
        if src == "3":
            assert ch.W >= 2
        rng = np.random.default_rng(1)
        pick = rng.choice(ch.n_fail, min(ch.n_fail, 400), replace=False)
        longest = np.argsort(-np.diff(ch.ptr.astype(np.int64)))[:12]
        check(ls, names, orc, s, ch.plan, ch, list(pick) + list(longest))


def test_overflow_into_workgroup_teams(monkeypatch):
    monkeypatch.setenv("SPF_WHATIF_WAVECAP", "64")
    ls, names, eng, orc, _ = setup(small("grid12"))
    plan = eng.whatif_plan(0)  # a corner
    ch = plan.changes()
    assert plan.stats()[1] > 0  # big repairs
    check(ls, names, orc, 0, plan, ch)


@pytest.mark.parametrize("group", [None, "1"], ids=["group_default", "one_workgroup"])
def test_group_teams(monkeypatch, group):
    monkeypatch.setenv("SPF_WHATIF_CLASSIFY", "16")
    if group:
        monkeypatch.setenv("SPF_WHATIF_GROUP", group)
    ls, names, eng, orc, _ = setup(small("grid12"))
    plan = eng.whatif_plan(0)
    ch = plan.changes()
    assert plan.stats()[1] > 0
    check(ls, names, orc, 0, plan, ch)


def test_unreachable_tail():
    nodes = [f"n{i}" for i in range(6)]
    topo = T._undirected_to_adj(nodes, [(i, i + 1) for i in range(5)], np.ones(5), np.ones(5),
                                "line6")
    ls, names, eng, orc, (rp, col, met, lid, ovl) = setup(topo)
    assert names == nodes
    plan = eng.whatif_plan(0)
    ch = plan.changes()
    assert plan.n_fail == 5
    check(ls, names, orc, 0, plan, ch)
    for i, l in enumerate(plan.links):
        ends = sorted(u for u in range(6) for e in range(rp[u], rp[u + 1]) if lid[e] == l)
        node, dist, nh = ch.of(i)
        assert list(node) == list(range(ends[1], 6))  # exactly the tail
        assert (dist == L.U64_MAX).all() and not nh.any()


def test_cold_and_mixed_explicit_lists():
    ls, names, eng, orc, _ = setup(small("rand0"))
    links, digests, base = eng.whatif(0)
    cold = [int(l) for l, d in zip(links, digests) if as_tuple(d) == as_tuple(base)]
    hot = [int(l) for l, d in zip(links, digests) if as_tuple(d) != as_tuple(base)]
    assert len(cold) >= 3 and len(hot) >= 3
    with eng.whatif_changes(0, cold) as ch:
        assert ch.n_entries == 0 and not ch.ptr.any() and len(ch.ptr) == len(cold) + 1
        assert len(ch.node) == 0 and ch.nh.shape == (0, ch.W)
        for i in range(len(cold)):
            node, dist, nh = ch.of(i)
            assert len(node) == len(dist) == len(nh) == 0
        check(ls, names, orc, 0, ch.plan, ch)
    mixed = [hot[0], cold[0], hot[1], cold[1], cold[2], hot[2]]
    with eng.whatif_changes(0, mixed) as ch:
        assert list(ch.plan.links) == mixed  # the order is kept
        sizes = np.diff(ch.ptr.astype(np.int64))
        assert [bool(x) for x in sizes] == [True, False, True, False, False, True]
        check(ls, names, orc, 0, ch.plan, ch)


def test_exact_plan_zero_metrics():
    from test_gpu_exact import with_metrics, zero_frac

    topo = with_metrics(T.random_graph(40, 100, 75, max_metric=3, parallel_frac=0.2,
                                       overload_frac=0.1, link_overload_frac=0.05),
                        zero_frac(0.35), 2)
    ls, names, eng, orc, _ = setup(topo)
    _, digests, _ = eng.whatif(0)
    with eng.whatif_changes(0) as ch:
        check(ls, names, orc, 0, ch.plan, ch)
        assert [as_tuple(d) for d in ch.digests] == [as_tuple(d) for d in digests]
        assert ch.n_entries > 0


def test_stability_and_errors():
    import ctypes as C

    ls, names, eng, orc, _ = setup(small("rand1"))
    plan = eng.whatif_plan(0)
    w = C.c_uint32()
    assert N.lib.spf_whatif_base(plan._h, None, None, C.byref(w)) == N.SPF_E_STATE
    n = C.c_uint64()
    assert N.lib.spf_whatif_changes_db(plan._h, 0, None, None, None, 0, C.byref(n)) == N.SPF_E_STATE
    _, before, _ = eng.whatif(0, plan.links)
    a, b = plan.changes(), plan.changes()
    assert np.array_equal(a.ptr, b.ptr)
    for i in range(plan.n_fail):
        for x, y in zip(a.of(i), b.of(i)):
            assert np.array_equal(x, y)
    _, after, _ = eng.whatif(0, plan.links)  # a digest-only execute after them
    assert np.array_equal(before, after)
    from openr_amd.hiprt import DeviceArray
    from openr_amd.engine import DIGEST_DTYPE

    d_out = DeviceArray(plan.n_fail, DIGEST_DTYPE)
    plan.execute(d_out.ptr)  # the same plan, its scratch as the passes left it
    plan.stats()
    assert np.array_equal(d_out.numpy(), before)
    i = int(np.argmax(np.diff(a.ptr.astype(np.int64))))
    m = int(a.ptr[i + 1] - a.ptr[i])
    assert m > 0
    node = np.zeros(m, np.uint32)
    st = N.lib.spf_whatif_changes_db(plan._h, i, N.ptr(node), None, None, m - 1, C.byref(n))
    assert st == N.SPF_E_NOMEM and n.value == m
    eng.set_metric([0], [7])
    with pytest.raises(N.SpfError) as e1:
        plan.changes()
    with pytest.raises(N.SpfError) as e2:
        plan.execute(d_out.ptr)
    d_out.free()
    assert e1.value.status == e2.value.status == N.SPF_E_STATE
    assert N.lib.spf_whatif_changes_db(plan._h, 0, None, None, None, 0, C.byref(n)) == N.SPF_E_STATE


def test_patched_distances_equal_single_source_runs():
    ls, names, eng, orc, _ = setup(small("rand0"))
    with eng.whatif_changes(0) as ch:
        base_d, base_nh, _ = ch.plan.base()
        for i, l in enumerate(ch.plan.links):
            node, dist, nh = ch.of(i)
            d, _ = L.patched(base_d, base_nh, node, dist, nh)
            want = eng.sssp(0, ignore_links=[int(l)]).astype(np.uint64)
            want[want == 0xFFFFFFFF] = L.U64_MAX
            assert np.array_equal(d, want), (i, int(l))
