"""spf_whatif_route_update where test_gpu_whatif_route_update.py does not go:
a source in the middle of the id range (row0 != 0, the source the higher end of
half of its links), a row of exactly and of one more than the slots the kernels
stage in LDS (the plain instantiations of the base, entry and record kernels)
with more touched failures than one workgroup of the touch and mask kernels
takes, touched failures on a plan without a single change-list entry, dead
slots and overloaded nodes in the loaded graph, and a source whose row is empty
or dead throughout.  The judge is that module's Bench.run: every failure
against the numpy checker (pinned to the oracle with the source in the middle
by test_whatif_route_update_host.py), a chosen subset against a second engine
with the failure applied.  Every case first asserts, on the expectation's side,
that its shape reaches the edge it is named after."""

import copy

import numpy as np
import pytest

import whatif_route_update as U
from openr_amd import _native as N
from test_gpu_whatif_route_update import Bench, failed_arrays, link_slots

pytestmark = pytest.mark.gpu

LOW32 = np.uint64(0xFFFFFFFF)


def loaded(g, arrays, names=None):
    """`g` with the CSR `arrays` in place of its own: what Bench loads, what
    its Row is built from and what its second engine fails further."""
    d = copy.copy(g)
    d.rp, d.col, d.met, d.lid, d.ovl = arrays
    if names is not None:
        d.names = names
    return d


def slot_link(g, s, t):
    return int(g.lid[int(g.rp[s]) + t])


def members(g, h, x):
    """The links hub - x: (the equal members, the heavier one)."""
    w = {int(g.lid[e]): int(g.met[e]) for e in range(int(g.rp[h.hub]), int(g.rp[h.hub + 1]))}
    links = g.links_between(h.hub, x)
    return sorted(l for l in links if w[l] == 2), [l for l in links if w[l] == 4]


def tie_moves(g, h):
    """Metric changes on the bundles that move a tie and no node: an equal
    member raised, the heavier one lowered onto the tie, in the direction out of
    the source (m_hi towards the lower neighbour, m_lo towards the upper) and
    in both."""
    (eq_lo, heavy_lo), (eq_hi, heavy_hi) = members(g, h, h.lower_bundle), members(g, h, h.upper_bundle)
    return [("metric", eq_lo[0], U.KEEP, 3), ("metric", eq_lo[1], 3, 3), ("metric", heavy_lo[0], U.KEEP, 2),
            ("metric", heavy_lo[0], 2, 2), ("metric", eq_hi[0], 3, U.KEEP), ("metric", eq_hi[1], 3, 3),
            ("metric", heavy_hi[0], 2, U.KEEP), ("metric", heavy_hi[0], 2, 2)]


def bundle_sets(g, h):
    (eq_lo, heavy_lo), (eq_hi, heavy_hi) = members(g, h, h.lower_bundle), members(g, h, h.upper_bundle)
    own = [slot_link(g, h.hub, t) for t in range(int(g.rp[h.hub + 1] - g.rp[h.hub]))]
    ring = g.links_between(h.nbrs[0], h.ring[0])
    return [("set", eq_lo), ("set", eq_hi), ("set", [eq_lo[0]]), ("set", [eq_hi[1]]),
            ("set", eq_lo + heavy_lo), ("set", eq_hi + heavy_hi), ("set", [eq_lo[0], eq_hi[0]]),
            ("set", heavy_lo + eq_hi), ("set", eq_lo + eq_hi), ("set", ring), ("set", ring + [eq_lo[1]]),
            ("set", own), ("set", [])]


@pytest.fixture(scope="module")
def small():
    g, h = U.hub_graph(8)
    b = Bench(g, h.hub, U.hub_sets(g, h))
    b.h = h
    yield b
    b.close()


@pytest.mark.parametrize("kind", ("link", "down", "drain", "set", "metric"))
def test_source_in_the_middle(small, kind):
    b, g, h = small, small.g, small.h
    row0 = int(g.rp[h.hub])
    assert row0 > 0 and min(h.nbrs) < h.hub < max(h.nbrs) and b.deg == 8
    fails = bundle_sets(g, h) if kind == "set" else [f for f in U.hub_failures(g, h) if f[0] == kind]
    assert len(fails) >= 8
    _, _, up, lists = b.run(kind, fails, range(len(fails)))
    recs = [r for _, _, rs in lists for r in rs if len(r)]
    assert recs and all(((r & LOW32) >= row0).all() for r in recs)  # edge indices, not slots of the row
    assert (up.rec & LOW32).min() >= row0 and (np.concatenate(up.base()) & LOW32).min() >= row0
    if kind == "metric":
        U.one_direction_moves(g, h, fails, lists)


def lds_failures(g, h, slots, L):
    """The failures of the long-row case by kind; by kind the indices of those
    on slot 0, slot L - 1 and the last slot, and of these the ones that touch
    the row whichever side of the source the slot's neighbour is on."""
    s, rng = h.hub, np.random.default_rng(13)
    sweep = int(N.lib.spf_whatif_route_update_sweep_sets())
    edge_slots = (0, L - 1, slots - 1)
    head = [int(g.col[int(g.rp[s]) + t]) for t in range(slots)]
    # the first and the last 130 slots of the row, and every slot beside slots 0, L - 1 and the last
    # one towards the same neighbour: more links of the source than a workgroup of the touch and
    # mask kernels takes failures
    ts = sorted(set(range(130)) | set(range(slots - 130, slots))
                | {t for t in range(slots) if head[t] in {head[e] for e in edge_slots}})
    assert len(ts) > sweep + 1 and set(edge_slots) <= set(ts)
    own = [slot_link(g, s, t) for t in range(slots)]
    far = sorted(set(g.up_links()) - set(own))
    link = [("link", own[t]) for t in ts] + [("link", int(l)) for l in rng.choice(far, 40, replace=False)]
    edge = [own[t] for t in edge_slots]
    (eq_lo, heavy_lo), (eq_hi, heavy_hi) = members(g, h, h.lower_bundle), members(g, h, h.upper_bundle)
    sets = [("set", edge), ("set", [edge[0]]), ("set", [edge[1]]), ("set", [edge[2]]), ("set", eq_lo),
            ("set", eq_hi + heavy_hi), ("set", [eq_lo[0], eq_hi[0]]), ("set", [])]
    for k in range(16):
        pool = own if k % 2 == 0 else far
        sets.append(("set", sorted(int(l) for l in rng.choice(pool, int(rng.integers(2, 6)), replace=False))))
    metric = [("metric", l, lo, hi) for l in edge for lo, hi in ((1, 1), (3, U.KEEP), (U.KEEP, 3), (3, 3))]
    metric += tie_moves(g, h)
    metric += [("metric", int(l), int(rng.integers(1, 5)), int(rng.integers(0, 5)))
               for l in rng.choice(far, 20, replace=False)]
    down = [("down", head[t]) for t in edge_slots] + [("down", h.lower_bundle), ("down", h.upper_bundle)]
    down += [("down", int(x)) for x in rng.choice([v for v in range(len(g.names)) if v != s], 30, replace=False)]
    fails = {"link": link, "set": sets, "metric": metric, "down": down}
    at_edge = {"link": [ts.index(t) for t in edge_slots], "set": [0, 1, 2, 3], "metric": list(range(12)),
               "down": [0, 1, 2]}
    touching = dict(at_edge, metric=[i for i in range(12) if i % 4 in (0, 3)])
    return fails, at_edge, touching


def long_row_sets(g, h, slots, L):
    """About fifty sets: the neighbours behind slot 0, slot L - 1 and the last
    slot, and the ring nodes behind them; the bundled neighbours; ring nodes
    and anycast sets across the words of the bitmap; the source's own prefix
    and an empty set."""
    s, k = h.hub, len(h.nbrs)
    at = {x: j for j, x in enumerate(h.nbrs)}
    sets = []
    for t in (0, L - 1, slots - 1):
        j = at[int(g.col[int(g.rp[s]) + t])]
        sets += [[h.nbrs[j]], [h.ring[j]], [h.ring[(j - 1) % k]]]
    sets += [[h.lower_bundle], [h.upper_bundle], [h.ring[at[h.lower_bundle]]], [h.ring[at[h.upper_bundle]]]]
    spread = [int(j) for j in np.linspace(0, k - 1, 24).astype(int)]
    sets += [[h.ring[j]] for j in spread[:16]] + [[h.nbrs[j]] for j in spread[16:]]
    sets += [[h.ring[spread[a]], h.ring[spread[-1 - a]]] for a in range(6)]
    sets += [[h.nbrs[0], h.nbrs[k - 1], h.ring[k // 2]], [h.ring[j] for j in spread], [s], [h.ring[0], s], []]
    return sets


@pytest.fixture(scope="module")
def lds_slots():
    return int(N.lib.spf_whatif_route_update_lds_slots())


@pytest.mark.parametrize("past", (0, 1))
def test_row_at_and_past_lds_capacity(lds_slots, past):
    L, slots = lds_slots, lds_slots + past
    sweep = int(N.lib.spf_whatif_route_update_sweep_sets())
    g, h = U.hub_graph(slots)
    row0, last = int(g.rp[h.hub]), int(g.rp[h.hub]) + slots - 1
    sets = long_row_sets(g, h, slots, L)
    assert 45 <= len(sets) <= 60
    b = Bench(g, h.hub, sets)
    try:
        assert b.deg == slots and row0 != 0 and len(b.row.q) == slots and b.row.bit.max() >= 32
        fails, at_edge, touching = lds_failures(g, h, slots, L)
        rng = np.random.default_rng(17)
        seen_base = seen_update = False
        for kind in ("link", "set", "metric", "down"):
            n = len(fails[kind])
            others = rng.choice(n, min(40 if kind == "link" else 8, n), replace=False)
            _, rt, up, lists = b.run(kind, fails[kind], sorted(set(at_edge[kind]) | set(int(i) for i in others)))
            assert rt.W >= 2
            if kind == "link":  # a second workgroup of the touch and mask kernels
                assert up.n_touched > sweep
            seen_base |= any((r & LOW32 == last).any() for r in up.base())
            seen_update |= any((r & LOW32 == last).any() for _, _, rs in lists for r in rs)
            assert all(b.row.touches(fails[kind][i]) for i in touching[kind])
        # the last slot -- past what LDS holds when slots == L + 1 -- is a next hop and is changed
        assert seen_base and seen_update
    finally:
        b.close()


def test_touched_failures_without_any_change_list(small):
    """Plans of bundle members only: cold at node level, so the table of change
    lists is empty and every metric is the base's, and touching throughout."""
    b, g, h = small, small.g, small.h
    eq = members(g, h, h.lower_bundle)[0] + members(g, h, h.upper_bundle)[0]
    assert len(eq) == 4
    for kind, fails in (("link", [("link", l) for l in eq]), ("metric", tie_moves(g, h))):
        ch, rt, up, lists = b.run(kind, fails, range(len(fails)))
        assert int(ch.ptr[-1]) == 0 and ch.n_entries == 0 and rt.n_entries == 0
        assert up.n_touched == len(fails) and up.n_entries > 0
        assert all(len(ids) for ids, _, _ in lists)


@pytest.fixture(scope="module")
def holed():
    """The small hub graph loaded with two links down: an equal member of the
    lower bundle (a dead slot inside a bundle) and the only link to the first
    neighbour (a neighbour whose every slot is dead: the others' bits shift)."""
    g, h = U.hub_graph(8)
    dead = [members(g, h, h.lower_bundle)[0][0]] + g.links_between(h.hub, h.nbrs[0])
    assert len(dead) == 2
    d = loaded(g, failed_arrays(g, ("set", dead), link_slots(g)))
    b = Bench(d, h.hub, U.hub_sets(g, h))
    b.h, b.dead, b.whole = h, dead, g
    yield b
    b.close()


@pytest.mark.parametrize("kind", ("link", "set", "metric", "down"))
def test_dead_slots_in_the_loaded_row(holed, kind):
    b, d, h, dead = holed, holed.g, holed.h, holed.dead
    whole = U.Row(b.whole.rp, b.whole.col, b.whole.met, b.whole.lid, h.hub)
    assert int((b.row.bit < 0).sum()) == 2 and b.row.bit.max() == 2 and whole.bit.max() == 3
    assert (b.row.bit[whole.bit > 0] == whole.bit[whole.bit > 0] - 1).sum() == 6  # the bits shifted
    eq_lo, heavy_lo = members(b.whole, h, h.lower_bundle)
    eq_hi, heavy_hi = members(b.whole, h, h.upper_bundle)
    live = eq_lo[1]
    if kind == "link":
        # a link plan takes up links only: a dead one is refused, not listed
        for l in dead:
            with pytest.raises(N.SpfError) as e:
                b.eng.whatif_plan(h.hub, [l])
            assert e.value.status == N.SPF_E_INVALID
        fails, on_dead = [("link", l) for l in d.up_links()], []
        assert not set(dead) & set(d.up_links())
    elif kind == "set":
        on_dead = [("set", [dead[0]]), ("set", [dead[1]]), ("set", dead)]
        fails = on_dead + [("set", [dead[0], live]), ("set", [dead[1]] + eq_hi), ("set", [live]),
                           ("set", dead + heavy_lo + [live]), ("set", eq_hi + heavy_hi),
                           ("set", [slot_link(d, h.hub, t) for t in range(8)]), ("set", [])]
    elif kind == "metric":
        on_dead = [("metric", dead[0], 1, 1), ("metric", dead[0], U.KEEP, 3), ("metric", dead[1], 1, U.KEEP),
                   ("metric", dead[1], 5, 5)]
        fails = on_dead + [("metric", live, U.KEEP, 3), ("metric", live, 3, U.KEEP), ("metric", live, 1, 1),
                           ("metric", heavy_lo[0], U.KEEP, 2), ("metric", heavy_lo[0], 1, 1),
                           ("metric", eq_hi[0], 3, U.KEEP), ("metric", heavy_hi[0], 2, 2)]
        fails += [("metric", l, 3, 3) for l in d.up_links()]
    else:
        on_dead = [("down", h.nbrs[0])]  # no slot of the row leads there any more
        fails = on_dead + [("down", x) for x in range(len(d.names)) if x not in (h.hub, h.nbrs[0])]
    _, _, up, lists = b.run(kind, fails, range(len(fails)))
    for f in on_dead:
        assert not b.row.touches(f)
        if kind != "down":  # (the node itself is withdrawn when it goes down)
            assert len(lists[fails.index(f)][0]) == 0
    assert up.n_touched == sum(b.row.touches(f) for f in fails) < len(fails)
    assert any(len(ids) for f, (ids, _, _) in zip(fails, lists) if b.row.touches(f))


@pytest.mark.parametrize("kind", ("link", "down", "drain"))
def test_overloaded_nodes_in_the_base_graph(small, kind):
    g, h = small.g, small.h
    plain = small.truth_base[1]
    for drained in (h.nbrs[0], h.hub):  # a neighbour that is transit for the ring behind it; the source
        ovl = np.array(g.ovl).copy()
        ovl[drained] = 1
        b = Bench(loaded(g, (g.rp, g.col, g.met, g.lid, ovl)), h.hub, small.sets)
        try:
            differ = sum(not np.array_equal(x, y) for x, y in zip(b.truth_base[1], plain))
            assert (differ > 0) == (drained != h.hub)  # an overloaded source still forwards
            if kind == "link":
                fails = [("link", l) for l in g.up_links()]
            else:
                fails = [(kind, x) for x in range(len(g.names)) if x != h.hub]
            _, _, up, lists = b.run(kind, fails, range(len(fails)))
            assert any(len(ids) for ids, _, _ in lists)
            if kind == "drain" and drained != h.hub:
                assert len(lists[fails.index(("drain", drained))][0]) == 0  # drained already
        finally:
            b.close()


def test_empty_and_all_dead_rows():
    """A source without a slot, and one whose every slot is a dead self-loop:
    no base record, no entry, no record, and the call succeeds."""
    g, h = U.hub_graph(8)
    rp, col, met, lid, ovl = failed_arrays(g, ("down", h.hub), link_slots(g))
    lone = len(g.names)
    d = loaded(g, (np.append(rp, rp[-1]), col, met, lid, np.append(ovl, 0)), list(g.names) + ["z"])
    for s, deg in ((lone, 0), (h.hub, 8)):
        sets = [[v] for v in range(len(d.names)) if v != s] + [[h.ring[0], h.ring[2]], h.nbrs, []]
        b = Bench(d, s, sets)
        try:
            assert b.deg == deg and not (b.row.bit >= 0).any()
            for kind in ("link", "down"):
                fails = ([("link", l) for l in d.up_links()] if kind == "link"
                         else [("down", x) for x in range(len(d.names)) if x != s])
                assert len(fails) >= 8
                _, rt, up, lists = b.run(kind, fails, range(0, len(fails), 3))
                assert (rt.base_metric == U.U64_MAX).all()
                assert up.base_records == 0 and not any(len(r) for r in up.base())
                assert up.n_entries == up.n_records == up.n_touched == 0 and not up.ptr.any()
        finally:
            b.close()
