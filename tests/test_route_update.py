"""DecisionRouteDb.calculateUpdate / update (Decision.cpp:111-162) restated
next to the solver: the expectation of the GPU route-delta tests.  No device
needed.

The pinned case is the reference's own (DecisionTest.cpp
SimpleRingTopologyFixture.DuplicateMplsRoutes, verifyRouteInUpdateNoDelete at
:1784-1799): on the ring 1-2, 1-3, 2-4, 3-4 (metric 10) nodes 1 and 2 first
share label 2, then node 1 takes label 1.  Against an empty database, and
against the database built before the change, label 2 is in the MPLS updates
exactly once and nothing is deleted.  Node 1's MPLS routes before and after
are data under tests/golden/route_update_duplicate_mpls.json, worked out from
that topology by buildRouteDb's rules (Decision.cpp:586-674) for the three
nodes the reference checks: 1, 2 and 3."""

import copy
import json
from pathlib import Path

import pytest

from openr_amd.spf_solver import (DecisionRouteDb, DecisionRouteUpdate, MplsAction, NextHopThrift,
                                  PrefixEntry, RibMplsEntry, RibUnicastEntry, createNextHop)


def nh(ifname, metric, action=None, swap=None, neighbor=None):
    act = None if action is None else (MplsAction(action, swap, None) if swap else MplsAction(action))
    return createNextHop(bytes(16), ifname, metric, act, "0", neighbor)


def mpls(routes):
    db = DecisionRouteDb()
    for label, nhs in routes.items():
        db.addMplsRoute(RibMplsEntry(label, set(nhs)))
    return db


GOLDEN = json.loads((Path(__file__).parent / "golden" / "route_update_duplicate_mpls.json").read_text())


def table(t):
    return {int(label): [POP] if nhs == "POP" else [nh(i, m, a, sw, nb) for i, m, a, sw, nb in nhs]
            for label, nhs in t.items()}


POP = NextHopThrift(bytes(16), None, 0, MplsAction("POP_AND_LOOKUP"), "0", None)
BEFORE, AFTER = table(GOLDEN["nodes"]["1"]["before"]), table(GOLDEN["nodes"]["1"]["after"])


@pytest.mark.parametrize("node", ["1", "2", "3"])
def test_reference_duplicate_mpls_routes_case(node):
    """verifyRouteInUpdateNoDelete(node, 2, db) of the reference, against the
    empty database (before and after the change) and against the database
    built before the change: label 2 once in the updates, nothing deleted."""
    g = GOLDEN["nodes"][node]
    before, after = table(g["before"]), table(g["after"])
    for old, new in ((DecisionRouteDb(), mpls(before)), (DecisionRouteDb(), mpls(after)),
                     (mpls(before), mpls(after))):
        d = old.calculateUpdate(new)
        assert [r.label for r in d.mplsRoutesToUpdate].count(2) == 1
        assert d.mplsRoutesToDelete == []
    d = mpls(before).calculateUpdate(mpls(after))
    assert [r.label for r in d.mplsRoutesToUpdate] == g["updates"]  # the others compare equal
    got = mpls(before)
    got.update(d)
    assert got == mpls(after)


def unicast(routes):
    db = DecisionRouteDb()
    for prefix, nhs in routes.items():
        db.addUnicastRoute(RibUnicastEntry(prefix, set(nhs), PrefixEntry(prefix), "0"))
    return db


def test_update_of_calculate_update_turns_old_into_new():
    old = unicast({"fd00::1/128": [nh("a", 1)], "fd00::2/128": [nh("a", 2), nh("b", 2)],
                   "fd00::3/128": [nh("b", 5)]})
    old.mplsRoutes = mpls(BEFORE).mplsRoutes
    new = unicast({"fd00::2/128": [nh("a", 2)], "fd00::3/128": [nh("b", 5)], "fd00::4/128": [nh("c", 9)]})
    new.mplsRoutes = mpls(AFTER).mplsRoutes
    d = old.calculateUpdate(copy.deepcopy(new))
    assert sorted(d.unicastRoutesToUpdate) == ["fd00::2/128", "fd00::4/128"]
    assert d.unicastRoutesToDelete == ["fd00::1/128"]
    got = copy.deepcopy(old)
    got.update(d)
    assert got == new and old != new
    # the other way: a label goes away
    back = new.calculateUpdate(copy.deepcopy(old))
    assert back.mplsRoutesToDelete == [1] and [r.label for r in back.mplsRoutesToUpdate] == [2]
    got.update(back)
    assert got == old


def test_equal_databases_give_an_empty_update():
    a, b = unicast({"fd00::1/128": [nh("a", 1), nh("b", 1)]}), unicast({"fd00::1/128": [nh("b", 1), nh("a", 1)]})
    d = a.calculateUpdate(b)
    assert d.empty() and d == DecisionRouteUpdate()
    # a metric alone changes the entry
    c = unicast({"fd00::1/128": [nh("a", 1), nh("b", 2)]})
    assert list(a.calculateUpdate(c).unicastRoutesToUpdate) == ["fd00::1/128"]
