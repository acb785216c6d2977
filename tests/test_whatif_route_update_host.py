"""What-if route updates without a device: the checker
(tests/whatif_route_update.py) on hand cases with known answers, the checker
against the oracle's link-level next hops (orc_ls_nexthops_json on an LSDB with
the failure applied), the facts the GPU tests rely on for their seeded
multigraph, and the row-table builder
(openr_amd/csrc/whatif_route_update_host.cpp) against brute force, compiled
into a temporary directory and run as a child process under the sanitizers."""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import whatif_route_update as U
import whatif_routes as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"

SETS = [[1], [2], [3], [4], [5], [6], [3, 5], [2, 6], [0, 3], []]
VIA_N1 = [0, 2, 3, 4, 6]  # the sets of SETS whose base route has n1 among its next hops


class Case:
    def __init__(self, g, s, sets):
        self.g, self.s = g, s
        self.flat = R.flatten(sets)
        self.sets = sets
        self.row = U.Row(g.rp, g.col, g.met, g.lid, s)
        self.base = U.oracle_result(g, s, U.failed_oracle(g, None))
        self.routes = R.routes(*self.base, self.flat, s)
        self.base_recs = U.base_records(self.row, *self.base, self.flat, self.routes)

    def under(self, fail):
        """(change list, route list ids, update list, oracle) of `fail`."""
        orc = U.failed_oracle(self.g, fail)
        node, dist, nh = R.changed_nodes(self.base, U.oracle_result(self.g, self.s, orc))
        ids, _, _ = R.expected(*self.base, node, dist, nh, self.flat, self.s, self.routes)
        upd = U.expected(self.row, fail, *self.base, node, dist, nh, self.flat, self.routes)
        return node, ids, upd, orc

    def check_oracle(self, fail, upd, orc, which=None):
        """Every set's records under the failure -- the update entry's where
        listed, the base's otherwise -- are the oracle's link-level next hops."""
        listed = {int(k): r for k, r in zip(upd[0], upd[2])}
        for k in (range(len(self.sets)) if which is None else which):
            members = self.sets[k]
            if not members or self.s in members:
                assert k not in listed
                continue
            want = U.oracle_records(self.g, self.s, orc, members)
            got = listed.get(k, self.base_recs[k])
            assert np.array_equal(got, want), (fail, k, got, want)
            if k in listed:
                assert not np.array_equal(want, self.base_recs[k]), (fail, k)


@pytest.fixture(scope="module")
def bundle():
    g = U.bundle_graph()
    c = Case(g, 0, SETS)
    links = g.links_between(0, 1)
    w = {l: int(g.met[next(e for e in range(g.rp[0], g.rp[1]) if g.lid[e] == l)]) for l in links}
    c.equal = sorted(l for l in links if w[l] == 1)
    c.heavy = next(l for l in links if w[l] == 3)
    assert len(c.equal) == 2
    return c


def test_base_records_of_the_bundle(bundle):
    c = bundle
    assert [len(r) for r in c.base_recs] == [2, 1, 3, 3, 2, 1, 3, 1, 0, 0]
    assert [int(r[0]) >> 32 for r in c.base_recs[:8]] == [1, 1, 2, 3, 2, 2, 2, 1]
    c.check_oracle(None, (np.zeros(0, np.uint32), None, []), U.failed_oracle(c.g, None))


def test_failing_a_bundle_member_is_cold_at_node_level(bundle):
    c = bundle
    for member in c.equal:
        node, ids, upd, orc = c.under(("link", member))
        assert len(node) == 0 and len(ids) == 0  # no change list entry, no route list entry
        assert list(upd[0]) == VIA_N1
        for k, m, rec in zip(*upd):
            assert int(m) == int(c.routes[0][k]) and len(rec) == len(c.base_recs[k]) - 1
            assert set(rec.tolist()) < set(c.base_recs[k].tolist())
        c.check_oracle(("link", member), upd, orc)


def test_raising_a_member_takes_it_out(bundle):
    c = bundle
    fail = ("metric", c.equal[0], 2, 2)
    node, ids, upd, orc = c.under(fail)
    assert len(node) == 0 and len(ids) == 0
    assert list(upd[0]) == VIA_N1
    assert [len(r) for r in upd[2]] == [len(c.base_recs[k]) - 1 for k in VIA_N1]
    c.check_oracle(fail, upd, orc)
    # a raise of the direction into the source alone changes nothing here
    fail = ("metric", c.equal[0], U.KEEP, 9)
    node, ids, upd, orc = c.under(fail)
    assert len(node) == 0 and len(upd[0]) == 0
    c.check_oracle(fail, upd, orc)


def test_lowering_the_heavier_link_onto_the_tie_adds_it(bundle):
    c = bundle
    fail = ("metric", c.heavy, 1, U.KEEP)
    node, ids, upd, orc = c.under(fail)
    assert len(node) == 0 and len(ids) == 0
    assert list(upd[0]) == VIA_N1
    assert [len(r) for r in upd[2]] == [len(c.base_recs[k]) + 1 for k in VIA_N1]
    c.check_oracle(fail, upd, orc)


def test_failing_both_equal_members_moves_the_metric(bundle):
    c = bundle
    fail = ("set", c.equal)
    node, ids, upd, orc = c.under(fail)
    assert 1 in node and len(ids) > 0
    got = {int(k): (int(m), len(r)) for k, m, r in zip(*upd)}
    # n1 moves to metric 3, over the heavier link and around through n2 and n3 alike, and n5
    # behind it to 4; n3 and n4 keep their metric through n2 alone
    assert got == {0: (3, 2), 2: (2, 1), 3: (3, 1), 4: (4, 2), 6: (2, 1)}
    assert set(int(k) for k in ids) <= set(got)
    c.check_oracle(fail, upd, orc)
    for kind in ("down", "drain"):
        for x in (1, 2, 3):
            fail = (kind, x)
            _, _, upd, orc = c.under(fail)
            c.check_oracle(fail, upd, orc)


@pytest.fixture(scope="module")
def seeded():
    g = U.seeded_graph()
    sets, at = R.case_sets(len(g.names), 0)
    return Case(g, 0, sets)


def test_the_seeded_multigraph_has_what_the_gpu_tests_rely_on(seeded):
    """At least 20 pairs that the route lists do not contain, a failure that
    touches the source's row and has a change list, and the checker equal to
    the oracle on the touching failures and on some others."""
    c = seeded
    extra = touching_with_changes = 0
    links = c.g.up_links()
    rng = np.random.default_rng(1)
    others = set(int(l) for l in rng.choice(links, 12, replace=False))
    probe = list(range(1, 30)) + list(range(len(c.g.names), len(c.g.names) + 20))
    for l in links:
        fail = ("link", l)
        touches = c.row.touches(fail)
        if not touches and l not in others:
            continue
        node, ids, upd, orc = c.under(fail)
        assert set(int(k) for k in ids) <= set(int(k) for k in upd[0])
        extra += len(set(int(k) for k in upd[0]) - set(int(k) for k in ids))
        touching_with_changes += bool(touches and len(node))
        if not touches:
            assert len(upd[0]) == len(ids)
        c.check_oracle(fail, upd, orc, probe)
    assert extra >= 20 and touching_with_changes >= 1, (extra, touching_with_changes)


@pytest.fixture(scope="module")
def hub():
    g, h = U.hub_graph(8)
    c = Case(g, h.hub, U.hub_sets(g, h))
    c.h = h
    return c


def test_the_checker_meets_the_oracle_with_the_source_in_the_middle(hub):
    """row0 != 0, and the source is the higher end of the links to half of its
    neighbours: Row.weights' m_lo / m_hi convention against the oracle."""
    c, g, h = hub, hub.g, hub.h
    assert len(g.names) == 9 and int(g.rp[h.hub]) > 0 and c.row.q[0] == int(g.rp[h.hub])
    assert min(h.nbrs) < h.hub < max(h.nbrs) and len(c.row.q) == 8
    for x in (h.lower_bundle, h.upper_bundle):
        assert sorted(int(c.row.w[t]) for t in range(8) if c.row.head[t] == x) == [2, 2, 4]
    ecmp = [k for k, r in enumerate(c.base_recs) if len(set(c.row.head[(r & np.uint64(0xFFFFFFFF)).astype(np.int64) - c.row.q[0]])) > 1]
    assert len(ecmp) >= 2  # sets with next hops towards two neighbours
    fails = U.hub_failures(g, h)
    lists = []
    for fail in fails:
        _, _, upd, orc = c.under(fail)
        c.check_oracle(fail, upd, orc)
        lists.append(upd)
    assert any(len(u[0]) for f, u in zip(fails, lists) if f[0] == "link")
    U.one_direction_moves(g, h, fails, lists)


def test_row_tables_against_brute_force_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "whatif_route_update_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "whatif_route_update_host_check.cpp"),
                    str(CSRC / "whatif_route_update_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
