"""Link-set what-if batches without a device: the expected-value helper
(tests/whatif_sets.py) pinned where it must agree with pins that exist --
a one-member set is the oracle's own single-link what-if, linksFromNode(x) is
whatif_nodes' DOWN of x -- and the set families of the GPU tests built and
their conditions asserted from the helper's base render alone.
"""

import numpy as np
import pytest

import whatif_lists as L
import whatif_nodes as WN
import whatif_sets as WS
from oracle import NameTable, OracleLinkState, whatif_digests
from openr_amd import topology as T
from openr_amd.link_state import LinkState

RAND = {f"rand{s}": (lambda s=s: T.random_graph(70, 180, 300 + s, max_metric=5, parallel_frac=0.2,
                                                overload_frac=0.1, link_overload_frac=0.05))
        for s in range(4)}
GRAPHS = dict(RAND, wan200=lambda: T.wan(200, 100, seed=6))
SEED = 11  # of the random sets; changed here, on the CPU, if a condition below fails


def flat(topo, s=0):
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names, rp, col, met, lid, ovl = ls.flatten()
    exp = WS.Expected(topo.lsdb, ls, names, rp, col, s)
    dag = WS.Dag(rp, col, met, lid, ovl, exp.base[0], s)
    return ls, names, exp, dag, (rp, col, met, lid, ovl)


@pytest.mark.parametrize("name", ["rand0", "rand1"])
def test_one_member_sets_are_the_oracles_single_link_digests(name):
    topo = RAND[name]()
    ls, names, exp, dag, _ = flat(topo)
    orc = OracleLinkState()
    orc.update_packed(topo.lsdb)
    fails = []
    for l in dag.up:
        lk = ls._link(l)
        fails.append((lk._n1, lk._if1))
    obase, want = whatif_digests(orc, NameTable(names), names[0], fails)
    assert exp.base_digest == obase
    for l, w in zip(dag.up, want):
        assert exp.digest([l]) == w, l
    # only a tight link can change anything (a tight link beside an equal
    # parallel one changes nothing)
    assert all(l in dag.tight for l, w in zip(dag.up, want) if w != obase)
    assert 0 < sum(w != obase for w in want) <= len(dag.tight)


@pytest.mark.parametrize("name", ["rand0", "rand1"])
def test_links_from_node_is_node_down(name):
    topo = RAND[name]()
    ls, names, exp, dag, (rp, col, met, lid, ovl) = flat(topo)
    nodes = WN.Expected(topo.lsdb, names, rp, col, 0)
    assert nodes.base_digest == exp.base_digest
    for x in range(1, len(names)):
        links = sorted(set(int(l) for l in lid[rp[x]: rp[x + 1]]))
        assert exp.digest(links) == nodes.digest(x, "down"), names[x]


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_families_meet_their_conditions(name):
    ls, names, exp, dag, (rp, col, met, lid, ovl) = flat(GRAPHS[name]())
    fam = WS.families(ls, dag, SEED)
    bd = exp.base[0]
    rand = name.startswith("rand")
    for k in ("nested", "disjoint", "cold", "empty", "random"):
        assert fam[k], k
    if rand:  # equal-cost paths (metrics U[1, 5]), parallel and overloaded links: the rand graphs'
        assert fam["ecmp_cut"] and fam["same_head"] and fam["parallel"]
        assert len(fam["mixed"]) == 2 and len(fam["cold"]) == 2
    for links in fam["ecmp_cut"]:
        (b,) = dag.heads(links)
        assert len(links) >= 2 and sorted(dag.into[b]) == links
        d = exp.result(links)[0]
        assert d[b] != bd[b]  # every tight in-link cut: the metric moves, or b is unreachable
    for links in fam["parallel"]:
        ends = {tuple(sorted((ls._link(l)._n1, ls._link(l)._n2))) for l in links}
        assert len(links) >= 2 and len(ends) == 1
    for l, m in fam["nested"]:
        assert dag.tight[m][1] in dag.desc(dag.tight[l][1]) and dag.tight[m][1] != dag.tight[l][1]
    for links in fam["same_head"]:
        assert len(links) == 2 and len(dag.heads(links)) == 1
    for l, m in fam["disjoint"]:
        assert not (dag.desc(dag.tight[l][1]) & dag.desc(dag.tight[m][1]))
    for links in fam["mixed"]:
        assert any(l in dag.tight for l in links) and any(l in dag.loose for l in links)
        assert any(not ls._link(l).isUp() for l in links)
        assert exp.digest(links) != exp.base_digest
    for links in fam["cold"] + fam["empty"]:
        assert not dag.heads(links) and exp.digest(links) == exp.base_digest
    assert sorted(len(x) for x in fam["random"]) == [2, 2, 3, 3, 5, 5, 8, 8]
    assert any(len(dag.heads(x)) >= 2 and exp.digest(x) != exp.base_digest for x in fam["random"])
    for links in fam["same_head"] + fam["nested"] + fam["disjoint"]:
        assert dag.heads(links)  # a tight member: hot (an equal parallel link may still absorb it)
