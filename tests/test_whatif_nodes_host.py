"""Node what-if batches without a device: the expected-value helper
(tests/whatif_nodes.py) pinned to the oracle's own what-if digests where the
two must agree, and the C ABI's new entry points.

Ignoring a leaf's only link and deleting the leaf are the same SPF run, so
DOWN of a degree-1 node x must give exactly oracle.whatif_digests for x's
link; draining a leaf, or a node that is drained already, changes nothing.
"""

import ctypes as C

import numpy as np
import pytest

import whatif_nodes as WN
from oracle import NameTable, OracleLinkState, whatif_digests
from openr_amd import topology as T
from openr_amd.link_state import LinkState


def line6():
    nodes = [f"n{i}" for i in range(6)]
    return T._undirected_to_adj(nodes, [(i, i + 1) for i in range(5)], np.ones(5), np.ones(5),
                                "line6")


def tree20():
    """A random tree on 16 nodes, 4 pendant nodes hung on it, metrics U[1, 9]
    per direction; two inner nodes drained."""
    rng = np.random.default_rng(20)
    nodes = [f"t{i:02d}" for i in range(20)]
    links = [(int(rng.integers(0, i)), i) for i in range(1, 16)]
    links += [(int(rng.integers(0, 16)), i) for i in range(16, 20)]
    topo = T._undirected_to_adj(nodes, links, rng.integers(1, 10, len(links)),
                                rng.integers(1, 10, len(links)), "tree20")
    inner = sorted({a for a, _ in links} - {0})[:2]
    for v in inner:
        topo.lsdb.dbs["is_overloaded"][WN.db_index(topo.lsdb, nodes[v])] = 1
    return topo


def flat(topo):
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names, rp, col, met, lid, ovl = ls.flatten()
    orc = OracleLinkState()
    orc.update_packed(topo.lsdb)
    return ls, names, orc, rp, col, lid, ovl


def leaves(rp, col, s):
    return [v for v in range(len(rp) - 1)
            if v != s and len(set(int(c) for c in col[rp[v]: rp[v + 1]]) - {v}) == 1
            and rp[v + 1] - rp[v] == 1]


@pytest.mark.parametrize("make,s", [(line6, 2), (tree20, 0)], ids=["line6", "tree20"])
def test_down_of_a_leaf_is_its_only_link_ignored(make, s):
    topo = make()
    ls, names, orc, rp, col, lid, ovl = flat(topo)
    exp = WN.Expected(topo.lsdb, names, rp, col, s)
    lv = leaves(rp, col, s)
    assert len(lv) >= 2
    fails = []
    for x in lv:
        lk = ls._link(int(lid[rp[x]]))
        fails.append((lk._n1, lk._if1))
    obase, want = whatif_digests(orc, NameTable(names), names[s], fails)
    assert exp.base_digest == obase
    for x, w in zip(lv, want):
        assert exp.digest(x, "down") == w, names[x]
    assert any(w != obase for w in want)  # a reachable leaf vanishes: not the base


@pytest.mark.parametrize("make,s", [(line6, 2), (tree20, 0)], ids=["line6", "tree20"])
def test_drain_of_a_leaf_changes_nothing(make, s):
    topo = make()
    ls, names, orc, rp, col, lid, ovl = flat(topo)
    exp = WN.Expected(topo.lsdb, names, rp, col, s)
    for x in leaves(rp, col, s):
        assert exp.digest(x, "drain") == exp.base_digest, names[x]


def test_drain_of_a_drained_node_changes_nothing_and_of_a_transit_does():
    topo = tree20()
    ls, names, orc, rp, col, lid, ovl = flat(topo)
    exp = WN.Expected(topo.lsdb, names, rp, col, 0)
    drained = [int(v) for v in np.nonzero(ovl)[0]]
    assert len(drained) == 2
    for x in drained:
        assert exp.digest(x, "drain") == exp.base_digest
    # the helper does drain: some inner node of the tree cuts its subtree off
    bd = exp.base[0]
    inner = [v for v in range(1, 20) if v not in drained and rp[v + 1] - rp[v] > 1
             and bd[v] != WN.L.U64_MAX]
    assert any(exp.digest(x, "drain") != exp.base_digest for x in inner)


def test_symbols_exported_and_null_arguments():
    from openr_amd import _native as N

    lib = C.CDLL(str(N.LIB_PATH))
    for name in ("spf_whatif_plan_create_nodes", "spf_whatif_plan_nodes", "spf_whatif_plan_kind"):
        assert hasattr(lib, name), name
        assert name in N.PROTOTYPES
    h = C.c_void_p(0x1234)
    st = N.lib.spf_whatif_plan_create_nodes(None, 0, N.SPF_WHATIF_NODE_DOWN, None, 0, C.byref(h))
    assert st == N.SPF_E_INVALID and h.value == 0x1234  # no ctx: *out untouched
    assert N.lib.spf_whatif_plan_create_nodes(None, 0, N.SPF_WHATIF_NODE_DRAIN, None, 0,
                                              None) == N.SPF_E_INVALID
    k = C.c_uint32(77)
    assert N.lib.spf_whatif_plan_kind(None, C.byref(k)) == N.SPF_E_INVALID and k.value == 77
    ids = np.zeros(1, np.uint32)
    assert N.lib.spf_whatif_plan_nodes(None, N.ptr(ids)) == N.SPF_E_INVALID
    assert (N.SPF_WHATIF_NODE_DOWN, N.SPF_WHATIF_NODE_DRAIN) == (1, 2)
