"""What-if impact by destination without a device: the restatement
(tests/whatif_impact.py) on hand cases with closed forms.

The per-failure results come from full oracle re-runs on the changed LSDB
(tests/whatif_sets.py Expected.result), reduced to change lists for the link
plan over every link, ascending by link id -- the order of the GPU's plan."""

import numpy as np

import whatif_impact as I
import whatif_routes as R
from openr_amd import topology as T
from test_whatif_routes_host import link_between, prepare

NONE, U64_MAX = I.NONE, I.U64_MAX


def link_plan(topo, s=0):
    """(names, csr, plan links ascending, base, impact of the change lists by node)."""
    names, exp, csr = prepare(topo, s)
    links = sorted(set(int(x) for x in csr[2]))
    W = exp.base[1].shape[1]
    lists = I.lists_of([R.changed_nodes(exp.base, exp.result([l])) for l in links], W)
    return names, csr, links, exp.base, lists, I.impact(*lists, *exp.base)


def ring(n):
    nodes = [f"n{i}" for i in range(n)]
    edges = [(i, (i + 1) % n) for i in range(n)]
    return T._undirected_to_adj(nodes, edges, np.ones(n), np.ones(n), f"ring{n}")


def line(n):
    nodes = [f"n{i}" for i in range(n)]
    return T._undirected_to_adj(nodes, [(i, i + 1) for i in range(n - 1)], np.ones(n - 1),
                                np.ones(n - 1), f"line{n}")


def test_line6_counts_the_links_before_a_node():
    names, csr, links, base, lists, (imp, tptr, tfail, tent) = link_plan(line(6))
    assert names == [f"n{i}" for i in range(6)] and len(links) == 5
    for k in range(6):
        x = imp[k]
        assert x["n_changed"] == x["n_unreachable"] == x["n_metric"] == k
        # cut off is not a metric: the base stays the worst, and nobody is named for it
        assert x["max_metric"] == k and x["max_fail"] == NONE
        assert x["min_width"] == (1 if k else 0)  # the base's: no entry reaches the node
        assert x["reserved"] == 0
        on_path = sorted(links.index(link_between(csr, j, j + 1)) for j in range(k))
        assert list(tfail[int(tptr[k]): int(tptr[k + 1])]) == on_path
    assert int(imp["n_changed"].sum()) == len(lists[1]) == int(tptr[-1]) == 15


def test_ring7_detours_and_their_ties():
    names, csr, links, base, lists, (imp, tptr, tfail, tent) = link_plan(ring(7))
    assert imp[0]["n_changed"] == 0 and imp[0]["max_fail"] == NONE and imp[0]["max_metric"] == 0
    for k in range(1, 7):
        # the node's arc from n0: k links clockwise for k <= 3, 7 - k the other way round
        arc = [(j, j + 1) for j in range(k)] if k <= 3 else [((j + 1) % 7, j) for j in range(k, 7)]
        x = imp[k]
        assert x["n_changed"] == x["n_metric"] == len(arc) == min(k, 7 - k)
        assert x["n_unreachable"] == 0 and x["min_width"] == 1
        assert x["max_metric"] == max(k, 7 - k)  # the other way round
        # every link of the arc sends the node the same detour: the first of them is named
        assert x["max_fail"] == min(links.index(link_between(csr, u, v)) for u, v in arc)
    # the link between n3 and n4 carries nobody: a cold failure inside the plan
    cold = links.index(link_between(csr, 3, 4))
    assert lists[0][cold] == lists[0][cold + 1] and cold not in tfail


def test_ring8_far_node_only_narrows():
    names, csr, links, base, lists, (imp, tptr, tfail, tent) = link_plan(ring(8))
    x = imp[4]
    assert I.popcount(base[1])[4] == 2 and base[0][4] == 4
    assert x["n_changed"] == 8 and x["n_metric"] == 0 and x["n_unreachable"] == 0
    assert x["min_width"] == 1 and x["max_metric"] == 4 and x["max_fail"] == NONE
    assert list(tfail[int(tptr[4]): int(tptr[5])]) == list(range(8))


def test_entries_point_back_into_the_lists():
    names, csr, links, base, (ptr, key, dist, nh), (imp, tptr, tfail, tent) = link_plan(ring(8))
    for k in range(8):
        for i, e in zip(tfail[int(tptr[k]): int(tptr[k + 1])], tent[int(tptr[k]): int(tptr[k + 1])]):
            assert key[int(e)] == k and int(ptr[i]) <= int(e) < int(ptr[i + 1])
    # any order within a key sorts back to the restatement's
    rng = np.random.default_rng(0)
    f, e = tfail.copy(), tent.copy()
    for k in range(8):
        lo, hi = int(tptr[k]), int(tptr[k + 1])
        p = rng.permutation(hi - lo)
        f[lo:hi], e[lo:hi] = f[lo:hi][p], e[lo:hi][p]
    sf, se = I.in_key_order(tptr, f, e)
    assert np.array_equal(sf, tfail) and np.array_equal(se, tent)


def test_wider_entries_do_not_hide_behind_the_base():
    """min_width is over the entries that reach the key, not a min with the
    base; max_fail needs a metric above the base; an unreachable base stays."""
    ptr = np.array([0, 2, 3, 3, 5], np.uint64)
    key = np.array([1, 2, 1, 2, 1], np.uint32)
    dist = np.array([9, U64_MAX, 9, 7, 5], np.uint64)
    nh = np.array([[0b111], [0], [0b11], [0b1], [0b1111]], np.uint32)
    base_dist = np.array([0, 5, 7, U64_MAX], np.uint64)
    base_nh = np.array([[0], [0b1], [0b11], [0]], np.uint32)
    imp, tptr, tfail, tent = I.impact(ptr, key, dist, nh, base_dist, base_nh)
    assert list(imp[1]) == [3, 0, 2, 2, 9, 0, 0]  # widths 3, 2, 4 against a base of 1
    assert list(imp[2]) == [2, 1, 1, 1, 7, NONE, 0]  # metric 7 again with other hops: not worse
    assert list(imp[0]) == [0, 0, 0, 0, 0, NONE, 0] and list(imp[3]) == [0, 0, 0, 0, U64_MAX, NONE, 0]
    assert list(tptr) == [0, 0, 3, 5, 5] and list(tfail) == [0, 1, 3, 0, 3] and list(tent) == [0, 2, 4, 1, 3]
