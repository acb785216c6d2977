"""What-if route lists without a device: the checker (tests/whatif_routes.py)
on hand cases with known answers, the oracle's word on the properties the GPU
tests assert of their seeded sets, and the inverse-index builder
(openr_amd/csrc/whatif_routes_host.cpp) against a brute-force one, compiled
into a temporary directory and run as a child process under the sanitizers.

The per-failure results come from full oracle re-runs on the changed LSDB
(tests/whatif_sets.py Expected.result), reduced to change lists."""

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import whatif_routes as R
import whatif_sets as WS
from openr_amd import topology as T
from openr_amd.link_state import LinkState

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"
U64_MAX = R.U64_MAX


def prepare(topo, s=0):
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names, rp, col, met, lid, ovl = ls.flatten()
    return names, WS.Expected(topo.lsdb, ls, names, rp, col, s), (rp, col, lid)


def link_between(csr, u, v):
    rp, col, lid = csr
    return next(int(lid[e]) for e in range(rp[u], rp[u + 1]) if col[e] == v)


def route_list(exp, link, sets, s=0):
    node, dist, nh = R.changed_nodes(exp.base, exp.result([link]))
    return R.expected(*exp.base, node, dist, nh, sets, s)


def bits(*js):
    return sum(1 << j for j in js)


def test_diamond_anycast_keeps_its_metric_and_loses_a_next_hop():
    nodes = [f"n{i}" for i in range(4)]
    edges = [(0, 1), (0, 2), (1, 3), (2, 3)]
    topo = T._undirected_to_adj(nodes, edges, np.ones(4), np.ones(4), "diamond")
    names, exp, csr = prepare(topo)
    assert names == nodes
    sets = [[1, 2], [3], [1], [2]]  # anycast on the two corners beside the source, the far corner
    bm, bw = R.routes(*exp.base, sets, 0)
    assert list(bm) == [1, 2, 1, 1] and [int(w[0]) for w in bw] == [bits(0, 1), bits(0, 1), 1, 2]
    ids, m, w = route_list(exp, link_between(csr, 0, 1), sets)
    # n1 moves to metric 3 behind n2: the anycast keeps metric 1 through n2 alone, the far
    # corner keeps metric 2 and loses the hop over n1, n1's own route moves, n2's does not
    assert list(ids) == [0, 1, 2]
    assert list(m) == [1, 2, 3] and [int(x[0]) for x in w] == [bits(1), bits(1), bits(1)]
    ids, m, w = route_list(exp, link_between(csr, 1, 3), sets)
    assert list(ids) == [1] and list(m) == [2] and int(w[0, 0]) == bits(1)


def test_line_tail_is_withdrawn():
    nodes = [f"n{i}" for i in range(6)]
    topo = T._undirected_to_adj(nodes, [(i, i + 1) for i in range(5)], np.ones(5), np.ones(5), "line6")
    names, exp, csr = prepare(topo)
    sets = [[4, 5], [2, 5], [5], [1], []]
    bm, _ = R.routes(*exp.base, sets, 0)
    assert list(bm) == [4, 2, 5, 1, U64_MAX]
    ids, m, w = route_list(exp, link_between(csr, 3, 4), sets)
    assert list(ids) == [0, 2]  # every member in the tail: withdrawn; [2, 5] keeps n2
    assert (m == U64_MAX).all() and not w.any()
    ids, m, w = route_list(exp, link_between(csr, 1, 2), sets)
    assert list(ids) == [0, 1, 2] and (m == U64_MAX).all() and not w.any()


def test_a_set_that_holds_the_source_never_moves():
    nodes = [f"n{i}" for i in range(4)]
    edges = [(0, 1), (0, 2), (1, 3), (2, 3)]
    topo = T._undirected_to_adj(nodes, edges, np.ones(4), np.ones(4), "diamond")
    names, exp, csr = prepare(topo)
    sets = [[0], [1, 0], [3, 1, 0, 0]]
    bm, bw = R.routes(*exp.base, sets, 0)
    assert list(bm) == [0, 0, 0] and not bw.any()
    for pair in edges:
        ids, _, _ = route_list(exp, link_between(csr, *pair), sets)
        assert len(ids) == 0


def test_repeated_members_and_identical_sets():
    nodes = [f"n{i}" for i in range(4)]
    topo = T._undirected_to_adj(nodes, [(0, 1), (0, 2), (1, 3), (2, 3)], np.ones(4), np.ones(4), "diamond")
    names, exp, csr = prepare(topo)
    ids, m, w = route_list(exp, link_between(csr, 0, 1), [[1, 1, 2], [1, 2], [1, 2]])
    assert list(ids) == [0, 1, 2] and list(m) == [1, 1, 1] and (w == bits(1)).all()


def test_the_seeded_sets_show_every_kind_of_change():
    """What test_gpu_whatif_routes.py asserts of its outputs, confirmed on the
    CPU with the oracle for the seed in use."""
    from test_gpu_whatif import SMALL

    names, exp, csr = prepare(next(make for n, make, _ in SMALL if n == "rand0")())
    sets, at = R.case_sets(len(names), 0)
    flat = R.flatten(sets)
    base = R.routes(*exp.base, flat, 0)
    nh_only = metric = listed_c = False
    for l in sorted(set(int(x) for x in csr[2])):
        node, dist, nh = R.changed_nodes(exp.base, exp.result([l]))
        ids, m, w = R.expected(*exp.base, node, dist, nh, flat, 0, base)
        nh_only |= bool((m == base[0][ids]).any())
        metric |= bool((m != base[0][ids]).any())
        listed_c |= at["c"] in ids
        assert at["e"] not in ids and at["h"] not in ids and 0 not in ids
    assert nh_only and metric and listed_c


def test_inverse_index_against_brute_force_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "whatif_routes_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "whatif_routes_host_check.cpp"),
                    str(CSRC / "whatif_routes_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
