"""spf_twin_classes (include/openr_spf.h): nodes with equal distinct-neighbour
lists share a class, classes numbered by their first member -- the classes
msbfs_kernel's quotient sweep keeps one frontier slot for.  Host only: no
device needed."""

import ctypes as C

import numpy as np

from openr_amd import _native as N
from openr_amd import topology as T


def neighbour_lists(n, src, dst):
    lists = [sorted(set(int(d) for s, d in zip(src, dst) if s == v)) for v in range(n)]
    ptr = np.zeros(n + 1, np.uint32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    ids = np.array([x for l in lists for x in l] or [0], np.uint32)
    return ptr, ids


def classes(ptr, ids):
    n = len(ptr) - 1
    cls = np.zeros(max(1, n), np.uint32)
    k = C.c_uint32()
    N.raise_for(N.lib.spf_twin_classes(n, N.ptr(ptr), N.ptr(ids), N.ptr(cls), C.byref(k)), N.global_error())
    return cls[:n], k.value


def test_small_fabric_classes_are_pods_racks_planes_spines_and_singletons():
    topo = T.fabric(2 * 2 + 3 * (2 + 3), ssw_per_plane=2, fsw_per_pod=2, rsw_per_pod=3)
    ptr, ids = neighbour_lists(topo.n_nodes, topo.adj_src.tolist(), topo.adj_dst.tolist())
    cls, k = classes(ptr, ids)
    want = {}
    for v, name in enumerate(topo.nodes):
        marker, group, sw = name.split("-")
        # spines by plane, rack switches by pod, every fabric switch alone
        want.setdefault((marker, group, sw if int(marker) == T.K_FSW else ""), []).append(v)
    got = {}
    for v, c in enumerate(cls.tolist()):
        got.setdefault(c, []).append(v)
    assert sorted(got.values()) == sorted(want.values())
    assert k == len(want) == 2 + 3 * 2 + 3
    # numbered by first member
    firsts = [min(m) for _, m in sorted(got.items())]
    assert firsts == sorted(firsts) and sorted(got) == list(range(k))


def test_lists_that_differ_in_one_element_are_not_merged():
    #  0 and 1: {4, 5, 6};  2: {4, 5, 7} (one element off);  3: {4, 5} (a prefix);
    #  8: {} and 9: {} (isolated nodes are twins of each other)
    lists = {0: [4, 5, 6], 1: [4, 5, 6], 2: [4, 5, 7], 3: [4, 5], 4: [0, 1, 2, 3], 5: [0, 1, 2, 3],
             6: [0, 1], 7: [2], 8: [], 9: []}
    ptr = np.zeros(11, np.uint32)
    ptr[1:] = np.cumsum([len(lists[v]) for v in range(10)])
    ids = np.array([x for v in range(10) for x in lists[v]], np.uint32)
    cls, k = classes(ptr, ids)
    assert cls.tolist() == [0, 0, 1, 2, 3, 3, 4, 5, 6, 6]
    assert k == 7


def test_arguments_and_symbols():
    ptr = np.zeros(1, np.uint32)
    k = C.c_uint32(5)
    cls = np.zeros(1, np.uint32)
    assert N.lib.spf_twin_classes(0, N.ptr(ptr), None, N.ptr(cls), C.byref(k)) == N.SPF_OK and k.value == 0
    assert N.lib.spf_twin_classes(0, None, None, N.ptr(cls), C.byref(k)) == N.SPF_E_INVALID
    bad = np.array([0, 2, 1], np.uint32)
    assert N.lib.spf_twin_classes(2, N.ptr(bad), N.ptr(bad), N.ptr(np.zeros(2, np.uint32)),
                                  C.byref(k)) == N.SPF_E_INVALID
    lib = C.CDLL(str(N.LIB_PATH))
    for name in ("spf_twin_classes", "spf_graph_quotient"):
        assert hasattr(lib, name) and name in N.PROTOTYPES
