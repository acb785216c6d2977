"""LinkState drop-in: the reference's ``openr::LinkState`` API over the MI355X engine.

Python mirror of ``openr/decision/LinkState.h:82-469`` (same method names,
argument meaning and error behaviour) backed by the C-ABI facade
``include/openr_linkstate.h``: LSDB bookkeeping on the host, every shortest
path batch on the GPU.  Parity tests drive this class exactly like the
reference's ``LinkStateTest.cpp`` / ``DecisionTest.cpp`` drive the C++ one.
"""

from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from collections.abc import Mapping
from typing import Dict, Iterable, List, Optional, Sequence, Set, Tuple, Union

from . import _native as N
from .lsdb import K_DEFAULT_AREA, AdjacencyDatabase, PackedLsdb, pack

LinkStateMetric = int


@dataclass(frozen=True)
class LinkStateChange:
    """``LinkState::LinkStateChange`` (LinkState.h:306-325)."""

    topologyChanged: bool = False
    linkAttributesChanged: bool = False
    nodeLabelChanged: bool = False


@dataclass
class PrefixTable:
    """The prefix table of allSourcesPrefixRoutes (spf_mplan_prefix_routes), in
    CSR form: prefix p's entries are [pfx_ptr[p], pfx_ptr[p + 1]) of node (csr
    id of the advertiser), path_preference, source_preference, distance (int32
    each) and min_nexthop (int64; <= 0: none).  prefixes: a name per prefix
    (spf_solver.prefixTable fills it; optional)."""

    pfx_ptr: "object"
    node: "object"
    path_preference: "object"
    source_preference: "object"
    distance: "object"
    min_nexthop: "object"
    prefixes: Optional[List[str]] = None


class Link:
    """Snapshot of ``openr::Link`` (LinkState.h:82-175) taken at query time."""

    __slots__ = ("_n1", "_n2", "_if1", "_if2", "_m1", "_m2", "_l1", "_l2",
                 "_o1", "_o2", "_up", "hash", "_key", "_area", "_v4", "_v6")

    def __init__(self, ls: "LinkState", d: N.LsLinkDesc, link_id: int = -1) -> None:
        name = ls._name
        self._n1, self._n2 = name(d.node1), name(d.node2)
        self._if1, self._if2 = d.if1.decode(), d.if2.decode()
        self._m1, self._m2 = int(d.metric1), int(d.metric2)
        self._l1, self._l2 = int(d.adj_label1), int(d.adj_label2)
        self._o1, self._o2 = bool(d.overload1), bool(d.overload2)
        self._up = bool(d.is_up)
        self.hash = int(d.hash)
        self._key = tuple(sorted([(self._n1, self._if1), (self._n2, self._if2)]))
        self._area = ls.getArea()
        self._v4 = (bytes(d.nh_v4_1[:4]), bytes(d.nh_v4_2[:4]))
        self._v6 = (bytes(d.nh_v6_1[:16]), bytes(d.nh_v6_2[:16]))

    def _side(self, node: str) -> int:
        if node == self._n1:
            return 0
        if node == self._n2:
            return 1
        raise ValueError(node)  # std::invalid_argument in the reference

    def getArea(self) -> str:
        return self._area

    def getOtherNodeName(self, node: str) -> str:
        return self._n2 if self._side(node) == 0 else self._n1

    def firstNodeName(self) -> str:
        return self._key[0][0]

    def secondNodeName(self) -> str:
        return self._key[1][0]

    def getIfaceFromNode(self, node: str) -> str:
        return (self._if1, self._if2)[self._side(node)]

    def getMetricFromNode(self, node: str) -> int:
        return (self._m1, self._m2)[self._side(node)]

    def getAdjLabelFromNode(self, node: str) -> int:
        return (self._l1, self._l2)[self._side(node)]

    def getOverloadFromNode(self, node: str) -> bool:
        return (self._o1, self._o2)[self._side(node)]

    def getNhV4FromNode(self, node: str) -> bytes:
        return self._v4[self._side(node)]

    def getNhV6FromNode(self, node: str) -> bytes:
        return self._v6[self._side(node)]

    def isUp(self) -> bool:
        return self._up

    @property
    def orderedNames(self) -> Tuple[Tuple[str, str], Tuple[str, str]]:
        return self._key  # type: ignore[return-value]

    def __eq__(self, other: object) -> bool:
        return isinstance(other, Link) and self.hash == other.hash and self._key == other._key

    def __lt__(self, other: "Link") -> bool:  # Link::operator< (LinkState.cpp:347-353)
        if self.hash != other.hash:
            return self.hash < other.hash
        return self._key < other._key

    def __hash__(self) -> int:
        return self.hash

    def toString(self) -> str:
        return f"{self._area} - {self._n1}%{self._if1} <---> {self._n2}%{self._if2}"

    def directionalToString(self, fromNode: str) -> str:
        other = self.getOtherNodeName(fromNode)
        return (f"{self._area} - {fromNode}%{self.getIfaceFromNode(fromNode)} ---> "
                f"{other}%{self.getIfaceFromNode(other)}")

    def __repr__(self) -> str:
        return f"Link({self.toString()})"


@dataclass(frozen=True)
class PathLink:
    """``NodeSpfResult::PathLink`` (LinkState.h:207-213)."""

    link: Link
    prevNode: str


class NodeSpfResult:
    """``LinkState::NodeSpfResult`` (LinkState.h:203-257)."""

    __slots__ = ("_metric", "_nh", "_pl")

    def __init__(self, metric: int, nh: Set[str], pl) -> None:
        # pl: the list, or a callable building it on first use (pathLinks are
        # derived only for the callers that read them)
        self._metric, self._nh, self._pl = metric, nh, pl

    def metric(self) -> int:
        return self._metric

    def nextHops(self) -> Set[str]:
        return self._nh

    def pathLinks(self) -> List[PathLink]:
        if callable(self._pl):
            self._pl = self._pl()
        return self._pl

    def __repr__(self) -> str:
        return f"NodeSpfResult(metric={self._metric}, nextHops={sorted(self._nh)})"


SpfResult = Dict[str, NodeSpfResult]
Path = List[Link]


def _change(c: N.LsChange) -> LinkStateChange:
    return LinkStateChange(bool(c.topology_changed), bool(c.link_attributes_changed),
                           bool(c.node_label_changed))


class _LazySpfResult(Mapping):
    """SpfResult (unordered_map<string, NodeSpfResult>) backed by numpy
    copies of the C-ABI view; a NodeSpfResult is built when first read.
    Like the reference's ``SpfResult const&`` into the memo, it is valid until
    the next topology change: link ids are resolved lazily through the
    LinkState's link table, so reading an unmaterialised entry after the
    topology changed raises instead of naming the wrong links."""

    def __init__(self, ls: "LinkState", v: "N.LsSpfView", key=None) -> None:
        import numpy as np

        def arr(ptr, n, dt):
            return np.ctypeslib.as_array(ptr, (n,)).astype(dt) if n else np.zeros(0, dt)

        n = int(v.n)
        self._ls = ls
        self._gen = ls._gen
        self._key = key
        self._node = arr(v.node, n, np.uint32)
        self._metric = arr(v.metric, n, np.uint64)
        self._nh_ptr = arr(v.nh_ptr, n + 1, np.uint32)
        self._nh_node = arr(v.nh_node, int(self._nh_ptr[-1]) if n else 0, np.uint32)
        self._pl_ptr = None
        if v.pl_ptr:
            self._take_pl(v)
        self._index: Optional[Dict[str, int]] = None
        self._made: Dict[str, NodeSpfResult] = {}

    def _take_pl(self, v) -> None:
        import numpy as np

        n = len(self._node)
        self._pl_ptr = np.ctypeslib.as_array(v.pl_ptr, (n + 1,)).astype(np.uint32) if n else np.zeros(1, np.uint32)
        m = int(self._pl_ptr[-1]) if n else 0
        self._pl_link = np.ctypeslib.as_array(v.pl_link, (m,)).astype(np.uint32) if m else np.zeros(0, np.uint32)
        self._pl_prev = np.ctypeslib.as_array(v.pl_prev, (m,)).astype(np.uint32) if m else np.zeros(0, np.uint32)

    def _path_links(self, i: int) -> List[PathLink]:
        ls = self._ls
        if ls._gen != self._gen:
            raise RuntimeError("SpfResult read after a topology change: call getSpfResult again")
        if self._pl_ptr is None:  # the same memo entry, its pathLinks now (spf_runs unchanged)
            self._take_pl(ls._spf_view(*self._key))
        a, b = int(self._pl_ptr[i]), int(self._pl_ptr[i + 1])
        return [PathLink(ls._link(int(l)), ls._name(int(p)))
                for l, p in zip(self._pl_link[a:b], self._pl_prev[a:b])]

    def _idx(self) -> Dict[str, int]:
        if self._index is None:
            name = self._ls._name
            self._index = {name(int(x)): i for i, x in enumerate(self._node)}
        return self._index

    def __getitem__(self, key: str) -> NodeSpfResult:
        r = self._made.get(key)
        if r is None:
            ls = self._ls
            if ls._gen != self._gen:
                raise RuntimeError("SpfResult read after a topology change: call getSpfResult again")
            i = self._idx()[key]
            a, b = int(self._nh_ptr[i]), int(self._nh_ptr[i + 1])
            nh = {ls._name(int(x)) for x in self._nh_node[a:b]}
            r = self._made[key] = NodeSpfResult(int(self._metric[i]), nh, lambda i=i: self._path_links(i))
        return r

    def __iter__(self):
        return iter(self._idx())

    def __len__(self) -> int:
        return len(self._node)

    def __contains__(self, key: object) -> bool:
        return key in self._idx()


class LinkState(N.NativeHandle):
    """``openr::LinkState`` (LinkState.h:177-469) on the MI355X engine.

    ``device`` selects the GPU; ``device=-1`` builds a host-only state (LSDB
    bookkeeping and graph flatten, no shortest-path queries).  ``close()``
    (or a ``with`` block) releases the engine context it owns.
    """

    _LEVEL = 1
    _destroy = "ls_destroy"

    def __init__(self, area: str = K_DEFAULT_AREA, device: int = 0,
                 devices: Optional[Sequence[int]] = None) -> None:
        h = C.c_void_p()
        if devices:  # several GPUs behind one state (ls_create_multi)
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            st = N.lib.ls_create_multi(area.encode(), ids, len(devices), C.byref(h))
        else:
            st = N.lib.ls_create(area.encode(), device, C.byref(h))
        N.raise_for(st, N.global_error())
        self._adopt(h)
        self._area = area
        self._n_members = len(devices) if devices else 1
        self._device = int(devices[0]) if devices else int(device)
        self._k2r = None  # allSourcesKsp2Routes' result
        self._names: List[Optional[str]] = []
        self._gen = 0
        self._spf_cache: Dict[Tuple[str, bool], SpfResult] = {}
        self._ksp_cache: Dict[Tuple[str, str, int], List[Path]] = {}
        self._link_cache: Dict[int, Link] = {}
        self._snaps: "weakref.WeakSet[RouteSnapshot]" = weakref.WeakSet()

    # -- helpers ---------------------------------------------------------------
    def _err(self, st: int) -> None:
        N.raise_for(st, (N.lib.ls_last_error(self._h) or b"").decode())

    def _name(self, i: int) -> str:
        while i >= len(self._names):
            self._names.append(None)
        s = self._names[i]
        if s is None:
            s = N.lib.ls_name(self._h, i).decode()
            self._names[i] = s
        return s

    def _topology(self, changes: Iterable[LinkStateChange]) -> None:
        if any(c.topologyChanged for c in changes):
            self._gen += 1
            self._spf_cache.clear()
            self._ksp_cache.clear()
            self._link_cache.clear()

    def _link(self, link_id: int) -> Link:
        lk = self._link_cache.get(link_id)
        if lk is None:
            d = N.LsLinkDesc()
            self._err(N.lib.ls_link_info(self._h, link_id, C.byref(d)))
            lk = Link(self, d, link_id)
            self._link_cache[link_id] = lk
        return lk

    # -- mutators (LinkState.h:327-337) -----------------------------------------
    def updateAdjacencyDatabase(self, adjacencyDb: AdjacencyDatabase, holdUpTtl: int = 0,
                                holdDownTtl: int = 0) -> LinkStateChange:
        return self.updateAdjacencyDatabases([adjacencyDb], holdUpTtl, holdDownTtl)[0]

    def updateAdjacencyDatabases(self, dbs: Union[PackedLsdb, Sequence[AdjacencyDatabase]],
                                 holdUpTtl: int = 0, holdDownTtl: int = 0
                                 ) -> List[LinkStateChange]:
        """Apply databases in order (one updateAdjacencyDatabase each)."""
        packed = dbs if isinstance(dbs, PackedLsdb) else pack(dbs)
        s = N.lsdb_struct(packed)
        out = (N.LsChange * max(1, len(packed)))()
        self._err(N.lib.ls_update_adjacency_databases(self._h, C.byref(s), holdUpTtl,
                                                      holdDownTtl, out))
        res = [_change(out[i]) for i in range(len(packed))]
        self._link_cache.clear()  # attributes may have changed
        self._topology(res)
        return res

    def processPublication(self, publication: bytes,
                           orderedFibNode: Optional[str] = None) -> LinkStateChange:
        """The link-state half of ``Decision::processPublication``
        (Decision.cpp:1709-1817) for this area: a serialized
        thrift::Publication (CompactProtocol); every ``"adj:"`` value is
        decoded and applied (in the reference's keyVals iteration order),
        every expired ``"adj:"`` key deletes its node's database.  With
        ``orderedFibNode`` (this node's name, enable_ordered_fib_programming)
        each database carries the hold-up / hold-down TTLs of
        Decision.cpp:1750-1758.  Returns the OR of the steps'
        LinkStateChanges; the counts of applied / deleted databases land in
        ``lastPublicationCounts``."""
        nu, nd, c = C.c_uint32(), C.c_uint32(), N.LsChange()
        st = N.lib.ls_apply_publication_ordered(
            self._h, publication, len(publication),
            orderedFibNode.encode() if orderedFibNode is not None else None, C.byref(nu),
            C.byref(nd), C.byref(c))
        N.raise_for(st, (N.lib.openr_wire_last_error() or b"").decode())
        self.lastPublicationCounts = (int(nu.value), int(nd.value))
        res = _change(c)
        self._link_cache.clear()
        self._topology([res])
        return res

    def deleteAdjacencyDatabase(self, nodeName: str) -> LinkStateChange:
        c = N.LsChange()
        self._err(N.lib.ls_delete_adjacency_database(self._h, nodeName.encode(), C.byref(c)))
        res = _change(c)
        self._link_cache.clear()
        self._topology([res])
        return res

    def decrementHolds(self) -> LinkStateChange:
        c = N.LsChange()
        self._err(N.lib.ls_decrement_holds(self._h, C.byref(c)))
        res = _change(c)
        self._link_cache.clear()
        self._topology([res])
        return res

    # -- const queries -----------------------------------------------------------
    def getArea(self) -> str:
        return self._area

    def hasHolds(self) -> bool:
        return bool(N.lib.ls_has_holds(self._h))

    def numLinks(self) -> int:
        return int(N.lib.ls_num_links(self._h))

    def numNodes(self) -> int:
        return int(N.lib.ls_num_nodes(self._h))

    def hasNode(self, nodeName: str) -> bool:
        return bool(N.lib.ls_has_node(self._h, nodeName.encode()))

    def isNodeOverloaded(self, nodeName: str) -> bool:
        return bool(N.lib.ls_is_node_overloaded(self._h, nodeName.encode()))

    def getAdjacencyDatabaseLabels(self) -> Dict[str, int]:
        """{node: nodeLabel} of every node with an adjacency database -- the
        part of getAdjacencyDatabases() (LinkState.h:357-359) SpfSolver reads."""
        cnt = C.c_uint32()
        self._err(N.lib.ls_adjacency_databases(self._h, None, None, 0, C.byref(cnt)))
        ids = (C.c_uint32 * max(1, cnt.value))()
        labels = (C.c_int32 * max(1, cnt.value))()
        self._err(N.lib.ls_adjacency_databases(self._h, ids, labels, cnt.value, C.byref(cnt)))
        return {self._name(ids[i]): int(labels[i]) for i in range(cnt.value)}

    def linksFromNode(self, nodeName: str) -> List[Link]:
        """Links of ``nodeName`` in the reference's LinkSet iteration order."""
        cnt = C.c_uint32()
        self._err(N.lib.ls_links_from_node(self._h, nodeName.encode(), None, 0, C.byref(cnt)))
        ids = (C.c_uint32 * max(1, cnt.value))()
        self._err(N.lib.ls_links_from_node(self._h, nodeName.encode(), ids, cnt.value,
                                           C.byref(cnt)))
        return [self._link(ids[i]) for i in range(cnt.value)]

    def spfRuns(self) -> int:
        """The reference's ``decision.spf_runs`` counter (LinkState.cpp:815)."""
        return int(N.lib.ls_spf_runs(self._h))

    # -- shortest paths ----------------------------------------------------------
    def getSpfResult(self, nodeName: str, useLinkMetric: bool = True) -> SpfResult:
        """``getSpfResult`` (LinkState.cpp:793-803): a read-only mapping node
        name -> NodeSpfResult over the C-ABI's result arrays (copied once);
        entries are materialised on access, pathLinks on the first
        ``pathLinks()`` of the result (ls_get_spf_metrics now, the same memo
        entry's pathLinks from ls_get_spf_result then: one spf_runs count)."""
        key = (nodeName, bool(useLinkMetric))
        hit = self._spf_cache.get(key)
        if hit is not None:
            return hit
        v = N.LsSpfView()  # metrics and next hops now, pathLinks when first read
        self._err(N.lib.ls_get_spf_metrics(self._h, nodeName.encode(), int(bool(useLinkMetric)),
                                           C.byref(v)))
        res = _LazySpfResult(self, v, key)
        self._spf_cache[key] = res
        return res

    def _spf_view(self, nodeName: str, useLinkMetric: bool = True) -> "N.LsSpfView":
        """The raw C-ABI result (ls_get_spf_result): arrays owned by the
        LinkState's memo, valid until the next topology change."""
        v = N.LsSpfView()
        self._err(N.lib.ls_get_spf_result(self._h, nodeName.encode(), int(bool(useLinkMetric)),
                                          C.byref(v)))
        return v

    def getKthPaths(self, src: str, dest: str, k: int) -> List[Path]:
        key = (src, dest, int(k))
        hit = self._ksp_cache.get(key)
        if hit is not None:
            return hit
        if k < 1:
            raise ValueError("getKthPaths: k must be >= 1")
        v = N.LsPathsView()
        self._err(N.lib.ls_get_kth_paths(self._h, src.encode(), dest.encode(), k, C.byref(v)))
        paths = [[self._link(v.link[j]) for j in range(v.path_ptr[p], v.path_ptr[p + 1])]
                 for p in range(v.n_paths)]
        self._ksp_cache[key] = paths
        return paths

    def prefetchKthPaths(self, src: str) -> None:
        """Fill the getKthPaths memo for (src, *, 1) and (src, *, 2) with one
        batched KSP2 launch (ls_prefetch_kth_paths)."""
        self._err(N.lib.ls_prefetch_kth_paths(self._h, src.encode()))

    def prefetchSpfResults(self, nodes: Sequence[str], useLinkMetric: bool = True) -> None:
        """Fill the getSpfResult memo for every node of `nodes` with one
        batched plan (ls_prefetch_spf_results); spfRuns() counts each when it
        is first read, as the reference's one-by-one calls would."""
        arr = (C.c_char_p * max(1, len(nodes)))(*[n.encode() for n in nodes])
        self._err(N.lib.ls_prefetch_spf_results(self._h, arr, len(nodes), int(bool(useLinkMetric))))

    def prefetchAllSources(self, useLinkMetric: bool = True) -> None:
        """getSpfResult for every node as one all-sources pass split over the
        state's GPUs (ls_prefetch_all_sources; needs ``devices=[...]``):
        results stay on their GPU and later getSpfResult(node) calls read
        node's share from it -- Decision::getDecisionRouteDb for every node
        (Decision.cpp:1480-1500)."""
        self._err(N.lib.ls_prefetch_all_sources(self._h, int(bool(useLinkMetric))))

    def allSourcesDigests(self):
        """Per-node digests (csr order) of the resident all-sources pass, on
        the owning GPUs (spf_mplan_digest); None when no pass is valid."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            return None
        n = C.c_uint32()
        e = C.c_uint32()
        self._err(N.lib.ls_flatten(self._h, C.byref(n), C.byref(e)))
        out = np.zeros(max(1, n.value), np.uint64)
        st = N.lib.spf_mplan_digest(C.c_void_p(mp), N.ptr(out, C.c_uint64))
        N.raise_for(st, N.global_error())
        return out[: n.value]

    def linkValueHashes(self):
        """u64 value identity of every link id of the flattened graph (FNV-1a
        over its ordered key, bench.link_value_hash's definition), for the
        engine's route / KSP2 digests; cached until the topology changes."""
        import numpy as np

        lid = self._csr_link_ids()
        # keyed on the flattened graph's epoch: a link id freed and reused by
        # another link changes the structure, hence the epoch
        key = int(N.lib.ls_graph_epoch(self._h))
        if getattr(self, "_lh_key", None) == key and self._lh is not None:
            return self._lh
        lh = np.zeros(max(1, int(lid.max()) + 1 if len(lid) else 1), np.uint64)
        M, P = (1 << 64) - 1, 0x100000001b3
        for l in np.unique(lid):
            try:
                (a, b), (c, d) = self._link(int(l)).orderedNames
            except N.SpfError:  # a withdrawn link's dead slots: never a result
                continue
            f = 0xcbf29ce484222325
            for part in (a, b, c, d):
                for ch in part.encode():
                    f = ((f ^ ch) * P) & M
                f = ((f ^ 0x01) * P) & M
            f = ((f ^ (f >> 30)) * 0xbf58476d1ce4e5b9) & M
            f = ((f ^ (f >> 27)) * 0x94d049bb133111eb) & M
            lh[int(l)] = f ^ (f >> 31)
        self._lh, self._lh_key = lh, key
        return lh

    def allSourcesRouteDigests(self, set_ptr, set_nodes, lfa: bool, mes=None):
        """Route selections of every node (or the csr ids in `mes`) towards
        every destination set from the resident all-sources pass
        (spf_mplan_route_digests, needs prefetchAllSources()): per node one
        u64 digest, and the slowest member's kernel ms."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesRouteDigests: no resident all-sources pass")
        n = self._csr_sizes()[0]
        mes = np.arange(n, dtype=np.uint32) if mes is None else np.ascontiguousarray(mes, np.uint32)
        sp = np.ascontiguousarray(set_ptr, np.uint32)
        sn = np.ascontiguousarray(set_nodes if len(set_nodes) else [0], np.uint32)
        lh = self.linkValueHashes()
        out = np.zeros(max(1, len(mes)), np.uint64)
        ms = C.c_double()
        st = N.lib.spf_mplan_route_digests(C.c_void_p(mp), N.ptr(mes), len(mes), N.ptr(sp), N.ptr(sn),
                                           len(sp) - 1, N.SPF_ROUTE_LFA if lfa else 0,
                                           N.ptr(lh, C.c_uint64), len(lh), N.ptr(out, C.c_uint64),
                                           C.byref(ms))
        N.raise_for(st, N.global_error())
        return out[: len(mes)], ms.value

    def allSourcesRouteRecords(self, set_ptr, set_nodes, lfa: bool, mes=None, compact: bool = False):
        """Every node's (or the csr ids in `mes`) route database materialised
        on its owning GPU from the resident all-sources pass
        (spf_mplan_route_records): returns (records over every node, the
        slowest member's kernel ms); read one node's with allSourcesRouteDb.
        compact: the exactly sized pool (SPF_ROUTE_COMPACT) instead of the
        tiled one; allSourcesRouteRecordPool() tells what either holds."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesRouteRecords: no resident all-sources pass")
        n = self._csr_sizes()[0]
        mes = np.arange(n, dtype=np.uint32) if mes is None else np.ascontiguousarray(mes, np.uint32)
        sp = np.ascontiguousarray(set_ptr, np.uint32)
        sn = np.ascontiguousarray(set_nodes if len(set_nodes) else [0], np.uint32)
        tot, ms = C.c_uint64(), C.c_double()
        st = N.lib.spf_mplan_route_records(C.c_void_p(mp), N.ptr(mes), len(mes), N.ptr(sp), N.ptr(sn),
                                           len(sp) - 1, (N.SPF_ROUTE_LFA if lfa else 0) |
                                           (N.SPF_ROUTE_COMPACT if compact else 0), C.byref(tot),
                                           C.byref(ms))
        N.raise_for(st, N.global_error())
        self._db_sets = len(sp) - 1
        self._db_mes = len(mes)
        self._db_me_ids = [int(v) for v in mes]
        return int(tot.value), ms.value

    def allSourcesRouteRecordPool(self):
        """The last allSourcesRouteRecords' pools (spf_mplan_route_record_pool):
        (layout -- 0 tiled, 1 compact --, the record pools' device bytes, 8 x
        records)."""
        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesRouteRecordPool: no resident all-sources pass")
        layout, pool, rec = C.c_uint32(), C.c_uint64(), C.c_uint64()
        N.raise_for(N.lib.spf_mplan_route_record_pool(C.c_void_p(mp), C.byref(layout), C.byref(pool),
                                                      C.byref(rec)), N.global_error())
        return int(layout.value), int(pool.value), int(rec.value)

    def allSourcesRouteDb(self, t: int):
        """Node t's (index into the last allSourcesRouteRecords' node list)
        database: (headers [n_sets] u64 = offset | count << 32, records u64 =
        CSR edge | metric << 32)."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesRouteDb: no resident all-sources pass")
        n = C.c_uint64()
        hdr = np.zeros(max(1, self._db_sets), np.uint64)
        N.raise_for(N.lib.spf_mplan_route_db(C.c_void_p(mp), int(t), N.ptr(hdr, C.c_uint64), None, 0,
                                             C.byref(n)), N.global_error())
        rec = np.zeros(max(1, n.value), np.uint64)
        N.raise_for(N.lib.spf_mplan_route_db(C.c_void_p(mp), int(t), None, N.ptr(rec, C.c_uint64),
                                             n.value, C.byref(n)), N.global_error())
        return hdr[: self._db_sets], rec[: n.value]

    def allSourcesLabelRoutes(self, lfa: bool, mes=None):
        """Every node's (or the csr ids in `mes`) node-label MPLS routes
        (Decision.cpp:586-674) materialised on its owning GPU from the
        resident all-sources pass (spf_mplan_label_routes), the labels taken
        from getAdjacencyDatabaseLabels(): returns (labels int32 [G] ascending
        -- the group index of allSourcesLabelRouteDb --, records over every
        node, the pools' bytes, the slowest member's kernel ms)."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesLabelRoutes: no resident all-sources pass")
        names = self.flatten()[0]
        n = len(names)
        adv = self.getAdjacencyDatabaseLabels()
        # (a label that does not fit the C-ABI's i32 is invalid either way)
        node_label = np.array([adv.get(s, 0) if -(1 << 31) <= adv.get(s, 0) < (1 << 31) else -1
                               for s in names] or [0], np.int32)
        mes = np.arange(n, dtype=np.uint32) if mes is None else np.ascontiguousarray(mes, np.uint32)
        labels = np.zeros(max(1, n), np.int32)
        g = C.c_uint32()
        N.raise_for(N.lib.spf_label_groups(N.ptr(node_label, C.c_int32), n, N.ptr(labels, C.c_int32),
                                           None, None, C.byref(g)), N.global_error())
        ng, tot, nbytes, ms = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_double()
        st = N.lib.spf_mplan_label_routes(C.c_void_p(mp), N.ptr(mes), len(mes),
                                          N.ptr(node_label, C.c_int32),
                                          N.SPF_ROUTE_LFA if lfa else 0, C.byref(ng), C.byref(tot),
                                          C.byref(nbytes), C.byref(ms))
        N.raise_for(st, N.global_error())
        assert ng.value == g.value
        self._lr = (labels[: g.value].copy(), [int(v) for v in mes], names)
        return self._lr[0], int(tot.value), int(nbytes.value), ms.value

    def allSourcesLabelRouteDb(self, t: int):
        """Node t's (index into the last allSourcesLabelRoutes' node list)
        label routes: (owner u32 [G] -- the csr id of label g's owner,
        SPF_UNREACHABLE: no route --, ptr u64 [G + 1], records u64 = CSR edge |
        metric << 32): label g's next hops are rec[ptr[g] : ptr[g + 1]], none
        when t itself owns it (POP_AND_LOOKUP)."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp or getattr(self, "_lr", None) is None:
            raise RuntimeError("allSourcesLabelRouteDb: no resident all-sources pass")
        g = len(self._lr[0])
        n = C.c_uint64()
        owner = np.zeros(max(1, g), np.uint32)
        ptr = np.zeros(g + 1, np.uint64)
        N.raise_for(N.lib.spf_mplan_label_route_db(C.c_void_p(mp), int(t), N.ptr(owner),
                                                   N.ptr(ptr, C.c_uint64), None, 0, C.byref(n)),
                    N.global_error())
        rec = np.zeros(max(1, n.value), np.uint64)
        N.raise_for(N.lib.spf_mplan_label_route_db(C.c_void_p(mp), int(t), None, None,
                                                   N.ptr(rec, C.c_uint64), n.value, C.byref(n)),
                    N.global_error())
        return owner[:g], ptr, rec[: n.value]

    def allSourcesPrefixRoutes(self, table: "PrefixTable", lfa: bool, mes=None, allBest: bool = False):
        """Every node's (or the csr ids in `mes`) SP_ECMP / IP unicast route
        decision for every prefix of `table` (createRouteForPrefix,
        Decision.cpp:390-554: reachable advertisers, best entries by
        PrefixMetrics, the drained filter, no route to oneself, minNexthop),
        materialised on its owning GPU from the resident all-sources pass
        (spf_mplan_prefix_routes); the overload flags are this link state's.
        allBest: best-route selection off (SPF_PREFIX_ALL_BEST).  Returns
        (records over every node, the pools' bytes, the slowest member's
        kernel ms); read one node's with allSourcesPrefixRouteDb."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesPrefixRoutes: no resident all-sources pass")
        self._px = None
        n = self._csr_sizes()[0]
        ovl = np.ascontiguousarray(self.flatten()[5], np.uint8)
        ovl = ovl if len(ovl) else np.zeros(1, np.uint8)
        mes = np.arange(n, dtype=np.uint32) if mes is None else np.ascontiguousarray(mes, np.uint32)
        pp = np.ascontiguousarray(table.pfx_ptr, np.uint32)

        def col(a, dt):
            a = np.ascontiguousarray(a, dt)
            return a if len(a) else np.zeros(1, dt)

        tot, nbytes, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        st = N.lib.spf_mplan_prefix_routes(
            C.c_void_p(mp), N.ptr(mes), len(mes), N.ptr(pp), N.ptr(col(table.node, np.uint32)),
            N.ptr(col(table.path_preference, np.int32), C.c_int32),
            N.ptr(col(table.source_preference, np.int32), C.c_int32),
            N.ptr(col(table.distance, np.int32), C.c_int32),
            N.ptr(col(table.min_nexthop, np.int64), C.c_int64), len(pp) - 1, N.ptr(ovl, C.c_uint8),
            (N.SPF_ROUTE_LFA if lfa else 0) | (N.SPF_PREFIX_ALL_BEST if allBest else 0),
            C.byref(tot), C.byref(nbytes), C.byref(ms))
        N.raise_for(st, N.global_error())
        self._px = len(pp) - 1
        return int(tot.value), int(nbytes.value), ms.value

    def allSourcesPrefixRouteDb(self, t: int):
        """Node t's (index into the last allSourcesPrefixRoutes' node list)
        prefix routes: (info u64 [P] = best node | |B| << 32 | status << 56 --
        status one of N.SPF_PREFIX_NONE / SELF / NO_NEXTHOP / MIN_NEXTHOP /
        ROUTE, best SPF_UNREACHABLE for NONE --, ptr u64 [P + 1], records u64 =
        CSR edge | metric << 32): prefix p's next hops are rec[ptr[p] :
        ptr[p + 1]], none unless its status is ROUTE."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp or getattr(self, "_px", None) is None:
            raise RuntimeError("allSourcesPrefixRouteDb: no prefix routes (call allSourcesPrefixRoutes)")
        P = self._px
        n = C.c_uint64()
        info = np.zeros(max(1, P), np.uint64)
        ptr = np.zeros(P + 1, np.uint64)
        N.raise_for(N.lib.spf_mplan_prefix_route_db(C.c_void_p(mp), int(t), N.ptr(info, C.c_uint64),
                                                    N.ptr(ptr, C.c_uint64), None, 0, C.byref(n)),
                    N.global_error())
        rec = np.zeros(max(1, n.value), np.uint64)
        N.raise_for(N.lib.spf_mplan_prefix_route_db(C.c_void_p(mp), int(t), None, None,
                                                    N.ptr(rec, C.c_uint64), n.value, C.byref(n)),
                    N.global_error())
        return info[:P], ptr, rec[: n.value]

    def allSourcesRouteSnapshot(self) -> "RouteSnapshot":
        """The resident pass's route databases (the last
        allSourcesRouteRecords and, when there was one, allSourcesLabelRoutes)
        kept as the old generation of a later allSourcesRouteDelta
        (ls_all_sources_route_snapshot): the device pools move into the
        snapshot, nothing is copied, and allSourcesRouteDb / LabelRouteDb raise
        SPF_E_STATE until the next materialising call.  Links are identified by
        linkValueHashes() as of now.  The snapshot survives this LinkState
        dropping its resident plan (a row patch, a reload); it is closed with
        the LinkState at the latest, before the engine context."""
        lh = self.linkValueHashes()
        h = C.c_void_p()
        self._err(N.lib.ls_all_sources_route_snapshot(self._h, N.ptr(lh, C.c_uint64), len(lh),
                                                      C.byref(h)))
        snap = RouteSnapshot(self, h)
        self._snaps.add(snap)
        return snap

    def allSourcesRouteDelta(self, snapshot: "RouteSnapshot"):
        """What changed since `snapshot` in every node's route database
        (spf_mplan_route_delta: DecisionRouteDb::calculateUpdate,
        Decision.cpp:111-146, for every node on its GPU): the current
        databases -- allSourcesRouteRecords and allSourcesLabelRoutes called
        again with the snapshot's node list, sets and LFA choice -- against
        the snapshot's.  Returns (per node t a tuple (updated sets, deleted
        sets, updated labels, deleted labels) of ascending int lists, totals
        [IP updates, IP deletes, label updates, label deletes, nodes compared
        as sets], the slowest member's kernel ms)."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesRouteDelta: no resident all-sources pass")
        if snapshot.closed or snapshot._ls is not self:
            raise ValueError("allSourcesRouteDelta: not an open snapshot of this LinkState")
        lh = self.linkValueHashes()
        tot = np.zeros(5, np.uint64)
        ms = C.c_double()
        N.raise_for(N.lib.spf_mplan_route_delta(C.c_void_p(mp), snapshot._h, N.ptr(lh, C.c_uint64),
                                                len(lh), N.ptr(tot, C.c_uint64), C.byref(ms)),
                    N.global_error())
        out = []
        for t in range(self._db_mes):  # (the delta checked the me list against the records call's)
            ni, nl = C.c_uint64(), C.c_uint64()
            N.raise_for(N.lib.spf_mplan_route_delta_db(C.c_void_p(mp), t, None, 0, C.byref(ni), None, 0,
                                                       C.byref(nl)), N.global_error())
            ip = np.zeros(max(1, ni.value), np.uint32)
            lb = np.zeros(max(1, nl.value), np.uint32)
            N.raise_for(N.lib.spf_mplan_route_delta_db(C.c_void_p(mp), t, N.ptr(ip), ni.value, None,
                                                       N.ptr(lb), nl.value, None), N.global_error())
            ip, lb = ip[: ni.value], lb[: nl.value]
            D, M = N.SPF_DELTA_DELETE, N.SPF_DELTA_DELETE - 1
            out.append(tuple([int(v & M) for v in a if bool(v & D) == dele]
                             for a, dele in ((ip, False), (ip, True), (lb, False), (lb, True))))
        return out, [int(v) for v in tot], ms.value

    def allSourcesRouteUpdate(self, snapshot: "RouteSnapshot"):
        """allSourcesRouteDelta(snapshot) with its payload
        (spf_mplan_route_update: what a DecisionRouteUpdate carries besides the
        routes' names): returns the delta's (lists, totals, kernel ms), then
        per node t a pair ({updated set: u64 records}, {updated label: (owner
        csr id, u64 records)}) -- the records as allSourcesRouteDb /
        allSourcesLabelRouteDb hold them, CSR edge | metric << 32 in t's link
        order, gathered on the GPU into one pool per member, read back in one
        copy per member and split here for the nodes that have entries -- and a dict of the update's own figures:
        totals [IP update entries, IP records, label update entries, label
        records], pool_bytes, kernel_ms, phase_ms [count, scan, fill]."""
        import numpy as np

        mp = N.lib.ls_all_sources_plan(self._h)
        if not mp:
            raise RuntimeError("allSourcesRouteUpdate: no resident all-sources pass")
        if snapshot.closed or snapshot._ls is not self:
            raise ValueError("allSourcesRouteUpdate: not an open snapshot of this LinkState")
        mp = C.c_void_p(mp)
        lh = self.linkValueHashes()
        dtot, ms = np.zeros(5, np.uint64), C.c_double()
        N.raise_for(N.lib.spf_mplan_route_delta(mp, snapshot._h, N.ptr(lh, C.c_uint64), len(lh),
                                                N.ptr(dtot, C.c_uint64), C.byref(ms)), N.global_error())
        tot, nbytes, ums = np.zeros(4, np.uint64), C.c_uint64(), C.c_double()
        N.raise_for(N.lib.spf_mplan_route_update(mp, N.ptr(tot, C.c_uint64), C.byref(nbytes),
                                                 C.byref(ums)), N.global_error())
        phase = (C.c_double * 3)()
        N.raise_for(N.lib.spf_mplan_route_update_timing(mp, phase), N.global_error())
        lists = [([], [], [], []) for _ in range(self._db_mes)]
        out = [({}, {}) for _ in range(self._db_mes)]
        D, M = N.SPF_DELTA_DELETE, N.SPF_DELTA_DELETE - 1
        for r in range(self._n_members):  # one copy per array and member, split here
            n = np.zeros(5, np.uint64)
            N.raise_for(N.lib.spf_mplan_route_update_read(mp, r, N.ptr(n, C.c_uint64), *([None] * 9)),
                        N.global_error())
            k, ei, ri, el, rl = (int(v) for v in n)
            if not k or not ei + el:
                continue
            slots = np.zeros(k, np.uint32)
            N.raise_for(N.lib.spf_mplan_route_delta_buffers(mp, r, None, None, None, None, N.ptr(slots), k,
                                                            None), N.global_error())
            dp = [np.zeros(k + 1, np.uint64) for _ in range(2)]
            ds = [np.zeros(max(1, e), np.uint32) for e in (ei, el)]
            up = [np.zeros(e + 1, np.uint64) for e in (ei, el)]
            ur = [np.zeros(max(1, c), np.uint64) for c in (ri, rl)]
            uo = np.zeros(max(1, el), np.uint32)
            N.raise_for(N.lib.spf_mplan_route_update_read(
                mp, r, None, N.ptr(dp[0], C.c_uint64), N.ptr(ds[0]), N.ptr(up[0], C.c_uint64),
                N.ptr(ur[0], C.c_uint64), N.ptr(dp[1], C.c_uint64), N.ptr(ds[1]), N.ptr(uo),
                N.ptr(up[1], C.c_uint64), N.ptr(ur[1], C.c_uint64)), N.global_error())
            for w in range(2):
                has = np.nonzero(dp[w][1:] > dp[w][:-1])[0]  # only the me that have entries
                for q in has.tolist():
                    t = int(slots[q])
                    a, b = int(dp[w][q]), int(dp[w][q + 1])
                    ent, at = ds[w][a:b].tolist(), up[w][a: b + 1].tolist()
                    for j, v in enumerate(ent):
                        if v & D:
                            lists[t][2 * w + 1].append(v & M)
                            continue
                        lists[t][2 * w].append(v)
                        rec = ur[w][at[j]: at[j + 1]].copy()
                        out[t][w][v] = rec if w == 0 else (int(uo[a + j]), rec)
        self._ru = (lists, out)
        info = {"totals": [int(v) for v in tot], "pool_bytes": int(nbytes.value),
                "kernel_ms": ums.value, "phase_ms": list(phase)}
        return lists, [int(v) for v in dtot], ms.value, out, info

    def allSourcesDecisionRouteUpdate(self, t: int, isV4: bool = False):
        """Node t's part of the last allSourcesRouteUpdate as the pieces of a
        DecisionRouteUpdate: ({updated set: set of NextHopThrift} -- one per
        record over the link as seen from t, no MPLS action --, the deleted
        sets, the RibMplsEntry of every updated node label -- POP_AND_LOOKUP /
        PHP / SWAP as allSourcesMplsRoutes decides them --, the deleted
        labels).  Adjacency-label routes are the host's (allSourcesMplsRoutes)."""
        from .spf_solver import MplsAction, NextHopThrift, RibMplsEntry, createNextHop

        lists, payload = self._ru
        up, dele, lup, ldel = lists[int(t)]
        uip, ulb = payload[int(t)]
        names, _, col, _, lid, _ = self.flatten()
        me_id = self._db_me_ids[int(t)]
        me = names[me_id]
        area = self.getArea()

        def hops(rec, action):
            nhs = set()
            for r in rec.tolist():
                e, metric = r & 0xFFFFFFFF, r >> 32
                link = self._link(int(lid[e]))
                addr = link.getNhV4FromNode(me) if isV4 else link.getNhV6FromNode(me)
                nhs.add(createNextHop(addr, link.getIfaceFromNode(me), metric, action(e), link.getArea(),
                                      link.getOtherNodeName(me)))
            return nhs

        unicast = {p: hops(uip[p], lambda e: None) for p in up}
        php = MplsAction("PHP")
        mpls = []
        for label in lup:
            o, rec = ulb[label]
            if o == me_id:
                mpls.append(RibMplsEntry(label, {NextHopThrift(
                    bytes(16), None, 0, MplsAction("POP_AND_LOOKUP"), area, None)}))
                continue
            swap = MplsAction("SWAP", label, None)
            mpls.append(RibMplsEntry(label, hops(rec, lambda e: php if int(col[e]) == o else swap)))
        return unicast, list(dele), mpls, list(ldel)

    def allSourcesKsp2Routes(self, set_ptr, set_nodes, prepend=None, mes=None):
        """Every node's (or the csr ids in `mes`) KSP2_ED_ECMP next hops
        towards every destination set ``set_nodes[set_ptr[p]:set_ptr[p + 1]]``
        (csr ids: a prefix's best advertisers of this area) --
        selectBestPathsKsp2, Decision.cpp:895-1018 -- on the GPU: one batched
        KSP2 pass, then spf_ksp2_routes over its device-resident paths.  The
        node labels come from getAdjacencyDatabaseLabels(); `prepend` is
        parallel to set_nodes (the entries' prependLabel, None or -1: none).
        addBestPaths (min-nexthop, static next hops of a self-advertised
        prefix) stays with the caller.  Returns (next hops, label words, pool
        bytes, kernel ms); allSourcesKsp2NextHops reads the routes."""
        import numpy as np

        from .engine import SpfEngine

        names, _, _, _, lid, _ = self.flatten()  # (loads the graph into the engine)
        h = self.engine_handle()
        if not h.value:
            raise RuntimeError("allSourcesKsp2Routes: LinkState created host-only (device < 0)")
        n = len(names)
        adv = self.getAdjacencyDatabaseLabels()
        node_label = np.array([adv.get(s, 0) for s in names] or [0], np.int32)
        pre = None if prepend is None else np.array(
            [-1 if v is None else int(v) for v in prepend], np.int32)
        mes = np.arange(n, dtype=np.uint32) if mes is None else np.ascontiguousarray(mes, np.uint32)
        self._close_ksp2_routes()
        eng = SpfEngine(device=self._device, handle=h, n_nodes=n)
        r = eng.ksp2_routes(mes, set_ptr, set_nodes, node_label, pre)
        self._k2r = (r, [int(v) for v in mes], names, lid, self._gen)
        return r.hops, r.label_words, r.pool_bytes, r.kernel_ms

    def allSourcesKsp2RouteDb(self, t: int):
        """Node mes[t]'s share of the last allSourcesKsp2Routes (rptr u64
        [sets + 1], rec u64 = CSR edge | cost << 32, lptr u64 [len(rec) + 1],
        lab i32): set p's next hops are rec[rptr[p]:rptr[p + 1]], next hop h's
        label stack is lab[lptr[h]:lptr[h + 1]]."""
        if self._k2r is None or self._k2r[4] != self._gen:
            raise RuntimeError("allSourcesKsp2RouteDb: no routes (call allSourcesKsp2Routes)")
        return self._k2r[0].db(int(t))

    def allSourcesKsp2NextHops(self, t: int, p: int, isV4: bool = False):
        """The set of NextHopThrift of route (mes[t], set p) of the last
        allSourcesKsp2Routes: one per record over its first link as seen from
        the node, PUSH of the label stack unless it is empty -- what
        ``SpfSolver._ksp2NextHops`` returns for the same node, advertisers and
        prefix entries."""
        if self._k2r is None or self._k2r[4] != self._gen:
            raise RuntimeError("allSourcesKsp2NextHops: no routes (call allSourcesKsp2Routes)")
        r, mes, names, lid, _ = self._k2r
        return self._ksp2_thrift(names[mes[int(t)]], lid, r.nexthops(int(t), int(p)), isV4)

    def _ksp2_thrift(self, me: str, lid, hops, isV4: bool):
        """[(CSR edge, cost, label stack)] of one of me's KSP2 routes as its
        set of NextHopThrift."""
        from .spf_solver import MplsAction, createNextHop

        nhs = set()
        for e, cost, labels in hops:
            link = self._link(int(lid[e]))
            addr = link.getNhV4FromNode(me) if isV4 else link.getNhV6FromNode(me)
            action = MplsAction("PUSH", None, tuple(labels)) if labels else None
            nhs.add(createNextHop(addr, link.getIfaceFromNode(me), cost, action, link.getArea(),
                                  link.getOtherNodeName(me)))
        return nhs

    def _ksp2_current(self, who: str, snapshot):
        if self._k2r is None or self._k2r[4] != self._gen:
            raise RuntimeError(f"{who}: no routes (call allSourcesKsp2Routes)")
        if snapshot is not None and (snapshot.closed or snapshot not in self._snaps):
            raise ValueError(f"{who}: not an open snapshot of this LinkState")
        return self._k2r[0]

    def allSourcesKsp2RouteSnapshot(self) -> "Ksp2RouteSnapshot":
        """The routes of the last allSourcesKsp2Routes kept as the old
        generation of a later allSourcesKsp2RouteDelta
        (spf_ksp2_route_snapshot): the device pools move into the snapshot,
        nothing is copied, and allSourcesKsp2RouteDb / NextHops raise
        SPF_E_STATE until the next allSourcesKsp2Routes.  Links are identified
        by linkValueHashes() as of now.  The snapshot survives this LinkState
        dropping its routes (a row patch, a reload, the next
        allSourcesKsp2Routes); it is closed with the LinkState at the latest,
        before the engine context."""
        r = self._ksp2_current("allSourcesKsp2RouteSnapshot", None)
        snap = r.snapshot(self.linkValueHashes())
        self._snaps.add(snap)
        return snap

    def allSourcesKsp2RouteDelta(self, snapshot: "Ksp2RouteSnapshot"):
        """What changed since `snapshot` in every node's KSP2 routes
        (spf_ksp2_route_delta: DecisionRouteDb::calculateUpdate,
        Decision.cpp:111-146, for every node on the GPU): the current routes --
        allSourcesKsp2Routes called again with the snapshot's node list and as
        many sets -- against the snapshot's.  A route's value is its set of
        next hops (link by value, cost, label stack).  Returns (per node t a
        pair (updated sets, deleted sets) of ascending int lists, totals
        [updates, deletes, routes compared as sets], kernel ms)."""
        r = self._ksp2_current("allSourcesKsp2RouteDelta", snapshot)
        out, totals, info = r.delta(snapshot, self.linkValueHashes(), update=False)
        return [(u, d) for u, d, _ in out], totals, info["delta_ms"]

    def allSourcesKsp2RouteUpdate(self, snapshot: "Ksp2RouteSnapshot"):
        """allSourcesKsp2RouteDelta(snapshot) with its payload
        (spf_ksp2_route_update: what a DecisionRouteUpdate carries besides the
        routes' names): returns the delta's (lists, totals, kernel ms), then
        per node t a dict {updated set: [(CSR edge, cost, label stack)]} -- the
        next hops as allSourcesKsp2RouteDb holds them, gathered on the GPU into
        one exactly sized pool, read back in one copy per array and split
        here -- and a dict of the update's own figures: update_totals [update
        entries, records, label words], pool_bytes, update_ms, phase_ms [count,
        scan, fill of the delta, then of the update].
        allSourcesKsp2DecisionRouteUpdate turns a node's part into
        NextHopThrift values."""
        r = self._ksp2_current("allSourcesKsp2RouteUpdate", snapshot)
        out, totals, info = r.delta(snapshot, self.linkValueHashes(), update=True)
        self._k2u = ([p for _, _, p in out], [d for _, d, _ in out], self._gen)
        return [(u, d) for u, d, _ in out], totals, info["delta_ms"], self._k2u[0], info

    def allSourcesKsp2DecisionRouteUpdate(self, t: int, isV4: bool = False):
        """Node mes[t]'s part of the last allSourcesKsp2RouteUpdate as the
        pieces of a DecisionRouteUpdate: ({updated set: set of NextHopThrift},
        the deleted sets) -- the next hops as allSourcesKsp2NextHops builds
        them."""
        k2u = getattr(self, "_k2u", None)
        if k2u is None or k2u[2] != self._gen or self._k2r is None:
            raise RuntimeError("allSourcesKsp2DecisionRouteUpdate: no update (call allSourcesKsp2RouteUpdate)")
        _, mes, names, lid, _ = self._k2r
        me = names[mes[int(t)]]
        return ({p: self._ksp2_thrift(me, lid, hops, isV4) for p, hops in k2u[0][int(t)].items()},
                list(k2u[1][int(t)]))

    def _close_ksp2_routes(self) -> None:
        k2r = getattr(self, "_k2r", None)
        if k2r is not None:
            k2r[0].close()
        self._k2r = None

    def close(self) -> None:
        for s in list(getattr(self, "_snaps", ())):
            s.close()
        self._close_ksp2_routes()
        super().close()

    def allSourcesMplsRoutes(self, t: int):
        """Node t's (index into the last allSourcesLabelRoutes' node list)
        MPLS routes as ``SpfSolver.buildRouteDb(node).mplsRoutes`` holds them
        ({label: RibMplsEntry}): its node-label routes expanded from the
        GPU's records -- POP_AND_LOOKUP for its own label, else one next hop
        per record, PHP over a link that ends at the label's owner and SWAP
        otherwise (Decision.cpp:586-674, 1247-1257) -- plus its adjacency-label
        routes from linksFromNode (:676-698, on the host: they need no SPF)."""
        from .spf_solver import (MplsAction, NextHopThrift, RibMplsEntry, createNextHop,
                                 isMplsLabelValid)

        owner, ptr, rec = self.allSourcesLabelRouteDb(t)
        labels, mes, names = self._lr
        me_id = mes[int(t)]
        me = names[me_id]
        area = self.getArea()
        _, _, col, _, lid, _ = self.flatten()
        out = {}
        php = MplsAction("PHP")
        for g, label in enumerate(labels.tolist()):
            o = int(owner[g])
            if o == N.SPF_UNREACHABLE:
                continue
            if o == me_id:
                out[label] = RibMplsEntry(label, {NextHopThrift(
                    bytes(16), None, 0, MplsAction("POP_AND_LOOKUP"), area, None)})
                continue
            swap = MplsAction("SWAP", label, None)
            nhs = set()
            for r in rec[int(ptr[g]): int(ptr[g + 1])].tolist():
                e, metric = r & 0xFFFFFFFF, r >> 32
                link = self._link(int(lid[e]))
                nhs.add(createNextHop(link.getNhV6FromNode(me), link.getIfaceFromNode(me), metric,
                                      php if int(col[e]) == o else swap, link.getArea(),
                                      link.getOtherNodeName(me)))
            out[label] = RibMplsEntry(label, nhs)
        for link in self.linksFromNode(me):
            top = link.getAdjLabelFromNode(me)
            if top == 0 or not isMplsLabelValid(top):
                continue
            out[top] = RibMplsEntry(top, {createNextHop(
                link.getNhV6FromNode(me), link.getIfaceFromNode(me), link.getMetricFromNode(me),
                php, link.getArea(), link.getOtherNodeName(me))})
        return out

    def debugPhaseNs(self) -> Tuple[int, int, int, int]:
        """Cumulative getSpfResult cost (ns): plan build, GPU execute + copy
        back, pathLinks, host assembly (ls_debug_phase_ns)."""
        out = (C.c_uint64 * 4)()
        N.lib.ls_debug_phase_ns(self._h, out)
        return tuple(int(x) for x in out)  # type: ignore[return-value]

    def getMetricFromAToB(self, a: str, b: str, useLinkMetric: bool = True) -> Optional[int]:
        m = C.c_uint64()
        has = C.c_int()
        self._err(N.lib.ls_get_metric_a_to_b(self._h, a.encode(), b.encode(),
                                             int(bool(useLinkMetric)), C.byref(m), C.byref(has)))
        return int(m.value) if has.value else None

    def getHopsFromAToB(self, a: str, b: str) -> Optional[int]:
        return self.getMetricFromAToB(a, b, False)

    def getMaxHopsToNode(self, nodeName: str) -> int:
        m = C.c_uint64()
        self._err(N.lib.ls_get_max_hops_to_node(self._h, nodeName.encode(), C.byref(m)))
        return int(m.value)

    @staticmethod
    def pathAInPathB(a: Sequence, b: Sequence) -> bool:
        """``LinkState::pathAInPathB`` (LinkState.h:395-410) through the C-ABI
        (``ls_path_a_in_path_b``): a is a contiguous run of b.  Links compare
        by value, as the reference's ``*a.at(i) == *b.at(j)`` does
        (Link::operator==, LinkState.cpp:356-361: hash and orderedNames), so
        equal links of different LinkStates, snapshots and ``OwnedLink``s
        match.  Each distinct value gets one integer code for the C-ABI."""
        import numpy as np

        ids: Dict[object, int] = {}

        def enc(p):
            return np.array([ids.setdefault((int(l.hash), l.orderedNames), len(ids))
                             for l in p] or [0], np.uint32)

        ea, eb = enc(a), enc(b)
        return bool(N.lib.ls_path_a_in_path_b(N.ptr(ea), len(a), N.ptr(eb), len(b)))

    # -- batch access to the flattened graph ---------------------------------------
    def _csr_sizes(self):
        """(nodes, directed edges) of the flattened graph, without copying it."""
        n = C.c_uint32()
        e = C.c_uint32()
        self._err(N.lib.ls_flatten(self._h, C.byref(n), C.byref(e)))
        return n.value, e.value

    def _csr_link_ids(self):
        """The flattened graph's link id per CSR edge (no node names)."""
        import numpy as np

        _, e = self._csr_sizes()
        lid = np.zeros(max(1, e), np.uint32)
        self._err(N.lib.ls_graph_csr(self._h, None, None, None, N.ptr(lid), None))
        return lid[:e]

    def flatten(self):
        """(node names in id order, row_ptr, col, metric, link_id, overloaded)."""
        import numpy as np

        n = C.c_uint32()
        e = C.c_uint32()
        self._err(N.lib.ls_flatten(self._h, C.byref(n), C.byref(e)))
        ids = np.zeros(n.value, np.uint32)
        rp = np.zeros(n.value + 1, np.uint32)
        col = np.zeros(max(1, e.value), np.uint32)
        met = np.zeros(max(1, e.value), np.int32)
        lid = np.zeros(max(1, e.value), np.uint32)
        ovl = np.zeros(max(1, n.value), np.uint8)
        if n.value:
            self._err(N.lib.ls_graph_node_names(self._h, N.ptr(ids)))
        self._err(N.lib.ls_graph_csr(self._h, N.ptr(rp), N.ptr(col), N.ptr(met, C.c_int32),
                                     N.ptr(lid), N.ptr(ovl, C.c_uint8)))
        names = [self._name(int(i)) for i in ids]
        return names, rp, col[: e.value], met[: e.value], lid[: e.value], ovl[: n.value]

    def engine_handle(self) -> C.c_void_p:
        return C.c_void_p(N.lib.ls_engine(self._h))


class RouteSnapshot(N.NativeHandle):
    """One generation of every node's route databases on the GPUs
    (``spf_route_snapshot``, from LinkState.allSourcesRouteSnapshot): owned by
    its LinkState, closed with it at the latest."""

    _LEVEL = 0

    def __init__(self, ls: "LinkState", h: C.c_void_p) -> None:
        self._ls = ls
        self._adopt(h)

    @property
    def deviceBytes(self) -> int:
        """Device memory the snapshot holds."""
        return int(N.lib.spf_route_snapshot_bytes(self._h))

    def close(self) -> None:
        h = getattr(self, "_h", None)
        ls = getattr(self, "_ls", None)
        lib = getattr(N, "lib", None)
        if h is not None and h.value and lib is not None and ls is not None and not ls.closed:
            lib.ls_route_snapshot_close(ls._h, h)
        self._h = C.c_void_p()
        N._LIVE.discard(self)


class OwnedLink(N.NativeHandle):
    """A standalone ``openr::Link`` (LinkState.h:82-175) built from two
    adjacencies, as ``Link(area, n1, adj1, n2, adj2)`` (LinkState.cpp:127-186)
    -- the C-ABI ``ls_link_*`` object.  Side accessors raise ValueError for a
    node not on the link (std::invalid_argument in the reference)."""

    _destroy = "ls_link_destroy"

    def __init__(self, area: str, node1: str, adj1, node2: str, adj2) -> None:
        h = C.c_void_p()
        N.raise_for(N.lib.ls_link_create(
            area.encode(), node1.encode(), adj1.ifName.encode(), adj1.metric, adj1.adjLabel,
            int(adj1.isOverloaded), node2.encode(), adj2.ifName.encode(), adj2.metric,
            adj2.adjLabel, int(adj2.isOverloaded), C.byref(h)), "ls_link_create")
        self._adopt(h)
        # orderedNames_ = minmax((n1, if1), (n2, if2)) (LinkState.cpp:127-137)
        self._key = tuple(sorted([(node1, adj1.ifName), (node2, adj2.ifName)]))

    @property
    def orderedNames(self) -> Tuple[Tuple[str, str], Tuple[str, str]]:
        return self._key  # type: ignore[return-value]

    def _side(self, fn, node: str, out):
        if fn(self._h, node.encode(), C.byref(out)) != N.SPF_OK:
            raise ValueError(node)
        return out.value

    def getArea(self) -> str:
        return N.lib.ls_link_area(self._h).decode()

    @property
    def hash(self) -> int:
        return int(N.lib.ls_link_hash(self._h))

    def getOtherNodeName(self, node: str) -> str:
        return self._side(N.lib.ls_link_other_node, node, C.c_char_p()).decode()

    def getIfaceFromNode(self, node: str) -> str:
        return self._side(N.lib.ls_link_iface, node, C.c_char_p()).decode()

    def getMetricFromNode(self, node: str) -> int:
        return int(self._side(N.lib.ls_link_metric, node, C.c_uint64()))

    def getAdjLabelFromNode(self, node: str) -> int:
        return int(self._side(N.lib.ls_link_adj_label, node, C.c_int32()))

    def getOverloadFromNode(self, node: str) -> bool:
        return bool(self._side(N.lib.ls_link_overload, node, C.c_int()))

    def isUp(self) -> bool:
        return bool(N.lib.ls_link_is_up(self._h))

    def setMetricFromNode(self, node: str, metric: int, holdUpTtl: int, holdDownTtl: int) -> bool:
        ch = C.c_int()
        if N.lib.ls_link_set_metric(self._h, node.encode(), metric, holdUpTtl, holdDownTtl,
                                    C.byref(ch)) != N.SPF_OK:
            raise ValueError(node)
        return bool(ch.value)

    def setOverloadFromNode(self, node: str, overload: bool, holdUpTtl: int,
                            holdDownTtl: int) -> bool:
        ch = C.c_int()
        if N.lib.ls_link_set_overload(self._h, node.encode(), int(overload), holdUpTtl,
                                      holdDownTtl, C.byref(ch)) != N.SPF_OK:
            raise ValueError(node)
        return bool(ch.value)

    def __eq__(self, other: object) -> bool:
        return isinstance(other, OwnedLink) and bool(N.lib.ls_link_equal(self._h, other._h))

    def __lt__(self, other: "OwnedLink") -> bool:
        return bool(N.lib.ls_link_less(self._h, other._h))

    def __hash__(self) -> int:  # equal links have equal Link::hash
        return self.hash


class HoldableValue(N.NativeHandle):
    """``openr::HoldableValue<bool>`` / ``<LinkStateMetric>`` (LinkState.h:36-58,
    LinkState.cpp:54-125), the C-ABI ``ls_holdable_*`` object."""

    _destroy = "ls_holdable_destroy"

    def __init__(self, value) -> None:
        self._bool = isinstance(value, bool)
        self._adopt(C.c_void_p(N.lib.ls_holdable_create(int(self._bool), int(value))))

    def value(self):
        v = int(N.lib.ls_holdable_value(self._h))
        return bool(v) if self._bool else v

    def hasHold(self) -> bool:
        return bool(N.lib.ls_holdable_has_hold(self._h))

    def decrementTtl(self) -> bool:
        return bool(N.lib.ls_holdable_decrement_ttl(self._h))

    def updateValue(self, value, holdUpTtl: int, holdDownTtl: int) -> bool:
        return bool(N.lib.ls_holdable_update_value(self._h, int(value), holdUpTtl, holdDownTtl))
