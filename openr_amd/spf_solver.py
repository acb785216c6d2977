"""SpfSolver drop-in: the route computation that consumes LinkState's SPF
results (reference ``openr/decision/Decision.cpp`` SpfSolver::SpfSolverImpl).

Covered, single area, over the MI355X engine:
  * ``buildRouteDb`` (:557-722): unicast routes for every prefix of the
    PrefixState (SP_ECMP, IP forwarding), node-label MPLS routes (POP for our
    own label, SWAP/PHP towards every other node, label collisions resolved
    as :605-617 does) and adjacency-label routes (PHP over each of our links);
  * ``createRouteForPrefix`` (:390-555): reachable advertisers, v4 sanity,
    openr (non-BGP) best-route selection = every advertiser, drained
    advertisers filtered (maybeFilterDrainedNodes :766-789), self-advertised
    prefixes skipped;
  * ``getMinCostNodes`` / ``getNextHopsWithMetric`` (with LFA) /
    ``getNextHopsThrift`` (:1082-1305): ONE batched call ``spf_routes``
    (include/openr_spf.h) for all prefixes and node labels of a route build --
    one SPF plan for me (+ every neighbour with LFA) and a next-hop selection
    kernel, one wavefront per destination set.

  * SR_MPLS forwarding (selectBestPathsSpf with perDestination, :829-893 and
    the push-label branch of getNextHopsThrift :1260-1290) over the memoised
    SPF results of me (and, with LFA, of every neighbour);
  * KSP2_ED_ECMP (selectBestPathsKsp2 :895-1018):
    k = 1 / k = 2 edge-disjoint paths to every advertiser from ONE batched
    KSP2 launch (LinkState.prefetchKthPaths -> ls_prefetch_kth_paths), the
    anycast filter LinkState.pathAInPathB, label stacks with PHP and prepend
    labels;
  * addBestPaths (:1020-1080): min-nexthop threshold, static next hops of a
    self-advertised prefix with a prepend label.

  * several areas (Decision.cpp:411-412, 556-722, 1107-1305): the areas
    walked in the order of the reference's std::unordered_map<std::string,
    LinkState> (ls_string_map_order), getMinCostNodes per area, ECMP across
    areas at equal metric, LFA per area, next hops from every area's links;
    node labels collected over every area;
  * best-route selection (selectBestRoutes :728-748): openr routes (every
    advertiser), enable_best_route_selection (selectBestPrefixMetrics /
    selectBestNodeArea, openr/common/Util.h:486-571, Util.cpp:1028-1040) and
    BGP metric vectors (runBestPathSelectionBgp :791-832 over
    MetricVectorUtils::compareMetricVectors, Util.cpp:1101-1217), drained
    advertisers filtered (maybeFilterDrainedNodes :766-789), the best-routes
    cache, doNotInstall = BGP && bgpDryRun.

One area takes the batched kernel path for SP_ECMP/IP prefixes and node
labels; several areas take the reference's per-prefix walk over the memoised
(GPU) SPF results of every area.
"""

from __future__ import annotations

import ctypes as C
from collections import deque
from dataclasses import dataclass, field
from typing import Dict, FrozenSet, List, NamedTuple, Optional, Sequence, Set, Tuple

import numpy as np

from . import _native as N
from .link_state import LinkState

MPLS_LABEL_MIN, MPLS_LABEL_MAX = 0, (1 << 20) - 1
Metric = int


def isMplsLabelValid(label: int) -> bool:
    """openr/common/Util.h isMplsLabelValid: 20-bit label space."""
    return MPLS_LABEL_MIN <= label <= MPLS_LABEL_MAX


class MplsAction(NamedTuple):
    """thrift::MplsAction (openr/if/Network.thrift); an immutable value (a
    named tuple: a route build makes ~10^5 of these objects)."""

    action: str  # "PUSH" | "SWAP" | "PHP" | "POP_AND_LOOKUP"
    swapLabel: Optional[int] = None
    pushLabels: Optional[Tuple[int, ...]] = None


_PHP = MplsAction("PHP")


class NextHopThrift(NamedTuple):
    """thrift::NextHopThrift (Network.thrift:65-86) as built by createNextHop
    (openr/common/Util.cpp:907-922): metric is an i32.  An immutable value
    (a named tuple, hashable, cheap to build)."""

    address: bytes
    ifName: Optional[str]
    metric: int
    mplsAction: Optional[MplsAction]
    area: Optional[str]
    neighborNodeName: Optional[str]


def createNextHop(addr: bytes, ifName: Optional[str], metric: int,
                  mplsAction: Optional[MplsAction] = None, area: Optional[str] = None,
                  neighborNodeName: Optional[str] = None) -> NextHopThrift:
    m = metric & 0xFFFFFFFF
    return NextHopThrift(bytes(addr), ifName, m - (1 << 32) if m >= 1 << 31 else m, mplsAction,
                         area, neighborNodeName)


@dataclass(frozen=True)
class PrefixMetrics:
    """thrift::PrefixMetrics (Lsdb.thrift:228-268)."""

    path_preference: int = 0    # prefer higher
    source_preference: int = 0  # prefer higher
    distance: int = 0           # prefer lower


@dataclass
class MetricEntity:
    """thrift::MetricEntity (Lsdb.thrift:182-204); op is a CompareType name."""

    type: int
    priority: int
    op: str = "WIN_IF_PRESENT"  # | "WIN_IF_NOT_PRESENT" | "IGNORE_IF_NOT_PRESENT"
    isBestPathTieBreaker: bool = False
    metric: Tuple[int, ...] = ()


@dataclass
class MetricVector:
    """thrift::MetricVector (Lsdb.thrift:206-212)."""

    version: int = 0
    metrics: List[MetricEntity] = field(default_factory=list)


@dataclass
class PrefixEntry:
    """The fields of thrift::PrefixEntry (Lsdb.thrift) route building reads."""

    prefix: str
    type: str = "LOOPBACK"
    forwardingType: str = "IP"
    forwardingAlgorithm: str = "SP_ECMP"
    prependLabel: Optional[int] = None
    minNexthop: Optional[int] = None
    metrics: PrefixMetrics = field(default_factory=PrefixMetrics)
    mv: Optional[MetricVector] = None
    data: Optional[bytes] = None

    @property
    def isV4(self) -> bool:
        return ":" not in self.prefix


def nodeAreaMapOrder(ops: Sequence[Tuple[int, Tuple[str, str]]]) -> List[Tuple[str, str]]:
    """The surviving keys of a PrefixEntries map (std::unordered_map<NodeAndArea,
    PrefixEntry>, openr/common/Types.h:24) in its iteration order, after the
    emplace (op 1) / erase (op 0) history ``ops`` (ls_node_area_map_order)."""
    n = len(ops)
    nodes = (C.c_char_p * n)(*[k[0].encode() for _, k in ops])
    areas = (C.c_char_p * n)(*[k[1].encode() for _, k in ops])
    code = (C.c_uint8 * n)(*[o for o, _ in ops])
    order = (C.c_uint32 * n)()
    got = C.c_uint32()
    st = N.lib.ls_node_area_map_order(nodes, areas, code, n, order, C.byref(got))
    if st != N.SPF_OK:
        N.raise_for(st, "ls_node_area_map_order")
    return [ops[order[i]][1] for i in range(got.value)]


_OPS = {"WIN_IF_PRESENT": 0, "WIN_IF_NOT_PRESENT": 1, "IGNORE_IF_NOT_PRESENT": 2}


class _NativePrefixState(N.NativeHandle):
    """dc_prefix_state (include/openr_decision.h): the C++ SpfSolver's PrefixState."""

    _LEVEL = 0
    _destroy = "dc_prefix_state_destroy"

    def __init__(self) -> None:
        self._adopt(C.c_void_p(N.lib.dc_prefix_state_create()))

    def update(self, node: str, area: str, e: "PrefixEntry") -> None:
        r = N.DcPrefixEntry()
        r.prefix = e.prefix.encode()
        r.is_v4 = e.isV4
        r.is_bgp = e.type == "BGP"
        r.forwarding_type = _FWD_TYPE[e.forwardingType]
        r.forwarding_algorithm = _FWD_ALGO[e.forwardingAlgorithm]
        r.has_prepend_label = e.prependLabel is not None
        r.prepend_label = e.prependLabel or 0
        r.has_min_nexthop = e.minNexthop is not None
        r.min_nexthop = e.minNexthop or 0
        r.path_preference = e.metrics.path_preference
        r.source_preference = e.metrics.source_preference
        r.distance = e.metrics.distance
        keep = []
        if e.mv is not None:
            ents = (N.DcMetricEntity * max(1, len(e.mv.metrics)))()
            for i, m in enumerate(e.mv.metrics):
                vals = (C.c_int64 * max(1, len(m.metric)))(*m.metric)
                keep.append(vals)
                ents[i].type, ents[i].priority = m.type, m.priority
                ents[i].op, ents[i].is_tie_breaker = _OPS[m.op], m.isBestPathTieBreaker
                ents[i].n_metric, ents[i].metric = len(m.metric), vals
            r.has_mv, r.mv_version, r.n_mv, r.mv = 1, e.mv.version, len(e.mv.metrics), ents
            keep.append(ents)
        N.raise_for(N.lib.dc_prefix_update(self._h, node.encode(), area.encode(), C.byref(r)),
                    "dc_prefix_update")


class PrefixState:
    """prefix -> {(node, area): PrefixEntry} (openr/decision/PrefixState.h).

    Each prefix's dict iterates in the order of the reference's PrefixEntries
    map (an std::unordered_map, Types.h:24): PrefixState.cpp:47-60 emplaces a
    new advertiser and erases a withdrawn one, and the map's order follows
    from that history, which is kept per prefix (dropped with the map when its
    last advertiser goes, PrefixState.cpp:49-50) and replayed natively
    whenever the key set of a prefix with several advertisers changes.
    runBestPathSelectionBgp's TIE_WINNER / TIE outcome (Decision.cpp:795-832)
    and addBestPaths' prepend-label walk (:1047-1053) depend on it."""

    def __init__(self) -> None:
        self._p: Dict[str, Dict[Tuple[str, str], PrefixEntry]] = {}
        self._ops: Dict[str, List[Tuple[int, Tuple[str, str]]]] = {}
        # the same state in the C++ SpfSolver's PrefixState (dc_prefix_state),
        # kept in step with every update (entries are taken as values: an
        # entry changed after updatePrefix must be updated again)
        self._nat = _NativePrefixState()

    def _reorder(self, prefix: str) -> None:
        ent = self._p[prefix]
        if len(ent) > 1:
            self._p[prefix] = {k: ent[k] for k in nodeAreaMapOrder(self._ops[prefix])}

    def updatePrefix(self, node: str, area: str, entry: PrefixEntry) -> None:
        self._nat.update(node, area, entry)
        key = (node, area)
        ent = self._p.get(entry.prefix)
        if ent is None:
            self._p[entry.prefix] = {key: entry}
            self._ops[entry.prefix] = [(1, key)]
        elif key in ent:  # emplace finds it: assigned in place (:60-68)
            ent[key] = entry
        else:
            ent[key] = entry
            self._ops[entry.prefix].append((1, key))
            self._reorder(entry.prefix)

    def deletePrefix(self, node: str, area: str, prefix: str) -> None:
        N.raise_for(N.lib.dc_prefix_delete(self._nat._h, node.encode(), area.encode(),
                                           prefix.encode()), "dc_prefix_delete")
        ent = self._p.get(prefix)
        if ent is not None and (node, area) in ent:
            del ent[(node, area)]
            if not ent:
                del self._p[prefix]
                del self._ops[prefix]
            else:
                self._ops[prefix].append((0, (node, area)))
                self._reorder(prefix)

    def prefixes(self) -> Dict[str, Dict[Tuple[str, str], PrefixEntry]]:
        return self._p


def prefixTable(prefixState: "PrefixState", area: str, names: Sequence[str]):
    """The arrays of LinkState.allSourcesPrefixRoutes from a PrefixState:
    (table, left).  table (link_state.PrefixTable; table.prefixes names its
    rows) covers the prefixes whose route decision is the SP_ECMP / IP one of
    area `area`; `left` lists the prefixes the host solver keeps: any entry of
    type BGP or with a metric vector, SR_MPLS forwarding, KSP2_ED_ECMP, a
    prepend label, or an entry in another area.  names: the link state's nodes
    in id order (flatten()[0]); an advertiser that is none of them is reached
    by nobody and is left out of its prefix."""
    from .link_state import PrefixTable

    id_of = {s: i for i, s in enumerate(names)}
    ptr, node, pp, sp, dist, mn = [0], [], [], [], [], []
    covered: List[str] = []
    left: List[str] = []
    for prefix, entries in prefixState.prefixes().items():
        if any(na[1] != area or e.type == "BGP" or e.mv is not None or e.forwardingType != "IP" or
               e.forwardingAlgorithm != "SP_ECMP" or e.prependLabel is not None
               for na, e in entries.items()):
            left.append(prefix)
            continue
        for na, e in entries.items():
            if na[0] not in id_of:
                continue
            node.append(id_of[na[0]])
            pp.append(e.metrics.path_preference)
            sp.append(e.metrics.source_preference)
            dist.append(e.metrics.distance)
            mn.append(0 if e.minNexthop is None else e.minNexthop)
        ptr.append(len(node))
        covered.append(prefix)
    table = PrefixTable(np.asarray(ptr, np.uint32), np.asarray(node, np.uint32), np.asarray(pp, np.int32),
                        np.asarray(sp, np.int32), np.asarray(dist, np.int32), np.asarray(mn, np.int64),
                        covered)
    return table, left


@dataclass
class RibUnicastEntry:
    prefix: str
    nexthops: Set[NextHopThrift]
    bestPrefixEntry: PrefixEntry
    bestArea: str
    doNotInstall: bool = False

    @property
    def prefixType(self) -> str:
        return self.bestPrefixEntry.type

    @property
    def data(self) -> Optional[bytes]:
        return self.bestPrefixEntry.data


@dataclass
class RibMplsEntry:
    label: int
    nexthops: Set[NextHopThrift]


@dataclass
class DecisionRouteDb:
    unicastRoutes: Dict[str, RibUnicastEntry] = field(default_factory=dict)
    mplsRoutes: Dict[int, RibMplsEntry] = field(default_factory=dict)

    def addUnicastRoute(self, r: RibUnicastEntry) -> None:
        self.unicastRoutes[r.prefix] = r

    def addMplsRoute(self, r: RibMplsEntry) -> None:
        self.mplsRoutes[r.label] = r

    def calculateUpdate(self, newDb: "DecisionRouteDb") -> "DecisionRouteUpdate":
        """``DecisionRouteDb::calculateUpdate`` (Decision.cpp:111-146): what
        turns this database into ``newDb`` -- entries of ``newDb`` that are new
        or compare unequal, and keys of this one that ``newDb`` lacks.  Routes
        are visited in ascending key order (the reference walks unordered
        maps: no order to reproduce)."""
        delta = DecisionRouteUpdate()
        for prefix in sorted(newDb.unicastRoutes):
            entry = newDb.unicastRoutes[prefix]
            if prefix not in self.unicastRoutes or self.unicastRoutes[prefix] != entry:
                delta.unicastRoutesToUpdate[prefix] = entry
        delta.unicastRoutesToDelete = [p for p in sorted(self.unicastRoutes)
                                       if p not in newDb.unicastRoutes]
        for label in sorted(newDb.mplsRoutes):
            entry = newDb.mplsRoutes[label]
            if label not in self.mplsRoutes or self.mplsRoutes[label] != entry:
                delta.mplsRoutesToUpdate.append(entry)
        delta.mplsRoutesToDelete = [l for l in sorted(self.mplsRoutes) if l not in newDb.mplsRoutes]
        return delta

    def update(self, update: "DecisionRouteUpdate") -> None:
        """``DecisionRouteDb::update`` (Decision.cpp:148-162): deletes first,
        then insert_or_assign of every updated entry."""
        for prefix in update.unicastRoutesToDelete:
            self.unicastRoutes.pop(prefix, None)
        for entry in update.unicastRoutesToUpdate.values():
            self.unicastRoutes[entry.prefix] = entry
        for label in update.mplsRoutesToDelete:
            self.mplsRoutes.pop(label, None)
        for entry in update.mplsRoutesToUpdate:
            self.mplsRoutes[entry.label] = entry


@dataclass
class DecisionRouteUpdate:
    """``DecisionRouteUpdate`` (RouteUpdate.h): the difference Decision
    publishes after a rebuild."""

    unicastRoutesToUpdate: Dict[str, RibUnicastEntry] = field(default_factory=dict)
    unicastRoutesToDelete: List[str] = field(default_factory=list)
    mplsRoutesToUpdate: List[RibMplsEntry] = field(default_factory=list)
    mplsRoutesToDelete: List[int] = field(default_factory=list)

    def empty(self) -> bool:
        return not (self.unicastRoutesToUpdate or self.unicastRoutesToDelete
                    or self.mplsRoutesToUpdate or self.mplsRoutesToDelete)


# enum values of OpenrConfig.thrift:77-85 (getPrefixForwardingTypeAndAlgorithm
# takes the minimum over the best entries)
_FWD_TYPE = {"IP": 0, "SR_MPLS": 1}
_FWD_ALGO = {"SP_ECMP": 0, "KSP2_ED_ECMP": 1}


def getPrefixForwardingTypeAndAlgorithm(entries: Dict[Tuple[str, str], "PrefixEntry"],
                                        best) -> Tuple[str, str]:
    """openr/common/Util.cpp:617-643."""
    if not entries:
        return "IP", "SP_ECMP"
    t, a = 1, 1
    for na, e in entries.items():
        if na not in best:
            continue
        t = min(t, _FWD_TYPE[e.forwardingType])
        a = min(a, _FWD_ALGO[e.forwardingAlgorithm])
        if t == 0 and a == 0:
            break
    return ("IP", "SR_MPLS")[t], ("SP_ECMP", "KSP2_ED_ECMP")[a]


# -- best-route selection helpers (openr/common/Util.h, Util.cpp) ------------------
NodeAndArea = Tuple[str, str]
WINNER, TIE_WINNER, TIE, TIE_LOOSER, LOOSER, ERROR = range(6)  # MetricVectorUtils::CompareResult


def _not(r: int) -> int:
    """MetricVectorUtils::operator! (Util.cpp:1074-1096)."""
    return {WINNER: LOOSER, TIE_WINNER: TIE_LOOSER, TIE: TIE, TIE_LOOSER: TIE_WINNER,
            LOOSER: WINNER, ERROR: ERROR}[r]


def _isDecisive(r: int) -> bool:
    return r in (WINNER, LOOSER, ERROR)


def _compareMetrics(l: Sequence[int], r: Sequence[int], tieBreaker: bool) -> int:
    """MetricVectorUtils::compareMetrics (Util.cpp:1135-1151)."""
    if len(l) != len(r):
        return ERROR
    for a, b in zip(l, r):
        if a > b:
            return TIE_WINNER if tieBreaker else WINNER
        if a < b:
            return TIE_LOOSER if tieBreaker else LOOSER
    return TIE


def _resultForLoner(e: MetricEntity) -> int:
    """MetricVectorUtils::resultForLoner (Util.cpp:1153-1164)."""
    if e.op == "WIN_IF_PRESENT":
        return TIE_WINNER if e.isBestPathTieBreaker else WINNER
    if e.op == "WIN_IF_NOT_PRESENT":
        return TIE_LOOSER if e.isBestPathTieBreaker else LOOSER
    return TIE  # IGNORE_IF_NOT_PRESENT


def maybeUpdate(target: int, update: int) -> int:
    """MetricVectorUtils::maybeUpdate (Util.cpp:1166-1171), returning the new target."""
    return update if (_isDecisive(update) or target == TIE) else target


compareMetrics = _compareMetrics
resultForLoner = _resultForLoner
isDecisive = _isDecisive
inverse = _not


def compareMetricVectors(l: MetricVector, r: MetricVector) -> int:
    """MetricVectorUtils::compareMetricVectors (Util.cpp:1173-1216).  Like
    sortMetricVector (:1120-1133, a const_cast sort) it puts an unsorted
    vector's entities in decreasing priority IN PLACE -- callers see their
    vectors reordered, as the reference's do.  (std::sort is not stable; a
    stable sort here, so equal priorities keep their order.)"""
    result = TIE

    def upd(u: int) -> None:
        nonlocal result
        if _isDecisive(u) or result == TIE:
            result = u

    if l.version != r.version:
        return ERROR

    def srt(mv: MetricVector) -> List[MetricEntity]:
        pr = [e.priority for e in mv.metrics]
        if any(pr[i] < pr[i + 1] for i in range(len(pr) - 1)):
            mv.metrics.sort(key=lambda e: -e.priority)
        return mv.metrics

    L, R = srt(l), srt(r)
    i = j = 0
    while not _isDecisive(result) and i < len(L) and j < len(R):
        a, b = L[i], R[j]
        if a.type == b.type:
            if a.isBestPathTieBreaker != b.isBestPathTieBreaker:
                upd(ERROR)
            else:
                upd(_compareMetrics(a.metric, b.metric, a.isBestPathTieBreaker))
            i += 1
            j += 1
        elif a.priority > b.priority:
            upd(_resultForLoner(a))
            i += 1
        elif a.priority < b.priority:
            upd(_not(_resultForLoner(b)))
            j += 1
        else:
            upd(ERROR)  # same priority, different types
    while not _isDecisive(result) and i < len(L):
        upd(_resultForLoner(L[i]))
        i += 1
    while not _isDecisive(result) and j < len(R):
        upd(_not(_resultForLoner(R[j])))
        j += 1
    return result


def selectBestPrefixMetrics(entries: Dict[NodeAndArea, PrefixEntry]) -> List[NodeAndArea]:
    """openr/common/Util.h:540-571: the keys with the best (path_preference,
    source_preference, -distance) tuple, starting from (0, 0, 0) -- so entries
    below it never enter (a positive distance with zero preferences); a
    std::set, here a sorted list."""
    best_t = (0, 0, 0)
    best: List[NodeAndArea] = []
    for key, e in entries.items():
        m = e.metrics
        t = (m.path_preference, m.source_preference, -m.distance)
        if t < best_t:
            continue
        if t > best_t:
            best_t, best = t, []
        best.append(key)
    return sorted(best)


def selectBestNodeArea(allNodeAreas: Sequence[NodeAndArea], myNodeName: str) -> NodeAndArea:
    """openr/common/Util.cpp:1028-1040: our own entry if we are among them,
    else the smallest."""
    for na in allNodeAreas:
        if na[0] == myNodeName:
            return na
    return allNodeAreas[0]


@dataclass
class BestRouteSelectionResult:
    """openr/decision/RibEntry.h BestRouteSelectionResult; allNodeAreas is a
    std::set (sorted list here)."""

    success: bool = False
    allNodeAreas: List[NodeAndArea] = field(default_factory=list)
    bestNodeArea: Optional[NodeAndArea] = None

    def hasNode(self, node: str) -> bool:
        return any(na[0] == node for na in self.allNodeAreas)


def areaOrder(areaLinkStates: Dict[str, LinkState]) -> List[Tuple[str, LinkState]]:
    """The areas in the iteration order of the reference's
    std::unordered_map<std::string, LinkState> when the dict's keys were
    emplaced in insertion order (ls_string_map_order)."""
    keys = list(areaLinkStates)
    if len(keys) <= 1:
        return list(areaLinkStates.items())
    arr = (C.c_char_p * len(keys))(*[k.encode() for k in keys])
    order = (C.c_uint32 * len(keys))()
    n = C.c_uint32()
    st = N.lib.ls_string_map_order(arr, len(keys), order, C.byref(n))
    if st != N.SPF_OK:
        N.raise_for(st, "ls_string_map_order")
    return [(keys[order[i]], areaLinkStates[keys[order[i]]]) for i in range(n.value)]


class _LazySetResults:
    """spf_routes' outputs as a sequence of _SetResult, built on access."""

    def __init__(self, mins, cnt, edge, metric, deg) -> None:
        self.mins, self.cnt, self.edge, self.metric, self.deg = mins, cnt, edge, metric, deg

    def __len__(self) -> int:
        return len(self.cnt)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        mm = int(self.mins[i])
        b = i * self.deg
        c = int(self.cnt[i])
        hops = list(zip(self.edge[b:b + c].tolist(), self.metric[b:b + c].tolist()))
        return _SetResult(None if mm == (1 << 64) - 1 else mm, hops)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


@dataclass
class _SetResult:
    min_metric: Optional[int]
    hops: List[Tuple[int, int]]  # (directed edge me -> neighbour, metric)


class _NativeSolver(N.NativeHandle):
    """dc_solver (include/openr_decision.h): the C++ SpfSolver."""

    _LEVEL = 0
    _destroy = "dc_solver_destroy"

    def __init__(self, me: str, enableV4: bool, lfa: bool, dryRun: bool, brs: bool) -> None:
        h = C.c_void_p()
        N.raise_for(N.lib.dc_solver_create(me.encode(), int(enableV4), int(lfa), int(dryRun),
                                           int(brs), C.byref(h)), "dc_solver_create")
        self._adopt(h)

    def set_static(self, label: int, nhs: Sequence["NextHopThrift"]) -> None:
        recs = (N.DcNexthop * max(1, len(nhs)))()
        strings: List[bytes] = []
        labels: List[int] = []

        def sid(x: Optional[str]) -> int:
            if x is None:
                return N.DC_NONE
            strings.append(x.encode())
            return len(strings) - 1

        for r, nh in zip(recs, nhs):
            r.address[:len(nh.address)] = list(nh.address)
            r.address_len = len(nh.address)
            r.metric = nh.metric
            a = nh.mplsAction
            if a is not None:
                r.mpls_action = N.DC_MPLS_ACTIONS.index(a.action)
                r.swap_label = a.swapLabel or 0
                if a.pushLabels:
                    r.push_off, r.n_push = len(labels), len(a.pushLabels)
                    labels.extend(a.pushLabels)
            r.ifname, r.area, r.neighbor = sid(nh.ifName), sid(nh.area), sid(nh.neighborNodeName)
        sarr = (C.c_char_p * max(1, len(strings)))(*strings)
        larr = (C.c_int32 * max(1, len(labels)))(*labels)
        N.raise_for(N.lib.dc_static_mpls_route_set(self._h, label, recs, len(nhs), sarr, larr),
                    (N.lib.dc_last_error(self._h) or b"").decode())


class NativeRouteDb(N.NativeHandle):
    """A DecisionRouteDb built by the C++ SpfSolver (dc_route_db): read as
    tables, or materialised into the Python route types (``routeDb()``)."""

    _LEVEL = 0
    _destroy = "dc_route_db_destroy"

    def __init__(self, h: C.c_void_p, prefixState: "PrefixState") -> None:
        self._adopt(h)
        self._ps = prefixState

    def unicastCount(self) -> int:
        return int(N.lib.dc_route_db_unicast_count(self._h))

    def mplsCount(self) -> int:
        return int(N.lib.dc_route_db_mpls_count(self._h))

    def nexthopCount(self) -> int:
        n = C.c_uint32()
        N.lib.dc_route_db_nexthops(self._h, C.byref(n))
        return int(n.value)

    def nexthopRecords(self) -> np.ndarray:
        n = C.c_uint32()
        p = N.lib.dc_route_db_nexthops(self._h, C.byref(n))
        if not n.value:
            return np.zeros(0, N.DC_NEXTHOP_DTYPE)
        raw = (C.c_char * (n.value * N.DC_NEXTHOP_DTYPE.itemsize)).from_address(p)
        return np.frombuffer(raw, N.DC_NEXTHOP_DTYPE).copy()

    def _table(self, fn, cols: int) -> np.ndarray:
        n = C.c_uint32()
        p = getattr(N.lib, fn)(self._h, C.byref(n))
        if not n.value:
            return np.zeros((0, cols), np.uint32)
        raw = (C.c_uint32 * (n.value * cols)).from_address(p)
        return np.frombuffer(raw, np.uint32).reshape(n.value, cols).copy()

    def routeDb(self) -> "DecisionRouteDb":
        recs = self.nexthopRecords()
        nl = C.c_uint32()
        lp = N.lib.dc_route_db_labels(self._h, C.byref(nl))
        pool = (np.frombuffer((C.c_int32 * nl.value).from_address(lp), np.int32).tolist()
                if nl.value else [])
        strs = [N.lib.dc_route_db_string(self._h, i).decode()
                for i in range(N.lib.dc_route_db_strings(self._h))]
        none = N.DC_NONE
        actions: Dict[tuple, MplsAction] = {}
        nhs: List[NextHopThrift] = []
        for r in recs.tolist():
            addr, alen, act, npush, _, metric, swap, poff, ifn, area, nb = r
            a = None
            if act:
                key = (act, swap, tuple(pool[poff:poff + npush]) if act == 1 else ())
                a = actions.get(key)
                if a is None:
                    name = N.DC_MPLS_ACTIONS[act]
                    a = actions[key] = MplsAction(name, swap if name == "SWAP" else None,
                                                  key[2] if name == "PUSH" else None)
            nhs.append(NextHopThrift(bytes(addr[:alen]), None if ifn == none else strs[ifn], metric, a,
                                     None if area == none else strs[area],
                                     None if nb == none else strs[nb]))
        db = DecisionRouteDb()
        prefixes = self._ps.prefixes()
        for p, node, area, dni, b, e in self._table("dc_route_db_unicast_table", 6).tolist():
            prefix = strs[p]
            na = (strs[node], strs[area])
            db.addUnicastRoute(RibUnicastEntry(prefix, set(nhs[b:e]), prefixes[prefix][na], na[1],
                                               bool(dni)))
        for label, b, e in self._table("dc_route_db_mpls_table", 3).tolist():
            label = label - (1 << 32) if label >= 1 << 31 else label
            db.addMplsRoute(RibMplsEntry(label, set(nhs[b:e])))
        return db


_COUNTERS = ("decision.no_route_to_prefix", "decision.skipped_unicast_route",
             "decision.no_route_to_label", "decision.incompatible_forwarding_type",
             "decision.duplicate_node_label")


class SpfSolver:
    """``openr::SpfSolver`` (Decision.h) on the MI355X engine.

    buildRouteDb runs the C++ SpfSolver (openr_amd/csrc/decision.cpp, the
    C-ABI of include/openr_decision.h a C++ Decision calls) and materialises
    its DecisionRouteDb here; ``native = False`` (or ``_generic``) takes the
    Python restatement below instead, which the tests hold it equal to."""

    native = True
    # one-advertiser prefixes skip the selection walk, and one-advertiser IP
    # routes and label routes are assembled inline (tests switch it off to
    # compare against the generic walk and getNextHopsThrift restatement)
    _single_fast = True

    def __init__(self, myNodeName: str, enableV4: bool, computeLfaPaths: bool,
                 enableOrderedFib: bool = False, bgpDryRun: bool = False,
                 enableBestRouteSelection: bool = False) -> None:
        self.myNodeName = myNodeName
        self.enableV4 = enableV4
        self.computeLfaPaths = computeLfaPaths
        self.bgpDryRun = bgpDryRun
        self.staticMplsRoutes: Dict[int, List[NextHopThrift]] = {}
        self.enableBestRouteSelection = enableBestRouteSelection
        self._bestRoutesCache: Dict[str, BestRouteSelectionResult] = {}
        self.counters: Dict[str, int] = {}  # the fb303 stats SpfSolver bumps (subset)
        self._nat: Dict[str, _NativeSolver] = {}  # C++ solvers by myNodeName
        self._nat_counts: Dict[str, Dict[str, int]] = {}
        self._nat_cache = None  # (solver, prefix state) of the last native build

    def getBestRoutesCache(self) -> Dict[str, BestRouteSelectionResult]:
        """SpfSolver::getBestRoutesCache: the last route build's selections."""
        if self._nat_cache is not None:  # read from the C++ solver on demand
            nat, ps = self._nat_cache
            cache: Dict[str, BestRouteSelectionResult] = {}
            for prefix in ps.prefixes():
                found, ok = C.c_int(), C.c_int()
                bn, ba = C.c_char_p(), C.c_char_p()
                cnt = C.c_uint32()
                pb = prefix.encode()
                N.raise_for(N.lib.dc_best_route(nat._h, pb, C.byref(found), C.byref(ok), C.byref(bn),
                                                C.byref(ba), None, None, 0, C.byref(cnt)), "dc_best_route")
                if not found.value:
                    continue
                nodes = (C.c_char_p * max(1, cnt.value))()
                areas = (C.c_char_p * max(1, cnt.value))()
                N.lib.dc_best_route(nat._h, pb, C.byref(found), C.byref(ok), C.byref(bn), C.byref(ba),
                                    nodes, areas, cnt.value, C.byref(cnt))
                cache[prefix] = BestRouteSelectionResult(
                    bool(ok.value), [(nodes[i].decode(), areas[i].decode()) for i in range(cnt.value)],
                    None if bn.value is None else (bn.value.decode(), ba.value.decode()))
            return cache
        return dict(self._bestRoutesCache)

    def _native_solver(self, me: str) -> _NativeSolver:
        nat = self._nat.get(me)
        if nat is None:
            nat = self._nat[me] = _NativeSolver(me, self.enableV4, self.computeLfaPaths,
                                                self.bgpDryRun, self.enableBestRouteSelection)
            self._nat_counts[me] = {}
            for label, nhs in self.staticMplsRoutes.items():
                nat.set_static(label, nhs)
        return nat

    def buildRouteDbNative(self, myNodeName: str, areaLinkStates: Dict[str, LinkState],
                           prefixState: PrefixState) -> Optional[NativeRouteDb]:
        """buildRouteDb on the C++ SpfSolver (dc_build_route_db), the route DB
        left native (tables; NativeRouteDb.routeDb() materialises it)."""
        nat = self._native_solver(myNodeName)
        names = list(areaLinkStates)
        arr = (C.c_char_p * max(1, len(names)))(*[a.encode() for a in names])
        hs = (C.c_void_p * max(1, len(names)))(*[areaLinkStates[a]._h.value for a in names])
        out = C.c_void_p()
        st = N.lib.dc_build_route_db(nat._h, arr, hs, len(names), prefixState._nat._h, C.byref(out))
        N.raise_for(st, (N.lib.dc_last_error(nat._h) or b"").decode())
        seen = self._nat_counts[myNodeName]
        for k in _COUNTERS:  # the fb303 counters bumped by this build
            now = int(N.lib.dc_counter(nat._h, k.encode()))
            if now != seen.get(k, 0):
                self.counters[k] = self.counters.get(k, 0) + now - seen.get(k, 0)
                seen[k] = now
        self._nat_cache = (nat, prefixState)
        return NativeRouteDb(out, prefixState) if out.value else None

    def _bump(self, key: str) -> None:
        self.counters[key] = self.counters.get(key, 0) + 1

    def updateStaticMplsRoutes(self, routesToUpdate: Dict[int, List[NextHopThrift]],
                               routesToDelete: Sequence[int] = ()) -> None:
        """SpfSolver::updateStaticMplsRoutes (Decision.cpp): label -> next hops."""
        for label, nhs in routesToUpdate.items():
            self.staticMplsRoutes[label] = list(nhs)
            for nat in self._nat.values():
                nat.set_static(label, nhs)
        for label in routesToDelete:
            self.staticMplsRoutes.pop(label, None)
            for nat in self._nat.values():
                N.raise_for(N.lib.dc_static_mpls_route_delete(nat._h, label), "static delete")

    # -- batched next-hop selection (getMinCostNodes/..WithMetric/..Thrift) ----
    def _select(self, ls: LinkState, me: str, sets: Sequence[Sequence[str]]) -> List[_SetResult]:
        names, rp, col, met, lid, ovl = ls.flatten()
        id_of = {n: i for i, n in enumerate(names)}
        if me not in id_of or not sets:
            # nothing selected: empty arrays of the same shapes, so
            # _buildSingleArea reads this build's (empty) selection, never a
            # previous build's
            self._lid = lid
            self._raw = (np.full(len(sets), (1 << 64) - 1, np.uint64), np.zeros(len(sets), np.uint32),
                         np.zeros(len(sets), np.uint32), np.zeros(len(sets), np.uint64), 1)
            return [_SetResult(None, []) for _ in sets]
        ptr = np.zeros(len(sets) + 1, np.uint32)
        members: List[int] = []
        for i, s in enumerate(sets):
            members.extend(id_of[d] for d in s if d in id_of)
            ptr[i + 1] = len(members)
        nodes = np.asarray(members if members else [0], np.uint32)
        m = id_of[me]
        deg = max(1, int(rp[m + 1] - rp[m]))
        mins = np.zeros(len(sets), np.uint64)
        cnt = np.zeros(len(sets), np.uint32)
        edge = np.zeros(len(sets) * deg, np.uint32)
        metric = np.zeros(len(sets) * deg, np.uint64)
        flags = N.SPF_ROUTE_LFA if self.computeLfaPaths else 0
        # A resident all-sources pass (LinkState.prefetchAllSources: every
        # node's row and bitmaps on the GPUs) answers from me's owner with
        # no new SPF plan; otherwise one batched plan for me (+ neighbours)
        mp = N.lib.ls_all_sources_plan(ls._h)
        st = N.SPF_E_UNSUPPORTED
        if mp:
            st = N.lib.spf_mplan_routes(C.c_void_p(mp), m, N.ptr(ptr), N.ptr(nodes), len(sets), flags,
                                        N.ptr(mins, C.c_uint64), N.ptr(cnt), N.ptr(edge),
                                        N.ptr(metric, C.c_uint64))
            if st not in (N.SPF_OK, N.SPF_E_UNSUPPORTED):
                N.raise_for(st, N.global_error())
        if st != N.SPF_OK:
            st = N.lib.spf_routes(ls.engine_handle(), m, N.ptr(ptr), N.ptr(nodes), len(sets), flags,
                                  N.ptr(mins, C.c_uint64), N.ptr(cnt), N.ptr(edge),
                                  N.ptr(metric, C.c_uint64))
        if st != N.SPF_OK:
            N.raise_for(st, (N.lib.spf_last_error(ls.engine_handle()) or b"").decode())
        self._lid = lid
        self._raw = (mins, cnt, edge, metric, deg)
        return _LazySetResults(mins, cnt, edge, metric, deg)

    def _next_hops(self, ls: LinkState, me: str, area: str, res, isV4: bool,
                   dsts: Set[str], swapLabel: Optional[int]) -> Set[NextHopThrift]:
        """getNextHopsThrift (Decision.cpp:1198-1305) from the kernel's
        (link, metric) selection (a _SetResult, or its hops: (edge, metric)
        pairs)."""
        out: Set[NextHopThrift] = set()
        cache = self._link_fields(ls, me)
        # one action object per call (the route's), the named tuples built
        # with tuple.__new__ (the generated __new__ wrapper was a third of
        # the host route assembly: ~10^5 next hops per fabric build)
        swap = None if swapLabel is None else tuple.__new__(MplsAction, ("SWAP", swapLabel, None))
        mk = tuple.__new__
        add = out.add
        for e, metric in (res.hops if isinstance(res, _SetResult) else res):
            li = cache.get(e)
            if li is None:
                li = self._link_field(ls, me, cache, e)
            nb, iface, v4, v6, larea = li
            action = None if swap is None else (_PHP if nb in dsts else swap)
            m = metric & 0xFFFFFFFF
            add(mk(NextHopThrift, (v4 if isV4 else v6, iface, m - (1 << 32) if m >= 1 << 31 else m,
                                   action, larea, nb)))
        return out

    def _link_fields(self, ls: LinkState, me: str) -> Dict[int, tuple]:
        """directed edge -> (neighbour, iface, v4, v6, area) of me's link, kept
        while the flattened graph (self._lid) is the same."""
        info = getattr(self, "_edge_info", None)
        if info is None or info[0] is not ls or info[1] != me or info[2] is not self._lid:
            info = self._edge_info = (ls, me, self._lid, {})
        return info[3]

    def _link_field(self, ls: LinkState, me: str, cache: Dict[int, tuple], e: int) -> tuple:
        link = ls._link(int(self._lid[e]))
        li = cache[e] = (link.getOtherNodeName(me), link.getIfaceFromNode(me),
                         bytes(link.getNhV4FromNode(me)), bytes(link.getNhV6FromNode(me)),
                         link.getArea())
        return li

    # -- SR_MPLS SP_ECMP: getNextHopsWithMetric / getNextHopsThrift with
    #    perDestination = true (Decision.cpp:829-893, 1107-1305) --------------------
    def _srSpfNextHops(self, ls: LinkState, me: str, area: str, best: List[Tuple[str, str]],
                       ents: Dict[Tuple[str, str], PrefixEntry], isV4: bool,
                       labels: Dict[str, int]) -> Set[NextHopThrift]:
        dsts = list(best)
        if any(na[0] == me for na in best):  # :848-857
            for na, e in ents.items():
                if na[0] == me and e.prependLabel is not None:
                    if na in dsts:
                        dsts.remove(na)
                    break
        dstSet = set(dsts)
        mine = ls.getSpfResult(me)
        shortest, minCost = (1 << 64) - 1, set()
        for d, _ in sorted(dsts):  # getMinCostNodes (:1082-1105)
            if d not in mine:
                continue
            m = mine[d].metric()
            if shortest >= m:
                if shortest > m:
                    shortest, minCost = m, set()
                minCost.add(d)
        nextHopNodes: Dict[Tuple[str, str], int] = {}
        for d in minCost:
            for nh in mine[d].nextHops():
                nextHopNodes[(nh, d)] = shortest - ls.getMetricFromAToB(me, nh)
        if self.computeLfaPaths and minCost:
            # me + every neighbour in one batched plan (Decision.cpp:1158-1165)
            ls.prefetchSpfResults([me] + [l.getOtherNodeName(me) for l in ls.linksFromNode(me)
                                          if l.isUp()])
            for link in ls.linksFromNode(me):
                if not link.isUp():
                    continue
                nb = link.getOtherNodeName(me)
                fromNb = ls.getSpfResult(nb)
                nbToHere = fromNb[me].metric()
                for d, a in sorted(dsts):
                    if a != area or d not in fromNb:
                        continue
                    dn = fromNb[d].metric()
                    if dn < shortest + nbToHere:  # RFC 5286 (:1180)
                        key = (nb, d)
                        if key not in nextHopNodes or nextHopNodes[key] > dn:
                            nextHopNodes[key] = dn
        out: Set[NextHopThrift] = set()
        if not nextHopNodes:
            return out
        for link in ls.linksFromNode(me):
            nb = link.getOtherNodeName(me)
            for d, a in sorted(dsts):
                if a != area:
                    continue
                via = nextHopNodes.get((nb, d))
                if via is None or not link.isUp():
                    continue
                if (nb, area) in dstSet and nb != d:
                    continue
                over = link.getMetricFromNode(me) + via
                if not self.computeLfaPaths and over != shortest:
                    continue
                push: List[int] = []
                pe = ents[(d, area)]
                if pe.prependLabel is not None:
                    push.append(pe.prependLabel)
                    if not isMplsLabelValid(push[-1]):
                        continue
                if d != nb:
                    push.append(labels.get(d, 0))
                    if not isMplsLabelValid(push[-1]):
                        continue
                action = MplsAction("PUSH", None, tuple(push)) if push else None
                addr = link.getNhV4FromNode(me) if isV4 else link.getNhV6FromNode(me)
                out.add(createNextHop(addr, link.getIfaceFromNode(me), over, action,
                                      link.getArea(), nb))
        return out

    # -- KSP2_ED_ECMP: selectBestPathsKsp2 (Decision.cpp:895-1018) -------------------
    def _ksp2NextHops(self, ls: LinkState, me: str, area: str, best: List[Tuple[str, str]],
                      ents: Dict[Tuple[str, str], PrefixEntry], isV4: bool,
                      labels: Dict[str, int]) -> Set[NextHopThrift]:
        paths = []
        for node, a in sorted(best):
            if node == me and a == area:
                continue
            paths.extend(ls.getKthPaths(me, node, 1))
        first = len(paths)
        for node, a in sorted(best):
            if a != area:
                continue
            for sec in ls.getKthPaths(me, node, 2):
                # anycast: drop a second path that contains a shortest one
                if not any(LinkState.pathAInPathB(paths[i], sec) for i in range(first)):
                    paths.append(sec)
        out: Set[NextHopThrift] = set()
        for path in paths:
            cost, stack, nxt = 0, deque(), me
            for link in path:
                cost += link.getMetricFromNode(nxt)
                nxt = link.getOtherNodeName(nxt)
                stack.appendleft(labels.get(nxt, 0))
            stack.pop()  # the first hop's label: PHP
            pe = ents[(nxt, area)]
            if pe.prependLabel is not None:
                stack.appendleft(pe.prependLabel)  # bottom of the stack
            head = path[0]
            action = MplsAction("PUSH", None, tuple(stack)) if stack else None
            addr = head.getNhV4FromNode(me) if isV4 else head.getNhV6FromNode(me)
            out.add(createNextHop(addr, head.getIfaceFromNode(me), cost, action, head.getArea(),
                                  head.getOtherNodeName(me)))
        return out

    # -- addBestPaths (Decision.cpp:1020-1080) ---------------------------------------
    def _addBestPaths(self, me: str, prefix: str, best: Sequence[Tuple[str, str]],
                      bestNA: Tuple[str, str], ents: Dict[Tuple[str, str], PrefixEntry],
                      nhs: Set[NextHopThrift], isBgp: bool = False) -> Optional[RibUnicastEntry]:
        need = None
        for na in best:  # getMinNextHopThreshold: the largest minNexthop
            m = ents[na].minNexthop
            if m is not None and (need is None or m > need):
                need = m
        if need is not None and need > len(nhs):
            return None  # min-nexthop requirement not met
        if any(na[0] == me for na in best):
            prepend = next((e.prependLabel for na, e in ents.items()  # map order (:1047-1053)
                            if na[0] == me and e.prependLabel is not None), None)
            assert prepend is not None, "self route must carry a prepend label"
            nhs = set(nhs)
            for nh in self.staticMplsRoutes.get(prepend, []):
                nhs.add(createNextHop(nh.address, None, 0, None))
        return RibUnicastEntry(prefix, nhs, ents[bestNA], bestNA[1], isBgp and self.bgpDryRun)

    # -- best-route selection (Decision.cpp:728-832) ---------------------------------
    def _maybeFilterDrainedNodes(self, res: BestRouteSelectionResult,
                                 areaLinkStates: Dict[str, LinkState]) -> BestRouteSelectionResult:
        """:766-789 -- the filtered copy keeps the unfiltered bestNodeArea (its
        `filtered.bestNodeArea != result.bestNodeArea` test compares a copy
        with its source)."""
        kept = [na for na in res.allNodeAreas
                if not areaLinkStates[na[1]].isNodeOverloaded(na[0])]
        if not kept:
            return res
        return BestRouteSelectionResult(res.success, kept, res.bestNodeArea)

    def _runBestPathSelectionBgp(self, ents: Dict[Tuple[str, str], PrefixEntry],
                                 areaLinkStates: Dict[str, LinkState]) -> BestRouteSelectionResult:
        """:791-832, visiting the entries in the order of the reference's
        PrefixEntries map (PrefixState keeps each prefix's dict in it; the
        reachable-entry filter of createRouteForPrefix, :409-420, erases in
        place and keeps the survivors' order): bestNodeArea (TIE_WINNER) and
        whether a TIE / ERROR aborts before a later WINNER follow it."""
        ret = BestRouteSelectionResult()
        bestVector: Optional[MetricVector] = None
        chosen: List[Tuple[str, str]] = []
        for na, e in ents.items():
            mv = e.mv
            r = WINNER if bestVector is None else compareMetricVectors(mv, bestVector)
            if r == WINNER:
                chosen = []
            if r in (WINNER, TIE_WINNER):
                bestVector = mv
                ret.bestNodeArea = na
            if r in (WINNER, TIE_WINNER, TIE_LOOSER):
                chosen.append(na)
            elif r in (TIE, ERROR):
                ret.allNodeAreas = sorted(chosen)
                return ret  # tie / error ordering the entries: no route
        ret.allNodeAreas = sorted(chosen)
        ret.success = True
        return self._maybeFilterDrainedNodes(ret, areaLinkStates)

    def _selectBestRoutes(self, me: str, ents: Dict[Tuple[str, str], PrefixEntry], isBgp: bool,
                          areaLinkStates: Dict[str, LinkState]) -> BestRouteSelectionResult:
        if self.enableBestRouteSelection:
            best = selectBestPrefixMetrics(ents)
            ret = BestRouteSelectionResult(True, best, selectBestNodeArea(best, me) if best else None)
        elif isBgp:
            ret = self._runBestPathSelectionBgp(ents, areaLinkStates)
        else:  # openr routes: every advertiser is best
            best = sorted(ents)
            ret = BestRouteSelectionResult(True, best, best[0])
        return self._maybeFilterDrainedNodes(ret, areaLinkStates)

    # -- several areas: the reference's per-prefix walk (Decision.cpp:1082-1305) ------
    _INF = (1 << 64) - 1

    @staticmethod
    def _getMinCostNodes(spf, dstNodeAreas) -> Tuple[int, Set[str]]:
        """:1082-1105 (the destination's area is not checked: a node of the
        set reached in any area counts)."""
        shortest, nodes = SpfSolver._INF, set()
        for d, _ in sorted(dstNodeAreas):
            if d not in spf:
                continue
            m = spf[d].metric()
            if shortest >= m:
                if shortest > m:
                    shortest, nodes = m, set()
                nodes.add(d)
        return shortest, nodes

    def _getNextHopsWithMetric(self, me: str, dstNodeAreas, perDestination: bool,
                               areas: List[Tuple[str, LinkState]]):
        """:1107-1196 over the areas in the reference's map order."""
        M = self._INF
        nh: Dict[Tuple[str, str], int] = {}
        shortest = M
        for area, ls in areas:
            here = ls.getSpfResult(me)
            mcm, mc = self._getMinCostNodes(here, dstNodeAreas)
            if shortest < mcm:
                continue
            if shortest > mcm:
                shortest = mcm
                nh.clear()
            if not mc:
                continue
            for d in mc:
                ref = d if perDestination else ""
                for hop in here[d].nextHops():
                    nh[(hop, ref)] = (shortest - ls.getMetricFromAToB(me, hop)) & M
            if self.computeLfaPaths:
                for link in ls.linksFromNode(me):
                    if not link.isUp():
                        continue
                    nb = link.getOtherNodeName(me)
                    fromNb = ls.getSpfResult(nb)
                    nbToHere = fromNb[me].metric()
                    for d, dArea in sorted(dstNodeAreas):
                        if area != dArea or d not in fromNb:
                            continue
                        dn = fromNb[d].metric()
                        if dn < ((shortest + nbToHere) & M):  # RFC 5286 (:1180)
                            key = (nb, d if perDestination else "")
                            if key not in nh or nh[key] > dn:
                                nh[key] = dn
        return shortest, nh

    def _getNextHopsThrift(self, me: str, dstNodeAreas, isV4: bool, perDestination: bool,
                           minMetric: int, nextHopNodes: Dict[Tuple[str, str], int],
                           swapLabel: Optional[int], areas: List[Tuple[str, LinkState]],
                           ents: Dict[Tuple[str, str], PrefixEntry]) -> Set[NextHopThrift]:
        """:1198-1305 over every area's links."""
        M = self._INF
        dsts = sorted(dstNodeAreas) if perDestination else [("", "")]
        dstSet = set(dstNodeAreas)
        out: Set[NextHopThrift] = set()
        for area, ls in areas:
            labels = ls.getAdjacencyDatabaseLabels() if perDestination else {}
            for link in ls.linksFromNode(me):
                nb = link.getOtherNodeName(me)
                for d, dArea in dsts:
                    if dArea and area != dArea:
                        continue
                    via = nextHopNodes.get((nb, d))
                    if via is None or not link.isUp():
                        continue
                    if d and (nb, area) in dstSet and nb != d:
                        continue
                    over = (link.getMetricFromNode(me) + via) & M
                    if not self.computeLfaPaths and over != minMetric:
                        continue
                    action = None
                    if swapLabel is not None:
                        action = (MplsAction("PHP") if (nb, area) in dstSet
                                  else MplsAction("SWAP", swapLabel))
                    if d:
                        push: List[int] = []
                        pe = ents[(d, area)]
                        if pe.prependLabel is not None:
                            push.append(pe.prependLabel)
                            if not isMplsLabelValid(push[-1]):
                                continue
                        if d != nb:
                            push.append(labels[d])  # getAdjacencyDatabases().at(dstNode)
                            if not isMplsLabelValid(push[-1]):
                                continue
                        if push:
                            action = MplsAction("PUSH", None, tuple(push))
                    addr = link.getNhV4FromNode(me) if isV4 else link.getNhV6FromNode(me)
                    out.add(createNextHop(addr, link.getIfaceFromNode(me), over, action,
                                          link.getArea(), nb))
        return out

    def _selectBestPathsSpf(self, me: str, prefix: str, res: BestRouteSelectionResult,
                            ents: Dict[Tuple[str, str], PrefixEntry], isBgp: bool, ftype: str,
                            areas: List[Tuple[str, LinkState]]) -> Optional[RibUnicastEntry]:
        """:834-893."""
        isV4 = next(iter(ents.values())).isV4
        perDest = ftype == "SR_MPLS"
        filtered = list(res.allNodeAreas)
        if res.hasNode(me) and perDest:
            for na, e in ents.items():  # map order (:855-862)
                if na[0] == me and e.prependLabel is not None:
                    if na in filtered:
                        filtered.remove(na)
                    break
        mn, nhn = self._getNextHopsWithMetric(me, filtered, perDest, areas)
        if not nhn:
            self._bump("decision.no_route_to_prefix")
            return None
        nhs = self._getNextHopsThrift(me, res.allNodeAreas, isV4, perDest, mn, nhn, None, areas, ents)
        return self._addBestPaths(me, prefix, res.allNodeAreas, res.bestNodeArea, ents, nhs, isBgp)

    def _selectBestPathsKsp2(self, me: str, prefix: str, res: BestRouteSelectionResult,
                             ents: Dict[Tuple[str, str], PrefixEntry], isBgp: bool, ftype: str,
                             areas: List[Tuple[str, LinkState]]) -> Optional[RibUnicastEntry]:
        """:895-1018, every area's k = 1 / k = 2 paths (a path's label stack
        and next hop are made once per area, as the reference does)."""
        if ftype != "SR_MPLS":
            self._bump("decision.incompatible_forwarding_type")
            return None
        paths = []
        for area, ls in areas:
            for node, bestArea in res.allNodeAreas:
                if node == me and bestArea == area:
                    continue
                paths.extend(ls.getKthPaths(me, node, 1))
            first = len(paths)
            for node, bestArea in res.allNodeAreas:
                if area != bestArea:
                    continue
                for sec in ls.getKthPaths(me, node, 2):
                    if not any(LinkState.pathAInPathB(paths[i], sec) for i in range(first)):
                        paths.append(sec)
        if not paths:
            return None
        isV4 = next(iter(ents.values())).isV4
        out: Set[NextHopThrift] = set()
        for path in paths:
            for area, ls in areas:
                labels = ls.getAdjacencyDatabaseLabels()
                cost, stack, nxt = 0, deque(), me
                for link in path:
                    cost += link.getMetricFromNode(nxt)
                    nxt = link.getOtherNodeName(nxt)
                    stack.appendleft(labels[nxt])
                stack.pop()  # the first hop's label: PHP
                pe = ents[(nxt, area)]
                if pe.prependLabel is not None:
                    stack.appendleft(pe.prependLabel)
                head = path[0]
                action = MplsAction("PUSH", None, tuple(stack)) if stack else None
                addr = head.getNhV4FromNode(me) if isV4 else head.getNhV6FromNode(me)
                out.add(createNextHop(addr, head.getIfaceFromNode(me), cost, action,
                                      head.getArea(), head.getOtherNodeName(me)))
        return self._addBestPaths(me, prefix, res.allNodeAreas, res.bestNodeArea, ents, out, isBgp)

    # -- buildRouteDb (Decision.cpp:557-722) ----------------------------------------
    def buildRouteDb(self, myNodeName: str, areaLinkStates: Dict[str, LinkState],
                     prefixState: PrefixState, _generic: bool = False) -> Optional[DecisionRouteDb]:
        """``_generic`` (tests): the Python restatement's several-area walk
        with one area too."""
        if self.native and not _generic:
            ndb = self.buildRouteDbNative(myNodeName, areaLinkStates, prefixState)
            if ndb is None:
                return None
            with ndb:
                return ndb.routeDb()
        self._nat_cache = None
        areas = areaOrder(areaLinkStates)
        if not any(ls.hasNode(myNodeName) for _, ls in areas):
            return None
        me = myNodeName
        db = DecisionRouteDb()
        self._bestRoutesCache = {}
        single = len(areas) == 1 and not _generic
        mine = {area: ls.getSpfResult(me) for area, ls in areas}  # memoised

        # ---- unicast: createRouteForPrefix (:390-555) ----
        uni: List[tuple] = []
        sr: List[tuple] = []
        for prefix, entries in prefixState.prefixes().items():
            if len(entries) == 1:  # one advertiser (most prefixes): the same flags, directly
                (na0, e0), = entries.items()
                if na0[1] in mine and na0[0] not in mine[na0[1]]:
                    self._bump("decision.no_route_to_prefix")
                    continue
                ents = entries
                isV4 = e0.isV4
                hasBGP = e0.type == "BGP"
                hasNonBGP = not hasBGP
                missingMv = hasBGP and e0.mv is None
                hasSelfPrepend = na0[0] != me or e0.prependLabel is not None
            else:
                # entries of nodes unreachable in their own area are dropped
                ents = {na: e for na, e in entries.items()
                        if na[1] not in mine or na[0] in mine[na[1]]}
                if not ents:
                    self._bump("decision.no_route_to_prefix")
                    continue
                isV4 = next(iter(ents.values())).isV4
                hasBGP = any(e.type == "BGP" for e in ents.values())
                hasNonBGP = any(e.type != "BGP" for e in ents.values())
                missingMv = any(e.type == "BGP" and e.mv is None for e in ents.values())
                hasSelfPrepend = all(e.prependLabel is not None
                                     for na, e in ents.items() if na[0] == me)
            if isV4 and not self.enableV4:
                self._bump("decision.skipped_unicast_route")
                continue
            if hasBGP and ((hasNonBGP and not self.enableBestRouteSelection) or missingMv):
                self._bump("decision.skipped_unicast_route")
                continue
            if ents is entries and self._single_fast and not self.enableBestRouteSelection:
                # one advertiser, no best-route selection: the openr walk and the
                # BGP walk (:791-832) both pick it, and the drained-node filter
                # (:766-789) keeps the result whether it is drained or not
                res = BestRouteSelectionResult(True, [na0], na0)
                self._bestRoutesCache[prefix] = res
                if na0[0] == me and not hasSelfPrepend:
                    continue  # self-advertised
                falgo = e0.forwardingAlgorithm
                if not single:
                    r = (self._selectBestPathsSpf if falgo == "SP_ECMP" else self._selectBestPathsKsp2)(
                        me, prefix, res, ents, hasBGP, e0.forwardingType, areas)
                    if r is not None:
                        db.addUnicastRoute(r)
                elif falgo == "SP_ECMP" and e0.forwardingType == "IP":
                    uni.append((prefix, ents, [na0[0]], res, hasBGP, isV4))
                else:
                    sr.append((prefix, ents, res, falgo, hasBGP))
                continue
            res = self._selectBestRoutes(me, ents, hasBGP, areaLinkStates)
            if not res.success:
                continue
            if not res.allNodeAreas:
                self._bump("decision.no_route_to_prefix")
                continue
            self._bestRoutesCache[prefix] = res
            if res.hasNode(me) and not hasSelfPrepend:
                continue  # self-advertised
            ftype, falgo = getPrefixForwardingTypeAndAlgorithm(ents, set(res.allNodeAreas))
            if not single:
                r = (self._selectBestPathsSpf if falgo == "SP_ECMP" else self._selectBestPathsKsp2)(
                    me, prefix, res, ents, hasBGP, ftype, areas)
                if r is not None:
                    db.addUnicastRoute(r)
            elif falgo == "SP_ECMP" and ftype == "IP":
                uni.append((prefix, ents, [na[0] for na in res.allNodeAreas], res, hasBGP, isV4))
            else:
                sr.append((prefix, ents, res, falgo, hasBGP))

        if single:
            self._buildSingleArea(me, areas[0][0], areas[0][1], db, uni, sr)
        else:
            # ---- node labels over every area (:583-664) ----
            labelToNode: Dict[int, Tuple[str, RibMplsEntry]] = {}
            for area, ls in areas:
                for node, top in ls.getAdjacencyDatabaseLabels().items():
                    if top == 0 or not isMplsLabelValid(top):
                        continue
                    cur = labelToNode.get(top)
                    if cur is not None:
                        self._bump("decision.duplicate_node_label")
                        if cur[0] < node:
                            continue
                    if node == me:
                        labelToNode[top] = (node, RibMplsEntry(top, {NextHopThrift(
                            bytes(16), None, 0, MplsAction("POP_AND_LOOKUP"), area, None)}))
                        continue
                    mn, nhn = self._getNextHopsWithMetric(me, [(node, area)], False, areas)
                    if not nhn:
                        self._bump("decision.no_route_to_label")
                        continue
                    labelToNode[top] = (node, RibMplsEntry(top, self._getNextHopsThrift(
                        me, [(node, area)], False, False, mn, nhn, top, areas, {})))
            for _, entry in labelToNode.values():
                db.addMplsRoute(entry)

        # ---- adjacency labels of every area (:667-698) ----
        for _, ls in areas:
            for link in ls.linksFromNode(me):
                top = link.getAdjLabelFromNode(me)
                if top == 0 or not isMplsLabelValid(top):
                    continue
                db.addMplsRoute(RibMplsEntry(top, {createNextHop(
                    link.getNhV6FromNode(me), link.getIfaceFromNode(me),
                    link.getMetricFromNode(me), MplsAction("PHP"), link.getArea(),
                    link.getOtherNodeName(me))}))
        # ---- static MPLS routes (:700-707) ----
        for top, nhs in self.staticMplsRoutes.items():
            db.addMplsRoute(RibMplsEntry(top, set(nhs)))
        return db

    def _buildSingleArea(self, me: str, area: str, ls: LinkState, db: DecisionRouteDb,
                         uni: List[tuple], sr: List[tuple]) -> None:
        """One area: every SP_ECMP/IP prefix and node label in ONE batched
        kernel call (spf_routes), SR_MPLS prefixes over the memoised SPF /
        one batched KSP2 launch."""
        labels = ls.getAdjacencyDatabaseLabels()
        # ---- node labels: each label's candidates in walk order (names
        # ascending), labels in first-seen order.  Every candidate gets a
        # selection set of its own (one set of all candidates would select the
        # nearest, not the smallest routed name); the collision rule of
        # Decision.cpp:605-668 is resolved below, once the counts are known
        label_to_nodes: Dict[int, List[str]] = {}
        for node, label in labels.items():
            if label == 0 or not isMplsLabelValid(label):
                continue
            label_to_nodes.setdefault(label, []).append(node)

        sets = [u[2] for u in uni] + [[n] for cands in label_to_nodes.values() for n in cands]
        sel = self._select(ls, me, sets)

        # IP routes with the same (link, metric) selection share one frozen
        # next-hop set (a fabric's destinations of one pod select alike)
        mins, cnt, edge, metric, deg = self._raw
        shared: Dict[tuple, FrozenSet[NextHopThrift]] = {}
        # the selections as bytes / lists once: per route only slices of them
        # (numpy scalar reads and slices cost ~1 us each, 10^4 routes a build)
        cnt_all = cnt.tolist()
        eb, mb = edge.tobytes(), metric.tobytes()
        dry = self.bgpDryRun
        unicast = db.unicastRoutes
        fast = self._single_fast
        for i, (prefix, ents, dsts, res, isBgp, isV4) in enumerate(uni):
            c = cnt_all[i]
            if not c:
                self._bump("decision.no_route_to_prefix")
                continue
            b = i * deg
            key = (eb[4 * b:4 * (b + c)], mb[8 * b:8 * (b + c)], isV4)
            nhs = shared.get(key)
            if nhs is None:
                nhs = frozenset(self._next_hops(ls, me, area, sel[i], isV4, set(dsts), None))
                shared[key] = nhs
            best = res.allNodeAreas
            if fast and len(best) == 1 and best[0][0] != me:  # _addBestPaths, one remote advertiser
                need = ents[best[0]].minNexthop
                if need is not None and need > len(nhs):
                    continue  # min-nexthop requirement not met
                bna = res.bestNodeArea  # (the drained filter keeps the unfiltered one)
                unicast[prefix] = RibUnicastEntry(prefix, nhs, ents[bna], bna[1], isBgp and dry)
                continue
            r = self._addBestPaths(me, prefix, best, res.bestNodeArea, ents, nhs, isBgp)
            if r is not None:
                db.addUnicastRoute(r)

        # ---- SR_MPLS prefixes: per-destination SP_ECMP or KSP2_ED_ECMP ----
        if any(falgo == "KSP2_ED_ECMP" for *_, falgo, _ in sr):
            ls.prefetchKthPaths(me)  # one batched KSP2 launch for every advertiser
        for prefix, ents, res, falgo, isBgp in sr:
            best = list(res.allNodeAreas)
            isV4 = next(iter(ents.values())).isV4
            if falgo == "KSP2_ED_ECMP":
                if any(ents[na].forwardingType != "SR_MPLS" for na in best):
                    self._bump("decision.incompatible_forwarding_type")
                    continue  # incompatible forwarding type (Decision.cpp:905-913)
                nhs = self._ksp2NextHops(ls, me, area, best, ents, isV4, labels)
            else:
                nhs = self._srSpfNextHops(ls, me, area, best, ents, isV4, labels)
            if not nhs:
                self._bump("decision.no_route_to_prefix")
                continue
            r = self._addBestPaths(me, prefix, best, res.bestNodeArea, ents, nhs, isBgp)
            if r is not None:
                db.addUnicastRoute(r)

        # (the label sets' selections straight from the kernel's arrays: one
        # tolist() each, not a _SetResult per label)
        cnt_l = cnt[len(uni):].tolist()
        first = len(uni) * deg
        edge_l = edge[first:first + len(cnt_l) * deg].tolist()
        metric_l = metric[first:first + len(cnt_l) * deg].astype(np.uint32).view(np.int32).tolist()
        # next hops of a label route inline (getNextHopsThrift with a SWAP /
        # PHP action, Decision.cpp:1198-1305): me's links' fields cached per
        # directed edge, metrics as signed i32 (the thrift field) in one pass
        info = self._link_fields(ls, me)
        mk = tuple.__new__
        mpls = db.mplsRoutes
        k0 = 0
        for label, cands in label_to_nodes.items():
            # the walk of :609-668 over this label's candidates: one installs
            # only if it is me or has next hops, a larger name than the
            # standing entry's is passed by (only the standing entry's
            # selection is read: a passed-by candidate's reaches no route)
            node, k = None, k0
            for j, cand in enumerate(cands, k0):
                if node is not None:
                    self._bump("decision.duplicate_node_label")
                    if node < cand:
                        continue
                if cand == me or cnt_l[j]:
                    node, k = cand, j
                else:
                    self._bump("decision.no_route_to_label")
            k0 += len(cands)
            if node is None:
                continue
            if node == me:
                db.addMplsRoute(RibMplsEntry(label, {NextHopThrift(
                    bytes(16), None, 0, MplsAction("POP_AND_LOOKUP"), area, None)}))
                continue
            c, b = cnt_l[k], k * deg
            if not fast:  # the generic getNextHopsThrift restatement (tests)
                db.addMplsRoute(RibMplsEntry(label, self._next_hops(
                    ls, me, area, zip(edge[first + b:first + b + c].tolist(),
                                      metric[first + b:first + b + c].tolist()), False, {node}, label)))
                continue
            swap = mk(MplsAction, ("SWAP", label, None))
            nhs = set()
            add = nhs.add
            for e, m in zip(edge_l[b:b + c], metric_l[b:b + c]):
                li = info.get(e)
                if li is None:
                    li = self._link_field(ls, me, info, e)
                nb = li[0]
                add(mk(NextHopThrift, (li[3], li[1], m, _PHP if nb == node else swap, li[4], nb)))
            mpls[label] = RibMplsEntry(label, nhs)

    def getNextHops(self, ls: LinkState, me: str, dsts: Sequence[str], isV4: bool = False,
                    swapLabel: Optional[int] = None) -> Tuple[Optional[int], Set[NextHopThrift]]:
        """(min metric, next hops) of one destination set: getNextHopsWithMetric
        + getNextHopsThrift with perDestination = false."""
        res = self._select(ls, me, [list(dsts)])[0]
        area = ls.getArea()
        return res.min_metric, self._next_hops(ls, me, area, res, isV4, set(dsts), swapLabel)

    def getNextHopsBatch(self, ls: LinkState, me: str, sets: Sequence[Sequence[str]],
                         isV4: bool = False) -> List[Tuple[Optional[int], Set[NextHopThrift]]]:
        res = self._select(ls, me, sets)
        area = ls.getArea()
        return [(r.min_metric, self._next_hops(ls, me, area, r, isV4, set(s), None))
                for r, s in zip(res, sets)]
