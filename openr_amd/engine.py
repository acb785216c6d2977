"""Batched all-sources SPF on device buffers (include/openr_spf.h).

This is the path ``SpfSolver`` takes when it needs many sources at once
(all-sources route builds, ``breeze decision routes --nodes all`` =
``Decision::getDecisionRouteDb`` per node, Decision.cpp:1480-1500; LFA's
SPF-from-every-neighbour, Decision.cpp:1158-1192).  One ``SpfPlan`` fixes the
source batch; ``execute`` enqueues the kernels on a HIP stream without host
synchronisation, so it can be timed with HIP events or captured in a graph.
"""

from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from ._native import NativeHandle, close_all  # noqa: F401



HOP_COUNT = N.SPF_FLAG_HOP_COUNT
DIST64 = N.SPF_FLAG_DIST64
UNREACHABLE = N.SPF_UNREACHABLE
UNREACHABLE64 = N.SPF_UNREACHABLE64


@dataclass
class SolveResult:
    dist: np.ndarray  # [n_src, n_nodes] uint32 (UNREACHABLE), uint64 for dist64 plans
    nh: np.ndarray  # destination bitmaps, one per (source, neighbour)
    nh_off: np.ndarray  # [n_src] uint64 word offset of each source's bitmaps
    words: np.ndarray  # [n_src] number of bitmaps (= distinct up neighbours)
    pitch: int

    def nh_matrix(self, i: int) -> np.ndarray:
        """bool [k_i, n_nodes]: row j = destinations whose next-hop set holds
        the source's j-th neighbour (ascending id)."""
        return nh_matrix(self.nh, int(self.nh_off[i]), int(self.words[i]), self.pitch,
                         self.dist.shape[1])


def nh_matrix(nh: np.ndarray, off: int, k: int, pitch: int, n: int) -> np.ndarray:
    wpm = pitch // 32
    words = nh[off: off + k * wpm].reshape(k, wpm).astype(np.uint32)
    bits = np.unpackbits(words.view(np.uint8).reshape(k, wpm * 4), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


class SpfPlan(NativeHandle):
    _destroy = "spf_plan_destroy"

    def __init__(self, eng: "SpfEngine", srcs: Sequence[int], flags: int) -> None:
        self._eng = eng
        self.srcs = np.ascontiguousarray(srcs, np.uint32)
        self.flags = flags
        h = C.c_void_p()
        eng._err(N.lib.spf_plan_create(eng._h, N.ptr(self.srcs), len(self.srcs), flags,
                                       C.byref(h)))
        self._adopt(h)
        self.nh_words = int(N.lib.spf_plan_nh_words(h))
        self.closure_rows = int(N.lib.spf_plan_closure_rows(h))
        self.nh_off = np.zeros(len(self.srcs), np.uint64)
        self.words = np.zeros(len(self.srcs), np.uint32)
        N.lib.spf_plan_nh_layout(h, N.ptr(self.nh_off, C.c_uint64), N.ptr(self.words))

    @property
    def n_src(self) -> int:
        return len(self.srcs)

    def execute(self, d_dist: int, d_nh: int, stream: int = 0) -> None:
        """Enqueue on `stream` (raw hipStream_t as int; 0 = engine stream)."""
        self._eng._err(N.lib.spf_plan_execute(self._h, C.c_void_p(d_dist), C.c_void_p(d_nh),
                                              C.c_void_p(stream) if stream else None))

    def copy_narrow_rows(self, d_out: int, stream: int = 0) -> None:
        """Enqueue a copy of the last execute's u8 rows (n_src x pitch bytes,
        254 = saturated, 255 = unreachable) to d_out (spf_plan_copy_narrow_rows)."""
        self._eng._err(N.lib.spf_plan_copy_narrow_rows(self._h, C.c_void_p(d_out),
                                                       C.c_void_p(stream) if stream else None))

    def digest(self, d_dist: int, d_nh: int, d_out: int, stream: int = 0) -> None:
        """Enqueue per-source u64 digests of an execute's output into d_out
        (n_src words, spf_plan_digest)."""
        self._eng._err(N.lib.spf_plan_digest(self._h, C.c_void_p(d_dist), C.c_void_p(d_nh),
                                             C.c_void_p(d_out),
                                             C.c_void_p(stream) if stream else None))

    def execute_host(self) -> "SolveResult":
        """Execute into host arrays (spf_plan_execute_host)."""
        n = self._eng.n_nodes
        dist = np.zeros((self.n_src, n), np.uint64 if self.flags & DIST64 else np.uint32)
        nh = np.zeros(max(1, self.nh_words), np.uint32)
        self._eng._err(N.lib.spf_plan_execute_host(self._h, N.ptr(dist), N.ptr(nh)))
        return SolveResult(dist, nh, self.nh_off, self.words, self._eng.pitch)

    BFS_KERNELS = ("sssp_kernel", "msbfs_kernel", "msbfs_planes_kernel", "exact_spf_kernel",
                   "spf_big_kernel", "mssp_kernel", "msbfs_team_kernel")
    ROW_MODES = ("u32", "u8", "sliced", "sliced_bfs")

    def kernels(self) -> Tuple[str, bool]:
        """(distance kernel name, next-hop pass reads u8 narrow rows or their
        bit-sliced form) of the next execute (spf_plan_kernels)."""
        bfs, narrow = self._kernel_codes()
        return self.BFS_KERNELS[bfs], bool(narrow)

    def _kernel_codes(self) -> Tuple[int, int]:
        bfs, narrow = C.c_uint32(), C.c_uint32()
        self._eng._err(N.lib.spf_plan_kernels(self._h, C.byref(bfs), C.byref(narrow)))
        return bfs.value, narrow.value

    def row_mode(self) -> str:
        """Rows the next-hop pass reads: "u32", "u8", "sliced" (bit planes from
        the u8 rows) or "sliced_bfs" (bit planes written by the team BFS)."""
        return self.ROW_MODES[self._kernel_codes()[1]]

    def phase_kernels(self) -> Tuple[str, Optional[str], Optional[str]]:
        """Kernel names of the execute's three timed phases (distance kernel,
        row slicing, next-hop pass); None where a phase launches nothing."""
        bfs, narrow = self._kernel_codes()
        name = self.BFS_KERNELS[bfs]
        if bfs in (3, 4) or not self.nh_words:  # exact / big kernels: next hops inside
            return name, None, None
        if narrow == 2:
            return name, "slice_rows_kernel", "ecmp_sliced_kernel"
        if narrow == 3:
            return name, None, "ecmp_sliced_kernel"
        return name, None, "ecmp_kernel"

    def traffic(self) -> Tuple[int, int]:
        """Compulsory HBM bytes of (distance kernel, next-hop pass incl. row
        slicing) per execute (spf_plan_traffic)."""
        a, b = C.c_uint64(), C.c_uint64()
        self._eng._err(N.lib.spf_plan_traffic(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def traffic_phases(self) -> Tuple[int, int, int]:
        """Compulsory bytes per phase (distance kernel, slicing, next hops)."""
        b = (C.c_uint64 * 3)()
        self._eng._err(N.lib.spf_plan_traffic_phases(self._h, b))
        return b[0], b[1], b[2]

    def enable_timing(self, max_executes: int) -> None:
        self._eng._err(N.lib.spf_plan_enable_timing(self._h, max_executes))

    def timing(self) -> Tuple[float, float, int]:
        """(summed SSSP ms, summed ECMP ms, executes) since enable/last call."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        self._eng._err(N.lib.spf_plan_timing(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def timing_phases(self) -> Tuple[Tuple[float, float, float], int]:
        """((distance, slicing, next-hop) summed ms, executes) since
        enable/last call (spf_plan_timing_phases)."""
        ms, n = (C.c_double * 3)(), C.c_uint32()
        self._eng._err(N.lib.spf_plan_timing_phases(self._h, ms, C.byref(n)))
        return (ms[0], ms[1], ms[2]), n.value

    def execute_torch(self, dist, nh, stream=None) -> None:
        """dist: int32/uint32 tensor [n_src, pitch] on the engine's device;
        nh: tensor with >= nh_words 32-bit words; stream: torch.cuda.Stream."""
        import torch

        assert dist.is_cuda and dist.numel() >= self.n_src * self._eng.pitch
        assert nh.is_cuda and nh.numel() >= max(1, self.nh_words)
        s = (stream or torch.cuda.current_stream(dist.device)).cuda_stream
        self.execute(dist.data_ptr(), nh.data_ptr(), s)


KSP2_NONE = N.SPF_KSP2_NONE
PAIR_DTYPE = np.dtype([("first", "<u4", (2,)), ("n_paths", "<u4", (2,))])  # spf_ksp2_pair


@dataclass
class Ksp2Result:
    """All-destinations KSP2 of a source batch (include/openr_spf.h)."""

    srcs: np.ndarray  # [n_src]
    n_nodes: int
    pairs: np.ndarray  # [n_src * n_nodes] PAIR_DTYPE
    pool: np.ndarray  # u32 path records [n_links, next, links...]

    def paths(self, i: int, d: int, k: int) -> List[List[int]]:
        """getKthPaths(srcs[i], d, k) for k in (1, 2): lists of link ids."""
        rec = self.pairs[i * self.n_nodes + d]
        out: List[List[int]] = []
        at = int(rec["first"][k - 1])
        for _ in range(int(rec["n_paths"][k - 1])):
            n = int(self.pool[at])
            out.append([int(x) for x in self.pool[at + 2: at + 2 + n]])
            at = int(self.pool[at + 1])
        return out


@dataclass(frozen=True)
class Ksp2PlanInfo:
    """What spf_ksp2_plan_create decided (spf_ksp2_plan_info)."""

    kind: str  # "EXACT", "HBM", "LDS_U32" or "LDS_U16"
    waves: int  # per workgroup of the pair kernel (0 on EXACT plans, as all below)
    redo_waves: int  # per workgroup of the redo pass (LDS_U16 only)
    chunk: int  # sources per workgroup
    delta: int  # bucket width of the k = 2 SPF
    grab: int  # pool words a wave reserves at a time
    lds_bytes: int  # dynamic LDS of the pair kernel


class Ksp2Plan(NativeHandle):
    """A fixed source batch for batched KSP2 (``spf_ksp2_plan``)."""

    _destroy = "spf_ksp2_plan_destroy"

    def __init__(self, eng: "SpfEngine", srcs: Sequence[int]) -> None:
        self._eng = eng
        self.srcs = np.ascontiguousarray(srcs, np.uint32)
        h = C.c_void_p()
        eng._err(N.lib.spf_ksp2_plan_create(eng._h, N.ptr(self.srcs), len(self.srcs), C.byref(h)))
        self._adopt(h)

    def execute(self, d_pairs: int, d_pool: int, pool_words: int, d_counters: int,
                stream: int = 0) -> None:
        self._eng._err(N.lib.spf_ksp2_execute(self._h, C.c_void_p(d_pairs), C.c_void_p(d_pool),
                                              pool_words, C.c_void_p(d_counters),
                                              C.c_void_p(stream) if stream else None))

    def digest(self, d_pairs: int, d_pool: int, d_link_hash: int, d_out: int,
               stream: int = 0) -> None:
        """Enqueue per-source u64 digests of an execute's pairs and pool into
        d_out (spf_ksp2_digest; d_link_hash: u64 value hash per link id)."""
        self._eng._err(N.lib.spf_ksp2_digest(self._h, C.c_void_p(d_pairs), C.c_void_p(d_pool),
                                             C.c_void_p(d_link_hash), C.c_void_p(d_out),
                                             C.c_void_p(stream) if stream else None))

    def chunk(self) -> int:
        """Sources per KSP2 workgroup (spf_ksp2_plan_chunk)."""
        return int(N.lib.spf_ksp2_plan_chunk(self._h))

    def info(self) -> Ksp2PlanInfo:
        """The kernel the plan's executes launch and its launch parameters."""
        x = N.SpfKsp2PlanInfo()
        self._eng._err(N.lib.spf_ksp2_plan_info(self._h, C.byref(x)))
        return Ksp2PlanInfo(N.KSP2_KIND_NAMES[x.kind], x.waves, x.redo_waves, x.chunk, x.delta,
                            x.grab, x.lds_bytes)

    def enable_timing(self, max_executes: int) -> None:
        self._eng._err(N.lib.spf_ksp2_enable_timing(self._h, max_executes))

    def timing(self) -> Tuple[float, float, int]:
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        self._eng._err(N.lib.spf_ksp2_timing(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    # ---- KSP2_ED_ECMP routes of every source (spf_ksp2_routes) ---------------------
    def routes(self, d_pairs: int, d_pool: int, set_ptr, set_nodes, node_label,
               set_prepend=None) -> Tuple[int, int, int, float]:
        """selectBestPathsKsp2's next hops of every source of the plan towards
        every set ``set_nodes[set_ptr[p]:set_ptr[p + 1]]``, built on the GPU
        from an execute's device pairs and pool (no overflow) into exactly
        sized device pools.  node_label: i32 per node (0 = none); set_prepend:
        i32 parallel to set_nodes (-1 = none).  Returns (next hops, label
        words, pool bytes, kernel ms of count + scan + fill)."""
        sp = np.ascontiguousarray(set_ptr, np.uint32)
        sn = np.ascontiguousarray(set_nodes, np.uint32)
        lab = np.ascontiguousarray(node_label, np.int32)
        pre = None if set_prepend is None else np.ascontiguousarray(set_prepend, np.int32)
        if len(sp) < 1 or len(sn) < int(sp.max()):
            raise ValueError("set_ptr / set_nodes length mismatch")
        if pre is not None and len(pre) != len(sn):
            raise ValueError("set_prepend must be parallel to set_nodes")
        if len(lab) < self._eng.n_nodes:
            raise ValueError("node_label needs one entry per node")
        pad = np.zeros(1, np.uint32)
        hops, words, nbytes, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        self._rt_sets = None
        self._eng._err(N.lib.spf_ksp2_routes(
            self._h, C.c_void_p(d_pairs), C.c_void_p(d_pool), N.ptr(sp), N.ptr(sn if len(sn) else pad),
            len(sp) - 1, None if pre is None else N.ptr(pre if len(pre) else pad.view(np.int32), C.c_int32),
            N.ptr(lab, C.c_int32), C.byref(hops), C.byref(words), C.byref(nbytes), C.byref(ms)))
        self._rt_sets = len(sp) - 1
        return hops.value, words.value, nbytes.value, ms.value

    def routes_timing(self) -> Tuple[float, float, float]:
        """(count, scan, fill) ms of the last routes() (spf_ksp2_routes_timing)."""
        ms = (C.c_double * 3)()
        self._eng._err(N.lib.spf_ksp2_routes_timing(self._h, ms))
        return ms[0], ms[1], ms[2]

    def route_db(self, i: int):
        """Source slot i's share of the last routes(), rebased to 0: (rptr u64
        [n_sets + 1], rec u64 = CSR edge | cost << 32, lptr u64 [len(rec) + 1],
        lab i32): route p's next hops are rec[rptr[p]:rptr[p + 1]], next hop
        h's label stack is lab[lptr[h]:lptr[h + 1]] (spf_ksp2_route_db)."""
        n_rec, n_lab = C.c_uint64(), C.c_uint64()
        sets = getattr(self, "_rt_sets", None) or 0
        rptr = np.zeros(sets + 1, np.uint64)
        self._eng._err(N.lib.spf_ksp2_route_db(self._h, int(i), N.ptr(rptr, C.c_uint64), None, 0,
                                               C.byref(n_rec), None, None, 0, C.byref(n_lab)))
        rec = np.zeros(max(1, n_rec.value), np.uint64)
        lptr = np.zeros(n_rec.value + 1, np.uint64)
        lab = np.zeros(max(1, n_lab.value), np.int32)
        self._eng._err(N.lib.spf_ksp2_route_db(self._h, int(i), None, N.ptr(rec, C.c_uint64),
                                               n_rec.value, None, N.ptr(lptr, C.c_uint64),
                                               N.ptr(lab, C.c_int32), n_lab.value, None))
        return rptr, rec[: n_rec.value], lptr, lab[: n_lab.value]

    def route_buffers(self) -> Tuple[int, int, int, int, int, int]:
        """Device addresses (rptr, rec, lptr, lab) of the last routes() and its
        (next hops, label words), for device-side consumers
        (spf_ksp2_route_buffers)."""
        p = [C.c_void_p() for _ in range(4)]
        hops, words = C.c_uint64(), C.c_uint64()
        self._eng._err(N.lib.spf_ksp2_route_buffers(self._h, *[C.byref(x) for x in p],
                                                    C.byref(hops), C.byref(words)))
        return tuple(int(x.value or 0) for x in p) + (hops.value, words.value)

    # ---- snapshot, delta and update payload of the routes (ksp2_route_delta.hip) ----
    def route_snapshot(self, link_hash) -> "Ksp2RouteSnapshot":
        """The routes of the last routes() kept as the old generation of a
        later route_delta (spf_ksp2_route_snapshot): the device pools move into
        the snapshot, nothing is copied, and the plan holds no routes until the
        next routes().  link_hash: u64 per link id, the link's identity by
        value (LinkState.linkValueHashes())."""
        lh = np.ascontiguousarray(link_hash, np.uint64)
        h = C.c_void_p()
        self._eng._err(N.lib.spf_ksp2_route_snapshot(self._h, N.ptr(lh, C.c_uint64), len(lh), C.byref(h)))
        self._rt_sets = None
        return self._eng._track(Ksp2RouteSnapshot(self._eng, h, self.srcs.copy()))

    def route_delta(self, snap: "Ksp2RouteSnapshot", link_hash):
        """The routes of the last routes() against `snap`
        (spf_ksp2_route_delta): (dptr u64 [n_src + 1], dset u32 -- source slot
        i's entries are dset[dptr[i]:dptr[i + 1]], the set index |
        SPF_DELTA_DELETE on a delete, ascending --, totals [updates, deletes,
        routes matched as sets], kernel ms)."""
        lh = np.ascontiguousarray(link_hash, np.uint64)
        tot, ms = np.zeros(3, np.uint64), C.c_double()
        self._eng._err(N.lib.spf_ksp2_route_delta(self._h, snap._h, N.ptr(lh, C.c_uint64), len(lh),
                                                  N.ptr(tot, C.c_uint64), C.byref(ms)))
        from .hiprt import read_device

        d_dptr, d_dset, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._eng._err(N.lib.spf_ksp2_route_delta_buffers(self._h, C.byref(d_dptr), C.byref(d_dset),
                                                          C.byref(n)))
        # (the call has waited for the context's stream)
        dptr = read_device(int(d_dptr.value), len(self.srcs) + 1, np.uint64)
        dset = read_device(int(d_dset.value), n.value, np.uint32)
        return dptr, dset, [int(v) for v in tot], ms.value

    def route_delta_db(self, i: int) -> np.ndarray:
        """Source slot i's entries of the last route_delta (spf_ksp2_route_delta_db)."""
        n = C.c_uint64()
        self._eng._err(N.lib.spf_ksp2_route_delta_db(self._h, int(i), None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), np.uint32)
        self._eng._err(N.lib.spf_ksp2_route_delta_db(self._h, int(i), N.ptr(out), n.value, None))
        return out[: n.value]

    def route_delta_timing(self) -> Tuple[float, ...]:
        """(count, scan, fill) ms of the last route_delta, then of its
        route_update (spf_ksp2_route_delta_timing)."""
        ms = (C.c_double * 6)()
        self._eng._err(N.lib.spf_ksp2_route_delta_timing(self._h, ms))
        return tuple(ms)

    def route_update(self):
        """The payload of the last route_delta gathered on the GPU
        (spf_ksp2_route_update) and read back in one copy per array: (dptr,
        dset, uptr u64 [entries + 1], urec u64, ulptr u64 [records + 1], ulab
        i32, totals [update entries, records, label words], pool bytes, kernel
        ms): entry j's records are urec[uptr[j]:uptr[j + 1]] (a delete owns
        none), record k's label stack is ulab[ulptr[k]:ulptr[k + 1]]."""
        tot, nbytes, ms = np.zeros(3, np.uint64), C.c_uint64(), C.c_double()
        self._eng._err(N.lib.spf_ksp2_route_update(self._h, N.ptr(tot, C.c_uint64), C.byref(nbytes),
                                                   C.byref(ms)))
        n = np.zeros(4, np.uint64)
        self._eng._err(N.lib.spf_ksp2_route_update_read(self._h, N.ptr(n, C.c_uint64), *([None] * 6)))
        ns, ne, nr, nw = (int(v) for v in n)
        dptr, dset = np.zeros(ns + 1, np.uint64), np.zeros(max(1, ne), np.uint32)
        uptr, urec = np.zeros(ne + 1, np.uint64), np.zeros(max(1, nr), np.uint64)
        ulptr, ulab = np.zeros(nr + 1, np.uint64), np.zeros(max(1, nw), np.int32)
        self._eng._err(N.lib.spf_ksp2_route_update_read(
            self._h, None, N.ptr(dptr, C.c_uint64), N.ptr(dset), N.ptr(uptr, C.c_uint64),
            N.ptr(urec, C.c_uint64), N.ptr(ulptr, C.c_uint64), N.ptr(ulab, C.c_int32)))
        return (dptr, dset[:ne], uptr, urec[:nr], ulptr, ulab[:nw], [int(v) for v in tot],
                int(nbytes.value), ms.value)

    def route_update_db(self, i: int):
        """Source slot i's payload of the last route_update, rebased to 0 and
        parallel to route_delta_db(i): (uptr, urec, ulptr, ulab)
        (spf_ksp2_route_update_db)."""
        m = len(self.route_delta_db(i))
        n_rec, n_lab = C.c_uint64(), C.c_uint64()
        uptr = np.zeros(m + 1, np.uint64)
        self._eng._err(N.lib.spf_ksp2_route_update_db(self._h, int(i), N.ptr(uptr, C.c_uint64), None, 0,
                                                      C.byref(n_rec), None, None, 0, C.byref(n_lab)))
        urec = np.zeros(max(1, n_rec.value), np.uint64)
        ulptr = np.zeros(n_rec.value + 1, np.uint64)
        ulab = np.zeros(max(1, n_lab.value), np.int32)
        self._eng._err(N.lib.spf_ksp2_route_update_db(self._h, int(i), None, N.ptr(urec, C.c_uint64),
                                                      n_rec.value, None, N.ptr(ulptr, C.c_uint64),
                                                      N.ptr(ulab, C.c_int32), n_lab.value, None))
        return uptr, urec[: n_rec.value], ulptr, ulab[: n_lab.value]

    def route_update_buffers(self) -> Tuple[int, int, int, int, int, int]:
        """Device addresses (uptr, urec, ulptr, ulab) of the last route_update
        and its (records, label words) (spf_ksp2_route_update_buffers)."""
        p = [C.c_void_p() for _ in range(4)]
        nr, nw = C.c_uint64(), C.c_uint64()
        self._eng._err(N.lib.spf_ksp2_route_update_buffers(self._h, *[C.byref(x) for x in p],
                                                           C.byref(nr), C.byref(nw)))
        return tuple(int(x.value or 0) for x in p) + (nr.value, nw.value)


class Ksp2RouteSnapshot(NativeHandle):
    """One generation of KSP2 routes moved out of its plan
    (``spf_ksp2_snapshot``, from Ksp2Plan.route_snapshot): owned by the engine
    context, it outlives the plan, row patches and reloads; ``close()`` (or
    the engine's) releases its device pools."""

    _destroy = "spf_ksp2_route_snapshot_destroy"

    def __init__(self, eng: "SpfEngine", h: C.c_void_p, srcs: np.ndarray) -> None:
        self._eng = eng
        self.srcs = srcs
        self._adopt(h)

    def bytes(self) -> int:
        return int(N.lib.spf_ksp2_route_snapshot_bytes(self._h))


class Ksp2Routes:
    """Every source's KSP2_ED_ECMP next hops (SpfEngine.ksp2_routes): the plan
    that holds the device pools, the path buffers they were built from and the
    totals.  ``close()`` releases them."""

    def __init__(self, plan: Ksp2Plan, bufs, totals: Tuple[int, int, int, float]) -> None:
        self.plan = plan
        self.srcs = plan.srcs
        self._bufs = bufs
        self.hops, self.label_words, self.pool_bytes, self.kernel_ms = totals
        self._dbs: dict = {}

    def db(self, i: int):
        hit = self._dbs.get(int(i))
        if hit is None:
            hit = self._dbs[int(i)] = self.plan.route_db(int(i))
        return hit

    def nexthops(self, i: int, p: int) -> List[Tuple[int, int, Tuple[int, ...]]]:
        """Route (srcs[i], set p): [(CSR edge, cost, label stack in labelVec
        order)] in candidate order, first occurrences kept."""
        rptr, rec, lptr, lab = self.db(i)
        out = []
        for h in range(int(rptr[p]), int(rptr[p + 1])):
            r = int(rec[h])
            out.append((r & 0xFFFFFFFF, r >> 32,
                        tuple(int(x) for x in lab[int(lptr[h]): int(lptr[h + 1])])))
        return out

    def snapshot(self, link_hash) -> "Ksp2RouteSnapshot":
        """These routes kept as the old generation of a later delta
        (Ksp2Plan.route_snapshot): the pools move into the snapshot and db() /
        nexthops() of this object raise SPF_E_STATE from then on."""
        self._dbs = {}
        return self.plan.route_snapshot(link_hash)

    def delta(self, snap: "Ksp2RouteSnapshot", link_hash, update: bool = True):
        """These routes (new) against `snap` (old): per source slot a tuple
        (updated sets, deleted sets, {updated set: [(CSR edge, cost, label
        stack)]}) -- ascending int lists; the dict is empty with update=False
        --, the delta's totals [updates, deletes, routes matched as sets], and
        a dict of figures (kernel ms of both calls, phase ms, pool bytes, the
        update's totals)."""
        D, M = N.SPF_DELTA_DELETE, N.SPF_DELTA_DELETE - 1
        dptr, dset, totals, ms = self.plan.route_delta(snap, link_hash)
        info = {"delta_ms": ms}
        payload = None
        if update:
            dptr, dset, uptr, urec, ulptr, ulab, utot, nbytes, ums = self.plan.route_update()
            info.update(update_ms=ums, pool_bytes=nbytes, update_totals=utot)
            payload = (uptr.tolist(), urec.tolist(), ulptr.tolist(), ulab.tolist())
        info["phase_ms"] = list(self.plan.route_delta_timing())
        out = []
        ent = dset.tolist()
        at = dptr.tolist()
        for i in range(len(self.srcs)):
            up, dele, pay = [], [], {}
            for j in range(int(at[i]), int(at[i + 1])):
                v = ent[j]
                if v & D:
                    dele.append(v & M)
                    continue
                up.append(v)
                if payload is not None:
                    uptr, urec, ulptr, ulab = payload
                    pay[v] = [(urec[k] & 0xFFFFFFFF, urec[k] >> 32, tuple(ulab[ulptr[k]: ulptr[k + 1]]))
                              for k in range(uptr[j], uptr[j + 1])]
            out.append((up, dele, pay))
        return out, totals, info

    def close(self) -> None:
        self.plan.close()
        for b in self._bufs:
            b.free()
        self._bufs = ()

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()


DIGEST_DTYPE =np.dtype([("n_dist_changed", "<u4"), ("n_nh_changed", "<u4"),
                         ("hash", "<u8")])  # spf_whatif_digest
IMPACT_DTYPE = np.dtype([("n_changed", "<u4"), ("n_unreachable", "<u4"), ("n_metric", "<u4"),
                         ("min_width", "<u4"), ("max_metric", "<u8"), ("max_fail", "<u4"),
                         ("reserved", "<u4")])  # spf_whatif_impact
WHATIF_NONE = 0xFFFFFFFF  # SPF_WHATIF_NONE


WHATIF_KINDS = {"link": 0, "down": N.SPF_WHATIF_NODE_DOWN, "drain": N.SPF_WHATIF_NODE_DRAIN,
                "sets": N.SPF_WHATIF_LINK_SET, "metric": N.SPF_WHATIF_LINK_METRIC}


def _flat_sets(sets) -> Tuple[np.ndarray, np.ndarray]:
    """A sequence of sequences, or a 2-D array with one row per set, as
    (ptr[n + 1], members[ptr[n]]) u32 arrays."""
    if isinstance(sets, np.ndarray) and sets.ndim == 2:  # equal sizes: one row per set
        ptr = (np.arange(len(sets) + 1, dtype=np.uint64) * sets.shape[1]).astype(np.uint32)
        return ptr, np.ascontiguousarray(sets, np.uint32).reshape(-1)
    members = [np.ascontiguousarray(s, np.uint32).reshape(-1) for s in sets]
    ptr = np.zeros(len(members) + 1, np.uint32)
    ptr[1:] = np.cumsum([len(m) for m in members])
    flat = np.concatenate(members) if members else np.zeros(0, np.uint32)
    return ptr, np.ascontiguousarray(flat, np.uint32)


def _pool_read(err, read, h, n_owners: int, n_entries: int, last: np.ndarray):
    """A list pool's ``_read`` call: (ptr[n_owners + 1] u64, key[n_entries] u32,
    val[n_entries] u64) and `last`, the call's fourth array (the rows, or the
    impact summaries), filled in place."""
    ptr = np.zeros(n_owners + 1, np.uint64)
    key, val = np.zeros(n_entries, np.uint32), np.zeros(n_entries, np.uint64)
    err(read(h, N.ptr(ptr, C.c_uint64), N.ptr(key), N.ptr(val, C.c_uint64), N.ptr(last)))
    return ptr, key, val, last


def _pool_of(err, db, h, i: int, W: Optional[int] = None):
    """A list pool's ``_db`` call for owner i, asking for the size first:
    (key[n] u32, val[n] u64) and, for a pool with rows, rows[n, W]."""
    n = C.c_uint64()
    err(db(h, i, *([None] * (2 if W is None else 3)), 0, C.byref(n)))
    m = int(n.value)
    out = [np.zeros(m, np.uint32), np.zeros(m, np.uint64)]
    out += [] if W is None else [np.zeros((m, W), np.uint32)]
    if m:
        err(db(h, i, N.ptr(out[0]), N.ptr(out[1], C.c_uint64), *[N.ptr(x) for x in out[2:]], m,
               C.byref(n)))
    return tuple(out)


class WhatIfPlan(NativeHandle):
    """One source and a list of failures (``spf_whatif_plan``): single links
    (``kind == "link"``, ``links``), or nodes down / drained (``"down"`` /
    ``"drain"``, ``nodes``; ``links`` is then empty, as ``nodes`` is for a
    link plan), or sets of links failing together (``"sets"``: `links` is a
    sequence of sequences of link ids; ``set_ptr`` / ``set_links`` / ``sets``
    hold them as the plan does, each ascending without duplicates, and
    ``links`` and ``nodes`` are empty), or link metric changes (``"metric"``:
    `links` is a sequence of ``(link, m_lo, m_hi)`` triples, 0 keeping a
    direction's metric; ``metric_changes`` holds them as an ``[n, 3]`` array and
    ``links`` their link ids, in the order given)."""

    _destroy = "spf_whatif_plan_destroy"

    def __init__(self, eng: "SpfEngine", src: int, links: Optional[Sequence[int]],
                 kind: str = "link") -> None:
        if kind not in WHATIF_KINDS:
            raise ValueError(f"what-if kind {kind!r}: one of {sorted(WHATIF_KINDS)}")
        self._eng = eng
        self.kind = kind
        h = C.c_void_p()
        none = np.zeros(0, np.uint32)
        self.set_ptr, self.set_links, self.sets = np.zeros(1, np.uint32), none, []
        self.metric_changes = np.zeros((0, 3), np.uint32)
        if kind == "sets":
            self._init_sets(eng, src, links)
            return
        if kind == "metric":
            self._init_metrics(eng, src, links)
            return
        arr = None if links is None else np.ascontiguousarray(links, np.uint32)
        a, n = (None if arr is None else N.ptr(arr)), (0 if arr is None else len(arr))
        if kind == "link":
            eng._err(N.lib.spf_whatif_plan_create(eng._h, src, a, n, C.byref(h)))
        else:
            eng._err(N.lib.spf_whatif_plan_create_nodes(eng._h, src, WHATIF_KINDS[kind], a, n,
                                                        C.byref(h)))
        self._adopt(h)
        self.n_fail = int(N.lib.spf_whatif_plan_failures(h))
        ids = np.zeros(max(1, self.n_fail), np.uint32)
        read = N.lib.spf_whatif_plan_links if kind == "link" else N.lib.spf_whatif_plan_nodes
        eng._err(read(h, N.ptr(ids)))
        self.links = ids[: self.n_fail] if kind == "link" else none
        self.nodes = none if kind == "link" else ids[: self.n_fail]

    def _init_sets(self, eng: "SpfEngine", src: int, sets) -> None:
        if sets is None:
            raise ValueError("a set plan needs its sets")
        ptr, flat = _flat_sets(sets)
        h = C.c_void_p()
        eng._err(N.lib.spf_whatif_plan_create_sets(eng._h, src, N.ptr(ptr),
                                                   N.ptr(flat) if len(flat) else None,
                                                   len(ptr) - 1, C.byref(h)))
        self._adopt(h)
        self.n_fail = int(N.lib.spf_whatif_plan_failures(h))
        self.links = self.nodes = np.zeros(0, np.uint32)
        self.set_ptr = np.zeros(self.n_fail + 1, np.uint32)
        eng._err(N.lib.spf_whatif_plan_sets(h, N.ptr(self.set_ptr), None))
        self.set_links = np.zeros(int(self.set_ptr[-1]), np.uint32)
        if len(self.set_links):
            eng._err(N.lib.spf_whatif_plan_sets(h, N.ptr(self.set_ptr), N.ptr(self.set_links)))
        self.sets = [self.set_links[int(a): int(b)]
                     for a, b in zip(self.set_ptr[:-1], self.set_ptr[1:])]

    def _init_metrics(self, eng: "SpfEngine", src: int, changes) -> None:
        if changes is None:
            raise ValueError("a metric plan needs its (link, m_lo, m_hi) changes")
        given = np.ascontiguousarray(changes, np.uint32).reshape(-1, 3)
        cols = [np.ascontiguousarray(given[:, k]) for k in range(3)]
        h = C.c_void_p()
        args = [N.ptr(c) if len(given) else None for c in cols]
        eng._err(N.lib.spf_whatif_plan_create_metrics(eng._h, src, *args, len(given), C.byref(h)))
        self._adopt(h)
        self.n_fail = int(N.lib.spf_whatif_plan_failures(h))
        self.nodes = np.zeros(0, np.uint32)
        held = [np.zeros(max(1, self.n_fail), np.uint32) for _ in range(3)]
        eng._err(N.lib.spf_whatif_plan_metrics(h, *[N.ptr(x) for x in held]))
        self.metric_changes = np.stack([x[: self.n_fail] for x in held], axis=1)
        self.links = self.metric_changes[:, 0].copy()

    def execute(self, d_out: int, d_base: int = 0, stream: int = 0) -> None:
        self._eng._err(N.lib.spf_whatif_execute(self._h, C.c_void_p(d_out),
                                                C.c_void_p(d_base) if d_base else None,
                                                C.c_void_p(stream) if stream else None))

    def stats(self) -> Tuple[int, int]:
        a, b = C.c_uint32(), C.c_uint32()
        self._eng._err(N.lib.spf_whatif_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def enable_timing(self, max_executes: int) -> None:
        self._eng._err(N.lib.spf_whatif_enable_timing(self._h, max_executes))

    def timing(self) -> Tuple[float, float, int]:
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        self._eng._err(N.lib.spf_whatif_timing(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def changes(self, stream: int = 0) -> "WhatIfChanges":
        """Every failure's change list (``spf_whatif_changes``), read back."""
        return WhatIfChanges(self, stream)

    def base(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """The unfailed result the lists patch: (dist[N] u64, nh[N, W], W)."""
        w = C.c_uint32()
        self._eng._err(N.lib.spf_whatif_base(self._h, None, None, C.byref(w)))
        n = self._eng.n_nodes
        dist = np.zeros(n, np.uint64)
        nh = np.zeros((n, w.value), np.uint32)
        self._eng._err(N.lib.spf_whatif_base(self._h, N.ptr(dist, C.c_uint64), N.ptr(nh), None))
        return dist, nh, int(w.value)


class WhatIfChanges:
    """The change lists of one ``spf_whatif_changes`` call on the host:
    failure i owns entries ``ptr[i] .. ptr[i + 1]`` of ``node`` / ``dist``
    (``SPF_UNREACHABLE64``: now unreachable) / ``nh[:, W]`` in device order;
    ``of(i)`` returns them ascending by node.  The device arrays stay with
    the plan until its next ``changes()``; ``close()`` closes the plan when
    this object owns it (``SpfEngine.whatif_changes``)."""

    def __init__(self, plan: WhatIfPlan, stream: int = 0, own_plan: bool = False) -> None:
        from .hiprt import DeviceArray, set_device

        self.plan, self._own = plan, own_plan
        eng = plan._eng
        set_device(eng.device)
        self.n_fail = plan.n_fail
        d_out = DeviceArray(max(1, self.n_fail), DIGEST_DTYPE)
        d_base = DeviceArray(1, DIGEST_DTYPE)
        try:
            n, nbytes, ms = C.c_uint64(), C.c_uint64(), C.c_double()
            eng._err(N.lib.spf_whatif_changes(plan._h, C.c_void_p(d_out.ptr), C.c_void_p(d_base.ptr),
                                              C.byref(n), C.byref(nbytes), C.byref(ms),
                                              C.c_void_p(stream) if stream else None))
            self.digests = d_out.numpy()[: self.n_fail]
            self.base_digest = d_base.numpy()[0]
        finally:
            d_out.free()
            d_base.free()
        self.n_entries, self.pool_bytes, self.kernel_ms = int(n.value), int(nbytes.value), ms.value
        w = C.c_uint32()
        eng._err(N.lib.spf_whatif_changes_buffers(plan._h, None, None, None, None, C.byref(w), None))
        self.W = int(w.value)
        self.ptr, self.node, self.dist, self.nh = _pool_read(
            eng._err, N.lib.spf_whatif_changes_read, plan._h, self.n_fail, self.n_entries,
            np.zeros((self.n_entries, self.W), np.uint32))

    def timing(self) -> Tuple[float, float, float]:
        """(count, scan, fill) ms of the call."""
        ms = (C.c_double * 3)()
        self.plan._eng._err(N.lib.spf_whatif_changes_timing(self.plan._h, ms))
        return ms[0], ms[1], ms[2]

    def of(self, i: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Failure i's (node[n], dist[n], nh[n, W]), ascending by node."""
        return _pool_of(self.plan._eng._err, N.lib.spf_whatif_changes_db, self.plan._h, i, self.W)

    def routes(self, sets, stream: int = 0) -> "WhatIfRoutes":
        """Every failure's changed routes over the destination sets `sets`
        (``spf_whatif_routes``): a sequence of sequences of node ids, or a
        2-D array with one row per set."""
        return WhatIfRoutes(self, sets, stream)

    def by_node(self, stream: int = 0) -> "WhatIfImpact":
        """These lists by destination node (``spf_whatif_by_node``): per node
        the failures that list it and its summary."""
        return WhatIfImpact(self.plan, "node", stream)

    def close(self) -> None:
        if self._own:
            self.plan.close()
            self._own = False

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()


class WhatIfRoutes:
    """The route lists of one ``spf_whatif_routes`` call on the host: failure
    i owns entries ``ptr[i] .. ptr[i + 1]`` of ``set`` / ``min_metric``
    (``SPF_UNREACHABLE64``: withdrawn) / ``nh[:, W]`` in device order;
    ``of(i)`` returns them ascending by set id.  ``base_metric[n_sets]`` /
    ``base_nh[n_sets, W]`` are the sets' routes on the unfailed graph.  The
    device arrays stay with the plan until its next ``routes()`` or
    ``changes()``."""

    def __init__(self, changes: WhatIfChanges, sets, stream: int = 0) -> None:
        self.changes, self.plan = changes, changes.plan
        eng, h = self.plan._eng, self.plan._h
        self.set_ptr, self.set_nodes = _flat_sets(sets)
        self.n_sets, self.n_fail, self.W = len(self.set_ptr) - 1, changes.n_fail, changes.W
        n, nbytes, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        eng._err(N.lib.spf_whatif_routes(h, N.ptr(self.set_ptr),
                                         N.ptr(self.set_nodes) if len(self.set_nodes) else None,
                                         self.n_sets, C.byref(n), C.byref(nbytes), C.byref(ms),
                                         C.c_void_p(stream) if stream else None))
        self.n_entries, self.pool_bytes, self.kernel_ms = int(n.value), int(nbytes.value), ms.value
        self.ptr, self.set, self.min_metric, self.nh = _pool_read(
            eng._err, N.lib.spf_whatif_routes_read, h, self.n_fail, self.n_entries,
            np.zeros((self.n_entries, self.W), np.uint32))
        self.base_metric = np.zeros(self.n_sets, np.uint64)
        self.base_nh = np.zeros((self.n_sets, self.W), np.uint32)
        eng._err(N.lib.spf_whatif_routes_base(h, N.ptr(self.base_metric, C.c_uint64),
                                              N.ptr(self.base_nh)))

    def timing(self) -> Tuple[float, float, float, float]:
        """(base routes + table, count, scan, fill) ms of the call."""
        ms = (C.c_double * 4)()
        self.plan._eng._err(N.lib.spf_whatif_routes_timing(self.plan._h, ms))
        return ms[0], ms[1], ms[2], ms[3]

    def of(self, i: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Failure i's (set[n], min_metric[n], nh[n, W]), ascending by set id."""
        return _pool_of(self.plan._eng._err, N.lib.spf_whatif_routes_db, self.plan._h, i, self.W)

    def by_set(self, stream: int = 0) -> "WhatIfImpact":
        """These lists by destination set (``spf_whatif_by_set``): per set the
        failures that list it and its summary."""
        return WhatIfImpact(self.plan, "set", stream)

    def update(self, stream: int = 0) -> "WhatIfRouteUpdate":
        """Every failure's sets whose link-level next hops change, with their
        records (``spf_whatif_route_update``)."""
        return WhatIfRouteUpdate(self, stream)


class WhatIfRouteUpdate:
    """The update lists of one ``spf_whatif_route_update`` call on the host:
    failure i owns entries ``ptr[i] .. ptr[i + 1]`` of ``set`` / ``min_metric``
    (``SPF_UNREACHABLE64``: withdrawn), entry e the records ``rec_ptr[e] ..
    rec_ptr[e + 1]`` of ``rec`` (``edge | min_metric << 32``, the records of
    ``spf_routes``, in the source's link order), all in device order;
    ``of(i)`` returns a failure's entries ascending by set id.  The device
    arrays stay with the plan until its next ``update()``, ``routes()`` or
    ``changes()``, after which the calls here raise."""

    def __init__(self, routes: WhatIfRoutes, stream: int = 0) -> None:
        self.routes, self.plan = routes, routes.plan
        eng, h = self.plan._eng, self.plan._h
        self.n_fail, self.n_sets = routes.n_fail, routes.n_sets
        n, nrec, nbytes, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        eng._err(N.lib.spf_whatif_route_update(h, C.byref(n), C.byref(nrec), C.byref(nbytes),
                                               C.byref(ms), C.c_void_p(stream) if stream else None))
        self.n_entries, self.n_records = int(n.value), int(nrec.value)
        self.pool_bytes, self.kernel_ms = int(nbytes.value), ms.value
        k, b = C.c_uint32(), C.c_uint64()
        eng._err(N.lib.spf_whatif_route_update_stats(h, C.byref(k), C.byref(b)))
        self.n_touched, self.base_records = int(k.value), int(b.value)
        self.ptr = np.zeros(self.n_fail + 1, np.uint64)
        self.set = np.zeros(self.n_entries, np.uint32)
        self.min_metric = np.zeros(self.n_entries, np.uint64)
        self.rec_ptr = np.zeros(self.n_entries + 1, np.uint64)
        self.rec = np.zeros(self.n_records, np.uint64)
        eng._err(N.lib.spf_whatif_route_update_read(
            h, N.ptr(self.ptr, C.c_uint64), N.ptr(self.set), N.ptr(self.min_metric, C.c_uint64),
            N.ptr(self.rec_ptr, C.c_uint64), N.ptr(self.rec, C.c_uint64)))

    def timing(self) -> Tuple[float, ...]:
        """(base records, touch, count, scan, fill, record scan, records) ms."""
        ms = (C.c_double * 7)()
        self.plan._eng._err(N.lib.spf_whatif_route_update_timing(self.plan._h, ms))
        return tuple(ms)

    def of(self, i: int) -> Tuple[np.ndarray, np.ndarray, List[np.ndarray]]:
        """Failure i's (set[n], min_metric[n], [records of each entry]),
        ascending by set id."""
        err, h = self.plan._eng._err, self.plan._h
        n, nrec = C.c_uint64(), C.c_uint64()
        err(N.lib.spf_whatif_route_update_db(h, i, None, None, None, None, 0, 0, C.byref(n),
                                             C.byref(nrec)))
        m, r = int(n.value), int(nrec.value)
        ids, met = np.zeros(m, np.uint32), np.zeros(m, np.uint64)
        rp, rec = np.zeros(m + 1, np.uint64), np.zeros(r, np.uint64)
        if m:
            err(N.lib.spf_whatif_route_update_db(h, i, N.ptr(ids), N.ptr(met, C.c_uint64),
                                                 N.ptr(rp, C.c_uint64), N.ptr(rec, C.c_uint64), m, r,
                                                 C.byref(n), C.byref(nrec)))
        return ids, met, [rec[int(a): int(b)] for a, b in zip(rp[:-1], rp[1:])]

    def base(self) -> List[np.ndarray]:
        """Every set's records on the unfailed graph."""
        rp = np.zeros(self.n_sets + 1, np.uint64)
        rec = np.zeros(self.base_records, np.uint64)
        self.plan._eng._err(N.lib.spf_whatif_route_update_base(
            self.plan._h, N.ptr(rp, C.c_uint64), N.ptr(rec, C.c_uint64)))
        return [rec[int(a): int(b)] for a, b in zip(rp[:-1], rp[1:])]


class WhatIfImpact:
    """A plan's change lists by node (``flavour == "node"``) or its route lists
    by set (``"set"``), on the host: key k owns transposed entries ``ptr[k] ..
    ptr[k + 1]`` of ``fail`` (the failure index) / ``ent`` (the index of that
    entry in the lists' pools: ``changes.dist[e]``, ``routes.min_metric[e]``) in
    device order; ``of(k)`` returns them ascending by failure.  ``impact`` holds
    the summaries (``IMPACT_DTYPE``, one per key).  The device arrays stay with
    the plan until its next call of the flavour, ``changes()`` or, by set,
    ``routes()``."""

    def __init__(self, plan: "WhatIfPlan", flavour: str, stream: int = 0) -> None:
        if flavour not in ("node", "set"):
            raise ValueError(f"impact flavour {flavour!r}: 'node' or 'set'")
        self.plan, self.flavour = plan, flavour
        eng, h = plan._eng, plan._h
        self._call = lambda name: getattr(N.lib, f"spf_whatif_by_{flavour}{name}")
        n, nbytes, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        eng._err(self._call("")(h, C.byref(n), C.byref(nbytes), C.byref(ms),
                                C.c_void_p(stream) if stream else None))
        self.n_entries, self.pool_bytes, self.kernel_ms = int(n.value), int(nbytes.value), ms.value
        k = C.c_uint32()
        eng._err(self._call("_buffers")(h, None, None, None, None, C.byref(k), None))
        self.n_keys = int(k.value)
        self.ptr, self.fail, self.ent, self.impact = _pool_read(
            eng._err, self._call("_read"), h, self.n_keys, self.n_entries,
            np.zeros(self.n_keys, IMPACT_DTYPE))

    def timing(self) -> Tuple[float, float, float]:
        """(count, scan, fill) ms of the call."""
        ms = (C.c_double * 3)()
        which = 0 if self.flavour == "node" else 1
        self.plan._eng._err(N.lib.spf_whatif_impact_timing(self.plan._h, which, ms))
        return ms[0], ms[1], ms[2]

    def of(self, key: int) -> Tuple[np.ndarray, np.ndarray]:
        """Key `key`'s (fail[n], ent[n]), ascending by failure index."""
        return _pool_of(self.plan._eng._err, self._call("_db"), self.plan._h, key)


class SpfEngine(NativeHandle):
    """An engine context with one graph loaded (``spf_ctx``).  ``close()``
    (or ``with SpfEngine(0) as eng:``) first closes the plans created on it,
    then destroys the context (its streams, events and device buffers)."""

    _LEVEL = 1
    _destroy = "spf_ctx_destroy"

    def __init__(self, device: int = 0, handle: Optional[C.c_void_p] = None,
                 n_nodes: int = 0) -> None:
        self._owned = handle is None
        self.device = device
        self._n_nodes = n_nodes  # (a wrapped handle's graph was loaded by its owner)
        self._plans: "weakref.WeakSet[NativeHandle]" = weakref.WeakSet()
        if handle is None:
            h = C.c_void_p()
            st = N.lib.spf_ctx_create(device, C.byref(h))
            N.raise_for(st, N.global_error())
            self._adopt(h)
        else:
            self._h = handle
        self._graph = None

    def close(self) -> None:
        for p in list(getattr(self, "_plans", ())):
            p.close()
        super().close()

    def _track(self, plan):
        self._plans.add(plan)
        return plan

    def _err(self, st: int) -> None:
        N.raise_for(st, (N.lib.spf_last_error(self._h) or b"").decode())

    # ---- graph -----------------------------------------------------------------
    def load(self, row_ptr, col, metric, link_id, overloaded) -> None:
        arrs = (np.ascontiguousarray(row_ptr, np.uint32), np.ascontiguousarray(col, np.uint32),
                np.ascontiguousarray(metric, np.int32), np.ascontiguousarray(link_id, np.uint32),
                np.ascontiguousarray(overloaded, np.uint8))
        g = N.SpfGraph()
        g.n_nodes = len(arrs[0]) - 1
        g.n_edges = len(arrs[1])
        g.row_ptr = N.ptr(arrs[0])
        g.col = N.ptr(arrs[1])
        g.metric = N.ptr(arrs[2], C.c_int32)
        g.link_id = N.ptr(arrs[3])
        g.overloaded = N.ptr(arrs[4], C.c_uint8)
        self._err(N.lib.spf_graph_load(self._h, C.byref(g)))
        self._graph = arrs

    def set_overload(self, nodes, overloaded) -> None:
        """Drain / undrain nodes in place (spf_graph_set_overload): SPF plans
        re-derive on their next execute, KSP2 / what-if plans must be recreated."""
        nodes = np.ascontiguousarray(nodes, np.uint32)
        vals = np.ascontiguousarray(overloaded, np.uint8)
        if len(nodes) != len(vals):
            raise ValueError("nodes / overloaded length mismatch")
        self._err(N.lib.spf_graph_set_overload(self._h, N.ptr(nodes), N.ptr(vals, C.c_uint8),
                                               len(nodes)))
        if self._graph is not None:
            self._graph[4][nodes] = vals

    def set_metric(self, edges, metric) -> None:
        """New metrics of directed CSR edges in place (spf_graph_set_metric)."""
        edges = np.ascontiguousarray(edges, np.uint32)
        mets = np.ascontiguousarray(metric, np.int32)
        if len(edges) != len(mets):
            raise ValueError("edges / metric length mismatch")
        self._err(N.lib.spf_graph_set_metric(self._h, N.ptr(edges), N.ptr(mets, C.c_int32),
                                             len(edges)))
        if self._graph is not None:
            self._graph[2][edges] = mets

    @property
    def epoch(self) -> int:
        """Graph version: bumped by every load and in-place patch."""
        return int(N.lib.spf_graph_epoch(self._h))

    @property
    def loads(self) -> int:
        """spf_graph_load calls so far (in-place patches do not count)."""
        return int(N.lib.spf_graph_loads(self._h))

    @property
    def pitch(self) -> int:
        return int(N.lib.spf_row_pitch(self._h))

    @property
    def n_nodes(self) -> int:
        return len(self._graph[0]) - 1 if self._graph is not None else self._n_nodes

    def neighbors(self, src: int) -> np.ndarray:
        cnt = C.c_uint32()
        self._err(N.lib.spf_src_neighbors(self._h, src, None, 0, C.byref(cnt)))
        out = np.zeros(max(1, cnt.value), np.uint32)
        self._err(N.lib.spf_src_neighbors(self._h, src, N.ptr(out), cnt.value, C.byref(cnt)))
        return out[: cnt.value]

    def debug_stamps(self) -> np.ndarray:
        """BFS phase clocks of workgroup 0 (needs SPF_STAMPS=1 at first execute):
        [16 waves, 64] -- column 0 is the count, columns 1.. the clocks."""
        return self._stamp_words()[: 64 * 16].reshape(16, 64)

    def _stamp_words(self) -> np.ndarray:
        out = np.zeros(64 * 16 + 1 + 2 * 1024, np.uint64)
        n = C.c_uint32()
        self._err(N.lib.spf_debug_stamps(self._h, N.ptr(out, C.c_uint64), out.size, C.byref(n)))
        return out

    def debug_timeline(self) -> np.ndarray:
        """Team BFS block timeline (SPF_STAMPS set): [block, (start, end)]
        s_memrealtime ticks (100 MHz), zeros for blocks that did not run."""
        return self._stamp_words()[64 * 16 + 1:].reshape(1024, 2)

    def solves(self) -> int:
        return int(N.lib.spf_solves(self._h))

    def copy_bandwidth(self, nbytes: int = 1 << 30, reps: int = 10) -> float:
        """Measured practical HBM ceiling in GB/s (spf_debug_copy_bandwidth)."""
        g = C.c_double()
        self._err(N.lib.spf_debug_copy_bandwidth(self._h, nbytes, reps, C.byref(g)))
        return g.value

    def check(self) -> None:
        """Wait for the device and raise if a grid-resident kernel's barrier
        gave up waiting since the last check (spf_device_check): the outputs
        of those launches are invalid."""
        self._err(N.lib.spf_device_check(self._h))

    # ---- solves -----------------------------------------------------------------
    @property
    def needs_dist64(self) -> bool:
        """Weighted solves of this graph need u64 distances (spf_graph_needs_dist64)."""
        return bool(N.lib.spf_graph_needs_dist64(self._h))

    def plan(self, srcs: Sequence[int], hop: bool = False, dist64: bool = False) -> SpfPlan:
        return self._track(SpfPlan(self, srcs, (HOP_COUNT if hop else 0) |
                                   (DIST64 if dist64 else 0)))

    def solve(self, srcs: Sequence[int], hop: bool = False, dist64: bool = False) -> SolveResult:
        """All of `srcs` in one plan, results on the host.  dist64: u64
        distance rows (the exact kernel; needed when needs_dist64)."""
        with self.plan(srcs, hop, dist64) as p:
            return p.execute_host()

    def solve_exact(self, src: int, hop: bool = False,
                    ignore_links: Optional[Sequence[int]] = None):
        """runSpf on the exact kernel (spf_solve_exact): (dist u64 [N],
        next-hop bitmaps [k, N] bool, pop rank [N] u32)."""
        ign = np.ascontiguousarray(ignore_links if ignore_links is not None else [], np.uint32)
        n = self.n_nodes
        k = len(self.neighbors(src))
        dist = np.zeros(n, np.uint64)
        nh = np.zeros(max(1, k * self.pitch // 32), np.uint32)
        pop = np.zeros(n, np.uint32)
        self._err(N.lib.spf_solve_exact(self._h, src, HOP_COUNT if hop else 0,
                                        N.ptr(ign) if len(ign) else None, len(ign),
                                        N.ptr(dist, C.c_uint64), None, N.ptr(nh), N.ptr(pop)))
        return dist, nh_matrix(nh, 0, k, self.pitch, n), pop

    def ksp2_plan(self, srcs: Sequence[int]) -> Ksp2Plan:
        return self._track(Ksp2Plan(self, srcs))

    def ksp2(self, srcs: Sequence[int]) -> Ksp2Result:
        """getKthPaths(s, d, 1) and (s, d, 2) for every s in srcs, every d."""
        srcs = np.ascontiguousarray(srcs, np.uint32)
        n = self.n_nodes
        pairs = np.zeros(len(srcs) * n, PAIR_DTYPE)
        used = C.c_uint64()
        pool = np.empty(len(pairs) * 12 + (1 << 20), np.uint32)  # lazily backed
        for _ in range(2):
            st = N.lib.spf_ksp2_solve(self._h, N.ptr(srcs), len(srcs),
                                      N.ptr(pairs.view(np.uint32)), N.ptr(pool), pool.size,
                                      C.byref(used))
            if st != N.SPF_E_NOMEM or used.value <= pool.size:
                break
            pool = np.empty(used.value, np.uint32)  # too small: size it exactly, rerun
        self._err(st)
        pool = pool[: used.value]
        return Ksp2Result(srcs, n, pairs, pool)

    def ksp2_routes(self, srcs: Sequence[int], set_ptr, set_nodes, node_label,
                    set_prepend=None) -> Ksp2Routes:
        """Every source's KSP2_ED_ECMP next hops towards every destination
        set, all on the GPU: plan, execute (the path pool grown on overflow, as
        ksp2() does), then Ksp2Plan.routes.  The paths never leave the device."""
        from .hiprt import DeviceArray, set_device, synchronize

        set_device(self.device)
        plan = self.ksp2_plan(srcs)
        bufs: list = []
        try:
            n_pairs = len(plan.srcs) * self.n_nodes
            d_pairs = DeviceArray(4 * n_pairs, np.uint32)
            d_cnt = DeviceArray(4, np.uint64)
            bufs += [d_pairs, d_cnt]
            words = n_pairs * 12 + (1 << 20)
            for _ in range(3):
                d_pool = DeviceArray(words, np.uint32)
                plan.execute(d_pairs.ptr, d_pool.ptr, words, d_cnt.ptr)
                synchronize()
                cnt = d_cnt.numpy()
                if not int(cnt[2]) & 1:
                    break
                d_pool.free()
                words = int(cnt[0]) + int(cnt[0]) // 4  # the counter says how much it wanted
            else:
                raise N.SpfError(N.SPF_E_NOMEM, "KSP2 path pool overflow")
            bufs.append(d_pool)
            totals = plan.routes(d_pairs.ptr, d_pool.ptr, set_ptr, set_nodes, node_label, set_prepend)
        except BaseException:
            plan.close()
            for b in bufs:
                b.free()
            raise
        return Ksp2Routes(plan, bufs, totals)

    def whatif_plan(self, src: int, links: Optional[Sequence[int]] = None) -> WhatIfPlan:
        return self._track(WhatIfPlan(self, src, links))

    def whatif(self, src: int, links: Optional[Sequence[int]] = None):
        """Digests of runSpf(src, true, {l}) for each failed link l (every up
        link when `links` is None): (links, digests[n], base digest)."""
        if links is None:
            links = self.whatif_plan(src).links
        arr = np.ascontiguousarray(links, np.uint32)
        out = np.zeros(max(1, len(arr)), DIGEST_DTYPE)
        base = np.zeros(1, DIGEST_DTYPE)
        self._err(N.lib.spf_whatif_solve(self._h, src, N.ptr(arr), len(arr),
                                         out.ctypes.data, base.ctypes.data))
        return arr, out[: len(arr)], base[0]

    def _digests_of(self, plan: WhatIfPlan):
        """(digests[n], base digest) of one execute of `plan`, which is closed."""
        from .hiprt import DeviceArray, set_device

        try:
            set_device(self.device)
            d_out = DeviceArray(max(1, plan.n_fail), DIGEST_DTYPE)
            d_base = DeviceArray(1, DIGEST_DTYPE)
            try:
                plan.execute(d_out.ptr, d_base.ptr)
                plan.stats()  # waits for the execute, checks the device's fault word
                return d_out.numpy()[: plan.n_fail], d_base.numpy()[0]
            finally:
                d_out.free()
                d_base.free()
        finally:
            plan.close()

    def _owned_changes(self, plan: WhatIfPlan) -> WhatIfChanges:
        """The change lists of `plan`, which they own (closed if they fail)."""
        try:
            return WhatIfChanges(plan, own_plan=True)
        except BaseException:
            plan.close()
            raise

    def whatif_changes(self, src: int, links: Optional[Sequence[int]] = None) -> WhatIfChanges:
        """What each failure changes: the nodes whose metric or next hops
        move under runSpf(src, true, {l}), with their new values, for each
        failed link l (every up link when `links` is None).  close() the
        result (it owns its plan)."""
        return self._owned_changes(self.whatif_plan(src, links))

    def whatif_routes(self, plan_or_changes, sets) -> WhatIfRoutes:
        """Which routes of the plan's source each failure changes, over the
        destination sets `sets` (``spf_whatif_routes``).  Takes a
        ``WhatIfChanges``, or a ``WhatIfPlan`` of any kind, whose change lists
        are then computed first (``result.changes``)."""
        ch = plan_or_changes.changes() if isinstance(plan_or_changes, WhatIfPlan) else plan_or_changes
        return ch.routes(sets)

    def whatif_impact(self, changes_or_routes) -> WhatIfImpact:
        """The lists of a ``WhatIfChanges`` by node, or of a ``WhatIfRoutes`` by
        set: per destination the failures that touch it and its summary
        (``spf_whatif_by_node`` / ``spf_whatif_by_set``)."""
        if isinstance(changes_or_routes, WhatIfRoutes):
            return changes_or_routes.by_set()
        return changes_or_routes.by_node()

    def whatif_route_update(self, routes: WhatIfRoutes) -> "WhatIfRouteUpdate":
        """Each failure's link-level next hops over the sets of a
        ``WhatIfRoutes`` (``spf_whatif_route_update``)."""
        return routes.update()

    def whatif_node_plan(self, src: int, nodes: Optional[Sequence[int]] = None,
                         kind: str = "down") -> WhatIfPlan:
        """A what-if plan whose failures are nodes: ``kind="down"`` (every
        link of the node ignored) or ``"drain"`` (the node overloaded); every
        node except `src` when `nodes` is None."""
        if kind not in ("down", "drain"):
            raise ValueError(f"node what-if kind {kind!r}: 'down' or 'drain'")
        return self._track(WhatIfPlan(self, src, nodes, kind))

    def whatif_nodes(self, src: int, nodes: Optional[Sequence[int]] = None, kind: str = "down"):
        """Digests of the SPF of `src` with each node of the list down or
        drained: (nodes, digests[n], base digest)."""
        plan = self.whatif_node_plan(src, nodes, kind)
        return (plan.nodes, *self._digests_of(plan))

    def whatif_node_changes(self, src: int, nodes: Optional[Sequence[int]] = None,
                            kind: str = "down") -> WhatIfChanges:
        """What each node failure changes (``whatif_changes`` for nodes down
        or drained).  close() the result (it owns its plan)."""
        return self._owned_changes(self.whatif_node_plan(src, nodes, kind))

    def whatif_set_plan(self, src: int, sets: Sequence[Sequence[int]]) -> WhatIfPlan:
        """A what-if plan whose failures are sets of links that fail together
        (shared-risk groups): failure i ignores every link of ``sets[i]``."""
        return self._track(WhatIfPlan(self, src, sets, "sets"))

    def whatif_sets(self, src: int, sets: Sequence[Sequence[int]]):
        """Digests of runSpf(src, true, set) for each set of links:
        (digests[n], base digest)."""
        return self._digests_of(self.whatif_set_plan(src, sets))

    def whatif_set_changes(self, src: int, sets: Sequence[Sequence[int]]) -> WhatIfChanges:
        """What each link-set failure changes (``whatif_changes`` for sets).
        close() the result (it owns its plan)."""
        return self._owned_changes(self.whatif_set_plan(src, sets))

    def whatif_metric_plan(self, src: int, changes: Sequence[Sequence[int]]) -> WhatIfPlan:
        """A what-if plan whose failures are link metric changes (cost-out,
        undrain): change i is ``(link, m_lo, m_hi)``, the new metrics of the
        link's direction from its endpoint with the smaller node id to the
        larger and of the opposite one; 0 keeps a direction's metric."""
        return self._track(WhatIfPlan(self, src, changes, "metric"))

    def whatif_metrics(self, src: int, changes: Sequence[Sequence[int]]):
        """Digests of runSpf(src) under each metric change:
        (digests[n], base digest)."""
        return self._digests_of(self.whatif_metric_plan(src, changes))

    def whatif_metric_changes(self, src: int, changes: Sequence[Sequence[int]]) -> WhatIfChanges:
        """What each link metric change changes (``whatif_changes`` for
        metric changes).  close() the result (it owns its plan)."""
        return self._owned_changes(self.whatif_metric_plan(src, changes))

    def sssp(self, src: int, hop: bool = False,
             ignore_links: Optional[Sequence[int]] = None) -> np.ndarray:
        ign = np.ascontiguousarray(ignore_links if ignore_links is not None else [], np.uint32)
        out = np.zeros(self.n_nodes, np.uint32)
        self._err(N.lib.spf_sssp(self._h, src, HOP_COUNT if hop else 0,
                                 N.ptr(ign) if len(ign) else None, len(ign), N.ptr(out)))
        return out

    def preds(self, src: int, dist: np.ndarray, hop: bool = False,
              ignore_links: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
        ign = np.ascontiguousarray(ignore_links if ignore_links is not None else [], np.uint32)
        dist = np.ascontiguousarray(dist, np.uint32)
        ptr_ = np.zeros(self.n_nodes + 1, np.uint32)
        cnt = C.c_uint32()
        args = (self._h, src, HOP_COUNT if hop else 0, N.ptr(ign) if len(ign) else None, len(ign),
                N.ptr(dist), N.ptr(ptr_))
        self._err(N.lib.spf_preds(*args, None, 0, C.byref(cnt)))
        edges = np.zeros(max(1, cnt.value), np.uint32)
        self._err(N.lib.spf_preds(*args, N.ptr(edges), cnt.value, C.byref(cnt)))
        return ptr_, edges[: cnt.value]


def partition_sources(nb_ptr, nb_id, srcs, n_parts: int, mode: str = "auto"):
    """Sources to parts (spf_partition_sources, host only): (part of each
    source [n_src] u32, the rule taken: "contiguous" | "locality").
    nb_ptr / nb_id: distinct up neighbours of every node in CSR form."""
    nb_ptr = np.ascontiguousarray(nb_ptr, np.uint32)
    nb_id = np.ascontiguousarray(nb_id if len(nb_id) else [0], np.uint32)
    srcs = np.ascontiguousarray(srcs, np.uint32)
    code = {"auto": N.SPF_PARTITION_AUTO, "contiguous": N.SPF_PARTITION_CONTIGUOUS,
            "locality": N.SPF_PARTITION_LOCALITY}[mode]
    part = np.zeros(max(1, len(srcs)), np.uint32)
    used = C.c_uint32()
    st = N.lib.spf_partition_sources(N.ptr(nb_ptr), N.ptr(nb_id), len(nb_ptr) - 1, N.ptr(srcs),
                                     len(srcs), n_parts, code, N.ptr(part), C.byref(used))
    N.raise_for(st, N.global_error())
    return part[: len(srcs)], N.PARTITION_NAMES[used.value]


class SpfMultiPlan(NativeHandle):
    """A source batch split over the members of an ``SpfMultiEngine``
    (``spf_mplan``): every member's rows and bitmaps stay on its device."""

    _destroy = "spf_mplan_destroy"

    def __init__(self, eng: "SpfMultiEngine", srcs: Sequence[int], flags: int,
                 mode: str = "auto") -> None:
        self._eng = eng
        self.srcs = np.ascontiguousarray(srcs, np.uint32)
        self.flags = flags
        code = {"auto": N.SPF_PARTITION_AUTO, "contiguous": N.SPF_PARTITION_CONTIGUOUS,
                "locality": N.SPF_PARTITION_LOCALITY}[mode]
        h = C.c_void_p()
        eng._err(N.lib.spf_mplan_create(eng._h, N.ptr(self.srcs), len(self.srcs), flags, code,
                                        C.byref(h)))
        self._adopt(h)
        self.partition = N.PARTITION_NAMES[int(N.lib.spf_mplan_partition(h))]
        self.members = eng.size
        self.closure_rows = [int(N.lib.spf_mplan_closure_rows(h, i)) for i in range(self.members)]

    def owner(self, i: int) -> Tuple[int, int]:
        """(member, row) holding request index i."""
        m, r = C.c_uint32(), C.c_uint32()
        self._eng._err(N.lib.spf_mplan_owner(self._h, i, C.byref(m), C.byref(r)))
        return m.value, r.value

    def shard_sizes(self) -> List[int]:
        out = []
        for i in range(self.members):
            n = C.c_uint32()
            self._eng._err(N.lib.spf_mplan_shard(self._h, i, C.byref(n), None, None, None))
            out.append(n.value)
        return out

    def member_kernels(self, i: int) -> Optional[Tuple[str, bool]]:
        """The member's plan kernels (SpfPlan.kernels), None for an idle member."""
        n, plan = C.c_uint32(), C.c_void_p()
        self._eng._err(N.lib.spf_mplan_shard(self._h, i, C.byref(n), C.byref(plan), None, None))
        if not plan.value:
            return None
        bfs, narrow = C.c_uint32(), C.c_uint32()
        N.raise_for(N.lib.spf_plan_kernels(plan, C.byref(bfs), C.byref(narrow)), "spf_plan_kernels")
        return SpfPlan.BFS_KERNELS[bfs.value], bool(narrow.value)

    def set_graphs(self, enable: bool) -> None:
        self._eng._err(N.lib.spf_mplan_set_graphs(self._h, int(bool(enable))))

    def set_enqueue_threads(self, mode: int) -> None:
        """1: each member's execute enqueued from its own host thread, 0: one
        after another from the caller's, -1: threads for distinct devices."""
        self._eng._err(N.lib.spf_mplan_set_enqueue_threads(self._h, int(mode)))

    def enqueue_ns(self) -> Tuple[np.ndarray, bool]:
        """The last execute's host enqueue: per member, ns from the execute's
        start until its launches were enqueued; and whether threads issued them."""
        n = len(self.shard_sizes())
        out = np.zeros(max(1, n), np.uint64)
        thr = C.c_int()
        self._eng._err(N.lib.spf_mplan_enqueue_ns(self._h, N.ptr(out, C.c_uint64), n, C.byref(thr)))
        return out[:n], bool(thr.value)

    def execute(self) -> None:
        self._eng._err(N.lib.spf_mplan_execute(self._h))

    def synchronize(self) -> None:
        self._eng._err(N.lib.spf_mplan_synchronize(self._h))

    def digest(self) -> np.ndarray:
        out = np.zeros(max(1, len(self.srcs)), np.uint64)
        self._eng._err(N.lib.spf_mplan_digest(self._h, N.ptr(out, C.c_uint64)))
        return out[: len(self.srcs)]

    def read(self, i: int) -> Tuple[np.ndarray, np.ndarray]:
        """Request i's (dist [n_nodes], next-hop bitmaps bool [k, n_nodes]) from its owner."""
        n = self._eng.n_nodes
        k = len(self._eng.neighbors(int(self.srcs[i])))
        dist = np.zeros(n, np.uint64 if self.flags & DIST64 else np.uint32)
        nh = np.zeros(max(1, k * self._eng.pitch // 32), np.uint32)
        self._eng._err(N.lib.spf_mplan_read(self._h, i, dist.ctypes.data, N.ptr(nh)))
        return dist, nh_matrix(nh, 0, k, self._eng.pitch, n)

    def preds(self, i: int) -> Tuple[np.ndarray, np.ndarray]:
        n = self._eng.n_nodes
        ptr_ = np.zeros(n + 1, np.uint32)
        cnt = C.c_uint32()
        self._eng._err(N.lib.spf_mplan_preds(self._h, i, N.ptr(ptr_), None, 0, C.byref(cnt)))
        edges = np.zeros(max(1, cnt.value), np.uint32)
        self._eng._err(N.lib.spf_mplan_preds(self._h, i, N.ptr(ptr_), N.ptr(edges), cnt.value,
                                             C.byref(cnt)))
        return ptr_, edges[: cnt.value]

    def enable_timing(self, max_executes: int) -> None:
        self._eng._err(N.lib.spf_mplan_enable_timing(self._h, max_executes))

    def timing(self) -> Tuple[List[float], int]:
        """(per-member summed execute ms, executes) since enable / the last call."""
        ms = (C.c_double * self.members)()
        n = C.c_uint32()
        self._eng._err(N.lib.spf_mplan_timing(self._h, ms, C.byref(n)))
        return [ms[i] for i in range(self.members)], n.value


class SpfMultiEngine(NativeHandle):
    """Several GPUs behind one context (``spf_mctx``): one member engine per
    device id (ids may repeat), the graph replicated to each."""

    _LEVEL = 1
    _destroy = "spf_mctx_destroy"

    def __init__(self, devices: Sequence[int]) -> None:
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        st = N.lib.spf_mctx_create(ids, len(devices), C.byref(h))
        N.raise_for(st, N.global_error())
        self._adopt(h)
        self._plans: "weakref.WeakSet[NativeHandle]" = weakref.WeakSet()
        self.devices = list(devices)
        # member 0 answers the graph queries (neighbours, pitch)
        self.member0 = SpfEngine(handle=C.c_void_p(N.lib.spf_mctx_member(h, 0)))

    @property
    def size(self) -> int:
        return int(N.lib.spf_mctx_size(self._h))

    def close(self) -> None:
        for p in list(getattr(self, "_plans", ())):
            p.close()
        super().close()

    def _err(self, st: int) -> None:
        N.raise_for(st, (N.lib.spf_mctx_last_error(self._h) or b"").decode())

    def load(self, row_ptr, col, metric, link_id, overloaded) -> None:
        arrs = (np.ascontiguousarray(row_ptr, np.uint32), np.ascontiguousarray(col, np.uint32),
                np.ascontiguousarray(metric, np.int32), np.ascontiguousarray(link_id, np.uint32),
                np.ascontiguousarray(overloaded, np.uint8))
        g = N.SpfGraph()
        g.n_nodes = len(arrs[0]) - 1
        g.n_edges = len(arrs[1])
        g.row_ptr = N.ptr(arrs[0])
        g.col = N.ptr(arrs[1])
        g.metric = N.ptr(arrs[2], C.c_int32)
        g.link_id = N.ptr(arrs[3])
        g.overloaded = N.ptr(arrs[4], C.c_uint8)
        self._err(N.lib.spf_mctx_graph_load(self._h, C.byref(g)))
        self.member0._graph = arrs

    def set_overload(self, nodes, overloaded) -> None:
        nodes = np.ascontiguousarray(nodes, np.uint32)
        vals = np.ascontiguousarray(overloaded, np.uint8)
        self._err(N.lib.spf_mctx_graph_set_overload(self._h, N.ptr(nodes), N.ptr(vals, C.c_uint8),
                                                    len(nodes)))
        self.member0._graph[4][nodes] = vals

    @property
    def pitch(self) -> int:
        return self.member0.pitch

    @property
    def n_nodes(self) -> int:
        return self.member0.n_nodes

    def neighbors(self, src: int) -> np.ndarray:
        return self.member0.neighbors(src)

    def plan(self, srcs: Sequence[int], hop: bool = False, dist64: bool = False,
             mode: str = "auto") -> SpfMultiPlan:
        p = SpfMultiPlan(self, srcs, (HOP_COUNT if hop else 0) | (DIST64 if dist64 else 0), mode)
        self._plans.add(p)
        return p


def graph_from_lsdb(lsdb, area: str = "0"):
    """Flatten a packed LSDB with the LinkState facade (host side only).
    Returns (node_names, row_ptr, col, metric, link_id, overloaded)."""
    from .link_state import LinkState

    ls = LinkState(area, device=-1)
    ls.updateAdjacencyDatabases(lsdb)
    return ls.flatten()
