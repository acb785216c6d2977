"""Time every node's route-database delta (spf_mplan_route_delta) on
fabric_full, one GPU, next to the materialisation it compares
(spf_mplan_route_records over the n single-node sets, set v = {v}).

    python tools/route_delta_time.py [--sws 10000] [--reps 5] [--lfa]

Each rep alternates an unchanged pass (records, snapshot, records, delta: every
list empty) and a one-uplink flap (records, snapshot, the first rack switch's
first uplink down or back up -- or, with --flap withdraw, withdrawn or
advertised again --, the pass and records again, delta).  Prints one
JSON line: median and best HIP-event kernel ms of the delta (unchanged and
flap) and of the records kernel, the bytes the delta reads (both generations'
written records and headers) with the GB/s that makes and
spf_debug_copy_bandwidth for that byte count, the flap's list sizes against
the pools they stand for, the me that took the set path, and the device memory
a live snapshot holds.
"""
import argparse
import copy
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from openr_amd import _native as N  # noqa: E402
from openr_amd import topology as T  # noqa: E402
from openr_amd.link_state import LinkState  # noqa: E402
from openr_amd.wire import unpack  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sws", type=int, default=10000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lfa", action="store_true")
ap.add_argument("--flap", choices=["down", "withdraw"], default="down",
                help="down: the uplink's adjacency overloaded (its slot and key stay: fast path); "
                     "withdraw: the adjacency withdrawn (both ends' rows reordered: set path)")
args = ap.parse_args()

topo = T.fabric(args.sws, full=True)
with LinkState(devices=[0]) as ls:
    ls.updateAdjacencyDatabases(topo.lsdb)
    dbs = {d.thisNodeName: d for d in unpack(topo.lsdb)}
    ls.prefetchAllSources()
    names, rp = ls.flatten()[:2]
    n = len(names)
    ptr = np.arange(n + 1, dtype=np.uint32)
    nodes = np.arange(n, dtype=np.uint32)
    flapper = min(dbs, key=lambda s: (len(dbs[s].adjacencies), s))  # a rack switch

    def delta_raw(snap):
        """(totals, kernel ms) without reading the lists back"""
        mp = N.lib.ls_all_sources_plan(ls._h)
        lh = ls.linkValueHashes()
        tot, ms = np.zeros(5, np.uint64), C.c_double()
        N.raise_for(N.lib.spf_mplan_route_delta(C.c_void_p(mp), snap._h, N.ptr(lh, C.c_uint64), len(lh),
                                                N.ptr(tot, C.c_uint64), C.byref(ms)), N.global_error())
        return [int(v) for v in tot], ms.value

    same_ms, flap_ms, rec_ms, flap_tot, held, recs = [], [], [], None, 0, []
    held_adj, set_path = None, []
    for rep in range(args.reps + 1):  # (the first: warm-up)
        n_rec, ms_r = ls.allSourcesRouteRecords(ptr, nodes, args.lfa)
        snap = ls.allSourcesRouteSnapshot()
        held = snap.deviceBytes
        n_rec2, ms_r2 = ls.allSourcesRouteRecords(ptr, nodes, args.lfa)
        tot, ms = delta_raw(snap)
        assert tot[:4] == [0, 0, 0, 0] and n_rec2 == n_rec
        snap.close()
        snap = ls.allSourcesRouteSnapshot()
        if args.flap == "down":
            a = dbs[flapper].adjacencies[0]
            a.isOverloaded = not a.isOverloaded
        elif held_adj is None:
            held_adj = dbs[flapper].adjacencies.pop(0)
        else:
            dbs[flapper].adjacencies.insert(0, held_adj)
            held_adj = None
        ls.updateAdjacencyDatabase(copy.deepcopy(dbs[flapper]))
        ls.prefetchAllSources()
        n_rec3, ms_r3 = ls.allSourcesRouteRecords(ptr, nodes, args.lfa)
        ftot, fms = delta_raw(snap)
        assert ftot[0] + ftot[1] > 0
        snap.close()
        if rep:
            same_ms.append(ms)
            flap_ms.append(fms)
            rec_ms += [ms_r, ms_r2, ms_r3]
            flap_tot = ftot
            set_path.append(ftot[4])
            recs = [n_rec, n_rec3]
    read_bytes = 8 * (recs[0] + recs[1]) + 2 * 8 * n * n
    gbs = C.c_double()
    N.raise_for(N.lib.spf_debug_copy_bandwidth(C.c_void_p(N.lib.ls_engine(ls._h)), read_bytes // 2, 3,
                                               C.byref(gbs)), N.global_error())
    med = statistics.median(same_ms)
    print(json.dumps({
        "workload": topo.name, "nodes": n, "directed_edges": int(rp[n]), "lfa": bool(args.lfa),
        "delta_unchanged_kernel_ms": {"median": med, "best": min(same_ms)},
        "delta_flap_kernel_ms": {"median": statistics.median(flap_ms), "best": min(flap_ms)},
        "route_records_kernel_ms": {"median": statistics.median(rec_ms), "best": min(rec_ms)},
        "delta_read_bytes": read_bytes, "delta_read_gbs": read_bytes / med / 1e6,
        "copy_bandwidth_gbs_same_bytes_moved": gbs.value,
        "flap": {"kind": args.flap, "node": flapper, "me_on_set_path_per_rep": set_path, "ip_updates": flap_tot[0], "ip_deletes": flap_tot[1],
                 "me_on_set_path": flap_tot[4], "list_bytes": 4 * (flap_tot[0] + flap_tot[1]) + 8 * (n + 1),
                 "pool_bytes_replaced": 8 * recs[1] + 8 * n * n},
        "snapshot_device_bytes": held, "reps": args.reps}))
