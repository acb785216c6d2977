"""Time the payload of every node's route-database delta
(spf_mplan_route_update) on fabric_full, one GPU, over the IP routes (set v =
{v}), next to what obtained the same next hops before it: spf_mplan_route_db
for every me that has an entry.

    python tools/route_update_time.py [--sws 10000] [--reps 5] [--lfa] [--baseline-me 48]

Two cases, each records, snapshot, the change, the pass and records again,
delta, update:
  flap    the first rack switch's first uplink overloaded
  drain   one spine switch overloaded (a large update: the share of all routes
          it touches is reported)
Prints one JSON line: per case the entries and records, the pool bytes, the
median HIP-event ms of count / scan / fill for every lane-group width of the
fill (SPF_UPDATE_GROUP; "group" names the default), the bytes the three passes
read and write with the GB/s that makes and spf_debug_copy_bandwidth for the
same bytes moved, the wall ms of the update plus the read-back of the lists and
the payload (spf_mplan_route_update_read: one copy per array), and the wall ms of spf_mplan_route_db for those me -- measured over
--baseline-me of them, evenly spaced, and scaled to all (each call copies me's
whole tiled region; all of them would read back most of the database) -- with
the ratio of the two.
"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys
import time
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
ap.add_argument("--baseline-me", type=int, default=48)
args = ap.parse_args()

WIDTHS = (4, 8, 16, 32, 64)
DEFAULT_GROUP = 16  # route_update.hip's width without SPF_UPDATE_GROUP
topo = T.fabric(args.sws, full=True)
with LinkState(devices=[0]) as ls:
    ls.updateAdjacencyDatabases(topo.lsdb)
    dbs = {d.thisNodeName: d for d in unpack(topo.lsdb)}
    ls.prefetchAllSources()
    names, rp = ls.flatten()[:2]
    n = len(names)
    ptr = np.arange(n + 1, dtype=np.uint32)
    nodes = np.arange(n, dtype=np.uint32)
    rack = min(dbs, key=lambda s: (len(dbs[s].adjacencies), s))
    spine = min(s for s in dbs if s.startswith("1-"))

    def flap(on):
        dbs[rack].adjacencies[0].isOverloaded = on
        ls.updateAdjacencyDatabase(copy.deepcopy(dbs[rack]))

    def drain(on):
        dbs[spine].isOverloaded = on
        ls.updateAdjacencyDatabase(copy.deepcopy(dbs[spine]))

    def update(mp):
        tot, nbytes, ms = np.zeros(4, np.uint64), C.c_uint64(), C.c_double()
        t0 = time.perf_counter()
        N.raise_for(N.lib.spf_mplan_route_update(mp, N.ptr(tot, C.c_uint64), C.byref(nbytes), C.byref(ms)),
                    N.global_error())
        wall = (time.perf_counter() - t0) * 1e3
        phase = (C.c_double * 3)()
        N.raise_for(N.lib.spf_mplan_route_update_timing(mp, phase), N.global_error())
        return [int(v) for v in tot], int(nbytes.value), list(phase), wall

    def case(change, node):
        ls.allSourcesRouteRecords(ptr, nodes, args.lfa)
        snap = ls.allSourcesRouteSnapshot()
        change(True)
        ls.prefetchAllSources()
        n_rec, _ = ls.allSourcesRouteRecords(ptr, nodes, args.lfa)
        lists, dtot, dms = ls.allSourcesRouteDelta(snap)
        mp = C.c_void_p(N.lib.ls_all_sources_plan(ls._h))
        with_entries = [t for t, l in enumerate(lists) if l[0] or l[1]]
        by_width, walls = {}, []
        for w in WIDTHS + (0,):  # (0: the default, last, so that its pools stay for the read-back)
            if w:
                os.environ["SPF_UPDATE_GROUP"] = str(w)
            else:
                os.environ.pop("SPF_UPDATE_GROUP", None)
            runs = [update(mp) for _ in range(args.reps + 1)][1:]  # (the first: warm-up, allocations)
            tot, pool_bytes = runs[0][0], runs[0][1]
            med = [statistics.median(r[2][k] for r in runs) for k in range(3)]
            by_width[w or "default"] = {"count": med[0], "scan": med[1], "fill": med[2]}
            if not w:
                walls = [r[3] for r in runs]
        entries, records = dtot[0] + dtot[1], tot[1]
        # the read-back: the member's lists and payload, one copy per array
        t0 = time.perf_counter()
        k5 = np.zeros(5, np.uint64)
        N.raise_for(N.lib.spf_mplan_route_update_read(mp, 0, N.ptr(k5, C.c_uint64), *([None] * 9)),
                    N.global_error())
        k, ei, ri = int(k5[0]), int(k5[1]), int(k5[2])
        dp, ds = np.zeros(k + 1, np.uint64), np.zeros(max(1, ei), np.uint32)
        up, ur = np.zeros(ei + 1, np.uint64), np.zeros(max(1, ri), np.uint64)
        N.raise_for(N.lib.spf_mplan_route_update_read(mp, 0, None, N.ptr(dp, C.c_uint64), N.ptr(ds),
                                                      N.ptr(up, C.c_uint64), N.ptr(ur, C.c_uint64), None, None,
                                                      None, None, None), N.global_error())
        readback = (time.perf_counter() - t0) * 1e3
        assert ri == records and int(up[-1]) == records and int(dp[-1]) == entries
        # what the same next hops cost before: spf_mplan_route_db per me
        k = min(args.baseline_me, len(with_entries))
        pick = [with_entries[i * len(with_entries) // k] for i in range(k)]
        hdr = np.zeros(n, np.uint64)
        t0 = time.perf_counter()
        for t in pick:
            c = C.c_uint64()
            N.raise_for(N.lib.spf_mplan_route_db(mp, t, N.ptr(hdr, C.c_uint64), None, 0, C.byref(c)),
                        N.global_error())
            rec = np.zeros(max(1, c.value), np.uint64)
            N.raise_for(N.lib.spf_mplan_route_db(mp, t, None, N.ptr(rec, C.c_uint64), c.value, None),
                        N.global_error())
        base = (time.perf_counter() - t0) * 1e3 * len(with_entries) / k
        snap.close()
        change(False)
        ls.prefetchAllSources()
        d = by_width["default"]
        kernel = d["count"] + d["scan"] + d["fill"]
        moved = 68 * entries + 16 * records
        gbs = C.c_double()
        N.raise_for(N.lib.spf_debug_copy_bandwidth(C.c_void_p(N.lib.ls_engine(ls._h)), max(moved // 2, 1 << 20),
                                                   3, C.byref(gbs)), N.global_error())
        ours = statistics.median(walls) + readback
        return {
            "node": node, "ip_updates": dtot[0], "ip_deletes": dtot[1], "entries": entries, "records": records,
            "records_share_of_database": records / max(1, n_rec), "me_with_entries": len(with_entries),
            "pool_bytes": pool_bytes, "delta_kernel_ms": dms, "phase_ms_by_group": by_width,
            "kernel_ms": kernel, "bytes_read_and_written": moved, "gbs": moved / max(kernel, 1e-9) / 1e6,
            "copy_bandwidth_gbs_same_bytes_moved": gbs.value,
            "fill_gbs": 16 * records / max(d["fill"], 1e-9) / 1e6,
            "update_wall_ms": statistics.median(walls), "readback_wall_ms": readback,
            "route_db_per_me_wall_ms": base, "route_db_me_measured": k,
            "ratio_route_db_over_update": base / ours, "database_records": n_rec,
        }

    out = {"workload": topo.name, "nodes": n, "directed_edges": int(rp[n]), "lfa": bool(args.lfa),
           "group": DEFAULT_GROUP, "reps": args.reps}
    out["flap"] = case(flap, rack)
    out["drain"] = case(drain, spine)
    for c in ("flap", "drain"):
        # routes = (me, set) pairs with a next hop: every me reaches every other node
        out[c]["share_of_routes"] = out[c]["entries"] / (n * (n - 1))
    print(json.dumps(out))
