"""Time every node's IP route database in the exactly sized pool
(spf_mplan_route_records with SPF_ROUTE_COMPACT) on fabric_full, one GPU, next
to the tiled layout over the same selections: every node as me, the n
single-node sets (set v = {v}), with and without LFA.

    python tools/route_records_compact_time.py [--sws 10000] [--reps 5] [--out profiles/route_records_compact.json]

Prints (and with --out writes) one JSON document: per LFA choice both
kernel_ms (median and best of --reps after one warm-up call each, the calls
alternating), the compact call's count / scan / fill apart, both pools'
bytes and the records.  Both layouts' record counts must agree -- asserted.
"""
import argparse
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

ap = argparse.ArgumentParser()
ap.add_argument("--sws", type=int, default=10000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def stat(v):
    return {"median": statistics.median(v), "best": min(v)}


topo = T.fabric(args.sws, full=True)
runs = []
with LinkState(devices=[0]) as ls:
    ls.updateAdjacencyDatabases(topo.lsdb)
    ls.prefetchAllSources()
    names, rp = ls.flatten()[:2]
    n = len(names)
    ptr = np.arange(n + 1, dtype=np.uint32)
    nodes = np.arange(n, dtype=np.uint32)
    mp = C.c_void_p(N.lib.ls_all_sources_plan(ls._h))
    for lfa in (False, True):
        tiled, compact, phases, pools, recs = [], [], [], {}, {}
        for rep in range(args.reps + 1):  # (the first of each: warm-up, pools allocated)
            for layout in (False, True):
                n_rec, ms = ls.allSourcesRouteRecords(ptr, nodes, lfa, compact=layout)
                recs[layout] = n_rec
                pools[layout] = ls.allSourcesRouteRecordPool()
                if layout:
                    ph = (C.c_double * 3)()
                    N.raise_for(N.lib.spf_mplan_route_records_timing(mp, ph), N.global_error())
                if rep:
                    (compact if layout else tiled).append(ms)
                    if layout:
                        phases.append(list(ph))
        assert recs[False] == recs[True]
        assert pools[False][0] == 0 and pools[True][0] == 1
        assert pools[True][2] == pools[False][2] == 8 * recs[True]
        runs.append({
            "lfa": lfa, "records": recs[True], "record_bytes": pools[True][2],
            "tiled_kernel_ms": stat(tiled), "compact_kernel_ms": stat(compact),
            "compact_count_ms": stat([p[0] for p in phases]), "compact_scan_ms": stat([p[1] for p in phases]),
            "compact_fill_ms": stat([p[2] for p in phases]),
            "tiled_pool_bytes": pools[False][1], "compact_pool_bytes": pools[True][1],
            "header_bytes": 8 * n * n})
doc = {"workload": topo.name, "nodes": n, "directed_edges": int(rp[n]), "reps": args.reps,
       "stage_records": int(N.lib.spf_route_compact_stage()), "runs": runs}
text = json.dumps(doc, indent=1)
print(text)
if args.out:
    Path(args.out).write_text(text + "\n")
