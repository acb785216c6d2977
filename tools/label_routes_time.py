"""Time every node's node-label MPLS routes (spf_mplan_label_routes) on
fabric_full, one GPU, against the existing materialisation over the same
selections: spf_mplan_route_records with the n single-node sets (set v = {v}).
With a distinct label per node, label = node id + 1, label group g is the set
{g}: both calls select the same next hops, so their record counts must agree
apart from the routes a node would have to itself (me == owner: no records in
the label pool) -- asserted below.

    python tools/label_routes_time.py [--sws 10000] [--reps 5] [--lfa]

Prints one JSON line: both kernel_ms (median and best of --reps after one
warm-up call each, the calls alternating), the record counts, the label
pools' bytes and the existing call's pool (record slots + headers).
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
ap.add_argument("--lfa", action="store_true")
args = ap.parse_args()

topo = T.fabric(args.sws, full=True)
rank = {s: i for i, s in enumerate(sorted(topo.nodes))}
topo.lsdb.dbs["node_label"] = np.array([rank[s] + 1 for s in topo.nodes], np.int32)
with LinkState(devices=[0]) as ls:
    ls.updateAdjacencyDatabases(topo.lsdb)
    ls.prefetchAllSources()
    names, rp = ls.flatten()[:2]
    n = len(names)
    assert list(names) == sorted(topo.nodes)
    ptr = np.arange(n + 1, dtype=np.uint32)
    nodes = np.arange(n, dtype=np.uint32)
    lab_ms, rec_ms = [], []
    for rep in range(args.reps + 1):  # (the first of each: warm-up, pools allocated)
        labels, n_lab, pool_bytes, ms = ls.allSourcesLabelRoutes(args.lfa)
        n_rec, ms2 = ls.allSourcesRouteRecords(ptr, nodes, args.lfa)
        if rep:
            lab_ms.append(ms)
            rec_ms.append(ms2)
    assert labels.tolist() == list(range(1, n + 1))
    # the existing call's records of route me -> {me}, from its headers
    mp = N.lib.ls_all_sources_plan(ls._h)
    hdr = np.zeros(n, np.uint64)
    cnt = C.c_uint64()
    own = 0
    for t in range(n):
        N.raise_for(N.lib.spf_mplan_route_db(C.c_void_p(mp), t, N.ptr(hdr, C.c_uint64), None, 0,
                                             C.byref(cnt)), N.global_error())
        own += int(hdr[t] >> np.uint64(32))
    assert n_lab == n_rec - own, (n_lab, n_rec, own)
    # spf_mplan_route_records' pool: per me ceil(sets / 1024) * 1024 * deg(me)
    # record slots, plus a header per (me, set)
    tiles = (n + 1023) // 1024 * 1024
    old_pool = 8 * tiles * int(rp[n]) + 8 * n * n
    print(json.dumps({
        "workload": topo.name, "nodes": n, "directed_edges": int(rp[n]), "lfa": bool(args.lfa),
        "label_routes_kernel_ms": {"median": statistics.median(lab_ms), "best": min(lab_ms)},
        "route_records_kernel_ms": {"median": statistics.median(rec_ms), "best": min(rec_ms)},
        "label_records": n_lab, "route_records": n_rec, "route_records_me_to_me": own,
        "label_pool_bytes": pool_bytes, "label_record_bytes": 8 * n_lab,
        "route_records_pool_bytes": old_pool, "reps": args.reps}))
