"""Time every node's prefix routes (spf_mplan_prefix_routes) on fabric_full,
one GPU: every node's loopback plus a few hundred anycast prefixes with mixed
preferences and a few drained advertisers.  Beside it, the same run's
spf_mplan_route_records(SPF_ROUTE_COMPACT) over the me-independent sets (set p
= every advertiser of prefix p): the yardstick -- the same count / scan / fill
shape without the per-me selection.

    python tools/prefix_routes_time.py [--sws 10000] [--anycast 300] [--reps 5] [--lfa]

Prints one JSON line: both calls' count / scan / fill ms (median of --reps
after one warm-up call each, the calls alternating) and kernel_ms, the record
counts, the prefix pools' bytes, the statuses' counts and the ratio of the two
kernel_ms medians.
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
from openr_amd.link_state import LinkState, PrefixTable  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sws", type=int, default=10000)
ap.add_argument("--anycast", type=int, default=300)
ap.add_argument("--drained", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--lfa", action="store_true")
args = ap.parse_args()

topo = T.fabric(args.sws, full=True)
rng = np.random.default_rng(1)
names = sorted(topo.nodes)
n = len(names)
# a few drained nodes, every one an anycast advertiser below
drained = rng.choice(n, args.drained, replace=False)
topo.lsdb.dbs["is_overloaded"][[topo.nodes.index(names[int(v)]) for v in drained]] = 1
ptr, node, pp, sp, dist, mn = [0], [], [], [], [], []
for v in range(n):  # loopbacks
    node.append(v), pp.append(0), sp.append(0), dist.append(0), mn.append(0)
    ptr.append(len(node))
for p in range(args.anycast):
    k = int(rng.integers(2, 9))
    adv = rng.choice(n, k, replace=False).tolist()
    if p < len(drained):
        adv[0] = int(drained[p])
    for v in dict.fromkeys(adv):
        node.append(v), pp.append(int(rng.integers(0, 3))), sp.append(int(rng.integers(0, 2)))
        dist.append(int(rng.integers(0, 3))), mn.append(int(rng.integers(0, 3)))
    ptr.append(len(node))
table = PrefixTable(np.asarray(ptr, np.uint32), np.asarray(node, np.uint32), np.asarray(pp, np.int32),
                    np.asarray(sp, np.int32), np.asarray(dist, np.int32), np.asarray(mn, np.int64))
with LinkState(devices=[0]) as ls:
    ls.updateAdjacencyDatabases(topo.lsdb)
    ls.prefetchAllSources()
    flat = ls.flatten()
    assert list(flat[0]) == names and int(flat[5].sum()) == len(drained)
    mp = C.c_void_p(N.lib.ls_all_sources_plan(ls._h))
    ms3 = (C.c_double * 3)()
    pfx, rec = [], []
    for rep in range(args.reps + 1):  # (the first of each: warm-up, pools allocated)
        n_pfx, pool_bytes, ms = ls.allSourcesPrefixRoutes(table, args.lfa)
        N.raise_for(N.lib.spf_mplan_prefix_routes_timing(mp, ms3), N.global_error())
        a = (ms, *ms3)
        n_rec, ms2 = ls.allSourcesRouteRecords(table.pfx_ptr, table.node, args.lfa, compact=True)
        N.raise_for(N.lib.spf_mplan_route_records_timing(mp, ms3), N.global_error())
        if rep:
            pfx.append(a)
            rec.append((ms2, *ms3))
    status = np.zeros(5, np.int64)
    ls.allSourcesPrefixRoutes(table, args.lfa)
    for t in range(n):
        info = ls.allSourcesPrefixRouteDb(t)[0]
        status += np.bincount((info >> np.uint64(56)).astype(np.int64), minlength=5)
    med = lambda rows, k: statistics.median(r[k] for r in rows)  # noqa: E731
    stages = lambda rows: {"kernel_ms": med(rows, 0), "count_ms": med(rows, 1), "scan_ms": med(rows, 2),  # noqa: E731
                           "fill_ms": med(rows, 3), "best_kernel_ms": min(r[0] for r in rows)}
    print(json.dumps({
        "workload": topo.name, "nodes": n, "directed_edges": int(flat[1][n]), "lfa": bool(args.lfa),
        "prefixes": len(ptr) - 1, "entries": len(node), "drained": len(drained),
        "prefix_routes": stages(pfx), "route_records_compact": stages(rec),
        "ratio_prefix_over_records": med(pfx, 0) / med(rec, 0),
        "prefix_records": n_pfx, "route_records": n_rec, "prefix_pool_bytes": pool_bytes,
        "prefix_record_bytes": 8 * n_pfx,
        "status_counts": dict(zip(["none", "self", "no_nexthop", "min_nexthop", "route"], status.tolist())),
        "reps": args.reps}))
