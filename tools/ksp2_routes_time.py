"""Time every node's KSP2_ED_ECMP routes (spf_ksp2_routes) on the WAN graph,
one GPU, beside the KSP2 pass that produced the paths it reads: all nodes as
sources, one destination set per node (set v = {v}), label = node id + 1.

    python tools/ksp2_routes_time.py [--nodes 2000] [--chords 1000] [--reps 5]

One process: a sizing execute, then per repetition one timed spf_ksp2_execute
(HIP events: the k = 1 SPF kernels and the KSP2 kernel, spf_ksp2_timing) and
one spf_ksp2_routes (HIP events: count, scan, fill); the first repetition of
each is the warm-up (code objects loaded, pools allocated) and is dropped.
Prints one JSON line: medians and bests, the totals and the pools' bytes.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from openr_amd import topology as T  # noqa: E402
from openr_amd.engine import SpfEngine, graph_from_lsdb  # noqa: E402
from openr_amd.hiprt import DeviceArray, synchronize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=2000)
ap.add_argument("--chords", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

topo = T.wan(args.nodes, args.chords, seed=1)
names, rp, col, met, lid, ovl = graph_from_lsdb(topo.lsdb)
n = len(names)
eng = SpfEngine(0)
eng.load(rp, col, met, lid, ovl)
plan = eng.ksp2_plan(list(range(n)))
d_pairs = DeviceArray(4 * n * n, np.uint32)
d_cnt = DeviceArray(4, np.uint64)
words = 1 << 20
d_pool = DeviceArray(words, np.uint32)
plan.execute(d_pairs.ptr, d_pool.ptr, words, d_cnt.ptr)  # sizing (the counter counts past an overflow)
synchronize()
words = int(int(d_cnt.numpy()[0]) * 1.05) + (1 << 22)
d_pool.free()
d_pool = DeviceArray(words, np.uint32)

set_ptr = np.arange(n + 1, dtype=np.uint32)
set_nodes = np.arange(n, dtype=np.uint32)
label = np.arange(1, n + 1, dtype=np.int32)
spf_ms, ksp_ms, rt_ms, parts = [], [], [], []
totals = None
for rep in range(args.reps + 1):
    plan.enable_timing(1)
    plan.execute(d_pairs.ptr, d_pool.ptr, words, d_cnt.ptr)
    synchronize()
    if int(d_cnt.numpy()[2]) & 1:
        raise SystemExit("KSP2 path pool overflowed")
    a, b, _ = plan.timing()
    hops, lab_words, nbytes, ms = plan.routes(d_pairs.ptr, d_pool.ptr, set_ptr, set_nodes, label)
    if totals is not None:
        assert totals == (hops, lab_words, nbytes)
    totals = (hops, lab_words, nbytes)
    if rep:
        spf_ms.append(a)
        ksp_ms.append(b)
        rt_ms.append(ms)
        parts.append(plan.routes_timing())


def stat(v):
    return {"median": statistics.median(v), "best": min(v)}


print(json.dumps({
    "workload": topo.name, "nodes": n, "directed_edges": int(rp[n]), "sets": n, "routes": n * n,
    "ksp2_spf_kernel_ms": stat(spf_ms), "ksp2_kernel_ms": stat(ksp_ms),
    "routes_kernel_ms": stat(rt_ms),
    "routes_count_ms": stat([p[0] for p in parts]), "routes_scan_ms": stat([p[1] for p in parts]),
    "routes_fill_ms": stat([p[2] for p in parts]),
    "next_hops": totals[0], "label_words": totals[1], "pool_bytes": totals[2],
    "path_pool_words": int(d_cnt.numpy()[0]), "reps": args.reps}))
eng.close()
