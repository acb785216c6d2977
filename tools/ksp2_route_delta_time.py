"""Time the KSP2 route-database delta and its payload (spf_ksp2_route_delta,
spf_ksp2_route_update) on the WAN graph, one GPU, next to the rebuild it
compares (spf_ksp2_routes): all nodes as sources, one loopback set per node
plus a few anycast sets, label = node id + 1.

    python tools/ksp2_route_delta_time.py [--nodes 2000] [--chords 1000] [--anycast 8] [--reps 3]

Each rep does an unchanged pass (routes, snapshot, routes, delta + update: every
list empty) and a one-link flap through the LinkState's row-patch path (routes,
snapshot, the first adjacency of one node withdrawn or advertised again, routes,
delta + update).  Prints one JSON line: median and best HIP-event kernel ms of
the delta and the update with their count / scan / fill phases, the entries and
the payload pool's bytes, the spf_ksp2_routes kernel ms of the same run, the
bytes the delta must read (both generations' pools) with the GB/s that makes
and spf_debug_copy_bandwidth for that byte count, and the device memory a live
snapshot holds.
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
ap.add_argument("--nodes", type=int, default=2000)
ap.add_argument("--chords", type=int, default=1000)
ap.add_argument("--anycast", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

topo = T.wan(args.nodes, args.chords, seed=1)
topo.lsdb.dbs["node_label"] = np.arange(1, len(topo.nodes) + 1, dtype=np.int32)
rng = np.random.default_rng(11)


def stat(v):
    return {"median": statistics.median(v), "best": min(v)}


with LinkState(device=0) as ls:
    ls.updateAdjacencyDatabases(topo.lsdb)
    dbs = {d.thisNodeName: d for d in unpack(topo.lsdb)}
    names, rp = ls.flatten()[:2]
    n = len(names)
    any_sets = [rng.choice(n, int(rng.integers(2, 5)), replace=False).astype(np.uint32) for _ in range(args.anycast)]
    set_nodes = np.concatenate([np.arange(n, dtype=np.uint32)] + any_sets)
    set_ptr = np.concatenate([np.arange(n + 1), n + np.cumsum([len(s) for s in any_sets])]).astype(np.uint32)
    n_sets = len(set_ptr) - 1
    flapper = max(dbs, key=lambda s: (len(dbs[s].adjacencies), s))  # a well-connected node

    def delta_raw(snap):
        """(delta totals, update totals, pool bytes, the six phase ms) without reading the lists back"""
        plan = ls._k2r[0].plan
        lh = ls.linkValueHashes()
        tot, utot, nbytes = np.zeros(3, np.uint64), np.zeros(3, np.uint64), C.c_uint64()
        plan._eng._err(N.lib.spf_ksp2_route_delta(plan._h, snap._h, N.ptr(lh, C.c_uint64), len(lh),
                                                  N.ptr(tot, C.c_uint64), None))
        plan._eng._err(N.lib.spf_ksp2_route_update(plan._h, N.ptr(utot, C.c_uint64), C.byref(nbytes), None))
        return [int(v) for v in tot], [int(v) for v in utot], int(nbytes.value), plan.route_delta_timing()

    same, flap, rt_ms, pools = [], [], [], []
    flap_tot = flap_utot = None
    flap_bytes = held = 0
    held_adj = None
    for rep in range(args.reps + 1):  # (the first: warm-up)
        _, _, pool0, ms0 = ls.allSourcesKsp2Routes(set_ptr, set_nodes)
        snap = ls.allSourcesKsp2RouteSnapshot()
        held = snap.bytes()
        _, _, pool1, ms1 = ls.allSourcesKsp2Routes(set_ptr, set_nodes)
        tot, utot, _, ph = delta_raw(snap)
        assert tot[:2] == [0, 0] and utot == [0, 0, 0] and pool1 == pool0
        snap.close()
        snap = ls.allSourcesKsp2RouteSnapshot()
        if held_adj is None:
            held_adj = dbs[flapper].adjacencies.pop(0)
        else:
            dbs[flapper].adjacencies.insert(0, held_adj)
            held_adj = None
        ls.updateAdjacencyDatabase(copy.deepcopy(dbs[flapper]))
        _, _, pool2, ms2 = ls.allSourcesKsp2Routes(set_ptr, set_nodes)
        ftot, futot, fbytes, fph = delta_raw(snap)
        assert ftot[0] + ftot[1] > 0
        snap.close()
        if rep:
            same.append(ph)
            flap.append(fph)
            rt_ms += [ms0, ms1, ms2]
            pools = [pool1, pool2]
            flap_tot, flap_utot, flap_bytes = ftot, futot, fbytes
    read_bytes = 2 * pools[0]  # the unchanged pass: both generations' pools, once each
    gbs = C.c_double()
    N.raise_for(N.lib.spf_debug_copy_bandwidth(C.c_void_p(N.lib.ls_engine(ls._h)), read_bytes // 2, 3,
                                               C.byref(gbs)), N.global_error())
    med_same = statistics.median(sum(p[:3]) for p in same)
    med_routes = statistics.median(rt_ms)
    phases = ("count", "scan", "fill")
    print(json.dumps({
        "workload": topo.name, "nodes": n, "directed_edges": int(rp[n]), "sets": n_sets, "routes": n * n_sets,
        "routes_kernel_ms": stat(rt_ms),
        "delta_unchanged_kernel_ms": stat([sum(p[:3]) for p in same]),
        "delta_unchanged_phase_ms": {k: stat([p[i] for p in same]) for i, k in enumerate(phases)},
        "delta_flap_kernel_ms": stat([sum(p[:3]) for p in flap]),
        "delta_flap_phase_ms": {k: stat([p[i] for p in flap]) for i, k in enumerate(phases)},
        "update_flap_kernel_ms": stat([sum(p[3:]) for p in flap]),
        "update_flap_phase_ms": {k: stat([p[3 + i] for p in flap]) for i, k in enumerate(phases)},
        "delta_over_routes": med_same / med_routes,
        "delta_read_bytes": read_bytes, "delta_read_gbs": read_bytes / med_same / 1e6,
        "copy_bandwidth_gbs_same_bytes_moved": gbs.value,
        "fraction_of_copy_rate": read_bytes / med_same / 1e6 / gbs.value,
        "flap": {"node": flapper, "updates": flap_tot[0], "deletes": flap_tot[1], "matched_as_sets": flap_tot[2],
                 "update_records": flap_utot[1], "update_label_words": flap_utot[2],
                 "payload_pool_bytes": flap_bytes, "route_pool_bytes": pools[1]},
        "snapshot_device_bytes": held, "reps": args.reps}))
