"""Time what-if impact by destination on the ba_whatif graph (Barabasi-Albert
N=250000 m=4 seed=1, source "0"), one GPU, one process: the link plan over
every link, its change lists, the route lists over them, then
spf_whatif_by_node and spf_whatif_by_set over the resident pools.

    python tools/whatif_impact_time.py [--n 250000]

Sets: one loopback set per node, plus 512 seeded anycast sets of 2 to 64
members (seed 1), as tools/whatif_routes_time.py.  2 warm-up and 5 timed rounds
of the four calls; per phase the median.  Nothing is read back inside a round.
Prints one JSON line and appends it to
profiles/whatif_impact/whatif_impact_time.jsonl: per flavour the entries, the
pool bytes and the count / scan / fill ms; beside them the same run's
spf_whatif_changes and spf_whatif_routes kernel ms and
spf_debug_copy_bandwidth; the ratios of each pass to the list pass and to the
route pass; and the count pass's achieved bytes/s over total x (12 + 4 W)
bytes read, as a fraction of the copy rate.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=250_000)
args = ap.parse_args()

WARM, REPS = 2, 5


def main() -> None:
    import numpy as np

    from openr_amd import _native as N
    from openr_amd import topology as T
    from openr_amd.engine import SpfEngine
    from openr_amd.link_state import LinkState

    topo = T.barabasi_albert(args.n, 4, seed=1)
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names, rp, col, met, lid, ovl = ls.flatten()
    eng = SpfEngine(0)
    eng.load(rp, col, met, lid, ovl)
    s = names.index("0")
    n_nodes = len(names)
    rng = np.random.default_rng(1)
    anycast = [rng.choice(n_nodes, int(rng.integers(2, 65)), replace=False) for _ in range(512)]
    sizes = np.concatenate([np.ones(n_nodes, np.int64), [len(x) for x in anycast]])
    set_ptr = np.zeros(len(sizes) + 1, np.uint32)
    set_ptr[1:] = np.cumsum(sizes)
    set_nodes = np.ascontiguousarray(np.concatenate([np.arange(n_nodes)] + anycast), np.uint32)
    n_sets = len(sizes)
    plan = eng.whatif_plan(s)
    h = plan._h

    def call(fn, *lead):
        n, nbytes, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        eng._err(fn(h, *lead, C.byref(n), C.byref(nbytes), C.byref(ms), None))
        return int(n.value), int(nbytes.value), ms.value

    def phases(which):
        ms = (C.c_double * 3)()
        eng._err(N.lib.spf_whatif_impact_timing(h, which, ms))
        return list(ms)

    lists_ms, routes_ms, node_parts, set_parts = [], [], [], []
    for k in range(WARM + REPS):
        lists = call(N.lib.spf_whatif_changes, None, None)
        routes = call(N.lib.spf_whatif_routes, N.ptr(set_ptr), N.ptr(set_nodes), n_sets)
        by_node = call(N.lib.spf_whatif_by_node)
        by_set = call(N.lib.spf_whatif_by_set)
        if k >= WARM:
            lists_ms.append(lists[2])
            routes_ms.append(routes[2])
            node_parts.append(phases(0))
            set_parts.append(phases(1))
    w = C.c_uint32()
    eng._err(N.lib.spf_whatif_changes_buffers(h, None, None, None, None, C.byref(w), None))
    W = int(w.value)
    copy_gbps = eng.copy_bandwidth(1 << 30, 10)
    out = {"graph": f"ba{args.n}_m4_seed1", "src": "0", "n_fail": plan.n_fail, "n_nodes": n_nodes,
           "n_sets": n_sets, "set_members": int(set_ptr[-1]), "W": W, "reps": REPS,
           "list_entries": lists[0], "list_pool_bytes": lists[1],
           "route_entries": routes[0], "route_pool_bytes": routes[1],
           "changes_kernel_ms": statistics.median(lists_ms), "changes_kernel_ms_min": min(lists_ms),
           "changes_kernel_ms_max": max(lists_ms),
           "routes_kernel_ms": statistics.median(routes_ms), "routes_kernel_ms_min": min(routes_ms),
           "routes_kernel_ms_max": max(routes_ms), "copy_gbps": copy_gbps}
    for name, got, parts in (("by_node", by_node, node_parts), ("by_set", by_set, set_parts)):
        med = [statistics.median(p[i] for p in parts) for i in range(3)]
        tot = [sum(p) for p in parts]
        read = got[0] * (12 + 4 * W)  # the count pass: key, metric and W words of every entry
        gbps = read / max(med[0], 1e-9) / 1e6
        out[name] = {"entries": got[0], "pool_bytes": got[1], "count_ms": med[0], "scan_ms": med[1],
                     "fill_ms": med[2], "ms": statistics.median(tot), "ms_min": min(tot),
                     "ms_max": max(tot), "ratio_to_changes": statistics.median(tot) / out["changes_kernel_ms"],
                     "ratio_to_routes": statistics.median(tot) / out["routes_kernel_ms"],
                     "count_read_bytes": read, "count_gbps": gbps,
                     "count_frac_of_copy": gbps / copy_gbps}
    line = json.dumps(out)
    print(line, flush=True)
    log = ROOT / "profiles" / "whatif_impact" / "whatif_impact_time.jsonl"
    log.parent.mkdir(parents=True, exist_ok=True)
    with log.open("a") as f:
        f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
