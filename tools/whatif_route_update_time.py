"""Time the what-if route update on the ba_whatif graph (Barabasi-Albert
N=250000 m=4 seed=1, source "0"), one GPU, one process: the link plan over every
link, its change lists, spf_whatif_routes over them, then
spf_whatif_route_update.

    python tools/whatif_route_update_time.py [--n 250000]

Sets: one loopback set per node, plus 512 seeded anycast sets of 2 to 64
members (seed 1), as tools/whatif_routes_time.py.  2 warm-up and 5 timed calls
of each (HIP events inside the calls); per phase the median.  Prints one JSON
line and appends it to profiles/whatif_route_update/whatif_route_update_time.jsonl:
entries, records, pool bytes, the failures that touch the source's row, the
seven phases of the update, and beside them the same run's spf_whatif_changes
and spf_whatif_routes with `ratio_to_routes` = the update as a multiple of the
route pass.
"""
import argparse
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
PHASES = ("base_records", "touch", "count", "scan", "fill", "record_scan", "records")


def main() -> None:
    import numpy as np

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
    rng = np.random.default_rng(1)
    sets = [[v] for v in range(len(names))]
    sets += [rng.choice(len(names), int(rng.integers(2, 65)), replace=False) for _ in range(512)]
    plan = eng.whatif_plan(s)
    lists_ms, routes_ms, parts = [], [], []
    for k in range(WARM + REPS):
        ch = plan.changes()
        rt = ch.routes(sets)
        up = rt.update()
        if k >= WARM:
            lists_ms.append(ch.kernel_ms)
            routes_ms.append(rt.kernel_ms)
            parts.append(up.timing())
    tot = [sum(p) for p in parts]
    out = {"graph": f"ba{args.n}_m4_seed1", "src": "0", "n_fail": plan.n_fail, "n_sets": len(sets),
           "row_slots": int(rp[s + 1] - rp[s]), "W": rt.W,
           "list_entries": ch.n_entries, "route_entries": rt.n_entries,
           "update_entries": up.n_entries, "update_records": up.n_records,
           "base_records": up.base_records, "update_pool_bytes": up.pool_bytes,
           "touched_failures": up.n_touched,
           **{f"{name}_ms": statistics.median(p[i] for p in parts) for i, name in enumerate(PHASES)},
           "update_ms": statistics.median(tot), "update_ms_min": min(tot), "update_ms_max": max(tot),
           "routes_ms": statistics.median(routes_ms), "routes_ms_min": min(routes_ms),
           "routes_ms_max": max(routes_ms),
           "changes_kernel_ms": statistics.median(lists_ms), "changes_kernel_ms_min": min(lists_ms),
           "changes_kernel_ms_max": max(lists_ms), "reps": REPS}
    out["ratio_to_routes"] = out["update_ms"] / out["routes_ms"]
    line = json.dumps(out)
    print(line, flush=True)
    log = ROOT / "profiles" / "whatif_route_update" / "whatif_route_update_time.jsonl"
    log.parent.mkdir(parents=True, exist_ok=True)
    with log.open("a") as f:
        f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
