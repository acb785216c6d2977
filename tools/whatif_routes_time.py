"""Time the what-if route pass on the ba_whatif graph (Barabasi-Albert N=250000
m=4 seed=1, source "0"), one GPU, one process: the link plan over every link,
its change lists, then spf_whatif_routes over them.

    python tools/whatif_routes_time.py [--n 250000]

Sets: one loopback set per node, plus 512 seeded anycast sets of 2 to 64
members (seed 1).  2 warm-up and 5 timed calls of each; per phase the median.
Prints one JSON line and appends it to
profiles/whatif_routes/whatif_routes_time.jsonl: entries, pool bytes, the four
phases of the route pass (base routes + table, count, scan, fill), and beside
them the same run's spf_whatif_changes kernel_ms with `ratio_to_changes` = the
route pass as a multiple of the list pass.
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
    lists_ms, parts = [], []
    for k in range(WARM + REPS):
        ch = plan.changes()
        rt = ch.routes(sets)
        if k >= WARM:
            lists_ms.append(ch.kernel_ms)
            parts.append(rt.timing())
    med = [statistics.median(p[i] for p in parts) for i in range(4)]
    tot = [sum(p) for p in parts]
    out = {"graph": f"ba{args.n}_m4_seed1", "src": "0", "n_fail": plan.n_fail, "n_sets": len(sets),
           "set_members": int(sum(len(x) for x in sets)), "W": rt.W,
           "list_entries": ch.n_entries, "list_pool_bytes": ch.pool_bytes,
           "route_entries": rt.n_entries, "route_pool_bytes": rt.pool_bytes,
           "base_index_ms": med[0], "count_ms": med[1], "scan_ms": med[2], "fill_ms": med[3],
           "routes_ms": statistics.median(tot), "routes_ms_min": min(tot), "routes_ms_max": max(tot),
           "changes_kernel_ms": statistics.median(lists_ms), "changes_kernel_ms_min": min(lists_ms),
           "changes_kernel_ms_max": max(lists_ms), "reps": REPS}
    out["ratio_to_changes"] = out["routes_ms"] / out["changes_kernel_ms"]
    line = json.dumps(out)
    print(line, flush=True)
    log = ROOT / "profiles" / "whatif_routes" / "whatif_routes_time.jsonl"
    log.parent.mkdir(parents=True, exist_ok=True)
    with log.open("a") as f:
        f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
