"""Time what-if batches for link-set failures on the ba_whatif graph
(Barabasi-Albert N=250000 m=4 seed=1, source "0"), one GPU, one process: each
set batch beside the plan of the same failures that predates set plans.

    python tools/whatif_sets_time.py [--n 250000]

Batches, in this order:
  link       every up link (spf_whatif_plan_create)            -- yardstick
  sets1      the same links as one-member sets                 -- ratio to link
  down       every node down (spf_whatif_plan_create_nodes)    -- yardstick
  sets_node  the same nodes as linksFromNode(x) sets           -- ratio to down
  sets4      as many seeded random 4-link sets as there are links (ratio to
             link: the same number of failures, not the same failures)

Per batch: 5 warm-up and 20 timed spf_whatif_execute, each timed on its own
(HIP events, spf_whatif_timing): the median, minimum and maximum of the
failures' ms, stats() (hot, big), then 5 warm-up and 20 timed
spf_whatif_changes (median count / scan / fill ms, entries, pool bytes).
SPF_WHATIF_DEBUG is set, so each plan's register / team line goes to stderr.
Prints one JSON line per batch; a set batch carries `ratio_failures` and
`ratio_changes` to its yardstick and whether its digests equal the
yardstick's.
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
os.environ.setdefault("SPF_WHATIF_DEBUG", "1")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=250_000)
args = ap.parse_args()

WARM, REPS = 5, 20


def main() -> None:
    import numpy as np

    from openr_amd import topology as T
    from openr_amd.engine import DIGEST_DTYPE, SpfEngine
    from openr_amd.hiprt import DeviceArray
    from openr_amd.link_state import LinkState

    topo = T.barabasi_albert(args.n, 4, seed=1)
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names, rp, col, met, lid, ovl = ls.flatten()
    eng = SpfEngine(0)
    eng.load(rp, col, met, lid, ovl)
    s = names.index("0")
    lplan = eng.whatif_plan(s)
    links = lplan.links.copy()
    lplan.close()
    nodes = np.array([v for v in range(len(names)) if v != s], np.uint32)
    rng = np.random.default_rng(7)
    batches = [
        ("link", None, lambda: eng.whatif_plan(s, links)),
        ("sets1", "link", lambda: eng.whatif_set_plan(s, links.reshape(-1, 1))),
        ("down", None, lambda: eng.whatif_node_plan(s, nodes, kind="down")),
        ("sets_node", "down", lambda: eng.whatif_set_plan(
            s, [np.unique(lid[rp[x]: rp[x + 1]]) for x in nodes])),
        ("sets4", "link", lambda: eng.whatif_set_plan(s, rng.choice(links, (len(links), 4)))),
    ]
    seen = {}
    for kind, yard, make in batches:
        plan = make()
        d_out = DeviceArray(max(1, plan.n_fail), DIGEST_DTYPE)
        d_base = DeviceArray(1, DIGEST_DTYPE)
        for _ in range(WARM):
            plan.execute(d_out.ptr, d_base.ptr)
        hot, big = plan.stats()
        plan.enable_timing(1)
        base_ms, fail_ms = [], []
        for _ in range(REPS):
            plan.execute(d_out.ptr, d_base.ptr)
            b, f, _n = plan.timing()
            base_ms.append(b)
            fail_ms.append(f)
        digests = d_out.numpy()[: plan.n_fail].copy()
        parts = []
        for k in range(WARM + REPS):
            ch = plan.changes()
            if k >= WARM:
                parts.append(ch.timing())
        med = [statistics.median(p[i] for p in parts) for i in range(3)]
        tot = [sum(p) for p in parts]
        out = {"kind": kind, "n_fail": plan.n_fail,
               "members": int(plan.set_ptr[-1]) if plan.kind == "sets" else plan.n_fail,
               "base_ms": statistics.median(base_ms), "failures_ms": statistics.median(fail_ms),
               "failures_ms_min": min(fail_ms), "failures_ms_max": max(fail_ms),
               "hot": hot, "big": big, "count_ms": med[0], "scan_ms": med[1], "fill_ms": med[2],
               "changes_ms": statistics.median(tot), "changes_ms_min": min(tot),
               "changes_ms_max": max(tot), "n_entries": ch.n_entries, "pool_bytes": ch.pool_bytes,
               "W": ch.W, "digests_equal_execute": bool(np.array_equal(digests, ch.digests))}
        seen[kind] = (out, digests)
        if yard:
            y, yd = seen[yard]
            out["yardstick"] = yard
            out["ratio_failures"] = out["failures_ms"] / y["failures_ms"]
            out["ratio_changes"] = out["changes_ms"] / y["changes_ms"]
            if kind != "sets4":
                out["digests_equal_yardstick"] = bool(np.array_equal(digests, yd))
                out["entries_equal_yardstick"] = out["n_entries"] == y["n_entries"]
        print(json.dumps(out), flush=True)
        d_out.free()
        d_base.free()
        plan.close()
    eng.close()


if __name__ == "__main__":
    main()
