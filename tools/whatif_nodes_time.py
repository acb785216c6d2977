"""Time what-if batches for node failures on the ba_whatif graph
(Barabasi-Albert N=250000 m=4 seed=1, source "0"), one GPU: every node down,
every node drained, and the single-link batch of the same run beside them.

    python tools/whatif_nodes_time.py [--n 250000] [--cpu-sample 256]

Per batch (links, down, drain): 5 warm-up and 20 timed spf_whatif_execute
(HIP events, spf_whatif_timing: base / failures ms), stats() (hot, big), then
5 warm-up and 20 timed spf_whatif_changes (count / scan / fill ms, entries,
pool bytes).  SPF_WHATIF_DEBUG is set, so each plan's register / team line
goes to stderr.  With --cpu-sample K > 0 the CPU side is timed too: the
oracle's full runSpf per node (on a fresh LinkState with the node deleted or
drained; building it is not timed) over K evenly spaced nodes on
--cpu-workers (16) processes, scaled to the batch -- the printed cpu_ms_scaled is that estimate,
not a measurement of the whole batch.  --cpu-only prints only that (no GPU).
Prints one JSON line per batch.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
os.environ.setdefault("SPF_WHATIF_DEBUG", "1")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=250_000)
ap.add_argument("--cpu-sample", type=int, default=0)
ap.add_argument("--cpu-only", action="store_true")
ap.add_argument("--cpu-workers", type=int, default=16)
args = ap.parse_args()

WARM, REPS = 5, 20
_cpu = {}


def _cpu_init(n):
    from openr_amd import topology as T

    _cpu["lsdb"] = T.barabasi_albert(n, 4, seed=1).lsdb


def _cpu_run(job):
    import whatif_nodes as WN

    name, kind = job
    orc = WN.failed_oracle(_cpu["lsdb"], name, kind)  # the changed LSDB: not timed
    t0 = time.perf_counter()
    orc.time_sources(["0"])  # runSpf("0") on it
    return time.perf_counter() - t0


def cpu_scaled_ms(names, nodes, kind, k):
    """The oracle's re-runs of k evenly spaced nodes of the batch over the
    worker processes, as ms for the whole batch: scaled by len(nodes) / k."""
    from multiprocessing import Pool

    pick = [names[int(nodes[i])] for i in range(0, len(nodes), max(1, len(nodes) // k))][:k]
    with Pool(args.cpu_workers, _cpu_init, (args.n,)) as pool:
        each = pool.map(_cpu_run, [(x, kind) for x in pick], chunksize=1)
    # each re-run timed on its own in its worker: the batch's wall time on that many cores
    return 1e3 * sum(each) / args.cpu_workers * len(nodes) / len(pick), len(pick)


def cpu_only() -> None:
    names = sorted(str(i) for i in range(args.n))
    nodes = [v for v in range(args.n) if names[v] != "0"]
    for kind in ("down", "drain"):
        ms, k = cpu_scaled_ms(names, nodes, kind, max(1, args.cpu_sample))
        print(json.dumps({"kind": kind, "n_fail": len(nodes), "cpu_ms_scaled": ms, "cpu_sample": k,
                          "cpu_workers": args.cpu_workers}), flush=True)


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
    for kind in ("link", "down", "drain"):
        plan = eng.whatif_plan(s) if kind == "link" else eng.whatif_node_plan(s, kind=kind)
        d_out = DeviceArray(max(1, plan.n_fail), DIGEST_DTYPE)
        d_base = DeviceArray(1, DIGEST_DTYPE)
        for _ in range(WARM):
            plan.execute(d_out.ptr, d_base.ptr)
        hot, big = plan.stats()
        plan.enable_timing(REPS)
        for _ in range(REPS):
            plan.execute(d_out.ptr, d_base.ptr)
        base_ms, fail_ms, n = plan.timing()
        digests = d_out.numpy()[: plan.n_fail]
        base = d_base.numpy()[0]
        parts = []
        for k in range(WARM + REPS):
            ch = plan.changes()
            if k >= WARM:
                parts.append(ch.timing())
        med = [statistics.median(p[i] for p in parts) for i in range(3)]
        out = {"kind": kind, "n_fail": plan.n_fail, "base_ms": base_ms / n, "failures_ms": fail_ms / n,
               "us_per_failure": 1e3 * fail_ms / n / max(1, plan.n_fail), "hot": hot, "big": big,
               "changed": int((digests["hash"] != base["hash"]).sum()),
               "count_ms": med[0], "scan_ms": med[1], "fill_ms": med[2],
               "n_entries": ch.n_entries, "pool_bytes": ch.pool_bytes, "W": ch.W,
               "digests_equal_execute": bool(np.array_equal(digests, ch.digests))}
        if args.cpu_sample and kind != "link":
            out["cpu_ms_scaled"], out["cpu_sample"] = cpu_scaled_ms(names, plan.nodes, kind,
                                                                     args.cpu_sample)
            out["cpu_workers"] = args.cpu_workers
        print(json.dumps(out), flush=True)
        d_out.free()
        d_base.free()
        plan.close()
    eng.close()


if __name__ == "__main__":
    cpu_only() if args.cpu_only else main()
