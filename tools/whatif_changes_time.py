"""Time what-if batches and their change lists on the ba_whatif graph
(Barabasi-Albert N=250000 m=4 seed=1, source "0", every up link), one GPU.

    python tools/whatif_changes_time.py [--other TREE] [--rounds 3]

One round = a fresh process per tree (this one, and --other: another built
checkout of the project, e.g. the parent commit, run first), interleaved round
by round on the same device.  Each process: 5 warm-up and 20 timed
spf_whatif_execute (HIP events, spf_whatif_timing), then -- where the library
has spf_whatif_changes -- 5 warm-up and 20 timed calls of it (HIP events
around count pass, scan and fill pass, spf_whatif_changes_timing), the
entries, pool bytes and W, and spf_debug_copy_bandwidth.  SPF_WHATIF_DEBUG is
set, so the plan's register / team line goes to stderr.  Prints one JSON line
per process, then a summary line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--other", default=None, help="another built checkout to interleave with")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
ap.add_argument("--n", type=int, default=250_000)
args = ap.parse_args()

WARM, REPS = 5, 20


def child(tree: str) -> None:
    sys.path.insert(0, tree)
    import numpy as np

    from openr_amd import _native as N
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
    plan = eng.whatif_plan(names.index("0"))
    d_out = DeviceArray(plan.n_fail, DIGEST_DTYPE)
    d_base = DeviceArray(1, DIGEST_DTYPE)
    out = {"tree": tree, "n_fail": plan.n_fail}
    for _ in range(WARM):
        plan.execute(d_out.ptr, d_base.ptr)
    plan.stats()
    plan.enable_timing(REPS)
    for _ in range(REPS):
        plan.execute(d_out.ptr, d_base.ptr)
    base_ms, fail_ms, n = plan.timing()
    out["execute_base_ms"], out["execute_fail_ms"] = base_ms / n, fail_ms / n
    digests = d_out.numpy()
    if hasattr(N.lib, "spf_whatif_changes"):
        ne, nb, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        parts = []
        for k in range(WARM + REPS):
            eng._err(N.lib.spf_whatif_changes(plan._h, C.c_void_p(d_out.ptr), C.c_void_p(d_base.ptr),
                                              C.byref(ne), C.byref(nb), C.byref(ms), None))
            t = (C.c_double * 3)()
            eng._err(N.lib.spf_whatif_changes_timing(plan._h, t))
            if k >= WARM:
                parts.append((t[0], t[1], t[2]))
        w = C.c_uint32()
        eng._err(N.lib.spf_whatif_changes_buffers(plan._h, None, None, None, None, C.byref(w), None))
        med = [statistics.median(p[i] for p in parts) for i in range(3)]
        out.update(count_ms=med[0], scan_ms=med[1], fill_ms=med[2], changes_ms=sum(med),
                   n_entries=int(ne.value), pool_bytes=int(nb.value), W=int(w.value),
                   digests_equal_execute=bool(np.array_equal(digests, d_out.numpy())))
    out["copy_gbps"] = eng.copy_bandwidth(1 << 30, 10)
    print(json.dumps(out), flush=True)
    eng.close()


if args.child:
    child(args.child)
    sys.exit(0)

here = str(Path(__file__).resolve().parents[1])
trees = ([str(Path(args.other).resolve())] if args.other else []) + [here]
rows = []
for r in range(args.rounds):
    for tree in trees:
        env = dict(os.environ, SPF_WHATIF_DEBUG="1")
        p = subprocess.run([sys.executable, __file__, "--child", tree, "--n", str(args.n)], env=env,
                           stdout=subprocess.PIPE, text=True, timeout=600)
        if p.returncode != 0:  # nothing more is started on the device after a failed run
            sys.exit(f"round {r}, {tree}: exit status {p.returncode}")
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
summary = {}
for tree in trees:
    mine = [x for x in rows if x["tree"] == tree]
    fm = [x["execute_fail_ms"] for x in mine]
    summary[tree] = {"execute_fail_ms": fm, "spread_ms": max(fm) - min(fm)}
    if "changes_ms" in mine[0]:
        for k in ("count_ms", "scan_ms", "fill_ms", "changes_ms"):
            summary[tree][k] = statistics.median(x[k] for x in mine)
        x = mine[-1]
        copy_ms = x["pool_bytes"] / (x["copy_gbps"] * 1e6)
        summary[tree].update(n_entries=x["n_entries"], pool_bytes=x["pool_bytes"], W=x["W"],
                             copy_gbps=x["copy_gbps"],
                             yardstick_ms=2 * statistics.median(fm) + copy_ms)
print(json.dumps({"summary": summary}), flush=True)
