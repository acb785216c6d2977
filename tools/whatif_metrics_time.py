"""Time what-if batches for link metric changes on the ba_whatif graph
(Barabasi-Albert N=250000 m=4 seed=1, source "0"), one GPU, one process: each
metric batch beside the link plan on the same links.

    python tools/whatif_metrics_time.py [--n 250000] [--max-ms 400] [--sample 4096]

Batches, in this order, over every up link:
  link   the link failed (spf_whatif_plan_create)                 -- yardstick
  raise  both directions raised to the largest metric 32-bit distances admit
         ((2^32 - 2) / N = 17,179 here, far above every distance of this
         graph): the link plan's affected sets, one more seed edge each
  x2     both directions doubled
  half   both directions halved (at least 1)

A lowered link's affected set is grown over edges of slack <= delta and is
repaired by one workgroup when it passes a wave team's capacity, so a batch of
lowers can take far longer than the others.  Every batch is first executed on
`--sample` links spread evenly over the list; when that projects to more than
`--max-ms` per execute over every link, the batch stays on the sample, and its
line says so (`sampled`, with the link plan on the same sample beside it).

Per batch: 3 warm-up and 10 timed spf_whatif_execute, each timed on its own
(HIP events, spf_whatif_timing): the median, minimum and maximum of the
failures' ms, stats() (hot, big = classified big + wave-team overflows), then
2 warm-up and 5 timed spf_whatif_changes (median count / scan / fill ms,
entries, pool bytes), and the longest list with the size of its affected set D
(tests/whatif_metrics.py: classify / grow, on the host).
SPF_WHATIF_DEBUG is set, so each plan's register / team line goes to stderr.
Prints one JSON line per batch; a metric batch carries `ratio_failures` and
`ratio_changes` to the link plan on the same links.
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
ap.add_argument("--max-ms", type=float, default=400.0)
ap.add_argument("--sample", type=int, default=4096)
args = ap.parse_args()

WARM, REPS, LWARM, LREPS = 3, 10, 2, 5


def main() -> None:
    import numpy as np

    import whatif_metrics as WM
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
    # current metrics per link: (smaller id -> larger, larger -> smaller)
    tail = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    up = tail != col
    w = np.zeros((int(lid.max()) + 1, 2), np.int64)
    w[lid[up], (tail[up] > col[up]).astype(np.int64)] = met[up]
    w = w[links]
    far = 0xFFFFFFFE // len(names)  # the largest metric spf_whatif_plan_create_metrics admits
    table = {
        "raise": np.full_like(w, far),
        "x2": 2 * w,
        "half": np.maximum(1, w // 2),
    }

    def metric_plan(kind, pick):
        return eng.whatif_metric_plan(s, np.column_stack([links[pick], table[kind][pick]]))

    def run(kind, plan):
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
        for k in range(LWARM + LREPS):
            ch = plan.changes()
            if k >= LWARM:
                parts.append(ch.timing())
        med = [statistics.median(p[i] for p in parts) for i in range(3)]
        tot = [sum(p) for p in parts]
        out = {"kind": kind, "n_fail": plan.n_fail, "base_ms": statistics.median(base_ms),
               "failures_ms": statistics.median(fail_ms), "failures_ms_min": min(fail_ms),
               "failures_ms_max": max(fail_ms), "hot": hot, "big": big, "count_ms": med[0],
               "scan_ms": med[1], "fill_ms": med[2], "changes_ms": statistics.median(tot),
               "changes_ms_min": min(tot), "changes_ms_max": max(tot), "n_entries": ch.n_entries,
               "pool_bytes": ch.pool_bytes, "W": ch.W,
               "n_dist_changed": int(digests["n_dist_changed"].astype(np.int64).sum()),
               "n_nh_changed": int(digests["n_nh_changed"].astype(np.int64).sum()),
               "digests_equal_execute": bool(np.array_equal(digests, ch.digests))}
        sizes = np.diff(ch.ptr.astype(np.int64))
        i = int(np.argmax(sizes)) if len(sizes) else 0
        out["longest_list"] = int(sizes[i]) if len(sizes) else 0
        if plan.kind == "metric" and out["longest_list"]:
            l, m_lo, m_hi = (int(x) for x in plan.metric_changes[i])
            dist = plan.base()[0]
            es = np.nonzero((lid == l) & up)[0]  # the link's two directed edges
            pair = (int(es[0]), int(es[1])) if tail[es[0]] < col[es[0]] else (int(es[1]), int(es[0]))
            root, delta = WM.classify(rp, col, met, ovl, dist, s, pair, (m_lo, m_hi))
            out["longest_list_delta"] = int(delta)
            out["longest_list_D"] = len(WM.grow(rp, col, met, ovl, dist, s, pair, (m_lo, m_hi),
                                                root, delta))
        if plan.kind == "metric" and plan.n_fail <= 2 * args.sample:
            out.update(grown_sets(plan))
        d_out.free()
        d_base.free()
        return out

    edge_of = np.zeros((int(lid.max()) + 1, 2), np.int64)  # link -> (edge lo -> hi, edge hi -> lo)
    edge_of[lid[up], (tail[up] > col[up]).astype(np.int64)] = np.nonzero(up)[0]
    drained = ovl.astype(bool)

    def grown_sets(plan, most=600):
        """|D| of the batch's lowers with delta > 0 (at most `most`, evenly
        spaced), grown on the host as the kernels grow it: the largest, and
        how many pass a wave team's 1024 nodes."""
        d = plan.base()[0]
        dist = np.where(d == np.uint64(0xFFFFFFFFFFFFFFFF), -1, d.astype(np.int64))
        ch = plan.metric_changes.astype(np.int64)
        todo = []
        for k in range(2):
            e = edge_of[ch[:, 0], k]
            a, b, w1 = tail[e], col[e], ch[:, 1 + k]
            hot = (w1 < met[e]) & (dist[a] >= 0) & (~drained[a] | (a == s)) & (dist[a] + w1 <= dist[b])
            delta = dist[b] - dist[a] - w1
            todo += [(int(i), int(b[i]), int(delta[i])) for i in np.nonzero(hot & (delta > 0))[0]]
        todo = todo[:: max(1, len(todo) // most)]
        sizes = []
        for i, v, delta in todo:
            pair, new = edge_of[ch[i, 0]], ch[i, 1:3]
            in_d = np.zeros(len(dist), bool)
            in_d[v] = True
            front = np.array([v])
            while len(front):
                front = front[~drained[front]]
                cnt = (rp[front + 1] - rp[front]).astype(np.int64)
                idx = np.repeat(rp[front].astype(np.int64) - np.cumsum(cnt) + cnt, cnt) + np.arange(cnt.sum())
                x, c, wt = np.repeat(front, cnt), col[idx], met[idx].astype(np.int64)
                wt[idx == pair[0]], wt[idx == pair[1]] = new[0], new[1]
                ok = (dist[c] >= 0) & (c != s) & ~in_d[c] & (dist[x] + wt <= dist[c] + delta)
                front = np.unique(c[ok])
                in_d[front] = True
            sizes.append(int(in_d.sum()))
        return {"lowers_grown": len(sizes), "largest_D": max(sizes, default=0),
                "D_over_1024": sum(z > 1024 for z in sizes)}

    every = np.arange(len(links))
    some = every[:: max(1, len(links) // max(1, args.sample))]
    yard = {}
    for kind in ("link", "raise", "x2", "half"):
        make = (lambda pick: eng.whatif_plan(s, links[pick])) if kind == "link" else \
            (lambda pick, kind=kind: metric_plan(kind, pick))
        sampled, sample_ms = False, 0.0
        if kind != "link" and len(some) < len(every):
            # one execute on the sample decides whether every link fits --max-ms
            # (the failures' own ms on the device: a small batch's wall time is
            # mostly the unfailed pass and the launches)
            plan = make(some)
            d = DeviceArray(max(1, plan.n_fail), DIGEST_DTYPE)
            plan.execute(d.ptr)
            plan.stats()
            plan.enable_timing(1)
            plan.execute(d.ptr)
            sample_ms = plan.timing()[1]
            d.free()
            plan.close()
            sampled = sample_ms * len(every) / len(some) > args.max_ms
        plan = make(some if sampled else every)
        out = run(kind, plan)
        plan.close()
        out.update(sampled=sampled, sample_execute_ms=sample_ms)
        if kind == "link":
            yard[False] = out
        else:
            if sampled and True not in yard:  # the link plan on the same sample
                plan = eng.whatif_plan(s, links[some])
                yard[True] = dict(run("link", plan), sampled=True)
                plan.close()
                print(json.dumps(yard[True]), flush=True)
            y = yard[sampled]
            out["ratio_failures"] = out["failures_ms"] / y["failures_ms"]
            out["ratio_changes"] = out["changes_ms"] / y["changes_ms"]
            if kind == "raise":  # reported, not checked: equal wherever no link is a bridge
                out["counts_equal_link_plan"] = (out["n_dist_changed"], out["n_nh_changed"]) == \
                    (y["n_dist_changed"], y["n_nh_changed"])
        print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
