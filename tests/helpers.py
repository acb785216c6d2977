"""Shared test helpers: fixture builders that mirror the reference's test utils."""

from __future__ import annotations

from typing import Dict, List, Sequence, Tuple, Union

from openr_amd.lsdb import AdjacencyDatabase, create_adj_db, create_adjacency

# libstdc++ _Prime_rehash_policy::_M_next_bkt fast path (hashtable_c++0x.cc)
_FAST_BKT = [2, 2, 2, 3, 5, 5, 7, 7, 11, 11, 11, 11, 13, 13]


def gpu_visible() -> bool:
    """Whether the HIP runtime the engine links sees a device, asked of that
    runtime itself.  (torch ships its own copy of the runtime; a test that
    asked torch.cuda.is_available() after the engine's library was loaded left
    every later engine in the process with 'no HIP device visible'.)"""
    import ctypes

    from openr_amd import hiprt

    n = ctypes.c_int(0)
    return hiprt._lib.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0


def libstdcxx_int_map_order(keys: Sequence[int]) -> List[int]:
    """Iteration order of ``std::unordered_map<int, T>`` built from an
    initializer list holding ``keys`` in this order (libstdc++, identity
    std::hash<int>, max_load_factor 1).  Exact for fewer than 14 keys, where
    the constructor's bucket count (_M_next_bkt fast path) never rehashes."""
    n = len(keys)
    if n >= len(_FAST_BKT):
        raise ValueError("emulation covers maps with < 14 keys")
    nb = _FAST_BKT[n]
    order: List[int] = []
    for k in keys:
        b = k % nb
        idx = next((i for i, x in enumerate(order) if x % nb == b), None)
        # a node goes first in its bucket's run; a new bucket's run goes first
        order.insert(0 if idx is None else idx, k)
    return order


def get_link_state_dbs(
    adj_map: Dict[int, Sequence[Union[int, Tuple[int, int]]]]
) -> List[AdjacencyDatabase]:
    """Adjacency databases in the order ``getLinkState`` applies them
    (reference openr/decision/tests/DecisionTestUtils.cpp:16-44): integer node
    names, ifName ``node/adj/k`` (k-th parallel adjacency), label
    ``(node << 16) + adj``, fe80::/192.168 addresses from the neighbour id."""
    dbs = []
    for node in libstdcxx_int_map_order(list(adj_map.keys())):
        assert node < (1 << 16)
        adjs = []
        num_parallel: Dict[int, int] = {}
        for entry in adj_map[node]:
            adj, weight = (entry, 1) if isinstance(entry, int) else entry
            k = num_parallel.get(adj, 0)
            num_parallel[adj] = k + 1
            bottom, top = adj & 0xFF, (adj & 0xFF00) >> 8
            adjs.append(create_adjacency(
                str(adj), f"{node}/{adj}/{k}", f"{adj}/{node}/{k}",
                f"fe80::{top:02x}{bottom:02x}", f"192.168.{top}.{bottom}", weight,
                (node << 16) + adj))
        dbs.append(create_adj_db(str(node), adjs, node))
    return dbs


def link_key(link) -> list:
    """Canonical [n1, if1, n2, if2] (ordered names) of a product Link."""
    (a, b), (c, d) = link.orderedNames
    return [a, b, c, d]


def run_plan(eng, srcs, n, kinds=None):
    """One spf_ksp2_execute of a fresh plan over `srcs` into device buffers
    sized from the plan's own counter (a second run when the first pool was
    too small): (Ksp2Result over the raw pool, the four counters).  `kinds`:
    the plan kinds (Ksp2Plan.info().kind) the caller means to run -- asserted
    before anything is launched.  Prints the kind (pytest -s / -rP)."""
    import numpy as np

    from openr_amd.engine import PAIR_DTYPE, Ksp2Result
    from openr_amd.hiprt import DeviceArray

    p = eng.ksp2_plan(srcs)
    pairs = cnt = pool = None
    try:
        info = p.info()
        print(f"ksp2 plan: {info}")
        if kinds is not None:
            assert info.kind in kinds, (info, kinds)
        pairs = DeviceArray(len(srcs) * n * 4, np.uint32)
        cnt = DeviceArray(4, np.uint64, zero=True)
        words = len(srcs) * n * 24 + (1 << 22)
        pool = DeviceArray(words, np.uint32)
        p.execute(pairs.ptr, pool.ptr, words, cnt.ptr)
        eng.check()
        c = cnt.numpy().astype(np.int64)
        if c[0] > words:  # size the pool from the counter and run again
            pool.free()
            words = int(c[0]) + int(c[0]) // 4 + (1 << 20)  # grab slack varies run to run
            pool = DeviceArray(words, np.uint32)
            p.execute(pairs.ptr, pool.ptr, words, cnt.ptr)
            eng.check()
            c = cnt.numpy().astype(np.int64)
        assert c[0] <= words and not (c[2] & 3), c
        res = Ksp2Result(np.asarray(srcs, np.uint32), n,
                         pairs.numpy().view(PAIR_DTYPE).copy(), pool.numpy()[: c[0]].copy())
        return res, c
    finally:
        p.close()
        for b in (pairs, cnt, pool):
            if b is not None:
                b.free()


def ksp2_canonical(res):
    """A Ksp2Result in a form that does not depend on where the records lie
    in the pool: (n_paths [pairs, 2], the path lengths in (pair, k, list)
    order, their links concatenated in that order).  Two results give equal
    triples exactly when paths(i, d, k) agree for every pair and k."""
    import numpy as np

    pool = np.asarray(res.pool, np.int64)
    n_paths = np.asarray(res.pairs["n_paths"], np.int64)
    pair_, k_, q_, at_ = [], [], [], []
    for k in (0, 1):
        at = np.asarray(res.pairs["first"][:, k], np.int64).copy()
        live = np.nonzero(n_paths[:, k] > 0)[0]
        q = 0
        while len(live):
            a = at[live]
            assert a.min() >= 0 and a.max() + 2 <= len(pool), "a record outside the pool"
            pair_.append(live)
            k_.append(np.full(len(live), k))
            q_.append(np.full(len(live), q))
            at_.append(a)
            at[live] = pool[a + 1]
            q += 1
            live = live[n_paths[live, k] > q]
    if not pair_:
        return n_paths, np.zeros(0, np.int64), np.zeros(0, np.int64)
    pair_, k_, q_, at_ = (np.concatenate(x) for x in (pair_, k_, q_, at_))
    order = np.lexsort((q_, k_, pair_))
    at_ = at_[order]
    lens = pool[at_]
    assert (at_ + 2 + lens).max() <= len(pool), "a record runs past the pool"
    first = np.cumsum(lens) - lens
    idx = np.repeat(at_ + 2, lens) + (np.arange(int(lens.sum())) - np.repeat(first, lens))
    return n_paths, lens, pool[idx]


def spf_canonical(res) -> dict:
    """Product SpfResult -> the oracle's JSON shape."""
    return {
        node: {
            "metric": r.metric(),
            "nextHops": sorted(r.nextHops()),
            "pathLinks": [[link_key(pl.link), pl.prevNode] for pl in r.pathLinks()],
        }
        for node, r in sorted(res.items())
    }


def planar_rows(ks, dist, mats, pitch):
    """Oracle dense results (dist [m, n] u64, mats[i] bool [>= k_i, n]) in the
    engine's plan layout: dist rows u32 padded to `pitch` (unreachable =
    0xFFFFFFFF, padding 0) and next-hop bitmaps, k_i rows of pitch/32 words
    per source, concatenated in source order."""
    import numpy as np

    m, n = dist.shape
    d32 = np.zeros((m, pitch), np.uint32)
    d32[:, :n] = np.where(dist == np.iinfo(np.uint64).max, 0xFFFFFFFF, dist).astype(np.uint32)
    rows = []
    for i in range(m):
        for j in range(int(ks[i])):
            row = np.zeros(pitch, bool)
            row[:n] = mats[i][j]
            rows.append(np.packbits(row, bitorder="little").view(np.uint32))
    nh = np.concatenate(rows) if rows else np.zeros(0, np.uint32)
    return d32, nh


def _mix64(z):
    """splitmix64's finaliser over a uint64 array (wrapping arithmetic)."""
    import numpy as np

    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def route_db_digest(hdr, rec, link_id, link_hash) -> int:
    """One node's materialised route database (spf_mplan_route_records:
    headers offset | count << 32, records CSR edge | metric << 32) reduced
    with spf_mplan_route_digests' formula keyed by the smallest next-hop
    metric (oracle route_digests(kept_min=True)): per set p with next hops,
    mix(mix(K (p + 1) + least) + sum mix(link_hash[link] + metric) + p),
    summed over p.  (Without LFA, least == the shortest distance and this is
    the digest kernel's value.)  Also checks each route's next hops are in
    link order."""
    import numpy as np

    hdr = np.asarray(hdr, np.uint64)
    rec = np.asarray(rec, np.uint64)
    off = (hdr & np.uint64(0xFFFFFFFF)).astype(np.int64)
    cnt = (hdr >> np.uint64(32)).astype(np.int64)
    edge = (rec & np.uint64(0xFFFFFFFF)).astype(np.int64)
    met = rec >> np.uint64(32)
    lh = np.asarray(link_hash, np.uint64)
    per = _mix64(lh[np.asarray(link_id, np.int64)[edge]] + met) if len(rec) else np.zeros(0, np.uint64)
    nz = np.nonzero(cnt)[0]
    if len(nz) == 0:
        return 0
    c = cnt[nz]
    seg = np.concatenate([[0], np.cumsum(c)[:-1]])
    idx = np.repeat(off[nz], c) + (np.arange(int(c.sum())) - np.repeat(seg, c))
    assert idx.max() < len(rec), "a route's records run past the node's region"
    e = edge[idx]
    inner = np.ones(len(idx), bool)
    inner[seg] = False
    assert np.all(np.diff(e)[inner[1:]] > 0), "next hops not in link order"
    with np.errstate(over="ignore"):
        sums = np.add.reduceat(per[idx], seg, dtype=np.uint64)
        shortest = np.minimum.reduceat(met[idx], seg)
        p = nz.astype(np.uint64)
        h = _mix64(_mix64(np.uint64(0x9e3779b97f4a7c15) * (p + np.uint64(1)) + shortest) + sums + p)
        total = h.sum(dtype=np.uint64)
    return int(total)


def label_candidates(label_of):
    """{label: candidates in ascending name} over the valid, non-zero labels."""
    from openr_amd.spf_solver import MPLS_LABEL_MAX, MPLS_LABEL_MIN

    out = {}
    for node in sorted(label_of):
        lab = label_of[node]
        if lab != 0 and MPLS_LABEL_MIN <= lab <= MPLS_LABEL_MAX:
            out.setdefault(lab, []).append(node)
    return dict(sorted(out.items()))


def expected_from(orc, label_of, mes, lfa):
    """{(me, label): (owner name, {(ifName, metric, neighbour, action, swap)})}
    for the pairs with a route, from the oracle alone (mes: names; None =
    every node): per me and label the candidates are walked in ascending
    name; the first that is me owns the label (POP_AND_LOOKUP, no rows),
    otherwise the first with a non-empty next-hop set owns it."""
    from oracle import nexthops

    cands = label_candidates(label_of)
    mes = sorted(label_of) if mes is None else mes
    out = {}
    for me in mes:
        for lab, cs in cands.items():
            for c in cs:
                if c == me:
                    out[(me, lab)] = (me, set())
                    break
                rows = nexthops(orc, me, [c], lfa, swap_label=lab)["nh"]
                if rows:
                    out[(me, lab)] = (c, {(r[0], r[1], r[2], r[4], r[5]) for r in rows})
                    break
    # the inputs are chosen so that most pairs have a route
    assert 2 * len(out) >= len(mes) * len(cands), (len(out), len(mes), len(cands))
    return out
