"""The KSP2 route kernels at the edges the other two modules do not reach
(test_gpu_ksp2_routes.py, test_gpu_ksp2_route_delta.py: 4 to 72 nodes, at most
208 sets):

A. ksp2_routes_kernel (csrc/ksp2_routes.hip) past its first 64 candidates with
   k = 2 paths: k = 2 candidates, k2_dropped, the n_hops / n_words carry and
   cross-chunk duplicates in a chunk after the first;
B. ksp2_delta_kernel and the update kernels (csrc/ksp2_route_delta.hip), the
   fill (delta_fill_kernel, csrc/route_delta.hip) and the scan
   (csrc/label_routes.hip) at their tile edges: more than 256 routes per
   source (two chunks), more than 2048 workgroups, entries and records (a scan
   across tiles), a mismatch only the second stride of the set pass sees, a
   route that changes in its cost alone, a hop-count change next to set-pass
   routes in one wave.

Expectations never come from the code under test.  Part A compares with the
oracle (oracle.sr_nexthops(..., ksp2=True)); the candidates a route has, in the
kernel's order, are restated here from the oracle's getKthPaths and tied to
the oracle's next hops before anything is read from them.  Part B follows
test_gpu_ksp2_route_delta.py: both generations are read back with
allSourcesKsp2RouteDb and calculateUpdate's rules are applied in Python.
Every test asserts on the expectation's side that its input reaches the case it
is for.  Integers, no tolerance.
"""

import collections
import copy

import numpy as np
import pytest

import test_gpu_ksp2_route_delta as DL
import test_gpu_ksp2_routes as RT
from oracle import OracleLinkState
from openr_amd import _native as N

pytestmark = pytest.mark.gpu

D, M = N.SPF_DELTA_DELETE, N.SPF_DELTA_DELETE - 1
CHUNK = 64  # candidates (ksp2_routes_kernel) / new hops (the set pass) per step of a wave
TILE = 2048  # label_routes.hip's kScanTile
WG = 256  # routes per workgroup of ksp2_delta_kernel and delta_fill_kernel


# ==== A. ksp2_routes_kernel beyond 64 candidates with k = 2 paths ======================
LEAVES = [f"t{i:02d}" for i in range(40)]
STAGED = ("LDS_U16", "LDS_U32")


def two_hub(leaf_label):
    """me -1- h1, me -2- h2, every leaf t00..t39 joined to both hubs at 1: for
    me every leaf has one k = 1 path [me-h1, h1-t] at 2 and one k = 2 path
    [me-h2, h2-t] at 3.  Returns the LSDB, {node: label}, {ifName: metric}."""
    links = [("me", "h1", 1, 1, False), ("me", "h2", 2, 2, False)]
    for t in LEAVES:
        links += [("h1", t, 1, 1, False), ("h2", t, 1, 1, False)]
    label = {"me": 1, "h1": 2, "h2": 3, **leaf_label}
    metric_of = {}
    for u, v, mu, mv, _ in links:
        metric_of[f"{u}/{v}/0"], metric_of[f"{v}/{u}/0"] = mu, mv
    return RT.lsdb_from_links(links, label), label, metric_of


def contains(b, a):
    """LinkState::pathAInPathB: a is a contiguous run of b."""
    return any(b[i: i + len(a)] == a for i in range(len(b) - len(a) + 1))


def candidates(orc, me, members, label, pre, metric_of):
    """selectBestPathsKsp2's candidates of route (me, members) in the order the
    kernel numbers them -- every member's k = 1 paths, then every member's
    k = 2 paths, members in the order given -- from the oracle's getKthPaths: per
    candidate its list k, its row (ifName, cost, neighbour, action, labels)
    and its fate: "dropped" (a k = 2 path that contains a k = 1 path),
    ("dup", index of the first occurrence) or "kept"."""
    raw = [(k, d, [tuple(l) for l in path]) for k in (1, 2) for d in members if d != me
           for path in orc.kth_paths(me, d, k)]
    k1 = [path for k, _, path in raw if k == 1]
    out, first_at = [], {}
    for idx, (k, d, path) in enumerate(raw):
        cur, cost, stack = me, 0, []
        for x, (n1, if1, n2, if2) in enumerate(path):
            ifn, nxt = (if1, n2) if cur == n1 else (if2, n1)
            cost += metric_of[ifn]
            if x == 0:
                first = (ifn, nxt)
            else:
                stack.insert(0, label[nxt])  # [L(vk), ..., L(v2)]
            cur = nxt
        assert cur == d
        if pre and pre.get(d) is not None:
            stack.insert(0, pre[d])
        row = (first[0], cost, first[1], "PUSH" if stack else None, tuple(stack) or None)
        if k == 2 and any(contains(path, a) for a in k1):
            fate = "dropped"
        elif row in first_at:
            fate = ("dup", first_at[row])
        else:
            first_at[row] = idx
            fate = "kept"
        out.append((k, row, fate))
    return out


MES = ["me", "t07", "h1"]


def two_hub_case(leaf_label, members, pre=None, kinds=STAGED):
    """The route of every me of MES against the oracle (test_gpu_ksp2_routes.
    check), and me's candidates: their kept rows are the oracle's next hops
    and, in candidate order, the product's records.  Returns (candidates, rows)."""
    lsdb, label, metric_of = two_hub(leaf_label)
    assert RT.names_of(lsdb) == sorted(label)  # csr order: h1, h2, me, t00 ..
    got, want = RT.check(lsdb, [members], [pre] if pre else None, MES, kinds=kinds)
    orc = OracleLinkState()
    orc.update_packed(lsdb)
    cand = candidates(orc, "me", sorted(members), label, pre, metric_of)  # (set_nodes ascend by id)
    kept = [row for _, row, fate in cand if fate == "kept"]
    assert set(kept) == want[("me", 0)] and len(set(kept)) == len(kept)  # the oracle's route
    assert got[("me", 0)] == kept  # first occurrences in candidate order
    assert all(got[(me, 0)] for me in MES)
    return cand, kept


def staged(monkeypatch):
    monkeypatch.delenv("SPF_KSP2_HBM", raising=False)


@pytest.mark.parametrize("hbm,kinds", [k[1:] for k in RT.KSP2_KERNELS], ids=[k[0] for k in RT.KSP2_KERNELS])
def test_k2_candidates_past_the_first_chunk(hbm, kinds, monkeypatch):
    """80 candidates, none dropped, none equal: the k = 2 list starts at
    candidate 40 and crosses the chunk boundary."""
    if hbm:
        monkeypatch.setenv("SPF_KSP2_HBM", hbm)
    else:
        staged(monkeypatch)
    cand, kept = two_hub_case({t: 100 + i for i, t in enumerate(LEAVES)}, LEAVES, kinds=kinds)
    assert [k for k, _, _ in cand] == [1] * 40 + [2] * 40
    assert all(fate == "kept" for _, _, fate in cand) and len(kept) == 80
    assert kept == ([("me/h1/0", 2, "h1", "PUSH", (100 + i,)) for i in range(40)] +
                    [("me/h2/0", 3, "h2", "PUSH", (100 + i,)) for i in range(40)])


def test_duplicates_of_a_k2_candidate_of_the_first_chunk(monkeypatch):
    staged(monkeypatch)
    cand, kept = two_hub_case({t: 555 for t in LEAVES}, LEAVES)
    assert kept == [("me/h1/0", 2, "h1", "PUSH", (555,)), ("me/h2/0", 3, "h2", "PUSH", (555,))]
    assert len(cand) == 80 and cand[40][0] == 2 and cand[40][2] == "kept"
    assert all(cand[i][2] == ("dup", 40) for i in range(CHUNK, 80))


def mirror_pairs():
    """t_i and t_{39 - i} share a label."""
    return {t: 100 + min(i, 39 - i) for i, t in enumerate(LEAVES)}


def mixed_pairs():
    """t_i and t_{39 - i} share a label for i < 12, t_i and t_{i + 1} for even
    i in 12..26: the mirrored pairs alone keep the first 20 candidates of
    either list, so no k = 2 candidate past 64 survives."""
    lab = mirror_pairs()
    for i in range(12, 28):
        lab[LEAVES[i]] = 200 + i // 2
    return lab


@pytest.mark.parametrize("pairs", [mirror_pairs, mixed_pairs])
def test_labels_equal_in_pairs(pairs, monkeypatch):
    staged(monkeypatch)
    leaf_label = pairs()
    assert sorted(collections.Counter(leaf_label.values()).values()) == [2] * 20
    cand, kept = two_hub_case(leaf_label, LEAVES)
    assert len(cand) == 80 and len(kept) == 40
    firsts = [i for i, c in enumerate(cand) if c[2] == "kept"]
    dups = [(i, c[2][1]) for i, c in enumerate(cand) if c[2] != "kept"]
    assert len(dups) == 40 and all(cand[i][2][0] == "dup" for i, _ in dups)
    # a duplicate of the second chunk whose first occurrence, a k = 2 candidate, is in the first
    assert any(i >= CHUNK and f < CHUNK and cand[f][0] == 2 for i, f in dups)
    assert any(i < CHUNK for i, _ in dups) and any(f < CHUNK for f in firsts)
    if pairs is mixed_pairs:
        # first occurrences and duplicates in both chunks; a k = 2 survivor past 64
        assert any(f >= CHUNK and cand[f][0] == 2 for f in firsts)
        assert any(i >= CHUNK and f >= CHUNK for i, f in dups)


def test_k2_dropped_on_both_sides_of_the_chunk_boundary(monkeypatch):
    """h2 in the set: its k = 1 path [me-h2] lies in every leaf's k = 2 path,
    and its own k = 2 path me-h1-t-h2 contains that leaf's k = 1 path."""
    staged(monkeypatch)
    cand, kept = two_hub_case({t: 100 + i for i, t in enumerate(LEAVES)}, ["h2"] + LEAVES)
    assert len(cand) == 82 and [k for k, _, _ in cand] == [1] * 41 + [2] * 41
    dropped = [i for i, c in enumerate(cand) if c[2] == "dropped"]
    assert dropped == list(range(41, 82)) and dropped[0] < CHUNK < dropped[-1]
    assert len(kept) == 41 and kept[0] == ("me/h2/0", 2, "h2", None, None)


def test_word_offsets_carried_into_the_second_chunk(monkeypatch):
    """A prepend label on every other leaf: the survivors' stacks have one or
    two words, and the second chunk's words start where the first's end."""
    staged(monkeypatch)
    pre = {t: (7000 + i if i % 2 == 0 else None) for i, t in enumerate(LEAVES)}
    cand, kept = two_hub_case({t: 100 + i for i, t in enumerate(LEAVES)}, LEAVES, pre)
    assert len(kept) == 80 and all(c[2] == "kept" for c in cand)
    for chunk in (kept[:CHUNK], kept[CHUNK:]):
        assert {len(r[4]) for r in chunk} == {1, 2}
    assert sum(len(r[4]) for r in kept[:CHUNK]) == 96  # != 64: not one word per survivor
    assert kept[CHUNK] == ("me/h2/0", 3, "h2", "PUSH", (7024, 124))


# ==== B. the delta, its fill and its update at their tile edges ========================
def set_pass_routes(g0, g1, n_mes, n_sets):
    """The routes ksp2_delta_kernel hands to its set pass: as many next hops
    on either side, at least one, and not equal position by position."""
    return sum(1 for t in range(n_mes) for p in range(n_sets)
               if len(g0.order[(t, p)]) == len(g1.order[(t, p)]) > 0 and g0.order[(t, p)] != g1.order[(t, p)])


def layout(w, n_sets, want):
    """test_determinism_and_layout's dptr / dset assertions; returns route_update()."""
    out = w.ls._k2r[0].plan.route_update()
    dptr, dset = out[:2]
    assert len(dptr) == w.n_mes + 1 and dptr[0] == 0 and int(dptr[-1]) == len(dset)
    assert np.all(np.diff(dptr.astype(np.int64)) >= 0)
    for t in range(w.n_mes):
        mine = dset[int(dptr[t]): int(dptr[t + 1])]
        sets = (mine & np.uint32(M)).astype(np.int64)
        assert np.all(np.diff(sets) > 0) and (len(sets) == 0 or sets[-1] < n_sets)
        up, dele = want[t]
        assert sets.tolist() == sorted(up + dele) and sets[(mine & np.uint32(D)) != 0].tolist() == dele
    return out


# ---- 1. two chunks per source -------------------------------------------------------------
CHUNK_LINK = ("n20", "n21", 0)  # a shortest n20 -> n21 path (asserted below)


def chunk_dbs():
    """random_dbs at 40 nodes, the leaf z behind n07, and a0 - a1 apart from
    both: sources that reach none of the sets that change."""
    return DL.random_dbs(seed=5, n=40, extra=36, more=[("n07", "z", 1, 1, False), ("a0", "a1", 1, 1, False)])


def chunk_sets(names, S):
    """S sets: all loopbacks, then anycast sets -- every third with z, every
    fourth with a member twice -- over and over; [n21] at 255, and [z] at 256
    and last (S > 256) or at 254 (S == 256)."""
    rng = np.random.default_rng(11)
    inner = [n for n in names if n.startswith("n")]
    anycast = []
    for k in range(24):
        s = [inner[int(i)] for i in rng.choice(len(inner), int(rng.integers(2, 5)), replace=False)]
        if k % 3 == 0:
            s.append("z")
        if k % 4 == 1:
            s.append(s[0])
        anycast.append(s)
    sets = [[n] for n in names]
    while len(sets) < S:
        sets.append(list(anycast[(len(sets) - len(names)) % len(anycast)]))
    sets[255] = [CHUNK_LINK[1]]
    if S > WG:
        sets[256] = ["z"]
        sets[S - 1] = ["z"]
    else:
        sets[254] = ["z"]
    return sets


@pytest.mark.parametrize("S", [256, 257, 400])
def test_two_chunks_per_source(S):
    """S = 257: the second workgroup of a source holds one route; 256: the
    exact fit; 400: the second workgroup's changed routes lie in three waves
    (delta_fill_kernel's rank over the waves before)."""
    dbs = chunk_dbs()
    u, v, k = CHUNK_LINK
    assert DL.host_direct_path(dbs, u, v, k)
    w = DL.World(dbs)
    try:
        assert w.names[:2] == ["a0", "a1"] and w.names[-1] == "z" and len(w.names) == 43
        sets = chunk_sets(w.names, S)
        assert len(sets) == S and (S + WG - 1) // WG == (2 if S > WG else 1)
        g0 = w.build(sets)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        patches = N.lib.ls_debug_row_patches(w.ls._h)
        dbs[u].adjacencies.remove(DL.adj(dbs, u, v, k))
        dbs["z"].adjacencies.remove(DL.adj(dbs, "z", "n07"))
        w.push(u, "z")
        g1 = w.build(sets)
        assert N.lib.ls_debug_row_patches(w.ls._h) > patches  # patched in place, not reloaded
        want = DL.expected(g0, g1, w.n_mes, S)
        ent = [sorted(up + dele) for up, dele in want]
        print(f"S={S} chunks={(S + WG - 1) // WG} entries per source={[len(e) for e in ent]}")
        assert ent[0] == [] and ent[1] == []  # a0, a1: the first workgroups have nothing
        me = w.id_of[u]
        assert 255 in want[me][0]  # the withdrawn link's far end
        if S > WG:
            both = [t for t, e in enumerate(ent) if e and e[0] < WG <= e[-1]]
            assert me in both and {255, 256} <= set(ent[me]) and len(both) >= 40
            assert all(256 in dele and S - 1 in dele for _, dele in want[2:-1])  # (z has no route to itself)
        else:
            assert 254 in want[me][1] and ent[me][-1] == 255
        if S == 400:  # changed routes in the waves 0, 1 and 2 of the second workgroup
            assert all(any(WG + 64 * x <= p < WG + 64 * (x + 1) for p in ent[me]) for x in range(3))
            assert any(p >= WG for p in want[me][0])  # UPDATEs of the second workgroup too
        DL.check(w, snap, g0, g1, S)
        layout(w, S, want)
    finally:
        w.close()


# ---- 2. scans past one tile ---------------------------------------------------------------
def restated_update(g0, g1, n_mes, n_sets):
    """spf_ksp2_route_update's six arrays from the read-back pools of both
    generations and calculateUpdate's rules."""
    dptr, dset, uptr, urec, ulptr, ulab = [0], [], [0], [], [0], []
    for t, (up, dele) in enumerate(DL.expected(g0, g1, n_mes, n_sets)):
        rptr, rec, lptr, lab = g1.raw[t]
        for p in sorted(up + dele):
            dset.append(p | D if p in dele else p)
            if p in up:
                for h in range(int(rptr[p]), int(rptr[p + 1])):
                    urec.append(int(rec[h]))
                    ulab += lab[int(lptr[h]): int(lptr[h + 1])].tolist()
                    ulptr.append(len(ulab))
            uptr.append(len(urec))
        dptr.append(len(dset))
    return (np.array(dptr, np.uint64), np.array(dset, np.uint32), np.array(uptr, np.uint64),
            np.array(urec, np.uint64), np.array(ulptr, np.uint64), np.array(ulab, np.int32))


def test_scans_past_one_tile():
    """2,108 sources (a 31-node graph's nodes 68 times over: the plan takes
    repeated sources), 4 sets: more than 2048 delta workgroups, update entries
    and update records, each with a partial last tile."""
    dbs = DL.random_dbs(seed=5, n=30, extra=25, more=[("n11", "z", 1, 1, False)])
    names = sorted(dbs)
    w = DL.World(dbs, mes=names * 68)
    try:
        sets = [["n03", "n17", "n25"], ["n08", "n21"], ["n14"], ["z"]]
        S = len(sets)
        pre0 = [{d: 7000 + 100 * p + i for i, d in enumerate(s)} for p, s in enumerate(sets)]
        pre1 = [{d: v + 1000 for d, v in pre.items()} for pre in pre0]
        g0 = w.build(sets, pre0)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        # an unchanged second generation: nothing on either side of a tile
        g_same = w.build(sets, pre0)
        assert g_same.routes == g0.routes and any(g0.routes.values())
        lists, totals, info = DL.check(w, snap, g0, g_same, S)
        assert totals == [0, 0, 0] and all(l == ([], []) for l in lists)
        dptr, dset, uptr, urec, ulptr, ulab = w.ls._k2r[0].plan.route_update()[:6]
        assert len(dptr) == w.n_mes + 1 and not dptr.any() and len(dset) == 0 and uptr.tolist() == [0]
        assert len(urec) == 0 and ulptr.tolist() == [0] and len(ulab) == 0
        # every prepend label changes, and z is cut off
        dbs["z"].adjacencies.remove(DL.adj(dbs, "z", "n11"))
        w.push("z")
        g1 = w.build(sets, pre1)
        want = DL.expected(g0, g1, w.n_mes, S)
        blocks = w.n_mes * ((S + WG - 1) // WG)
        changed = [t for t, (up, dele) in enumerate(want) if up or dele]
        exp = restated_update(g0, g1, w.n_mes, S)
        entries, records, words = len(exp[1]), len(exp[3]), len(exp[5])
        print(f"workgroups={blocks} entries={entries} records={records} words={words} "
              f"updates={sum(len(u) for u, _ in want)} deletes={sum(len(d) for _, d in want)}")
        assert blocks == 2108 and min(blocks, entries, records) > TILE
        assert all(x % TILE for x in (blocks, entries, records))  # a partial last tile
        assert changed[0] < TILE < changed[-1] and len(changed) == w.n_mes
        assert any(d for _, d in want[:TILE]) and any(d for _, d in want[TILE:])  # DELETEs between the UPDATEs
        DL.check(w, snap, g0, g1, S)
        got = layout(w, S, want)
        for name, a, b in zip(("dptr", "dset", "uptr", "urec", "ulptr", "ulab"), got[:6], exp):
            assert a.dtype == b.dtype and np.array_equal(a, b), name
        assert got[6] == [sum(len(u) for u, _ in want), records, words]
    finally:
        w.close()


# ---- 3. a mismatch only the second stride of the set pass sees ---------------------------
def test_mismatch_in_the_second_stride():
    dbs = DL.hub_dbs(70)
    leaves = [f"l{i:03d}" for i in range(70)]
    w = DL.World(dbs, mes=["hub", "l000", "l001", "l035", "l069"])
    try:
        sets = [[n] for n in w.names] + [leaves]
        p = len(sets) - 1
        rev = sets[:p] + [leaves[::-1]]
        g0 = w.build(sets)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        for leaf, side in (("l003", "new"), ("l067", "old")):
            old_label = dbs[leaf].nodeLabel
            dbs[leaf].nodeLabel = 9999
            w.push(leaf)
            g1 = w.build(rev)
            for t in range(1, w.n_mes):  # the changed hop sits past 64 in the new (old) pool order
                assert len(g1.order[(t, p)]) == len(g0.order[(t, p)]) == 69
                new_at = [j for j, h in enumerate(g1.order[(t, p)]) if h[2] == (9999,)]
                old_at = [j for j, h in enumerate(g0.order[(t, p)]) if h[2] == (old_label,)]
                assert len(new_at) == len(old_at) == 1
                print(f"{leaf}: source {t}: new position {new_at[0]}, old position {old_at[0]}")
                assert (new_at[0] if side == "new" else old_at[0]) >= CHUNK
                assert (old_at[0] if side == "new" else new_at[0]) < CHUNK
                # ... and it is the only difference
                assert g1.routes[(t, p)] ^ g0.routes[(t, p)] == {g1.order[(t, p)][new_at[0]],
                                                                 g0.order[(t, p)][old_at[0]]}
            lists, totals, _ = DL.check(w, snap, g0, g1, len(sets))
            loop = w.id_of[leaf]
            assert lists[0] == ([], [])  # the hub's own next hops carry no labels
            assert all(lists[t] == ([loop, p], []) for t in range(1, w.n_mes))
            assert totals[2] == set_pass_routes(g0, g1, w.n_mes, len(sets)) >= w.n_mes
            dbs[leaf].nodeLabel = old_label
            w.push(leaf)
    finally:
        w.close()


# ---- 4. cost only -------------------------------------------------------------------------
def line_dbs():
    label = {"p1": 11, "p2": 12, "p3": 13, "p4": 14}
    return DL.dbs_from_links([("p1", "p2", 1, 1, False), ("p2", "p3", 1, 1, False), ("p3", "p4", 1, 1, False)],
                             label)


def ring_dbs():
    nodes = [f"r{i}" for i in range(6)]
    return DL.dbs_from_links([(nodes[i], nodes[(i + 1) % 6], 1, 1, False) for i in range(6)],
                             {n: 200 + i for i, n in enumerate(nodes)})


# graph, the link whose metric rises (both directions), a route that keeps its links
COST_ONLY = {"line": (line_dbs, ("p2", "p3"), 5, ("p1", "p4")),
             "ring": (ring_dbs, ("r1", "r2"), 2, ("r0", "r2"))}  # r0-r1-r2 at 3 stays under r0-r5-..-r2 at 4


@pytest.mark.parametrize("graph", list(COST_ONLY))
def test_cost_only(graph):
    make, (a, b), metric, (src, dst) = COST_ONLY[graph]
    dbs = make()
    w = DL.World(dbs)
    try:
        sets = w.loopbacks([[dst, src]])
        S = len(sets)
        g0 = w.build(sets)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        DL.adj(dbs, a, b).metric = metric
        DL.adj(dbs, b, a).metric = metric
        w.push(a, b)
        g1 = w.build(sets)
        # routes that differ in cost alone: hop by hop the same link, the same stack
        strip = lambda hops: [(h[0], h[2]) for h in hops]  # noqa: E731
        cost_only = [key for key in g0.order
                     if g0.order[key] and strip(g0.order[key]) == strip(g1.order[key])
                     and [h[1] for h in g0.order[key]] != [h[1] for h in g1.order[key]]]
        print(f"{graph}: routes that change in cost alone: {cost_only}")
        assert (w.id_of[src], w.id_of[dst]) in cost_only and len(cost_only) >= 2
        lists, totals, _ = DL.check(w, snap, g0, g1, S)
        payload = w.ls._k2u[0]
        for t, p in cost_only:
            assert p in lists[t][0]
            costs = [h[1] for h in payload[t][p]]
            assert costs == [h[1] for h in g1.order[(t, p)]] != [h[1] for h in g0.order[(t, p)]]
        assert totals[1] == 0
    finally:
        w.close()


# ---- 5. a hop-count change next to set-pass routes in one wave ---------------------------
def test_hop_count_change_beside_set_pass_routes():
    """Routes p, p + 1, p + 2 of one source, one wave: p loses next hops
    (UPDATE before the set pass), p + 1 only reorders (the set pass: same),
    p + 2 reorders and one of its labels changes (the set pass: UPDATE)."""
    make, anycast, _ = DL.GRAPHS["random"]
    w = DL.World(make())
    try:
        four = anycast[1]
        loops = [[n] for n in w.names]
        p = len(loops)
        assert p // 64 == (p + 2) // 64  # one wave
        pre0 = [{d: None for d in s} for s in loops] + [{d: None for d in four}] * 2 + [{d: 7000 + i for i, d in enumerate(four)}]
        pre1 = copy.deepcopy(pre0)
        pre1[p + 2][four[0]] = 8000
        g0 = w.build(loops + [four, four, four], pre0)
        snap = w.ls.allSourcesKsp2RouteSnapshot()
        g1 = w.build(loops + [four[:-1], four[::-1], four[::-1]], pre1)
        S = p + 3
        src = [t for t in range(w.n_mes)
               if 0 < len(g1.routes[(t, p)]) < len(g0.routes[(t, p)])
               and g1.routes[(t, p + 1)] == g0.routes[(t, p + 1)] and g1.order[(t, p + 1)] != g0.order[(t, p + 1)]
               and len(g1.order[(t, p + 2)]) == len(g0.order[(t, p + 2)])
               and g1.routes[(t, p + 2)] != g0.routes[(t, p + 2)]
               and [h for h in g1.order[(t, p + 2)] if h in g0.routes[(t, p + 2)]] !=
               [h for h in g0.order[(t, p + 2)] if h in g1.routes[(t, p + 2)]]]
        print(f"sources with all three routes: {src}")
        assert src
        lists, totals, _ = DL.check(w, snap, g0, g1, S)
        for t in src:
            assert [q for q in lists[t][0] if q >= p] == [p, p + 2] and not lists[t][1]
        assert totals[2] == set_pass_routes(g0, g1, w.n_mes, S) >= 2 * len(src)
    finally:
        w.close()
