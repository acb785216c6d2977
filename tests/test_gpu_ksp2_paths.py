"""Which kernel a batched KSP2 plan runs (openr_amd/csrc/ksp2.hip), and every
one of them against the CPU oracle's getKthPaths (LinkState.cpp:762-791),
path for path and link for link -- no tolerances.

spf_ksp2_plan_create chooses between exact_ksp2_kernel (EXACT), ksp2_kernel
(HBM: the graph read from HBM, 32-bit DFS stack, bitmaps by link id, 4 waves)
and the staged-graph ksp2_lds_kernel<u32 | u16> (LDS_U32, LDS_U16).  Every
test here first asserts Ksp2Plan.info().kind, so a change of the selection
fails the test instead of moving it to another kernel:

  a. SPF_KSP2_HBM=1 on the small graphs of test_gpu_ksp2: oracle, and the
     staged kernel's paths and k = 2 SPF count;
  b. the natural triggers of HBM (a metric >= 65536 and the 65535 edge below
     it, >= 65536 directed edges, a staged graph past the LDS) and of EXACT
     (per-wave rows past the LDS);
  c. SPF_KSP2_CHUNK / _GRAB / _DELTA: the same paths and k = 2 SPF count;
  d. a pool that is too small: reported, contained, and sized by the counter;
  e. spf_ksp2_solve's repack: byte-identical whichever kernel ran.

The oracle is the slow part (it keeps the reference's containers): the dense
case's 1200 pairs and the 400 pairs past the LDS spend seconds in its
Dijkstras over 66k and 30k edges; the kernels take milliseconds.
"""

import numpy as np
import pytest

from helpers import ksp2_canonical, run_plan
from openr_amd import _native as N
from openr_amd import topology as T
from openr_amd.engine import PAIR_DTYPE, Ksp2Result
from openr_amd.hiprt import DeviceArray
from test_gpu_ksp2 import SMALL, setup

pytestmark = pytest.mark.gpu

STAGED = ("LDS_U16", "LDS_U32")
ENV = ("SPF_KSP2_HBM", "SPF_KSP2_EXACT", "SPF_KSP2_U16", "SPF_KSP2_CHUNK", "SPF_KSP2_GRAB",
       "SPF_KSP2_DELTA", "SPF_KSP2_PROF")
SENTINEL = 0xA5C3F00D


@pytest.fixture(autouse=True)
def plain_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


class Graph:
    """setup()'s engine, oracle and link keys of one topology; closes the engine."""

    def __init__(self, topo):
        self.names, self.eng, self.orc, self.key, self.csr = setup(topo)
        self.n = len(self.names)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()

    def run(self, srcs, kinds):
        return run_plan(self.eng, srcs, self.n, kinds=kinds)

    def check_oracle(self, res, srcs, dsts=None):
        for i, s in enumerate(srcs):
            for d in (range(self.n) if dsts is None else dsts):
                for k in (1, 2):
                    got = [[self.key(l) for l in p] for p in res.paths(i, d, k)]
                    want = self.orc.kth_paths(self.names[s], self.names[d], k)
                    assert got == want, (self.names[s], self.names[d], k, got, want)


def assert_same_paths(a, b, what):
    """paths(i, d, k) of two results agree for every pair and k."""
    if all(np.array_equal(x, y) for x, y in zip(ksp2_canonical(a), ksp2_canonical(b))):
        return
    for i in range(len(a.srcs)):  # name the first pair that differs
        for d in range(a.n_nodes):
            for k in (1, 2):
                assert a.paths(i, d, k) == b.paths(i, d, k), (what, int(a.srcs[i]), d, k)
    raise AssertionError(f"{what}: canonical forms differ, every pair's paths agree")


def rand3():
    return dict(SMALL)["rand3"]()  # parallel links, 5 drained nodes, drained links


def ring():
    return T.wan(1100, 0, seed=3, max_metric=3)  # paths of up to 1099 links


# ---- a. the HBM kernel forced onto the small graphs -----------------------------------
@pytest.mark.parametrize("name,make", SMALL, ids=[s[0] for s in SMALL])
def test_forced_hbm_matches_oracle_and_staged(name, make, monkeypatch):
    with Graph(make()) as g:
        n = g.n
        srcs = list(range(n)) if n <= 80 else list(range(0, n, max(1, n // 24)))
        monkeypatch.setenv("SPF_KSP2_HBM", "1")
        hbm, c_hbm = g.run(srcs, ("HBM",))
        monkeypatch.delenv("SPF_KSP2_HBM")
        staged, c_staged = g.run(srcs, STAGED)
        g.check_oracle(hbm, srcs)
        assert_same_paths(hbm, staged, name)
        assert c_hbm[1] == c_staged[1]  # k = 2 SPF runs
        assert c_hbm[3] == 0  # (no u16 waves, nothing to redo)
        if n <= 80:  # the canonical form agrees with paths() where that is cheap
            flat = [l for i in range(len(srcs)) for d in range(n) for k in (1, 2)
                    for p in hbm.paths(i, d, k) for l in p]
            assert flat == ksp2_canonical(hbm)[2].tolist()


# ---- b. natural triggers ------------------------------------------------------------
def wan_metrics(cap=None, bump=False):
    """T.wan(60, 30) with metrics U[1, 70000]; capped at `cap`; `bump`: the
    first metric equal to the cap raised by one."""
    topo = T.wan(60, 30, seed=6, max_metric=70_000)
    m = topo.lsdb.adjs["metric"]
    assert int(m.max()) >= 65536
    if cap is not None:
        m[:] = np.minimum(m, cap)
        assert int(m.max()) == cap and int(np.sum(m == cap)) >= 1
        if bump:
            m[int(np.argmax(m == cap))] = cap + 1
            assert int(m.max()) == cap + 1 and int(np.sum(m > cap)) == 1
    return topo


def test_metric_past_16_bits_takes_hbm():
    with Graph(wan_metrics()) as g:
        assert int(g.csr[2].max()) >= 65536 and int(g.csr[2].max()) * g.n < 2 ** 32
        srcs = list(range(g.n))
        res, _ = g.run(srcs, ("HBM",))
        g.check_oracle(res, srcs)


def test_metric_65535_is_staged_and_65536_is_not():
    """cw[e] = head | metric << 16 of the staged graph at its last metric."""
    with Graph(wan_metrics(cap=65535)) as g:
        assert int(g.csr[2].max()) == 65535
        srcs = list(range(g.n))
        res, _ = g.run(srcs, STAGED)
        g.check_oracle(res, srcs)
    with Graph(wan_metrics(cap=65535, bump=True)) as g:
        assert int(g.csr[2].max()) == 65536
        res, _ = g.run(srcs, ("HBM",))
        g.check_oracle(res, srcs)


def test_65536_directed_edges_take_hbm():
    """300 nodes, 32800 links (most node pairs joined, many by parallel
    links), metrics 1-2: up to ~100 equal-cost link-disjoint paths per pair."""
    with Graph(T.random_graph(300, 32800, 21, max_metric=2, overload_frac=0.02)) as g:
        rp, col, met, lid, ovl = g.csr
        assert len(col) >= 65536 and int(met.max()) < 65536 and int(np.diff(rp).max()) < 32768
        drained = np.nonzero(ovl)[0]
        srcs = [0, 150, 299, int(drained[0])]  # (a drained source is expanded all the same)
        assert len(drained) >= 2 and len(set(srcs)) == 4
        res, _ = g.run(srcs, ("HBM",))
        assert int(res.pairs["n_paths"].max()) > 64  # more paths than lanes in a wave
        g.check_oracle(res, srcs)


def test_staged_graph_past_lds_takes_hbm():
    with Graph(T.random_graph(1000, 15000, 22, max_metric=3, overload_frac=0.01)) as g:
        rp, col, met, lid, ovl = g.csr
        assert len(col) < 65536 and int(np.diff(rp).max()) < 32768
        assert np.all(np.bincount(lid)[np.unique(lid)] == 2)  # every link one edge pair
        rng = np.random.default_rng(9)
        srcs = sorted(int(x) for x in rng.choice(g.n, 4, replace=False))
        dsts = sorted(int(x) for x in rng.choice(g.n, 100, replace=False))
        res, _ = g.run(srcs, ("HBM",))
        g.check_oracle(res, srcs, dsts)


def test_rows_past_lds_take_exact():
    """Positive u32 metrics, 6000 nodes: neither the staged graph nor the HBM
    kernel's per-wave rows fit 160 KB -- the exact kernel, nothing forced."""
    with Graph(T.wan(6000, 2000, seed=8)) as g:
        assert int(g.csr[2].min()) > 0 and int(g.csr[2].max()) * g.n < 2 ** 32 and g.n <= 65535
        rng = np.random.default_rng(10)
        srcs = sorted(int(x) for x in rng.choice(g.n, 2, replace=False))
        dsts = sorted(int(x) for x in rng.choice(g.n, 40, replace=False))
        res, _ = g.run(srcs, ("EXACT",))
        g.check_oracle(res, srcs, dsts)


# ---- c. chunks, grabs, bucket width -----------------------------------------------------
GRAPHS = [("ring", ring), ("rand3", rand3)]
KINDS = [("hbm", ("HBM",)), ("staged", STAGED)]
on_graphs = pytest.mark.parametrize("gname,make", GRAPHS, ids=[x[0] for x in GRAPHS])
on_kinds = pytest.mark.parametrize("kname,kinds", KINDS, ids=[x[0] for x in KINDS])


def seven_sources(n):
    return sorted(int(x) for x in np.random.default_rng(11).choice(n, 7, replace=False))


@on_graphs
@on_kinds
def test_chunk_grab_delta_give_the_same_paths(gname, make, kname, kinds, monkeypatch):
    if kname == "hbm":
        monkeypatch.setenv("SPF_KSP2_HBM", "1")
    with Graph(make()) as g:
        srcs = seven_sources(g.n)
        base, c_base = g.run(srcs, kinds)
        if gname == "ring":
            g.check_oracle(base, srcs[:2], sorted(
                int(x) for x in np.random.default_rng(12).choice(g.n, 30, replace=False)))
            assert int(ksp2_canonical(base)[1].max()) > 512  # deeper than a compact wave's stack
            assert (c_base[3] > 0) == (kname == "staged")    # ... whose pairs are redone
        else:
            g.check_oracle(base, srcs)
        for var, val in (("SPF_KSP2_CHUNK", 1), ("SPF_KSP2_CHUNK", 3), ("SPF_KSP2_GRAB", 64),
                         ("SPF_KSP2_DELTA", 1), ("SPF_KSP2_DELTA", 4294967295)):
            monkeypatch.setenv(var, str(val))
            p = g.eng.ksp2_plan(srcs)
            info = p.info()
            p.close()
            assert info.kind in kinds
            assert getattr(info, var[len("SPF_KSP2_"):].lower()) == val, (var, info)
            res, c = g.run(srcs, kinds)
            monkeypatch.delenv(var)
            assert_same_paths(base, res, (gname, kname, var, val))
            assert c[1] == c_base[1], (var, val)


# ---- d. a pool that is too small ------------------------------------------------------
def execute_into(g, plan, srcs, pool_words, null_pool=False):
    """One execute into a sentinel-filled pool of pool_words + 4096 words, told
    it holds pool_words (or into no pool at all): counters, result, and whether
    the words past pool_words still hold the sentinel."""
    pairs = DeviceArray(len(srcs) * g.n * 4, np.uint32)
    cnt = DeviceArray(4, np.uint64, zero=True)
    pool = DeviceArray(pool_words + 4096, np.uint32)
    try:
        pool.upload(np.full(pool_words + 4096, SENTINEL, np.uint32))
        plan.execute(pairs.ptr, 0 if null_pool else pool.ptr, pool_words, cnt.ptr)
        g.eng.check()
        c = cnt.numpy().astype(np.int64)
        words = pool.numpy()
        res = Ksp2Result(np.asarray(srcs, np.uint32), g.n, pairs.numpy().view(PAIR_DTYPE).copy(),
                         words[:pool_words].copy())
        return c, res, bool(np.all(words[pool_words:] == SENTINEL))
    finally:
        for b in (pairs, cnt, pool):
            b.free()


@on_graphs
@on_kinds
def test_pool_overflow_is_reported_and_contained(gname, make, kname, kinds, monkeypatch):
    if kname == "hbm":
        monkeypatch.setenv("SPF_KSP2_HBM", "1")
    with Graph(make()) as g:
        srcs = seven_sources(g.n)
        want, c_want = g.run(srcs, kinds)
        plan = g.eng.ksp2_plan(srcs)
        assert plan.info().kind in kinds
        need = int(ksp2_canonical(want)[1].sum() + 2 * len(ksp2_canonical(want)[1]))  # records, no slack
        assert need >= 8
        small = need // 4
        c, _, tail_ok = execute_into(g, plan, srcs, small)
        assert c[2] & 1 and c[0] >= small and tail_ok, (c, small, tail_ok)
        claimed = int(c[0])
        assert claimed >= need  # the counter kept counting what was wanted
        # no room at all: a pool of 0 words, and no pool
        c0, _, tail_ok = execute_into(g, plan, srcs, 0)
        assert c0[2] & 1 and c0[0] >= need and tail_ok, (c0, tail_ok)
        c0, _, tail_ok = execute_into(g, plan, srcs, 0, null_pool=True)
        assert c0[2] & 1 and c0[0] >= need and tail_ok, (c0, tail_ok)
        # sized from the overflowed run's counter, as run_plan sizes it
        words = claimed + claimed // 4 + 2 ** 20
        c, res, tail_ok = execute_into(g, plan, srcs, words)
        assert not (c[2] & 3) and c[0] <= words and tail_ok, (c, words, tail_ok)
        assert c[1] == c_want[1]
        assert_same_paths(want, res, (gname, kname, "resized pool"))
        if gname == "ring":
            g.check_oracle(res, srcs[:2], sorted(
                int(x) for x in np.random.default_rng(13).choice(g.n, 30, replace=False)))
        else:
            g.check_oracle(res, srcs)
        plan.close()


# ---- e. spf_ksp2_solve's repack, and the info call's refusal ----------------------------
def test_solve_repack_is_the_same_on_either_kernel(monkeypatch):
    with Graph(rand3()) as g:
        srcs = list(range(g.n))
        out = {}
        for kname, kinds in KINDS:
            if kname == "hbm":
                monkeypatch.setenv("SPF_KSP2_HBM", "1")
            else:
                monkeypatch.delenv("SPF_KSP2_HBM")
            p = g.eng.ksp2_plan(srcs)
            info = p.info()
            print(f"ksp2 plan: {info}")
            assert info.kind in kinds
            # a NULL output is refused, the plan stays usable
            assert N.lib.spf_ksp2_plan_info(p._h, None) == N.SPF_E_INVALID
            assert p.info() == info
            p.close()
            out[kname] = g.eng.ksp2(srcs)
        a, b = out["hbm"], out["staged"]
        assert len(a.pool) == len(b.pool) and len(a.pool) > 0  # pool_used
        assert a.pairs.tobytes() == b.pairs.tobytes()
        assert a.pool.tobytes() == b.pool.tobytes()
        g.check_oracle(a, srcs)
