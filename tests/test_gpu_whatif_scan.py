"""The what-if pools' scan (whatif_scan_kernel) under spf_whatif_routes, past
one tile of counts: a link plan over every up link of a graph with more than
8192 of them, the number no multiple of the 8 counts a thread takes.  The
route lists' offsets must be a scan, and a failure's slice must hold what the
host model of test_gpu_whatif_routes.py derives from that failure's change
list -- at the tile edges (1024 counts was the edge of the scan the route
lists used to have, 8192 is this one's), at the ends and at fifty failures in
between.

No oracle here: the lists are pinned to it at small sizes by
test_gpu_whatif_lists.py and test_gpu_whatif_routes.py, and nine thousand CPU
SPFs are no few-second test.  Barabasi-Albert rather than a grid: from a
grid's corner nearly every node keeps both first hops whatever link fails, so
nearly every count would be zero."""

import numpy as np
import pytest

import whatif_routes as R
from openr_amd import topology as T
from openr_amd.engine import SpfEngine
from openr_amd.link_state import LinkState

pytestmark = pytest.mark.gpu


def test_route_offsets_past_one_scan_tile():
    topo = T.barabasi_albert(3000, 3, seed=4)
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    names, rp, col, met, lid, ovl = ls.flatten()
    s = names.index("0")
    rng = np.random.default_rng(5)
    sets = [[int(v) for v in rng.choice(len(names), int(rng.integers(1, 7)), replace=False)]
            for _ in range(300)]
    flat = R.flatten(sets)
    with SpfEngine(0) as eng:
        eng.load(rp, col, met, lid, ovl)
        with eng.whatif_changes(s) as ch:
            nf = ch.n_fail
            assert nf > 8192 and nf % 8 != 0
            rt = ch.routes(sets)
            assert rt.n_fail == nf and len(rt.ptr) == nf + 1
            assert int(rt.ptr[0]) == 0 and int(rt.ptr[-1]) == rt.n_entries == len(rt.set)
            size = np.diff(rt.ptr.astype(np.int64))
            assert (size >= 0).all()
            # counts on both sides of either tile edge, or the edges would check nothing
            assert size[:1024].any() and size[1024:8192].any() and size[8192:].any()
            base_d, base_nh, W = ch.plan.base()
            base = R.routes(base_d, base_nh, flat, s)
            idx = {0, 1023, 1024, 8191, 8192, nf - 1} | {int(i) for i in np.linspace(0, nf - 1, 50)}
            listed = 0
            for i in sorted(idx):
                node, dist, nh = ch.of(i)
                want = R.expected(base_d, base_nh, node, dist, nh, flat, s, base)
                got = rt.of(i)
                assert len(got[0]) == size[i]
                for g, w, what in zip(got, want, ("sets", "metrics", "words")):
                    assert np.array_equal(g, w), (i, what)
                listed += len(got[0])
            assert listed > 0
