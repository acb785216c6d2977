"""bench.py's parity plumbing that runs on the host: the link value hash its
KSP2 line feeds spf_ksp2_digest equals the oracle's (the hash the committed
fixtures were made with), for every link of the config-4 WAN graph; and
--dump-outputs' sampling and file format."""

import sys
from pathlib import Path

import numpy as np

from helpers import link_key
from oracle import link_keyhash
from openr_amd import topology as T
from openr_amd.link_state import LinkState

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import bench  # noqa: E402
from bench import link_value_hash  # noqa: E402


def test_link_value_hash_equals_oracle_keyhash():
    topo = T.wan(2000, 1000, seed=1)
    ls = LinkState(device=-1)
    ls.updateAdjacencyDatabases(topo.lsdb)
    lid = ls.flatten()[4]
    links = np.unique(lid)
    assert len(links) == 3000
    for l in links:
        lk = ls._link(int(l))
        (a, b), (c, d) = lk.orderedNames
        assert link_value_hash(a, b, c, d) == link_keyhash(link_key(lk))
    ls.close()


class _Results:
    """A stand-in for a workload after its timed steps: source s has distance
    row s + arange(n) and s % 5 neighbours whose bitmaps are seeded by s."""

    n = 203  # no multiple of 8: the last packed byte is partly used

    def matrix(self, s):
        return np.random.default_rng(s).integers(0, 2, (s % 5, self.n)).astype(bool)

    def reader(self):
        return lambda s: ((s + np.arange(self.n)).astype(np.uint32), self.matrix(s))


def test_dump_outputs_writes_a_fixed_sample_in_float_arrays(tmp_path, monkeypatch):
    wl = _Results()
    info = bench.dump_outputs(wl, str(tmp_path / "a"))
    a = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert sorted(a) == ["dist", "next_hop_rows", "next_hops", "sources"]
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    srcs = a["sources"].astype(int)
    assert len(srcs) == min(bench.DUMP_SOURCES, wl.n) == info["sources"]
    assert len(set(srcs)) == len(srcs)
    rows = a["next_hop_rows"].astype(int)
    for i, s in enumerate(srcs):
        assert np.array_equal(a["dist"][i], s + np.arange(wl.n))
        bits = np.unpackbits(a["next_hops"][rows[i]:rows[i + 1]].astype(np.uint8), axis=1,
                             bitorder="little")[:, :wl.n]
        assert np.array_equal(bits.astype(bool), wl.matrix(int(s)))
    # the same arguments sample the same sources; a smaller budget cuts the sample
    bench.dump_outputs(wl, str(tmp_path / "b"))
    for name, x in a.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / f"{name}.npy"))
    monkeypatch.setattr(bench, "DUMP_BUDGET", 20 * (8 * wl.n + 16))
    cut = bench.dump_outputs(wl, str(tmp_path / "c"))
    assert 0 < cut["sources"] < len(srcs) and cut["bytes"] <= bench.DUMP_BUDGET
    assert np.array_equal(np.load(tmp_path / "c" / "sources.npy"), a["sources"][:cut["sources"]])
