"""helpers.ksp2_canonical -- the layout-free form the KSP2 path tests compare
results in -- against Ksp2Result.paths() on hand-made pools (no device)."""

import numpy as np
import pytest

from helpers import ksp2_canonical
from openr_amd.engine import KSP2_NONE, PAIR_DTYPE, Ksp2Result


def build(paths, n_src, n, order, slack):
    """paths[(i, d, k)] = [[links]]: records laid out in `order` (a permutation
    of all records), `slack` junk words after each."""
    recs = [(key, q) for key in sorted(paths) for q in range(len(paths[key]))]
    at, pool = {}, []
    for j in order:
        key, q = recs[j]
        at[(key, q)] = len(pool)
        pool += [len(paths[key][q]), 0] + list(paths[key][q]) + [0xDEAD] * slack
    pairs = np.zeros(n_src * n, PAIR_DTYPE)
    pairs["first"] = KSP2_NONE
    for (i, d, k), ps in paths.items():
        pairs["n_paths"][i * n + d, k - 1] = len(ps)
        pairs["first"][i * n + d, k - 1] = at[((i, d, k), 0)]
        for q in range(len(ps)):
            pool[at[((i, d, k), q)] + 1] = at[((i, d, k), q + 1)] if q + 1 < len(ps) else KSP2_NONE
    return Ksp2Result(np.arange(n_src, dtype=np.uint32), n, pairs, np.asarray(pool, np.uint32))


PATHS = {(0, 1, 1): [[5], [7, 8, 9]], (0, 1, 2): [[1, 2]], (0, 2, 1): [[3, 4]],
         (1, 0, 1): [[9, 8, 7], [6], [5, 4]], (1, 0, 2): [[2, 1], [0, 3]]}


def test_canonical_is_layout_free_and_equals_paths():
    n_rec = sum(len(v) for v in PATHS.values())
    a = build(PATHS, 2, 3, list(range(n_rec)), 0)
    b = build(PATHS, 2, 3, list(reversed(range(n_rec))), 3)
    assert a.pool.tobytes() != b.pool.tobytes()
    ca, cb = ksp2_canonical(a), ksp2_canonical(b)
    assert all(np.array_equal(x, y) for x, y in zip(ca, cb))
    flat = [l for i in range(2) for d in range(3) for k in (1, 2) for p in b.paths(i, d, k) for l in p]
    assert ca[2].tolist() == flat
    assert ca[1].tolist() == [len(p) for i in range(2) for d in range(3) for k in (1, 2)
                              for p in b.paths(i, d, k)]
    for (i, d, k), ps in PATHS.items():
        assert b.paths(i, d, k) == ps


@pytest.mark.parametrize("change", ["link", "order", "split"])
def test_canonical_sees_a_difference(change):
    other = {k: [list(p) for p in v] for k, v in PATHS.items()}
    if change == "link":
        other[(1, 0, 2)][1][1] = 4
    elif change == "order":  # the same paths, another list order
        other[(1, 0, 1)] = [other[(1, 0, 1)][1], other[(1, 0, 1)][0], other[(1, 0, 1)][2]]
    else:  # the same links, cut differently
        other[(0, 1, 1)] = [[5, 7], [8, 9]]
    n_rec = sum(len(v) for v in PATHS.values())
    ca = ksp2_canonical(build(PATHS, 2, 3, list(range(n_rec)), 0))
    cb = ksp2_canonical(build(other, 2, 3, list(range(n_rec)), 0))
    assert not all(np.array_equal(x, y) for x, y in zip(ca, cb))
