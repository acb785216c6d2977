"""Restatement of what-if impact by destination (spf_whatif_by_node /
spf_whatif_by_set), in numpy.

From failure-major lists -- ptr[n_fail + 1], key[total], dist[total] (U64_MAX:
cut off / withdrawn), nh[total, W] -- and the base per key (base_dist[n_keys],
base_nh[n_keys, W]) it computes what include/openr_spf.h says of
spf_whatif_impact, field by field, and the lists transposed to key-major with
each key's entries ascending by failure.  The lists themselves are pinned to
the CPU oracle by the callers first.
"""

import numpy as np

import whatif_lists as L

U64_MAX = L.U64_MAX
NONE = 0xFFFFFFFF  # SPF_WHATIF_NONE
DTYPE = np.dtype([("n_changed", "<u4"), ("n_unreachable", "<u4"), ("n_metric", "<u4"),
                  ("min_width", "<u4"), ("max_metric", "<u8"), ("max_fail", "<u4"),
                  ("reserved", "<u4")])  # spf_whatif_impact, as the header lays it out


def popcount(rows):
    """Set bits per row of a [n, W] u32 array."""
    rows = np.ascontiguousarray(rows, np.uint32)
    if rows.shape[0] == 0:
        return np.zeros(0, np.int64)
    return np.unpackbits(rows.view(np.uint8).reshape(rows.shape[0], -1), axis=1).sum(axis=1).astype(np.int64)


def owners(ptr):
    """The failure of every entry: entry e belongs to i with ptr[i] <= e < ptr[i + 1]."""
    sizes = np.diff(np.asarray(ptr).astype(np.int64))
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)


def impact(ptr, key, dist, nh, base_dist, base_nh):
    """(imp[n_keys] of DTYPE, tptr[n_keys + 1], tfail[total], tent[total]): the
    summaries, and per key its (failure, entry) pairs ascending by failure."""
    n_keys = len(base_dist)
    key = np.asarray(key).astype(np.int64)
    dist = np.asarray(dist, np.uint64)
    base_dist = np.asarray(base_dist, np.uint64)
    fail = owners(ptr)
    assert len(fail) == len(key) == len(dist) == len(nh)
    finite = dist != U64_MAX
    imp = np.zeros(n_keys, DTYPE)
    imp["n_changed"] = np.bincount(key, minlength=n_keys)
    imp["n_unreachable"] = np.bincount(key[~finite], minlength=n_keys)
    imp["n_metric"] = np.bincount(key[dist != base_dist[key]], minlength=n_keys)
    # the narrowest of the entries that still reach the key; the base's when there is none
    width = np.full(n_keys, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(width, key[finite], popcount(nh)[finite])
    none = np.bincount(key[finite], minlength=n_keys) == 0
    imp["min_width"] = np.where(none, popcount(base_nh), width)
    # the worst finite metric, never below the base (an unreachable base stays U64_MAX)
    worst = base_dist.copy()
    np.maximum.at(worst, key[finite], dist[finite])
    imp["max_metric"] = worst
    at_worst = finite & (dist == worst[key]) & (dist > base_dist[key])
    first = np.full(n_keys, NONE, np.int64)
    np.minimum.at(first, key[at_worst], fail[at_worst])
    imp["max_fail"] = first
    tptr = np.zeros(n_keys + 1, np.uint64)
    tptr[1:] = np.cumsum(imp["n_changed"].astype(np.uint64))
    ent = np.arange(len(key), dtype=np.int64)
    order = np.lexsort((ent, fail, key))
    return imp, tptr, fail[order].astype(np.uint32), ent[order].astype(np.uint64)


def in_key_order(tptr, tfail, tent):
    """A transposition in any order within a key, sorted within each key by
    (failure, entry): how the device arrays compare with impact()'s."""
    slot_key = owners(tptr)
    order = np.lexsort((np.asarray(tent).astype(np.int64), np.asarray(tfail).astype(np.int64), slot_key))
    return np.asarray(tfail)[order], np.asarray(tent)[order]


def lists_of(failures, W):
    """Failure-major lists from per-failure (node, dist, nh) triples."""
    ptr = np.zeros(len(failures) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(f[0]) for f in failures])
    if not failures or not int(ptr[-1]):
        return ptr, np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros((0, W), np.uint32)
    key = np.concatenate([np.asarray(f[0], np.uint32) for f in failures])
    dist = np.concatenate([np.asarray(f[1], np.uint64) for f in failures])
    nh = np.concatenate([np.asarray(f[2], np.uint32).reshape(-1, W) for f in failures])
    return ptr, key, dist, nh
