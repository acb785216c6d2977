// ============================================================================
//  whatif_pool_host.h -- the part of a list pool's _db call (pool_db,
//  whatif_pool.cpp) that needs no device, as whatif_routes_host.h:
//  tests/host/whatif_pool_host_check.cpp runs it on the CPU.  The checks come
//  before the owner's slice is copied to the host, the order after it, so they
//  are two functions.
// ============================================================================
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "openr_spf.h"

namespace spfi {

// An owner's slice [lo, hi) of a pool of `total` entries, for a caller with
// room for `cap` entries who wants them (`want`: an output array is not NULL)
// or only their number.  SPF_E_HIP: the offsets decrease or end past the pool
// (*n untouched).  Otherwise *n = hi - lo (n may be NULL), and SPF_E_NOMEM
// when the entries are wanted and cap < *n.  *copy: there is something to copy.
spf_status pool_slice(uint64_t lo, uint64_t hi, uint64_t total, bool want, uint64_t cap, uint64_t* n,
                      bool* copy);

// The order a _db call returns a slice's m entries in: order[k] = the index in
// the slice of the k-th entry, ascending by (key, val).
std::vector<size_t> pool_order(const uint32_t* key, const uint64_t* val, size_t m);

}  // namespace spfi
