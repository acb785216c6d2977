// What the kernels that walk a list by its entries share -- the what-if lists'
// consumers (whatif_routes.hip, whatif_impact.hip, whatif_route_update.hip) and
// the route deltas' payloads (route_update.hip, ksp2_route_delta.hip): their
// launch arithmetic and the owner of entry e under scanned offsets.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spfi {

// blocks of per_block threads for a thread per item
inline uint32_t blocks_for(unsigned long long items, uint32_t per_block) {
  return (uint32_t)((items + per_block - 1) / per_block);
}

// ptr[0 .. n] ascending, ptr[0] = 0, e < ptr[n], n >= 1: the last i with
// ptr[i] <= e.  Owners of nothing (ptr[i] == ptr[i + 1]: cold failures, me
// slots without entries) are stepped over wherever a run of them lies: of
// equal offsets the last one wins, and ptr[i + 1] > e.  I: the owners' index
// type (64 bits where the owners are themselves entries of a list).
template <typename I>
__device__ __forceinline__ I list_owner(const unsigned long long* __restrict__ ptr, I n,
                                        unsigned long long e) {
  I lo = 0, hi = n;  // ptr[lo] <= e < ptr[hi]
  while (hi - lo > 1) {
    const I mid = lo + (hi - lo) / 2;
    if (ptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace spfi
