// What the device-side consumers of the failure-major lists share,
// whatif_routes.hip and whatif_impact.hip: their launch arithmetic and the
// failure that owns entry e of a list (the change lists' or the route lists'
// offsets).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace spfi {

// blocks of per_block threads for a thread per item
inline uint32_t blocks_for(unsigned long long items, uint32_t per_block) {
  return (uint32_t)((items + per_block - 1) / per_block);
}

// ptr[0 .. n_fail] ascending, ptr[0] = 0, e < ptr[n_fail], n_fail >= 1: the
// last i with ptr[i] <= e.  Cold failures own nothing (ptr[i] == ptr[i + 1]),
// so a run of them at the start, in the middle or at the end of the plan is
// stepped over: of equal offsets the last one wins, and ptr[i + 1] > e.
__device__ __forceinline__ uint32_t list_owner(const unsigned long long* __restrict__ ptr,
                                               uint32_t n_fail, unsigned long long e) {
  uint32_t lo = 0, hi = n_fail;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

}  // namespace spfi
