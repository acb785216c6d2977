// ============================================================================
//  route_update.hip -- the payload of every node's route-database delta
//  (spf_mplan_route_update, mplan_routes.cpp).
//
//  Reference: DecisionRouteDb::calculateUpdate in openr/decision/Decision.cpp
//    :111-146   a DecisionRouteUpdate carries the updated ENTRIES -- a route's
//               next hops, for an MPLS route its action too -- not only their
//               names
//  spf_mplan_route_delta's lists name the changed routes of every me (set
//  indices, label values); this gathers their next hops out of the plan's
//  CURRENT databases (spf_mplan_route_records' tiled regions, spf_mplan_label_
//  routes' CSR pool; the snapshot is not read) into one exactly sized,
//  contiguous pool per member and kind, parallel to the delta's lists:
//    count  a thread per delta entry j: the records of its route (0 for a
//           delete) into uptr[j], where they start and how far apart they sit
//           into src[j], for a label route its new owner into uowner[j]
//    scan   label_routes.hip's deterministic exclusive scan of uptr, in place
//    fill   a group of lanes per entry, lane k of the group copies records k,
//           k + W, ...: consecutive lanes store consecutive pool words, and
//           consecutive entries' runs are adjacent, so a wave's store covers
//           one contiguous stretch of urec whatever the routes' lengths
//  Three ordinary launches: no workgroup waits for another, no route takes an
//  atomic, the launch boundaries order the passes.
// ============================================================================
#include "engine_internal.h"
#include "list_owner.h"

#include <cstdlib>

using namespace spfi;

namespace {

constexpr uint32_t kUpThreads = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr unsigned long long kSrcMask = (1ull << 48) - 1;  // src[j] = first record | stride << 48

// IP routes.  Entry j = dset[j]: a set index p of me slot list_owner(dptr, n_me, j), SPF_DELTA_DELETE
// set on a delete.  Route (slot, p)'s header = offset | count << 32 | stride <<
// 48 within me's region at base[slot]: record k at pool[base[slot] + offset +
// k * stride] (the stride is the writing kernel's tile width).
__global__ __launch_bounds__(kUpThreads) void update_count_ip_kernel(
    const unsigned long long* __restrict__ dptr, const uint32_t* __restrict__ dset, uint32_t n_me,
    unsigned long long entries, const unsigned long long* __restrict__ hdr,
    const unsigned long long* __restrict__ base, uint32_t S, unsigned long long* __restrict__ uptr,
    unsigned long long* __restrict__ src) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kUpThreads + threadIdx.x;
  if (j >= entries) return;
  const uint32_t v = dset[j];
  unsigned long long cnt = 0, from = 0;
  if (!(v & SPF_DELTA_DELETE)) {
    const uint32_t slot = list_owner(dptr, n_me, j);
    const unsigned long long h = hdr[(size_t)slot * S + v];
    cnt = (h >> 32) & 0xFFFFull;
    from = (base[slot] + (h & 0xFFFFFFFFull)) | (h >> 48) << 48;
  }
  uptr[j] = cnt;
  src[j] = from;
}

// Label routes.  Entry j = dset[j]: a label VALUE; lab[0 .. U) = the labels of
// either generation, ascending (the delta's union), map_new[u] = label u's group
// in the new generation.  The value is searched in lab (it is one of them: the
// delta wrote it from there), the group's owner and offsets are the new
// generation's: a route me owns itself has no records (POP_AND_LOOKUP).
__global__ __launch_bounds__(kUpThreads) void update_count_label_kernel(
    const unsigned long long* __restrict__ dptr, const uint32_t* __restrict__ dset, uint32_t n_me,
    unsigned long long entries, const uint32_t* __restrict__ lab, const uint32_t* __restrict__ map_new,
    uint32_t U, const uint32_t* __restrict__ owner, const unsigned long long* __restrict__ ptr, uint32_t G,
    unsigned long long* __restrict__ uptr, unsigned long long* __restrict__ src,
    uint32_t* __restrict__ uowner) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kUpThreads + threadIdx.x;
  if (j >= entries) return;
  const uint32_t v = dset[j];
  unsigned long long cnt = 0, from = 0;
  uint32_t own = kInf;
  if (!(v & SPF_DELTA_DELETE)) {
    uint32_t lo = 0, hi = U;  // the first u with lab[u] >= v
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (lab[mid] < v)
        lo = mid + 1;
      else
        hi = mid;
    }
    const uint32_t g = lo < U && lab[lo] == v ? map_new[lo] : kNone;
    if (g != kNone && g < G) {  // (an update's label is advertised in the new generation)
      const size_t at = (size_t)list_owner(dptr, n_me, j) * G + g;
      own = owner[at];
      from = ptr[at];
      cnt = ptr[at + 1] - from;
      from |= 1ull << 48;
    }
  }
  uptr[j] = cnt;
  src[j] = from;
  uowner[j] = own;
}

// W lanes per entry, kUpThreads / W entries per block turn, the blocks striding
// over the entries.  uptr = the scanned counts (uptr[entries] = the total).
template <uint32_t W>
__global__ __launch_bounds__(kUpThreads) void update_fill_kernel(
    const unsigned long long* __restrict__ uptr, const unsigned long long* __restrict__ src,
    unsigned long long entries, const unsigned long long* __restrict__ pool,
    unsigned long long* __restrict__ urec) {
  constexpr uint32_t kPer = kUpThreads / W;
  const uint32_t k0 = threadIdx.x % W;
  for (unsigned long long j = (unsigned long long)blockIdx.x * kPer + threadIdx.x / W; j < entries;
       j += (unsigned long long)gridDim.x * kPer) {
    const unsigned long long at = uptr[j], n = uptr[j + 1] - at, s = src[j];
    const unsigned long long* from = pool + (s & kSrcMask);
    const unsigned long long stride = s >> 48;
    for (unsigned long long k = k0; k < n; k += W) urec[at + k] = from[k * stride];
  }
}

}  // namespace

namespace spfi {

uint32_t route_update_group() {
  // lanes per entry of the fill (SPF_UPDATE_GROUP=4|8|16|32|64: A/B)
  const char* e = std::getenv("SPF_UPDATE_GROUP");
  const int w = e ? std::atoi(e) : 0;
  return w == 4 || w == 8 || w == 16 || w == 32 || w == 64 ? (uint32_t)w : 16u;
}

spf_status launch_update_count_ip(spf_ctx* c, const unsigned long long* dptr, const uint32_t* dset,
                                  uint32_t n_me, uint64_t entries, const unsigned long long* hdr,
                                  const unsigned long long* base, uint32_t S, unsigned long long* uptr,
                                  unsigned long long* src, hipStream_t s) {
  if (!entries) return SPF_OK;
  const uint64_t blocks = (entries + kUpThreads - 1) / kUpThreads;
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "route update: grid too large");
  hipLaunchKernelGGL(update_count_ip_kernel, dim3((uint32_t)blocks), dim3(kUpThreads), 0, s, dptr, dset, n_me,
                     (unsigned long long)entries, hdr, base, S, uptr, src);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_update_count_labels(spf_ctx* c, const unsigned long long* dptr, const uint32_t* dset,
                                      uint32_t n_me, uint64_t entries, const uint32_t* lab,
                                      const uint32_t* map_new, uint32_t U, const uint32_t* owner,
                                      const unsigned long long* ptr, uint32_t G, unsigned long long* uptr,
                                      unsigned long long* src, uint32_t* uowner, hipStream_t s) {
  if (!entries) return SPF_OK;
  const uint64_t blocks = (entries + kUpThreads - 1) / kUpThreads;
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "route update: grid too large");
  hipLaunchKernelGGL(update_count_label_kernel, dim3((uint32_t)blocks), dim3(kUpThreads), 0, s, dptr, dset,
                     n_me, (unsigned long long)entries, lab, map_new, U, owner, ptr, G, uptr, src, uowner);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_update_fill(spf_ctx* c, const unsigned long long* uptr, const unsigned long long* src,
                              uint64_t entries, const unsigned long long* pool, unsigned long long* urec,
                              hipStream_t s) {
  if (!entries) return SPF_OK;
  const uint32_t W = route_update_group();
  // (the blocks stride: any grid covers every entry)
  const uint64_t want = (entries + kUpThreads / W - 1) / (kUpThreads / W);
  const dim3 grid((uint32_t)std::min<uint64_t>(want, 1u << 20)), block(kUpThreads);
  const unsigned long long n = entries;
  switch (W) {
    case 4: hipLaunchKernelGGL(update_fill_kernel<4>, grid, block, 0, s, uptr, src, n, pool, urec); break;
    case 8: hipLaunchKernelGGL(update_fill_kernel<8>, grid, block, 0, s, uptr, src, n, pool, urec); break;
    case 32: hipLaunchKernelGGL(update_fill_kernel<32>, grid, block, 0, s, uptr, src, n, pool, urec); break;
    case 64: hipLaunchKernelGGL(update_fill_kernel<64>, grid, block, 0, s, uptr, src, n, pool, urec); break;
    default: hipLaunchKernelGGL(update_fill_kernel<16>, grid, block, 0, s, uptr, src, n, pool, urec); break;
  }
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

}  // namespace spfi
