// ============================================================================
//  label_routes.hip -- every node's node-label MPLS routes from a RESIDENT
//  all-sources pass (spf_mplan_label_routes, mplan_routes.cpp).
//
//  Reference: SpfSolver::SpfSolverImpl in openr/decision/Decision.cpp
//    buildRouteDb           :586-674    one MPLS route per node segment label:
//                                       the label's owner among the nodes that
//                                       advertise it (:605-617: the smallest
//                                       name that has a route), POP_AND_LOOKUP
//                                       for me's own label, else the next hops
//                                       towards the owner
//    getNextHopsWithMetric  :1107-1196  shortest-path next hops (+ LFA)
//    getNextHopsThrift      :1198-1305  one next hop per up link of me, PHP
//                                       when the link ends at the owner, SWAP
//                                       otherwise
//  for one area.  The selection per (me, owner) is route_sets_kernel's for the
//  destination set {owner} (routes.hip); the output is a CSR-shaped pool sized
//  exactly, built by three ordinary launches per member:
//    count  per (me slot t, label group g): the owner and the kept next hops
//    scan   exclusive scan of the counts into u64 offsets ptr[n_me * G + 1]
//    fill   the links walked again, route (t, g)'s records written
//           contiguously at rec[ptr[t * G + g] ..], in me's link order
//  No workgroup waits for another: the launch boundaries order the passes.
// ============================================================================
#include "engine_internal.h"

#include <cstdlib>

using namespace spfi;

namespace {

constexpr uint64_t kInf64 = ~0ull;
constexpr uint32_t kLrThreads = 256;
constexpr uint32_t kLrGroup = 4;    // consecutive me slots per XCD turn (as route_sets_kernel)
constexpr uint32_t kLrLinks = 256;  // me's links staged in LDS per pass

// A thread per label group, a run of blocks per me (me block-uniform: its CSR
// row, its neighbours' rows arrive once per block through LDS).  Groups are in
// label order; with one advertiser per label in node order consecutive lanes
// read consecutive entries of me's row and bitmaps.
//   rowp[v] / nhp[v]: device addresses of v's u32 distance row and of its first
//   next-hop bitmap (bitmap j = neighbour j, ascending id, wpm words), as
//   route_sets_kernel receives them; with LFA a neighbour's row may live on a
//   peer device.
//   grp_ptr / grp_nodes: label group g's candidates, ascending id (= name).
// Owner (Decision.cpp:605-617): the first candidate that is me or has a finite
// d_me; none: no route (owner = kInf).  Owner == me: POP_AND_LOOKUP, no
// records.  Otherwise per up link e of me towards x: over = w(e) + via(x),
// via(x) = d_me(owner) - d_me(x) when x is a next hop towards the owner,
// lowered (LFA) to d_x(owner) < d_me(owner) + d_x(me); kept when LFA or over ==
// d_me(owner).
// FILL = false: owner[t * G + g] and the count (into ptr[t * G + g], scanned in
// place afterwards).  FILL = true: the same walk, record k of the route at
// rec[ptr[t * G + g] + k] = CSR edge | over << 32; an over past 2^32 - 1 sets
// flags bit 1.
template <bool FILL>
__global__ __launch_bounds__(kLrThreads) void label_routes_kernel(
    const unsigned long long* __restrict__ rowp, const unsigned long long* __restrict__ nhp,
    uint32_t wpm, const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
    const uint32_t* __restrict__ wt, const uint32_t* __restrict__ edge_nb,
    const uint32_t* __restrict__ me_ids, const uint32_t* __restrict__ grp_ptr,
    const uint32_t* __restrict__ grp_nodes, uint32_t G, uint32_t lfa, uint32_t n_me,
    uint32_t n_chunks, uint32_t* __restrict__ owner, unsigned long long* __restrict__ ptr,
    unsigned long long* __restrict__ rec, uint32_t* __restrict__ flags, uint32_t nt) {
  // XCD-aware block order, as route_sets_kernel: me slots in groups of
  // kLrGroup, group q to XCD q % 8, every chunk of one me back to back there
  const uint32_t xg = blockIdx.x & 7u, i = blockIdx.x >> 3;
  const uint32_t L = i / n_chunks;
  const uint32_t slot = ((L / kLrGroup) * 8 + xg) * kLrGroup + L % kLrGroup;
  if (slot >= n_me) return;  // whole block
  const uint32_t me = me_ids[slot];
  const uint32_t g = (i % n_chunks) * kLrThreads + threadIdx.x;
  const bool live = g < G;
  const size_t at = (size_t)slot * G + g;
  const uint32_t* Dme = reinterpret_cast<const uint32_t*>(rowp[me]);
  const uint32_t* NHme = reinterpret_cast<const uint32_t*>(nhp[me]);
  const uint32_t e0 = row_ptr[me], e1 = row_ptr[me + 1];
  uint32_t own = kInf;
  if (live) {
    if constexpr (FILL) {
      own = owner[at];
    } else {
      for (uint32_t k = grp_ptr[g]; k < grp_ptr[g + 1]; ++k) {
        const uint32_t c = grp_nodes[k];
        if (c == me || Dme[c] != kInf) {
          own = c;
          break;
        }
      }
    }
  }
  const bool walk = own != kInf && own != me;
  const uint64_t shortest = walk ? Dme[own] : 0ull;
  unsigned long long* const out = FILL && walk ? rec + ptr[at] : nullptr;
  __shared__ uint32_t s_j[kLrLinks], s_dmx[kLrLinks], s_back[kLrLinks], s_w[kLrLinks];
  __shared__ unsigned long long s_row[kLrLinks];
  uint32_t cnt = 0;
  bool wide = false;
  for (uint32_t c0 = e0; c0 < e1; c0 += kLrLinks) {  // block-uniform
    const uint32_t nl = min(kLrLinks, e1 - c0);
    __syncthreads();  // the previous chunk's reads are done
    for (uint32_t t = threadIdx.x; t < nl; t += kLrThreads) {
      const uint32_t q = c0 + t, x = col[q];
      const unsigned long long rx = lfa && x != me ? rowp[x] : 0ull;
      s_j[t] = edge_nb[q];
      s_dmx[t] = Dme[x];
      s_w[t] = wt[q];
      s_row[t] = rx;
      s_back[t] = rx ? reinterpret_cast<const uint32_t*>(rx)[me] : kInf;
    }
    __syncthreads();
    if (!walk) continue;  // (every thread still meets the barriers)
    for (uint32_t t = 0; t < nl; ++t) {
      if (s_j[t] == kInf) continue;  // a dead slot (no link)
      uint64_t via = kInf64;
      const uint32_t bw = NHme[(size_t)s_j[t] * wpm + (own >> 5)];
      const uint32_t* Dx = reinterpret_cast<const uint32_t*>(s_row[t]);
      const uint32_t dxd = Dx ? Dx[own] : kInf;  // (Dx is null without LFA)
      const uint64_t back = s_back[t];
      if ((bw >> (own & 31)) & 1u) via = shortest - s_dmx[t];
      if (lfa && dxd != kInf && back != kInf && (uint64_t)dxd < shortest + back &&
          (via == kInf64 || via > dxd))
        via = dxd;
      if (via == kInf64) continue;
      const uint64_t over = (uint64_t)s_w[t] + via;
      if (!lfa && over != shortest) continue;
      if constexpr (FILL) {
        // A guard no resident pass can trip (and no test tries to): a pass
        // exists only when max metric x N < 2^32 - 1 (needs64, metric_flags;
        // ls_prefetch_all_sources makes no plan otherwise).  via
        // is a loop-free path x -> owner that avoids me -- the shortest one's
        // tail, or with LFA d_x(owner) < d_me(owner) + d_x(me), which no path
        // through me satisfies -- so it has at most N - 2 links and over =
        // w + via <= max metric x (N - 1).  (shortest + back above is at most
        // max metric x N for the same reason: it fits 32 bits too.)
        wide |= (over >> 32) != 0;
        const unsigned long long r = (unsigned long long)(c0 + t) | (over << 32);
        if (nt)  // (block-uniform)
          __builtin_nontemporal_store(r, out + cnt);
        else
          out[cnt] = r;
      }
      ++cnt;
    }
  }
  if constexpr (FILL) {
    if (wide) atomicOr(flags, 2u);
  } else if (live) {
    owner[at] = own;
    ptr[at] = cnt;
  }
}

// ---- exclusive scan of u64 counts, in place -------------------------------
// Tiles of kScanTile entries: a tile's sum (scan_sums_kernel), the tiles'
// sums scanned by one block (scan_top_kernel, which also writes the grand
// total behind the last entry), each tile scanned from its offset
// (scan_apply_kernel).  Integer sums in a fixed order: deterministic.
constexpr uint32_t kScanPer = 8;
constexpr uint32_t kScanTile = kLrThreads * kScanPer;

// exclusive scan of one value per thread over the block; *total = the block's
// sum.  s_wave = [kLrThreads / 64] words of LDS; every thread calls it.
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long x,
                                                             unsigned long long* total,
                                                             unsigned long long* s_wave) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  unsigned long long v = x;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(v, d, 64);
    if (lane >= d) v += y;
  }
  if (lane == 63) s_wave[w] = v;
  __syncthreads();
  unsigned long long pre = 0, all = 0;
#pragma unroll
  for (uint32_t k = 0; k < kLrThreads / 64; ++k) {
    if (k < w) pre += s_wave[k];
    all += s_wave[k];
  }
  __syncthreads();  // s_wave may be written again
  *total = all;
  return pre + v - x;
}

__global__ __launch_bounds__(kLrThreads) void scan_sums_kernel(
    const unsigned long long* __restrict__ a, unsigned long long n,
    unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long s_wave[kLrThreads / 64];
  const unsigned long long base = (unsigned long long)blockIdx.x * kScanTile + threadIdx.x * kScanPer;
  unsigned long long x = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j)
    if (base + j < n) x += a[base + j];
  unsigned long long total;
  (void)block_excl_scan(x, &total, s_wave);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kLrThreads) void scan_top_kernel(unsigned long long* __restrict__ sums,
                                                              uint32_t n_tiles,
                                                              unsigned long long* __restrict__ end) {
  __shared__ unsigned long long s_wave[kLrThreads / 64];
  unsigned long long carry = 0;
  for (uint32_t b0 = 0; b0 < n_tiles; b0 += kLrThreads) {  // block-uniform
    const uint32_t k = b0 + threadIdx.x;
    const unsigned long long x = k < n_tiles ? sums[k] : 0ull;
    unsigned long long total;
    const unsigned long long ex = block_excl_scan(x, &total, s_wave);
    if (k < n_tiles) sums[k] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *end = carry;
}

__global__ __launch_bounds__(kLrThreads) void scan_apply_kernel(
    unsigned long long* __restrict__ a, unsigned long long n,
    const unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long s_wave[kLrThreads / 64];
  const unsigned long long base = (unsigned long long)blockIdx.x * kScanTile + threadIdx.x * kScanPer;
  unsigned long long v[kScanPer], x = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    v[j] = base + j < n ? a[base + j] : 0ull;
    x += v[j];
  }
  unsigned long long total;
  unsigned long long run = block_excl_scan(x, &total, s_wave) + sums[blockIdx.x];
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    if (base + j < n) a[base + j] = run;
    run += v[j];
  }
}

}  // namespace

namespace spfi {

uint64_t label_scan_tiles(uint64_t n) { return (n + kScanTile - 1) / kScanTile; }
uint32_t label_scan_tile() { return kScanTile; }

spf_status launch_label_routes(spf_ctx* c, bool fill, const unsigned long long* d_rowp,
                               const unsigned long long* d_nhp, const uint32_t* d_me, uint32_t n_me,
                               const uint32_t* d_grp_ptr, const uint32_t* d_grp_nodes, uint32_t G,
                               bool lfa, uint32_t* d_owner, unsigned long long* d_ptr,
                               unsigned long long* d_rec, uint32_t* d_flags, hipStream_t s) {
  if (!n_me || !G) return SPF_OK;
  const uint32_t n_chunks = (G + kLrThreads - 1) / kLrThreads;
  const uint32_t groups = (n_me + kLrGroup - 1) / kLrGroup;
  const uint64_t blocks = 8ull * ((groups + 7) / 8 * kLrGroup) * n_chunks;
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "label routes: grid too large");
  const dim3 grid((uint32_t)blocks), block(kLrThreads);
  const uint32_t wpm = c->pitch / 32, lf = lfa ? 1u : 0u;
  // a route's records go out as the walk finds them, 8 bytes per lane and 64
  // lines per store instruction: streaming (nontemporal) stores, or plain
  // ones that leave the write combining to L2 (SPF_LABEL_NT=0: A/B)
  const char* nte = std::getenv("SPF_LABEL_NT");
  const uint32_t nt = nte && nte[0] == '0' ? 0u : 1u;
  if (fill)
    hipLaunchKernelGGL(label_routes_kernel<true>, grid, block, 0, s, d_rowp, d_nhp, wpm, c->d_row_ptr.p,
                       c->d_col.p, c->d_wt.p, c->d_edge_nb.p, d_me, d_grp_ptr, d_grp_nodes, G, lf, n_me,
                       n_chunks, d_owner, d_ptr, d_rec, d_flags, nt);
  else
    hipLaunchKernelGGL(label_routes_kernel<false>, grid, block, 0, s, d_rowp, d_nhp, wpm, c->d_row_ptr.p,
                       c->d_col.p, c->d_wt.p, c->d_edge_nb.p, d_me, d_grp_ptr, d_grp_nodes, G, lf, n_me,
                       n_chunks, d_owner, d_ptr, d_rec, d_flags, nt);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_label_scan(spf_ctx* c, unsigned long long* d_ptr, uint64_t n,
                             unsigned long long* d_sums, hipStream_t s) {
  if (n == 0) {
    HIP_TRY(c, hipMemsetAsync(d_ptr, 0, 8, s));
    return SPF_OK;
  }
  const uint64_t tiles = label_scan_tiles(n);
  if (tiles >= (1ull << 31)) return fail(c, SPF_E_INVALID, "label routes: scan too large");
  const dim3 grid((uint32_t)tiles), block(kLrThreads);
  hipLaunchKernelGGL(scan_sums_kernel, grid, block, 0, s, d_ptr, (unsigned long long)n, d_sums);
  hipLaunchKernelGGL(scan_top_kernel, dim3(1), block, 0, s, d_sums, (uint32_t)tiles, d_ptr + n);
  hipLaunchKernelGGL(scan_apply_kernel, grid, block, 0, s, d_ptr, (unsigned long long)n, d_sums);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

}  // namespace spfi
