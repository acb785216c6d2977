// ============================================================================
//  prefix_routes.hip -- every node's unicast route decision from prefix
//  entries, over a RESIDENT all-sources pass (spf_mplan_prefix_routes,
//  mplan_prefix_routes.cpp).
//
//  Reference: SpfSolver::SpfSolverImpl in openr/decision/Decision.cpp
//    createRouteForPrefix     :390-554    per me: the advertisers me reaches
//                                         (:411-424), the best of them, no route
//                                         when me is one (:510-513)
//    selectBestRoutes         :725-752    best entries by PrefixMetrics
//                                         (selectBestPrefixMetrics, Util.h:
//                                         541-570), or every entry
//    maybeFilterDrainedNodes  :771-792    without the drained ones, unless all are
//    getMinNextHopThreshold   :755-768    the largest minNexthop of the selected
//    addBestPaths             :1031-1041  fewer next hops than that: no route
//    getNextHopsWithMetric    :1107-1196  shortest-path next hops (+ LFA)
//    getNextHopsThrift        :1198-1305  one next hop per up link of me
//  for one area, perDestination = false, SP_ECMP / IP.  The selection of the
//  set B is per (me, prefix); the next hops are route_sets_kernel's for the
//  set B (routes.hip).  The output is a CSR-shaped pool sized exactly, built by
//  three ordinary launches per member, as label_routes.hip:
//    count  per (me slot t, prefix p): info (best, |B|, status) and the count
//    scan   launch_label_scan over the counts: u64 offsets ptr[n_me * P + 1]
//    fill   the same walk, route (t, p)'s records written contiguously at
//           rec[ptr[t * P + p] ..], in me's link order
//  No workgroup waits for another: the launch boundaries order the passes.
// ============================================================================
#include "engine_internal.h"
#include "prefix_table_host.h"

#include <cstdlib>

using namespace spfi;

namespace {

constexpr uint64_t kInf64 = ~0ull;
constexpr uint32_t kPrThreads = 256;
constexpr uint32_t kPrGroup = 4;    // consecutive me slots per XCD turn (as route_sets_kernel)
constexpr uint32_t kPrLinks = 256;  // me's links staged in LDS per pass

// What one pass over a prefix's entries leaves: of the entries me reaches, the
// ones of the greatest rank (B0) -- all of them (a) and the undrained (u).
// Scalars, no arrays: the kernel selects between a and u by value.
struct Pick {
  uint32_t top = 0;                      // B0's rank
  uint32_t n_a = 0, n_u = 0;             // members
  uint32_t need_a = 0, need_u = 0;       // largest min_nh
  uint32_t near_a = kInf, near_u = kInf;  // smallest d_me
  uint32_t last_a = 0, last_u = 0;       // a member (the member, of a set of one)
  uint32_t low = kInf;                   // B0's smallest id
  bool mine = false, mine_drained = false;  // me in B0; and drained
};

__device__ __forceinline__ Pick pick_entries(const uint4* __restrict__ ent, uint32_t b, uint32_t e,
                                             uint32_t me, const uint32_t* __restrict__ Dme) {
  Pick s;
  for (uint32_t k = b; k < e; ++k) {
    const uint4 x = ent[k];  // node, rank, min_nh, drained
    const uint32_t d = x.x == me ? 0u : Dme[x.x];
    if (d == kInf) continue;
    if (s.n_a == 0 || x.y > s.top) {
      s = Pick();
      s.top = x.y;
    } else if (x.y < s.top) {
      continue;
    }
    ++s.n_a;
    s.need_a = max(s.need_a, x.z);
    s.near_a = min(s.near_a, d);
    s.last_a = x.x;
    if (!x.w) {
      ++s.n_u;
      s.need_u = max(s.need_u, x.z);
      s.near_u = min(s.near_u, d);
      s.last_u = x.x;
    }
    s.low = min(s.low, x.x);
    if (x.x == me) {
      s.mine = true;
      s.mine_drained = x.w != 0;
    }
  }
  return s;
}

// A thread per prefix, a run of blocks per me (me block-uniform: its CSR row,
// its neighbours' rows arrive once per block through LDS).
//   rowp[v] / nhp[v]: device addresses of v's u32 distance row and of its first
//   next-hop bitmap (bitmap j = neighbour j, ascending id, wpm words), as
//   route_sets_kernel receives them; with LFA a neighbour's row may live on a
//   peer device.
//   pfx_ptr / ent: prefix p's entries (PrefixEnt, prefix_table_host.h).
// Per (me, p): B0 = the entries me reaches (node == me, or a finite d_me) of
// the greatest rank; best = me when me is in B0 (not with all_best), else B0's
// smallest id; B = B0 without its drained nodes, or B0 when all are drained.
// B0 empty: NONE.  me in B: SELF.  Otherwise per up link e of me towards x:
// over = w(e) + via(x), via(x) = shortest - d_me(x) when x is a next hop
// towards a member of B at shortest = min over B of d_me, lowered (LFA) to any
// member's d_x(dst) < shortest + d_x(me); kept when LFA or over == shortest.
// None kept: NO_NEXTHOP.  Fewer than B's largest min_nh: MIN_NEXTHOP.  Else
// ROUTE, the only status with records.
// FILL = false: info[t * P + p] = best | |B| << 32 | status << 56 and the
// record count (into ptr[t * P + p], scanned in place afterwards).  FILL =
// true: the ROUTE entries walked again, record k of the route at rec[ptr[t * P
// + p] + k] = CSR edge | over << 32; an over past 2^32 - 1 sets flags bit 1.
template <bool FILL>
__global__ __launch_bounds__(kPrThreads) void prefix_routes_kernel(
    const unsigned long long* __restrict__ rowp, const unsigned long long* __restrict__ nhp,
    uint32_t wpm, const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
    const uint32_t* __restrict__ wt, const uint32_t* __restrict__ edge_nb,
    const uint32_t* __restrict__ me_ids, const uint32_t* __restrict__ pfx_ptr,
    const uint4* __restrict__ ent, uint32_t P, uint32_t lfa, uint32_t all_best, uint32_t n_me,
    uint32_t n_chunks, unsigned long long* __restrict__ info, unsigned long long* __restrict__ ptr,
    unsigned long long* __restrict__ rec, uint32_t* __restrict__ flags) {
  // XCD-aware block order, as route_sets_kernel: me slots in groups of
  // kPrGroup, group q to XCD q % 8, every chunk of one me back to back there
  const uint32_t xg = blockIdx.x & 7u, i = blockIdx.x >> 3;
  const uint32_t L = i / n_chunks;
  const uint32_t slot = ((L / kPrGroup) * 8 + xg) * kPrGroup + L % kPrGroup;
  if (slot >= n_me) return;  // whole block
  const uint32_t me = me_ids[slot];
  const uint32_t p = (i % n_chunks) * kPrThreads + threadIdx.x;
  const bool live = p < P;
  const size_t at = (size_t)slot * P + p;
  const uint32_t* Dme = reinterpret_cast<const uint32_t*>(rowp[me]);
  const uint32_t* NHme = reinterpret_cast<const uint32_t*>(nhp[me]);
  const uint32_t e0 = row_ptr[me], e1 = row_ptr[me + 1];
  const uint32_t b = live ? pfx_ptr[p] : 0u, e = live ? pfx_ptr[p + 1] : 0u;
  // (fill) only a ROUTE is walked again
  const bool pick = FILL ? live && (info[at] >> 56) == SPF_PREFIX_ROUTE : live;
  Pick s;
  if (pick) s = pick_entries(ent, b, e, me, Dme);
  const bool w = s.n_u != 0;  // B: the undrained members, or all
  const uint32_t n_b = w ? s.n_u : s.n_a, need = w ? s.need_u : s.need_a;
  const bool self = s.mine && (!w || !s.mine_drained);
  const bool walk = s.n_a != 0 && !self;
  const uint64_t shortest = w ? s.near_u : s.near_a;
  const bool one = n_b == 1;
  const uint32_t d0 = w ? s.last_u : s.last_a;
  unsigned long long* const out = FILL && walk ? rec + ptr[at] : nullptr;
  __shared__ uint32_t s_j[kPrLinks], s_dmx[kPrLinks], s_back[kPrLinks], s_w[kPrLinks];
  __shared__ unsigned long long s_row[kPrLinks];
  uint32_t cnt = 0;
  bool wide = false;
  for (uint32_t c0 = e0; c0 < e1; c0 += kPrLinks) {  // block-uniform
    const uint32_t nl = min(kPrLinks, e1 - c0);
    __syncthreads();  // the previous chunk's reads are done
    for (uint32_t t = threadIdx.x; t < nl; t += kPrThreads) {
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
      const uint32_t* bm = NHme + (size_t)s_j[t] * wpm;
      const uint32_t* Dx = reinterpret_cast<const uint32_t*>(s_row[t]);  // (null without LFA)
      const uint64_t back = s_back[t];
      if (one) {  // Dme[d0] == shortest
        const uint32_t dxd = Dx ? Dx[d0] : kInf;
        if ((bm[d0 >> 5] >> (d0 & 31)) & 1u) via = shortest - s_dmx[t];
        if (lfa && dxd != kInf && back != kInf && (uint64_t)dxd < shortest + back &&
            (via == kInf64 || via > dxd))
          via = dxd;
      } else {
        // the members of B: me's reachable entries of rank top, undrained when
        // w (me itself is none of them: that is SELF)
        for (uint32_t k = b; k < e; ++k) {
          const uint4 x = ent[k];
          if (x.y != s.top || (w && x.w) || Dme[x.x] != shortest) continue;
          if ((bm[x.x >> 5] >> (x.x & 31)) & 1u) {
            via = shortest - s_dmx[t];
            break;
          }
        }
        if (Dx && back != kInf)
          for (uint32_t k = b; k < e; ++k) {
            const uint4 x = ent[k];
            if (x.y != s.top || (w && x.w) || Dme[x.x] == kInf) continue;
            const uint32_t dxd = Dx[x.x];
            if (dxd == kInf) continue;
            if ((uint64_t)dxd < shortest + back && (via == kInf64 || via > dxd)) via = dxd;
          }
      }
      if (via == kInf64) continue;
      const uint64_t over = (uint64_t)s_w[t] + via;
      if (!lfa && over != shortest) continue;
      // (over fits 32 bits on every resident pass, as in label_routes_kernel:
      // the guard is the same)
      wide |= (over >> 32) != 0;
      if constexpr (FILL) out[cnt] = (unsigned long long)(c0 + t) | (over << 32);
      ++cnt;
    }
  }
  if (wide) atomicOr(flags, 2u);
  if constexpr (!FILL) {
    if (live) {
      uint32_t status = SPF_PREFIX_ROUTE, best = kInf;
      if (s.n_a == 0) {
        status = SPF_PREFIX_NONE;
      } else {
        best = s.mine && !all_best ? me : s.low;
        if (self)
          status = SPF_PREFIX_SELF;
        else if (cnt == 0)
          status = SPF_PREFIX_NO_NEXTHOP;
        else if (need > cnt)
          status = SPF_PREFIX_MIN_NEXTHOP;
      }
      info[at] = (unsigned long long)best | ((unsigned long long)n_b << 32) |
                 ((unsigned long long)status << 56);
      ptr[at] = status == SPF_PREFIX_ROUTE ? cnt : 0u;
    }
  }
}

}  // namespace

namespace spfi {

uint32_t prefix_routes_threads() { return kPrThreads; }
uint32_t prefix_routes_links() { return kPrLinks; }

spf_status launch_prefix_routes(spf_ctx* c, bool fill, const unsigned long long* d_rowp,
                                const unsigned long long* d_nhp, const uint32_t* d_me, uint32_t n_me,
                                const uint32_t* d_pfx_ptr, const PrefixEnt* d_ent, uint32_t P, bool lfa,
                                bool all_best, unsigned long long* d_info, unsigned long long* d_ptr,
                                unsigned long long* d_rec, uint32_t* d_flags, hipStream_t s) {
  static_assert(sizeof(PrefixEnt) == sizeof(uint4), "an entry is one 16-byte load");
  if (!n_me || !P) return SPF_OK;
  const uint32_t n_chunks = (P + kPrThreads - 1) / kPrThreads;
  const uint32_t groups = (n_me + kPrGroup - 1) / kPrGroup;
  const uint64_t blocks = 8ull * ((groups + 7) / 8 * kPrGroup) * n_chunks;
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "prefix routes: grid too large");
  const dim3 grid((uint32_t)blocks), block(kPrThreads);
  const uint32_t wpm = c->pitch / 32, lf = lfa ? 1u : 0u, ab = all_best ? 1u : 0u;
  const uint4* ent = reinterpret_cast<const uint4*>(d_ent);
  if (fill)
    hipLaunchKernelGGL(prefix_routes_kernel<true>, grid, block, 0, s, d_rowp, d_nhp, wpm, c->d_row_ptr.p,
                       c->d_col.p, c->d_wt.p, c->d_edge_nb.p, d_me, d_pfx_ptr, ent, P, lf, ab, n_me,
                       n_chunks, d_info, d_ptr, d_rec, d_flags);
  else
    hipLaunchKernelGGL(prefix_routes_kernel<false>, grid, block, 0, s, d_rowp, d_nhp, wpm, c->d_row_ptr.p,
                       c->d_col.p, c->d_wt.p, c->d_edge_nb.p, d_me, d_pfx_ptr, ent, P, lf, ab, n_me,
                       n_chunks, d_info, d_ptr, d_rec, d_flags);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

}  // namespace spfi
