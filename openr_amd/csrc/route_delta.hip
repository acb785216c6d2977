// ============================================================================
//  route_delta.hip -- every node's route-database delta between two passes
//  (spf_mplan_route_delta, mplan_routes.cpp).
//
//  Reference: DecisionRouteDb::calculateUpdate in openr/decision/Decision.cpp
//    :111-146   routes to update (new, or the entry differs) and routes to
//               delete (gone), unicast and MPLS, against the previous database
//  for every me at once, over the databases spf_mplan_route_records and
//  spf_mplan_label_routes materialised: the old generation held by a
//  spf_route_snapshot, the new one by the plan.  A route's value is its set of
//  next hops, each a (link identity, metric) pair -- interface, neighbour,
//  address and area follow from the link as seen from me -- and for a label
//  route its owner too (the PHP / SWAP action follows from it).
//
//  Records name CSR edges, and the CSR moves between generations (a row patch
//  reorders a row's slots, a reload may re-issue link ids), so edges compare
//  through key[e] = link_hash[link_id[e]] of their own generation:
//    fast path  me's row has the same key sequence in both generations
//               (delta_rows_kernel decides it per me): equal routes have equal
//               records position by position, up to the row's start;
//    set path   otherwise: equal counts and every old (key, metric) among the
//               new ones (a route keeps at most one next hop per link, so the
//               keys of one route are distinct and this is set equality).  One
//               lane does a route's whole search: c^2 / 2 record loads for c
//               next hops, c <= deg(me) (below 65,536 for IP routes by the
//               header's count field, unbounded for label routes).  Only the
//               me whose row moved take it -- the ends of the changed links --
//               so the bound is deg(me)^2 per route of those few me; a hub of
//               tens of thousands of links whose row moved would want a
//               sorted merge instead.
//  Output per member, CSR-shaped and exactly sized: three ordinary launches --
//  count (a kind byte per route, a count per block), the label routes'
//  deterministic scan over the block counts, fill.  No workgroup waits for
//  another and no route takes an atomic: the launch boundaries order the
//  passes.
// ============================================================================
#include "engine_internal.h"

using namespace spfi;

namespace {

constexpr uint32_t kDlThreads = 256;  // routes per block, one per thread
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint8_t kSame = 0, kUpdate = 1, kDelete = 2;

// same[slot] = 1 when me's row holds the same key sequence in both
// generations (dead slots included: their key is whatever the caller's
// link_hash holds for the withdrawn id).  One block per me slot.
__global__ __launch_bounds__(kDlThreads) void delta_rows_kernel(
    const uint32_t* __restrict__ me_ids, const uint32_t* __restrict__ row_ptr,
    const uint32_t* __restrict__ old_e0, const uint32_t* __restrict__ old_deg,
    const unsigned long long* __restrict__ key_old, const unsigned long long* __restrict__ key_new,
    uint32_t* __restrict__ same) {
  const uint32_t slot = blockIdx.x, me = me_ids[slot];
  const uint32_t e0n = row_ptr[me], dn = row_ptr[me + 1] - e0n;
  const uint32_t e0o = old_e0[slot], dold = old_deg[slot];
  int ok = dn == dold;
  if (ok)
    for (uint32_t i = threadIdx.x; i < dn; i += kDlThreads) ok &= key_old[e0o + i] == key_new[e0n + i];
  ok = __syncthreads_and(ok);
  if (threadIdx.x == 0) same[slot] = ok ? 1u : 0u;
}

// Two routes' records: old record i at ro[i * so], new record j at rn[j * sn],
// n of each (the counts were equal).  Block-uniform `same` picks the path.
__device__ __forceinline__ bool records_equal(const unsigned long long* __restrict__ ro, uint32_t so,
                                              const unsigned long long* __restrict__ rn, uint32_t sn,
                                              uint32_t n, bool same, uint32_t e0o, uint32_t e0n,
                                              const unsigned long long* __restrict__ key_old,
                                              const unsigned long long* __restrict__ key_new) {
  if (same) {
    // the rows agree slot by slot: records are in link order on both sides
    const unsigned long long shift = (unsigned long long)e0n - e0o;  // (mod 2^32 below)
    bool eq = true;
    for (uint32_t k = 0; k < n; ++k) {
      const unsigned long long a = ro[(size_t)k * so], b = rn[(size_t)k * sn];
      eq &= (a >> 32) == (b >> 32) && (uint32_t)(a + shift) == (uint32_t)b;
    }
    return eq;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const unsigned long long a = ro[(size_t)i * so];
    const unsigned long long ka = key_old[(uint32_t)a];
    bool found = false;
    for (uint32_t j = 0; j < n && !found; ++j) {
      const unsigned long long b = rn[(size_t)j * sn];
      found = (a >> 32) == (b >> 32) && key_new[(uint32_t)b] == ka;
    }
    if (!found) return false;
  }
  return true;
}

// IP routes.  A thread per destination set, a run of blocks per me: the lanes
// of a wave read 64 consecutive headers and, record position by record
// position, the adjacent slots of one tile row of either pool (the tiled
// layout of spf_mplan_route_records).  old_hdr[slot] / old_pool[slot]: device
// addresses of me's old headers and of its old region (on a peer device when
// the old database lives on another member).  kind[slot * S + p], and the
// block's changed routes into blk[blockIdx].
__global__ __launch_bounds__(kDlThreads) void delta_ip_kernel(
    const unsigned long long* __restrict__ new_hdr, const unsigned long long* __restrict__ new_pool,
    const unsigned long long* __restrict__ new_base, const unsigned long long* __restrict__ old_hdr,
    const unsigned long long* __restrict__ old_pool, const uint32_t* __restrict__ me_ids,
    const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ old_e0,
    const uint32_t* __restrict__ same, const unsigned long long* __restrict__ key_old,
    const unsigned long long* __restrict__ key_new, uint32_t S, uint32_t n_chunks,
    uint8_t* __restrict__ kind, unsigned long long* __restrict__ blk) {
  const uint32_t slot = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
  const uint32_t p = chunk * kDlThreads + threadIdx.x;
  uint8_t kd = kSame;
  if (p < S) {
    const unsigned long long ho = reinterpret_cast<const unsigned long long*>(old_hdr[slot])[p];
    const unsigned long long hn = new_hdr[(size_t)slot * S + p];
    const uint32_t co = (uint32_t)(ho >> 32) & 0xFFFFu, cn = (uint32_t)(hn >> 32) & 0xFFFFu;
    if (cn == 0) {
      kd = co ? kDelete : kSame;
    } else if (co != cn) {
      kd = kUpdate;
    } else {
      const unsigned long long* ro =
          reinterpret_cast<const unsigned long long*>(old_pool[slot]) + (uint32_t)ho;
      const unsigned long long* rn = new_pool + new_base[slot] + (uint32_t)hn;
      const bool eq = records_equal(ro, (uint32_t)(ho >> 48), rn, (uint32_t)(hn >> 48), cn, same[slot] != 0,
                                    old_e0[slot], row_ptr[me_ids[slot]], key_old, key_new);
      kd = eq ? kSame : kUpdate;
    }
    kind[(size_t)slot * S + p] = kd;
  }
  const int c = __syncthreads_count(kd != kSame);
  if (threadIdx.x == 0) blk[blockIdx.x] = (unsigned long long)c;
}

// Label routes.  A thread per label of the union of both generations' labels
// (ascending), a run of blocks per me: map_old[u] / map_new[u] = the label's
// group index in its generation (kNone: not advertised then).  A route exists
// when its owner is not SPF_UNREACHABLE; the owner is part of its value; a
// route me owns itself (POP_AND_LOOKUP) has no records to compare.
// old_owner[slot] / old_ptr[slot] / old_rec[slot]: device addresses of me's first
// entry in the old owner array and in the old offset array (both one CSR over
// every (me slot, group) of that member, G_old entries per me: the end of me's
// last route is the next me's first offset, or the total behind the last
// entry) and of the old record pool those offsets index.
__global__ __launch_bounds__(kDlThreads) void delta_label_kernel(
    const uint32_t* __restrict__ new_owner, const unsigned long long* __restrict__ new_ptr,
    const unsigned long long* __restrict__ new_rec, uint32_t Gn,
    const unsigned long long* __restrict__ old_owner, const unsigned long long* __restrict__ old_ptr,
    const unsigned long long* __restrict__ old_rec, const uint32_t* __restrict__ map_old,
    const uint32_t* __restrict__ map_new, const uint32_t* __restrict__ me_ids,
    const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ old_e0,
    const uint32_t* __restrict__ same, const unsigned long long* __restrict__ key_old,
    const unsigned long long* __restrict__ key_new, uint32_t U, uint32_t n_chunks,
    uint8_t* __restrict__ kind, unsigned long long* __restrict__ blk) {
  const uint32_t slot = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
  const uint32_t u = chunk * kDlThreads + threadIdx.x;
  uint8_t kd = kSame;
  if (u < U) {
    const uint32_t me = me_ids[slot];
    const uint32_t go = map_old[u], gn = map_new[u];
    const uint32_t* oo = reinterpret_cast<const uint32_t*>(old_owner[slot]);
    const unsigned long long* po = reinterpret_cast<const unsigned long long*>(old_ptr[slot]);
    const uint32_t own_o = go != kNone ? oo[go] : kInf;
    const uint32_t own_n = gn != kNone ? new_owner[(size_t)slot * Gn + gn] : kInf;
    if (own_n == kInf) {
      kd = own_o != kInf ? kDelete : kSame;
    } else if (own_o != own_n) {
      kd = kUpdate;  // a new route, or another owner (another action) over whatever next hops
    } else if (own_n != me) {
      const unsigned long long o0 = po[go], o1 = po[go + 1];
      const unsigned long long n0 = new_ptr[(size_t)slot * Gn + gn], n1 = new_ptr[(size_t)slot * Gn + gn + 1];
      if (o1 - o0 != n1 - n0) {
        kd = kUpdate;
      } else {
        const unsigned long long* ro = reinterpret_cast<const unsigned long long*>(old_rec[slot]) + o0;
        const bool eq = records_equal(ro, 1u, new_rec + n0, 1u, (uint32_t)(n1 - n0), same[slot] != 0,
                                      old_e0[slot], row_ptr[me], key_old, key_new);
        kd = eq ? kSame : kUpdate;
      }
    }
    kind[(size_t)slot * U + u] = kd;
  }
  const int c = __syncthreads_count(kd != kSame);
  if (threadIdx.x == 0) blk[blockIdx.x] = (unsigned long long)c;
}

// Fill: blk holds the exclusive scan of the block counts (blk[n_me * n_chunks]
// = the total).  Each block ranks its changed routes in route order and writes
// their entries -- the cell's value (vals[cell], or the cell index itself) with
// SPF_DELTA_DELETE set on a delete -- at blk[blockIdx] + rank: ascending within a
// me.  dptr[slot] = me's first entry, dptr[n_me] = the total; deletes[0] += the
// deleted routes, one atomic per block that has any.
__global__ __launch_bounds__(kDlThreads) void delta_fill_kernel(
    const uint8_t* __restrict__ kind, uint32_t C, uint32_t n_chunks, uint32_t n_me,
    const unsigned long long* __restrict__ blk, const uint32_t* __restrict__ vals,
    uint32_t* __restrict__ dset, unsigned long long* __restrict__ dptr,
    unsigned long long* __restrict__ deletes) {
  const uint32_t slot = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
  const uint32_t cell = chunk * kDlThreads + threadIdx.x;
  const uint8_t kd = cell < C ? kind[(size_t)slot * C + cell] : kSame;
  const bool hit = kd != kSame;
  __shared__ uint32_t s_wave[kDlThreads / 64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(hit);
  if (lane == 0) s_wave[w] = (uint32_t)__popcll(mask);
  __syncthreads();
  uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
  for (uint32_t k = 0; k < w; ++k) rank += s_wave[k];
  const unsigned long long at = blk[blockIdx.x];
  if (hit) dset[at + rank] = (vals ? vals[cell] : cell) | (kd == kDelete ? SPF_DELTA_DELETE : 0u);
  const int nd = __syncthreads_count(kd == kDelete);
  if (threadIdx.x == 0) {
    if (nd) atomicAdd(deletes, (unsigned long long)nd);
    if (chunk == 0) {
      dptr[slot] = at;
      if (slot == 0) dptr[n_me] = blk[(size_t)n_me * n_chunks];
    }
  }
}

}  // namespace

namespace spfi {

uint32_t route_delta_chunks(uint32_t cells) { return (cells + kDlThreads - 1) / kDlThreads; }

spf_status launch_delta_rows(spf_ctx* c, const RouteDeltaIn& in, uint32_t n_me, hipStream_t s) {
  if (!n_me) return SPF_OK;
  hipLaunchKernelGGL(delta_rows_kernel, dim3(n_me), dim3(kDlThreads), 0, s, in.me, c->d_row_ptr.p, in.old_e0,
                     in.old_deg, in.key_old, in.key_new, in.same);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_delta_ip(spf_ctx* c, const RouteDeltaIn& in, uint32_t n_me, uint32_t S,
                           const unsigned long long* new_hdr, const unsigned long long* new_pool,
                           const unsigned long long* new_base, const unsigned long long* old_hdr,
                           const unsigned long long* old_pool, uint8_t* kind, unsigned long long* blk,
                           hipStream_t s) {
  if (!n_me || !S) return SPF_OK;
  const uint64_t blocks = (uint64_t)n_me * route_delta_chunks(S);
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "route delta: grid too large");
  hipLaunchKernelGGL(delta_ip_kernel, dim3((uint32_t)blocks), dim3(kDlThreads), 0, s, new_hdr, new_pool,
                     new_base, old_hdr, old_pool, in.me, c->d_row_ptr.p, in.old_e0, in.same, in.key_old,
                     in.key_new, S, route_delta_chunks(S), kind, blk);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_delta_labels(spf_ctx* c, const RouteDeltaIn& in, uint32_t n_me, uint32_t U,
                               const uint32_t* new_owner, const unsigned long long* new_ptr,
                               const unsigned long long* new_rec, uint32_t Gn,
                               const unsigned long long* old_owner, const unsigned long long* old_ptr,
                               const unsigned long long* old_rec, const uint32_t* map_old,
                               const uint32_t* map_new, uint8_t* kind, unsigned long long* blk,
                               hipStream_t s) {
  if (!n_me || !U) return SPF_OK;
  const uint64_t blocks = (uint64_t)n_me * route_delta_chunks(U);
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "route delta: grid too large");
  hipLaunchKernelGGL(delta_label_kernel, dim3((uint32_t)blocks), dim3(kDlThreads), 0, s, new_owner, new_ptr,
                     new_rec, Gn, old_owner, old_ptr, old_rec, map_old, map_new, in.me, c->d_row_ptr.p,
                     in.old_e0, in.same, in.key_old, in.key_new, U, route_delta_chunks(U), kind, blk);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_delta_fill(spf_ctx* c, const uint8_t* kind, uint32_t cells, uint32_t n_me,
                             const unsigned long long* blk, const uint32_t* vals, uint32_t* dset,
                             unsigned long long* dptr, unsigned long long* deletes, hipStream_t s) {
  if (!n_me || !cells) return SPF_OK;
  const uint32_t n_chunks = route_delta_chunks(cells);
  hipLaunchKernelGGL(delta_fill_kernel, dim3(n_me * n_chunks), dim3(kDlThreads), 0, s, kind, cells, n_chunks,
                     n_me, blk, vals, dset, dptr, deletes);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

}  // namespace spfi
