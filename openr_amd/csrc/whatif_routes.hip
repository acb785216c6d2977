// ============================================================================
//  whatif_routes.hip -- what-if route impact: for every failure of a what-if
//  plan, the destination sets (prefixes) of the source whose route changes.
//
//  A set's route is the reference's getMinCostNodes over its members
//  (Decision.cpp:1082-1105) and the union of the min-cost members' next hops
//  (getNextHopsWithMetric without LFA, :1107-1155), here as
//  (min_metric, nh words) in the change lists' own bitset.  The lists of
//  spf_whatif_changes say which NODES moved under failure i; this unit joins
//  them with the sets on the device:
//    base     the unfailed result in the lists' layout (u64 metric, W words,
//             zero rows where unreachable), every set's base route, and one
//             open-addressed table over all list entries,
//             key (i << 32 | node) -> entry index;
//    count    driven by the entries (i, v): for every set s that holds v,
//             exactly one entry of failure i owns the pair (i, s) -- the
//             changed member that comes first in s's member order.  The owner
//             walks s with patched values (the list entry where the table has
//             one, the base otherwise), takes the min and the OR and compares
//             with the base route;
//    scan     cnt -> rptr (u64);
//    fill     the count pass again, an entry per changed route at
//             rptr[i] + k, k from a per-failure cursor.
//  An entry that is not the owner learns so at the first changed member before
//  its own; sets of up to kLaneSet members are walked by the entry's lane,
//  longer ones by the whole wave (lanes stride the members, min and OR across
//  lanes).  No buffer is n_fail x n_sets or n_fail x n_nodes.
//
//  A set that holds the source is the source's own prefix: metric 0 and no
//  next hops, under every failure; it is never listed (the index leaves it
//  out).  Empty sets and sets unreachable in the base cannot be listed either:
//  no failure kind makes a node reachable.
// ============================================================================
#include "engine_internal.h"
#include "grid_ops.h"
#include "wave_ops.h"
#include "list_owner.h"
#include "whatif_routes_host.h"

#include <numeric>

using namespace spfi;

namespace {

constexpr unsigned long long kNoRoute = ~0ull;  // metric: no member reachable; key: empty slot
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLaneSet = 8;  // members up to which an entry's lane walks a set alone
constexpr uint32_t kThreads = 256;

struct WrArgs {
  // the caller's sets and their inverse index (SetIndex)
  const uint32_t* set_ptr;
  const uint32_t* set_nodes;
  const uint32_t* inv_ptr;
  const uint32_t* inv_set;
  const uint32_t* inv_pos;
  // the unfailed result, lists' layout
  const unsigned long long* bd;
  const uint32_t* bnh;
  // the change lists and their table (keys NULL: no failure, the base pass)
  const uint32_t* cnode;
  const unsigned long long* cdist;
  const uint32_t* cnh;
  const uint32_t* efail;
  const unsigned long long* keys;
  const uint32_t* vals;
  uint32_t mask;
  // base routes (written by the base pass)
  unsigned long long* rbm;
  uint32_t* rbnh;
  // route lists
  uint32_t* cnt;
  uint32_t* cur;
  const unsigned long long* rptr;
  uint32_t* rset;
  unsigned long long* rmet;
  uint32_t* rnh;
  uint32_t* fault;
  uint32_t W, src, n_sets;
  unsigned long long total;
};

__device__ __forceinline__ uint32_t wr_hash(unsigned long long k) {
  k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
  k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)(k ^ (k >> 31));
}

// The entry of node u in failure i's list, kNone when u did not change.  The
// table is at most half full, so a probe ends at an empty slot.
__device__ __forceinline__ uint32_t wr_find(const WrArgs& a, uint32_t i, uint32_t u) {
  if (!a.keys) return kNone;
  const unsigned long long key = ((unsigned long long)i << 32) | u;
  for (uint32_t h = wr_hash(key) & a.mask;; h = (h + 1) & a.mask) {
    const unsigned long long k = a.keys[h];
    if (k == key) return a.vals[h];
    if (k == kNoRoute) return kNone;
  }
}

// min over the wave of a u64 (every lane active): max of the complement, high
// word first, then the low words of the lanes that hold that high word
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long x) {
  const unsigned long long y = ~x;
  const uint32_t hi = wave_max32((uint32_t)(y >> 32));
  const uint32_t lo = wave_max32((uint32_t)(y >> 32) == hi ? (uint32_t)y : 0u);
  return ~(((unsigned long long)hi << 32) | lo);
}

// normalise the plan's unfailed result: u64 metrics, rows zero where nothing is defined
__global__ __launch_bounds__(kThreads) void wr_base_rows_kernel(
    const uint32_t* __restrict__ d32, const unsigned long long* __restrict__ d64,
    const uint32_t* __restrict__ nh, uint32_t N, uint32_t W, uint32_t no_nbr,
    unsigned long long* __restrict__ bd, uint32_t* __restrict__ bnh) {
  const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (uint64_t)N * W) return;
  const uint32_t v = (uint32_t)(t / W);
  const unsigned long long d = d64 ? d64[v] : (d32[v] == kInf ? kNoRoute : d32[v]);
  if (t % W == 0) bd[v] = d;
  bnh[t] = d == kNoRoute || no_nbr ? 0u : nh[t];
}

__global__ __launch_bounds__(kThreads) void wr_table_kernel(
    const unsigned long long* __restrict__ cptr, const uint32_t* __restrict__ cnode, uint32_t n_fail,
    unsigned long long total, unsigned long long* keys, uint32_t* __restrict__ vals, uint32_t mask,
    uint32_t* __restrict__ efail) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const uint32_t lo = list_owner(cptr, n_fail, e);
  efail[e] = lo;
  const unsigned long long key = ((unsigned long long)lo << 32) | cnode[e];
  for (uint32_t h = wr_hash(key) & mask;; h = (h + 1) & mask) {
    if (atomicCAS(&keys[h], kNoRoute, key) == kNoRoute) {
      vals[h] = (uint32_t)e;
      return;
    }
  }
}

// A changed route of failure i: counted, or written at the failure's next slot.
template <bool FILL>
__device__ __forceinline__ unsigned long long wr_claim(const WrArgs& a, uint32_t i) {
  if constexpr (!FILL) {
    atomicAdd(&a.cnt[i], 1u);
    return kNoRoute;
  } else {
    const unsigned long long at = a.rptr[i] + atomicAdd(&a.cur[i], 1u);
    if (at >= a.rptr[i + 1]) {  // more entries than were counted: dropped
      atomicOr(a.fault, kFaultListRoom);
      return kNoRoute;
    }
    return at;
  }
}

// Set s (members set_nodes[b .. b + len), len <= kLaneSet) under failure i, by
// the lane of the entry that is s's member at position pos.
template <bool FILL>
__device__ __forceinline__ void wr_lane(const WrArgs& a, uint32_t i, uint32_t s, uint32_t b,
                                        uint32_t len, uint32_t pos) {
  unsigned long long d[kLaneSet], m = kNoRoute;
  const uint32_t* row[kLaneSet];
  const uint32_t W = a.W;
#pragma unroll
  for (uint32_t k = 0; k < kLaneSet; ++k) {
    d[k] = kNoRoute;
    row[k] = a.bnh;
    if (k < len) {
      const uint32_t u = a.set_nodes[b + k];
      const uint32_t x = wr_find(a, i, u);
      if (x != kNone) {
        if (k < pos) return;  // an earlier changed member owns (i, s)
        d[k] = a.cdist[x];
        row[k] = a.cnh + (size_t)x * W;
      } else {
        d[k] = a.bd[u];
        row[k] = a.bnh + (size_t)u * W;
      }
      m = d[k] < m ? d[k] : m;
    }
  }
  auto word = [&](uint32_t w) {
    uint32_t x = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLaneSet; ++k)
      if (d[k] == m && m != kNoRoute) x |= row[k][w];
    return x;
  };
  bool changed = m != a.rbm[s];
  for (uint32_t w = 0; w < W && !changed; ++w) changed = word(w) != a.rbnh[(size_t)s * W + w];
  if (!changed) return;
  const unsigned long long at = wr_claim<FILL>(a, i);
  if (at == kNoRoute) return;
  a.rset[at] = s;
  a.rmet[at] = m;
  for (uint32_t w = 0; w < W; ++w) a.rnh[at * W + w] = word(w);
}

// Set s by the whole wave (every lane active, the arguments wave-uniform).
// MODE 0: the base route of s into rbm / rbnh; 1: count; 2: fill.
template <int MODE>
__device__ __forceinline__ void wr_wave(const WrArgs& a, uint32_t i, uint32_t s, uint32_t b,
                                        uint32_t len, uint32_t pos, uint32_t lane) {
  const uint32_t W = a.W;
  unsigned long long lm = kNoRoute;
  bool own_prefix = false;  // (base) the set holds the source
  for (uint32_t k0 = 0; k0 < len; k0 += 64) {
    const uint32_t k = k0 + lane;
    bool earlier = false;
    if (k < len) {
      const uint32_t u = a.set_nodes[b + k];
      const uint32_t x = MODE ? wr_find(a, i, u) : kNone;
      const unsigned long long d = x != kNone ? a.cdist[x] : a.bd[u];
      earlier = x != kNone && k < pos;
      own_prefix |= u == a.src;
      lm = d < lm ? d : lm;
    }
    if (__ballot(earlier)) return;  // an earlier changed member owns (i, s)
  }
  const unsigned long long m = wave_min64(lm);
  // word w0 + lane of the OR over the members at the min: the members again,
  // each lane resolving its own; the rows of those at the min are read by the
  // wave together, a word per lane
  auto words = [&](uint32_t w0) {
    uint32_t acc = 0;
    if (m == kNoRoute) return acc;
    for (uint32_t k0 = 0; k0 < len; k0 += 64) {
      const uint32_t k = k0 + lane;
      unsigned long long rp = 0;
      bool at_min = false;
      if (k < len) {
        const uint32_t u = a.set_nodes[b + k];
        const uint32_t x = MODE ? wr_find(a, i, u) : kNone;
        at_min = (x != kNone ? a.cdist[x] : a.bd[u]) == m;
        rp = (unsigned long long)(x != kNone ? a.cnh + (size_t)x * W : a.bnh + (size_t)u * W);
      }
      for (unsigned long long todo = __ballot(at_min); todo; todo &= todo - 1) {
        const uint32_t* r = (const uint32_t*)__shfl(rp, (int)__ffsll((long long)todo) - 1);
        if (w0 + lane < W) acc |= r[w0 + lane];
      }
    }
    return acc;
  };
  if constexpr (MODE == 0) {
    const bool mine = __ballot(own_prefix) != 0;
    if (lane == 0) a.rbm[s] = mine ? 0ull : m;
    for (uint32_t w0 = 0; w0 < W; w0 += 64) {
      const uint32_t acc = words(w0);
      if (w0 + lane < W) a.rbnh[(size_t)s * W + w0 + lane] = mine ? 0u : acc;
    }
  } else {
    bool changed = m != a.rbm[s];
    for (uint32_t w0 = 0; w0 < W && !changed; w0 += 64) {
      const uint32_t acc = words(w0);
      changed = __ballot(w0 + lane < W && acc != a.rbnh[(size_t)s * W + w0 + lane]) != 0;
    }
    if (!changed) return;
    unsigned long long at = kNoRoute;
    if (lane == 0) at = wr_claim<MODE == 2>(a, i);
    at = __shfl(at, 0);
    if (at == kNoRoute) return;
    if (lane == 0) {
      a.rset[at] = s;
      a.rmet[at] = m;
    }
    for (uint32_t w0 = 0; w0 < W; w0 += 64) {
      const uint32_t acc = words(w0);
      if (w0 + lane < W) a.rnh[at * W + w0 + lane] = acc;
    }
  }
}

// every set's base route, a wave per set
__global__ __launch_bounds__(kThreads) void wr_base_routes_kernel(WrArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t s = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (s >= a.n_sets) return;  // wave-uniform
  const uint32_t b = a.set_ptr[s];
  wr_wave<0>(a, 0, (uint32_t)s, b, a.set_ptr[s + 1] - b, 0, lane);
}

// count / fill: a lane per list entry, then the wave over the long sets its lanes met
template <bool FILL>
__global__ __launch_bounds__(kThreads) void wr_routes_kernel(WrArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  uint32_t i = 0, tb = 0, te = 0;
  bool longer = false;
  if (e < a.total) {
    i = a.efail[e];
    const uint32_t v = a.cnode[e];
    tb = a.inv_ptr[v];
    te = a.inv_ptr[v + 1];
    for (uint32_t t = tb; t < te; ++t) {
      const uint32_t s = a.inv_set[t], b = a.set_ptr[s], len = a.set_ptr[s + 1] - b;
      if (len <= kLaneSet) wr_lane<FILL>(a, i, s, b, len, a.inv_pos[t]);
      else longer = true;
    }
  }
  for (unsigned long long todo = __ballot(longer); todo; todo &= todo - 1) {
    const int j = (int)__ffsll((long long)todo) - 1;
    const uint32_t ij = __builtin_amdgcn_readfirstlane(__shfl(i, j));
    const uint32_t tj = __builtin_amdgcn_readfirstlane(__shfl(tb, j));
    const uint32_t ej = __builtin_amdgcn_readfirstlane(__shfl(te, j));
    for (uint32_t t = tj; t < ej; ++t) {
      const uint32_t s = a.inv_set[t], b = a.set_ptr[s], len = a.set_ptr[s + 1] - b;
      if (len > kLaneSet) wr_wave<FILL ? 2 : 1>(a, ij, s, b, len, a.inv_pos[t], lane);
    }
  }
}

}  // namespace

extern "C" {

spf_status spf_whatif_routes(spf_whatif_plan* p, const uint32_t* set_ptr, const uint32_t* set_nodes,
                             uint32_t n_sets, uint64_t* n_entries, uint64_t* pool_bytes,
                             double* kernel_ms, void* stream) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_whatif_routes: NULL plan");
  WiListsView v;
  whatif_lists_view(p, &v);
  spf_ctx* c = v.ctx;
  WiRoutes& r = *v.rt;
  WiPool& R = r.pool;
  const WiPool& L = *v.changes;
  R.valid = false;  // after a failed call the plan holds no route lists
  v.imp[SPF_WHATIF_BY_SET]->pool.valid = false;  // ... and none transposed from the old ones
  v.up->ent.valid = v.up->rec.valid = false;     // ... nor route updates
  if (const char* why = route_sets_check(c->N, set_ptr, set_nodes, n_sets))
    return fail(c, SPF_E_INVALID, "spf_whatif_routes: %s", why);
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (v.epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  if (!L.valid)
    return fail(c, SPF_E_STATE, "spf_whatif_routes: the plan holds no lists (spf_whatif_changes first)");
  if (L.total >> 31)
    return fail(c, SPF_E_NOMEM, "spf_whatif_routes: %llu list entries, the table indexes 2^31",
                (unsigned long long)L.total);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const uint32_t N = c->N, W = v.W, nf = v.n_fail;
  const uint32_t members = n_sets ? set_ptr[n_sets] : 0;

  // host, once per call: the inverse index; the sets and the index go up
  const uint32_t zero = 0;
  const SetIndex ix = route_sets_index(N, n_sets ? set_ptr : &zero, set_nodes, n_sets, v.src);
  for (hipEvent_t& e : r.ev)
    if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  HIP_TRY(c, r.d_set_ptr.upload(n_sets ? set_ptr : &zero, (size_t)n_sets + 1, s));
  HIP_TRY(c, r.d_set_nodes.upload(set_nodes, members, s));
  HIP_TRY(c, r.d_inv_ptr.upload(ix.ptr.data(), ix.ptr.size(), s));
  HIP_TRY(c, r.d_inv_set.upload(ix.set.data(), ix.set.size(), s));
  HIP_TRY(c, r.d_inv_pos.upload(ix.pos.data(), ix.pos.size(), s));
  HIP_TRY(c, r.d_bd.alloc(N));
  HIP_TRY(c, r.d_bnh.alloc((size_t)N * W));
  HIP_TRY(c, r.d_rbm.alloc(std::max<uint32_t>(1, n_sets)));
  HIP_TRY(c, r.d_rbnh.alloc(std::max<size_t>(1, (size_t)n_sets * W)));
  HIP_TRY(c, r.d_cnt.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, r.d_cur.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, R.ptr.alloc((size_t)nf + 1));
  // the table: a power of two >= 2 x entries, so a probe always meets an empty slot
  size_t cap = 64;
  while (cap < 2 * (size_t)L.total) cap <<= 1;
  if (L.total) {
    HIP_TRY(c, r.d_keys.alloc(cap));
    HIP_TRY(c, r.d_vals.alloc(cap));
    HIP_TRY(c, r.d_efail.alloc((size_t)L.total));
  }

  WrArgs a{};
  a.set_ptr = r.d_set_ptr.p;
  a.set_nodes = r.d_set_nodes.p;
  a.inv_ptr = r.d_inv_ptr.p;
  a.inv_set = r.d_inv_set.p;
  a.inv_pos = r.d_inv_pos.p;
  a.bd = r.d_bd.p;
  a.bnh = r.d_bnh.p;
  a.rbm = r.d_rbm.p;
  a.rbnh = r.d_rbnh.p;
  a.fault = c->d_fault.p;
  a.W = W;
  a.src = v.src;
  a.n_sets = n_sets;
  a.total = L.total;

  // base: the unfailed result in the lists' layout, the sets' base routes, the table
  HIP_TRY(c, hipEventRecord(r.ev[0], s));
  hipLaunchKernelGGL(wr_base_rows_kernel, dim3(blocks_for((unsigned long long)N * W, kThreads)),
                     dim3(kThreads), 0, s, v.base_d32,
                     reinterpret_cast<const unsigned long long*>(v.base_d64), v.base_nh, N, W,
                     (uint32_t)v.no_nbr, r.d_bd.p, r.d_bnh.p);
  HIP_TRY(c, hipGetLastError());
  if (n_sets) {
    hipLaunchKernelGGL(wr_base_routes_kernel, dim3(blocks_for(n_sets, kThreads / 64)), dim3(kThreads),
                       0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  const bool work = L.total && !ix.set.empty();  // else: nothing can be listed
  if (work) {
    HIP_TRY(c, hipMemsetAsync(r.d_keys.p, 0xFF, 8 * cap, s));
    hipLaunchKernelGGL(wr_table_kernel, dim3(blocks_for(L.total, kThreads)), dim3(kThreads), 0, s,
                       L.ptr.p, L.key.p, nf, (unsigned long long)L.total, r.d_keys.p, r.d_vals.p,
                       (uint32_t)(cap - 1), r.d_efail.p);
    HIP_TRY(c, hipGetLastError());
  }
  a.cnode = L.key.p;
  a.cdist = L.val.p;
  a.cnh = L.rows.p;
  a.efail = r.d_efail.p;
  a.keys = r.d_keys.p;
  a.vals = r.d_vals.p;
  a.mask = (uint32_t)(cap - 1);
  a.cnt = r.d_cnt.p;
  a.cur = r.d_cur.p;
  // count
  HIP_TRY(c, hipMemsetAsync(r.d_cnt.p, 0, 4ull * std::max<uint32_t>(1, nf), s));
  HIP_TRY(c, hipMemsetAsync(r.d_cur.p, 0, 4ull * std::max<uint32_t>(1, nf), s));
  HIP_TRY(c, hipEventRecord(r.ev[1], s));
  if (work) {
    hipLaunchKernelGGL(wr_routes_kernel<false>, dim3(blocks_for(L.total, kThreads)), dim3(kThreads), 0,
                       s, a);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(r.ev[2], s));
  HIP_TRY(c, whatif_scan(r.d_cnt.p, 1, nf, R.ptr.p, s));
  HIP_TRY(c, hipEventRecord(r.ev[3], s));
  // the pool is sized from the scan's total
  unsigned long long total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, R.ptr.p + nf, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = pool_size(c, &R, total, W, "spf_whatif_routes"); st != SPF_OK) return st;
  // fill
  a.rptr = R.ptr.p;
  a.rset = R.key.p;
  a.rmet = R.val.p;
  a.rnh = R.rows.p;
  if (work && total) {
    hipLaunchKernelGGL(wr_routes_kernel<true>, dim3(blocks_for(L.total, kThreads)), dim3(kThreads), 0,
                       s, a);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(r.ev[4], s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  for (int k = 0; k < 4; ++k) {
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, r.ev[k], r.ev[k + 1]));
    r.ms[k] = ms;
  }
  r.n_sets = n_sets;
  r.tab_mask = work ? (uint32_t)(cap - 1) : 0u;
  R.n_owners = nf;
  R.total = total;
  R.valid = true;
  if (n_entries) *n_entries = total;
  if (pool_bytes) *pool_bytes = spfi::pool_bytes(R);
  if (kernel_ms) *kernel_ms = std::accumulate(r.ms, r.ms + 4, 0.0);
  return SPF_OK;
}

spf_status spf_whatif_routes_timing(const spf_whatif_plan* p, double* ms) {
  if (!p || !ms) return SPF_E_INVALID;
  WiListsView v;
  if (const spf_status st = pool_held(const_cast<spf_whatif_plan*>(p), kPoolRoutes,
                                      "spf_whatif_routes_timing", &v); st != SPF_OK)
    return st;
  for (int k = 0; k < 4; ++k) ms[k] = v.rt->ms[k];
  return SPF_OK;
}

spf_status spf_whatif_routes_buffers(spf_whatif_plan* p, const uint64_t** d_ptr, const uint32_t** d_set,
                                     const uint64_t** d_metric, const uint32_t** d_nh, uint32_t* W,
                                     uint64_t* n_entries) {
  return pool_buffers(p, kPoolRoutes, "spf_whatif_routes_buffers", d_ptr, d_set, d_metric, d_nh, nullptr,
                      W, n_entries);
}

spf_status spf_whatif_routes_base(spf_whatif_plan* p, uint64_t* min_metric, uint32_t* nh) {
  WiListsView v;
  if (const spf_status st = pool_held(p, kPoolRoutes, "spf_whatif_routes_base", &v); st != SPF_OK) return st;
  spf_ctx* c = v.ctx;
  const WiRoutes& r = *v.rt;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = r.n_sets;
  if (min_metric && n) HIP_TRY(c, hipMemcpy(min_metric, r.d_rbm.p, 8 * n, hipMemcpyDeviceToHost));
  if (nh && n) HIP_TRY(c, hipMemcpy(nh, r.d_rbnh.p, 4 * n * v.W, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status spf_whatif_routes_read(spf_whatif_plan* p, uint64_t* ptr, uint32_t* set, uint64_t* min_metric,
                                  uint32_t* nh) {
  return pool_read(p, kPoolRoutes, "spf_whatif_routes_read", ptr, set, min_metric, nh);
}

spf_status spf_whatif_routes_db(spf_whatif_plan* p, uint32_t i, uint32_t* set, uint64_t* min_metric,
                                uint32_t* nh, uint64_t cap, uint64_t* n) {
  return pool_db(p, kPoolRoutes, "spf_whatif_routes_db", i, set, min_metric, nh, cap, n);
}

}  // extern "C"
