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
#include "wave_ops.h"
#include "whatif_owner.h"
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
      atomicOr(a.fault, 64u);
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

// rptr[0 .. n] = the exclusive scan of cnt[0 .. n) and the total: one
// workgroup, a count per thread and tile, the DPP wave scan over the two
// halves of a count (64 halves stay below 2^32).
__global__ __launch_bounds__(1024) void wr_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t n,
                                                      unsigned long long* __restrict__ rptr) {
  __shared__ unsigned long long s_wave[16];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint64_t t0 = 0; t0 < n; t0 += 1024) {  // block-uniform
    const uint64_t t = t0 + threadIdx.x;
    const uint32_t x = t < n ? cnt[t] : 0u;
    uint32_t tl = 0, th = 0;
    const uint32_t el = wave_excl_scan(x & 0xFFFFu, &tl);
    const uint32_t eh = wave_excl_scan(x >> 16, &th);
    if (lane == 0) s_wave[wv] = tl + ((unsigned long long)th << 16);
    __syncthreads();
    unsigned long long run = carry + el + ((unsigned long long)eh << 16);
    for (uint32_t w = 0; w < 16; ++w) {
      const unsigned long long sum = s_wave[w];
      if (w < wv) run += sum;
      carry += sum;
    }
    if (t < n) rptr[t] = run;
    __syncthreads();  // s_wave is rewritten by the next tile
  }
  if (threadIdx.x == 0) rptr[n] = carry;
}

uint32_t blocks_for(unsigned long long items, uint32_t per_block) {
  return (uint32_t)((items + per_block - 1) / per_block);
}

spf_status no_routes(spf_whatif_plan* p, const char* who) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "%s: NULL plan", who);
  WiListsView v;
  whatif_lists_view(p, &v);
  if (!v.rt->valid) return fail(v.ctx, SPF_E_STATE, "%s: the plan holds no route lists", who);
  return SPF_OK;
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
  r.valid = false;  // after a failed call the plan holds no route lists
  v.imp[SPF_WHATIF_BY_SET]->valid = false;  // ... and none transposed from the old ones
  if (const char* why = route_sets_check(c->N, set_ptr, set_nodes, n_sets))
    return fail(c, SPF_E_INVALID, "spf_whatif_routes: %s", why);
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (v.epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  if (!v.has_lists)
    return fail(c, SPF_E_STATE, "spf_whatif_routes: the plan holds no lists (spf_whatif_changes first)");
  if (v.total >> 31)
    return fail(c, SPF_E_NOMEM, "spf_whatif_routes: %llu list entries, the table indexes 2^31",
                (unsigned long long)v.total);
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
  HIP_TRY(c, r.d_rptr.alloc((size_t)nf + 1));
  // the table: a power of two >= 2 x entries, so a probe always meets an empty slot
  size_t cap = 64;
  while (cap < 2 * (size_t)v.total) cap <<= 1;
  if (v.total) {
    HIP_TRY(c, r.d_keys.alloc(cap));
    HIP_TRY(c, r.d_vals.alloc(cap));
    HIP_TRY(c, r.d_efail.alloc((size_t)v.total));
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
  a.total = v.total;

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
  const bool work = v.total && !ix.set.empty();  // else: nothing can be listed
  if (work) {
    HIP_TRY(c, hipMemsetAsync(r.d_keys.p, 0xFF, 8 * cap, s));
    hipLaunchKernelGGL(wr_table_kernel, dim3(blocks_for(v.total, kThreads)), dim3(kThreads), 0, s,
                       v.cptr, v.cnode, nf, (unsigned long long)v.total, r.d_keys.p, r.d_vals.p,
                       (uint32_t)(cap - 1), r.d_efail.p);
    HIP_TRY(c, hipGetLastError());
  }
  a.cnode = v.cnode;
  a.cdist = v.cdist;
  a.cnh = v.cnh;
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
    hipLaunchKernelGGL(wr_routes_kernel<false>, dim3(blocks_for(v.total, kThreads)), dim3(kThreads), 0,
                       s, a);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(r.ev[2], s));
  hipLaunchKernelGGL(wr_scan_kernel, dim3(1), dim3(1024), 0, s, r.d_cnt.p, nf, r.d_rptr.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(r.ev[3], s));
  // the pools are sized from the scan's total
  unsigned long long total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, r.d_rptr.p + nf, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const size_t room = std::max<size_t>(1, (size_t)total);
  if (r.d_rset.alloc(room) != hipSuccess || r.d_rmet.alloc(room) != hipSuccess ||
      r.d_rnh.alloc(room * W) != hipSuccess) {  // (kept while they are large enough)
    (void)hipGetLastError();
    r.d_rset.reset();
    r.d_rmet.reset();
    r.d_rnh.reset();
    return fail(c, SPF_E_NOMEM, "spf_whatif_routes: no memory for %llu entries of %u bytes", total,
                12u + 4u * W);
  }
  // fill
  a.rptr = r.d_rptr.p;
  a.rset = r.d_rset.p;
  a.rmet = r.d_rmet.p;
  a.rnh = r.d_rnh.p;
  if (work && total) {
    hipLaunchKernelGGL(wr_routes_kernel<true>, dim3(blocks_for(v.total, kThreads)), dim3(kThreads), 0,
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
  r.total = total;
  r.valid = true;
  if (n_entries) *n_entries = total;
  if (pool_bytes) *pool_bytes = 8ull * ((uint64_t)nf + 1) + total * (12ull + 4ull * W);
  if (kernel_ms) *kernel_ms = std::accumulate(r.ms, r.ms + 4, 0.0);
  return SPF_OK;
}

spf_status spf_whatif_routes_timing(const spf_whatif_plan* p, double* ms) {
  if (!p || !ms) return SPF_E_INVALID;
  if (const spf_status st = no_routes(const_cast<spf_whatif_plan*>(p), "spf_whatif_routes_timing"); st != SPF_OK)
    return st;
  WiListsView v;
  whatif_lists_view(const_cast<spf_whatif_plan*>(p), &v);
  for (int k = 0; k < 4; ++k) ms[k] = v.rt->ms[k];
  return SPF_OK;
}

spf_status spf_whatif_routes_buffers(spf_whatif_plan* p, const uint64_t** d_ptr, const uint32_t** d_set,
                                     const uint64_t** d_metric, const uint32_t** d_nh, uint32_t* W,
                                     uint64_t* n_entries) {
  if (const spf_status st = no_routes(p, "spf_whatif_routes_buffers"); st != SPF_OK) return st;
  WiListsView v;
  whatif_lists_view(p, &v);
  const WiRoutes& r = *v.rt;
  if (d_ptr) *d_ptr = reinterpret_cast<const uint64_t*>(r.d_rptr.p);
  if (d_set) *d_set = r.d_rset.p;
  if (d_metric) *d_metric = reinterpret_cast<const uint64_t*>(r.d_rmet.p);
  if (d_nh) *d_nh = r.d_rnh.p;
  if (W) *W = v.W;
  if (n_entries) *n_entries = r.total;
  return SPF_OK;
}

spf_status spf_whatif_routes_base(spf_whatif_plan* p, uint64_t* min_metric, uint32_t* nh) {
  if (const spf_status st = no_routes(p, "spf_whatif_routes_base"); st != SPF_OK) return st;
  WiListsView v;
  whatif_lists_view(p, &v);
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
  if (const spf_status st = no_routes(p, "spf_whatif_routes_read"); st != SPF_OK) return st;
  WiListsView v;
  whatif_lists_view(p, &v);
  spf_ctx* c = v.ctx;
  const WiRoutes& r = *v.rt;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t t = (size_t)r.total;
  if (ptr) HIP_TRY(c, hipMemcpy(ptr, r.d_rptr.p, 8ull * ((size_t)v.n_fail + 1), hipMemcpyDeviceToHost));
  if (set && t) HIP_TRY(c, hipMemcpy(set, r.d_rset.p, 4ull * t, hipMemcpyDeviceToHost));
  if (min_metric && t) HIP_TRY(c, hipMemcpy(min_metric, r.d_rmet.p, 8ull * t, hipMemcpyDeviceToHost));
  if (nh && t) HIP_TRY(c, hipMemcpy(nh, r.d_rnh.p, 4ull * t * v.W, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status spf_whatif_routes_db(spf_whatif_plan* p, uint32_t i, uint32_t* set, uint64_t* min_metric,
                                uint32_t* nh, uint64_t cap, uint64_t* n) {
  if (const spf_status st = no_routes(p, "spf_whatif_routes_db"); st != SPF_OK) return st;
  WiListsView v;
  whatif_lists_view(p, &v);
  spf_ctx* c = v.ctx;
  const WiRoutes& r = *v.rt;
  if (i >= v.n_fail) return fail(c, SPF_E_INVALID, "spf_whatif_routes_db: failure %u of %u", i, v.n_fail);
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long at[2] = {0, 0};
  HIP_TRY(c, hipMemcpy(at, r.d_rptr.p + i, 16, hipMemcpyDeviceToHost));
  if (at[1] < at[0] || at[1] > r.total) return fail(c, SPF_E_HIP, "spf_whatif_routes_db: offsets not monotone");
  const size_t m = (size_t)(at[1] - at[0]), W = v.W;
  if (n) *n = m;
  if (!set && !min_metric && !nh) return SPF_OK;
  if (cap < m) return fail(c, SPF_E_NOMEM, "spf_whatif_routes_db: %zu entries, room for %llu", m,
                           (unsigned long long)cap);
  if (!m) return SPF_OK;
  std::vector<uint32_t> hs(m), hw(m * W);
  std::vector<uint64_t> hm(m);
  HIP_TRY(c, hipMemcpy(hs.data(), r.d_rset.p + at[0], 4 * m, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(hm.data(), r.d_rmet.p + at[0], 8 * m, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(hw.data(), r.d_rnh.p + at[0] * W, 4 * m * W, hipMemcpyDeviceToHost));
  std::vector<size_t> order(m);  // the device order is the cursor's: ascending by set here
  std::iota(order.begin(), order.end(), (size_t)0);
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return hs[x] < hs[y]; });
  for (size_t k = 0; k < m; ++k) {
    const size_t q = order[k];
    if (set) set[k] = hs[q];
    if (min_metric) min_metric[k] = hm[q];
    if (nh) std::memcpy(nh + k * W, hw.data() + q * W, 4 * W);
  }
  return SPF_OK;
}

}  // extern "C"
