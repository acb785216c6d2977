// ============================================================================
//  whatif_route_update.hip -- what-if route updates: for every failure of a
//  what-if plan, the destination sets of the source whose LINK-LEVEL next hops
//  change, with the records a FIB would be programmed with.
//
//  A route's records are the reference's getNextHopsThrift without LFA
//  (Decision.cpp:1198-1305): the slots q of src's CSR row, in row order, that
//  are live, survive the failure, lead to a neighbour in the route's next-hop
//  bitset and are tight (w'(q) == d'(head)), each as q | min_metric << 32 --
//  the record of spf_routes.  The route lists of spf_whatif_routes say which
//  sets' (min_metric, nh) moved; this unit walks src's row for them and for
//  the pairs (failure, set) the node-level lists cannot see: a failure that
//  removes or re-weighs a slot of src's own row (a bundle member, a parallel
//  link lowered onto the tie) changes the records of every route through that
//  neighbour though no node's metric or neighbour set moves.
//    base     every set's base records (count, scan, fill);
//    touch    a lane per failure: does it change a slot of src's row?  The
//             touched failures are compacted, each with the mask T of the
//             neighbours whose slots it changes;
//    count    a lane per route-list entry walks the row under the entry's
//             failure and compares with the set's base records (and marks the
//             pairs of touched failures in a hash set); then, for the touched
//             failures only, a sweep over the sets the route lists do not
//             hold: where a base route's words meet T, the row is walked with
//             the base route under the failure;
//    scan     cnt -> uptr;
//    fill     the count pass again, an entry per changed sequence;
//    scan     the entries' record counts -> urec_ptr;
//    records  a lane per entry walks the row once more and writes.
//  Launch boundaries order the passes.  No buffer is n_fail x n_sets or
//  n_fail x n_nodes.
//
//  Why the sweep is complete (positive metrics, which the plans this call
//  accepts have): a pair outside the route lists keeps (min, nh).  A neighbour
//  x in nh has a tight surviving slot in the base, d(x) = w(q).  If the
//  failure leaves x's slots alone, q still stands, so d'(x) <= d(x); and
//  d'(x) < d(x) would leave x no tight slot and take it out of every next-hop
//  set, against nh' = nh.  So only a failure that changes a slot of a
//  neighbour in nh can change the records: exactly the pairs whose base words
//  meet T.  The walk itself decides, T only selects.
// ============================================================================
#include "engine_internal.h"
#include "grid_ops.h"
#include "list_owner.h"
#include "whatif_pool_host.h"
#include "whatif_route_update_host.h"

#include <numeric>

using namespace spfi;

namespace {

constexpr unsigned long long kNoRoute = ~0ull;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kThreads = 256;      // also the sets a workgroup of the sweep takes per round
constexpr uint32_t kLdsSlots = 2048;    // row slots staged in LDS (32 KB); longer rows are read from L2
constexpr uint32_t kNoFail = 0xFFu;     // Fd::kind of the base pass
constexpr uint32_t kSweepBlocks = 1u << 16;

static_assert(sizeof(UpdateSlot) == sizeof(uint4) && sizeof(UpdateLink) == sizeof(uint2),
              "the row tables are uploaded as they are");

extern __shared__ uint4 s_row[];

struct WuArgs {
  // src's row (whatif_route_update_host.h) and the plan's failures (WiListsView)
  const uint4* row;
  const uint2* row_link;
  uint32_t n_row, n_link, row0;
  uint32_t kind, n_fail, n_sets, W;
  const uint32_t* fails;
  const uint32_t* set_links;
  const uint4* met;
  const uint32_t* nbr_bit;
  // the unfailed result, the change lists and the table over them (WiRoutes)
  const unsigned long long* bd;
  const unsigned long long* cdist;
  const unsigned long long* keys;  // NULL: no list entry, every metric is the base's
  const uint32_t* vals;
  uint32_t mask;
  // base routes and route lists
  const unsigned long long* rbm;
  const uint32_t* rbnh;
  const unsigned long long* rptr;
  const uint32_t* rset;
  const unsigned long long* rmet;
  const uint32_t* rnh;
  unsigned long long rtotal;
  // base records
  uint32_t* bcnt;
  const unsigned long long* bptr;
  unsigned long long* brec;
  // touched failures
  uint32_t* tidx;
  uint32_t* tlist;
  uint32_t* tmask;
  uint2* trange;
  uint32_t* tn;  // [0] touched failures, [2..3] u64: their route-list entries
  uint32_t n_touch;
  unsigned long long* mkeys;  // (failure << 32 | set) of those entries, ~0: empty
  uint32_t mmask;
  // update lists
  uint32_t* cnt;
  uint32_t* cur;
  const unsigned long long* uptr;
  uint32_t* uset;
  unsigned long long* umet;
  uint32_t* usrc;  // the route-list entry an update entry was made from, kNone: the base route
  uint32_t* rcnt;
  unsigned long long utotal;
  const unsigned long long* urp;
  unsigned long long* urec;
  uint32_t* fault;
};

__device__ __forceinline__ uint32_t wu_hash(unsigned long long k) {
  k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
  k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)(k ^ (k >> 31));
}

// d'(u) under failure i: the change-list entry where the table of
// spf_whatif_routes has one (same hash, same probe), the base otherwise
__device__ __forceinline__ unsigned long long wu_dist(const WuArgs& a, uint32_t i, uint32_t u) {
  if (i == kNone || !a.keys) return a.bd[u];
  const unsigned long long key = ((unsigned long long)i << 32) | u;
  for (uint32_t h = wu_hash(key) & a.mask;; h = (h + 1) & a.mask) {
    const unsigned long long k = a.keys[h];
    if (k == key) return a.cdist[a.vals[h]];
    if (k == kNoRoute) return a.bd[u];
  }
}

// the slot of `link` in src's row, kNone when src has no live slot of it
__device__ __forceinline__ uint32_t wu_find_link(const WuArgs& a, uint32_t link) {
  uint32_t lo = 0, hi = a.n_link;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.row_link[mid].x < link) lo = mid + 1;
    else hi = mid;
  }
  return lo < a.n_link && a.row_link[lo].x == link ? a.row_link[lo].y : kNone;
}

// failure i as the walk reads it
struct Fd {
  uint32_t kind, x, lo, hi;
  uint4 chg;
};
__device__ __forceinline__ Fd wu_fail(const WuArgs& a, uint32_t i) {
  Fd f{kNoFail, 0u, 0u, 0u, make_uint4(kNone, kNone, 0u, 0u)};
  if (i == kNone) return f;
  f.kind = a.kind;
  if (a.kind == SPF_WHATIF_LINK_SET) {
    f.lo = a.fails[i];
    f.hi = a.fails[i + 1];
  } else if (a.kind == SPF_WHATIF_LINK_METRIC) {
    f.chg = a.met[i];
  } else {
    f.x = a.fails[i];
  }
  return f;
}

__device__ __forceinline__ bool wu_in_set(const WuArgs& a, const Fd& f, uint32_t link) {
  uint32_t lo = f.lo, hi = f.hi;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.set_links[mid] < link) lo = mid + 1;
    else hi = mid;
  }
  return lo < f.hi && a.set_links[lo] == link;
}

// w'(slot t) under the failure, 0 when the slot does not survive it (metrics are positive)
__device__ __forceinline__ uint32_t wu_weight(const WuArgs& a, const Fd& f, uint32_t t, const uint4& r) {
  switch (f.kind) {
    case 0u: return r.z == f.x ? 0u : r.y;
    case SPF_WHATIF_NODE_DOWN: return r.w == f.x ? 0u : r.y;
    case SPF_WHATIF_LINK_SET: return wu_in_set(a, f, r.z) ? 0u : r.y;
    case SPF_WHATIF_LINK_METRIC: {
      const uint32_t q = a.row0 + t;
      return q == f.chg.x ? f.chg.z : q == f.chg.y ? f.chg.w : r.y;
    }
    default: return r.y;  // a drain, or no failure
  }
}

// The records of a route (nh words, metrics d') under failure i: emit(k, t)
// for the k-th qualifying slot t, in slot order; returns their number.  The
// word of nh is kept while consecutive slots share it (rows are mostly in
// neighbour order).
template <bool LDS, class F>
__device__ __forceinline__ uint32_t wu_walk(const WuArgs& a, uint32_t i, const Fd& f, const uint32_t* nh,
                                            F&& emit) {
  uint32_t n = 0, cw = kNone, word = 0;
  for (uint32_t t = 0; t < a.n_row; ++t) {
    uint4 r;
    if constexpr (LDS) r = s_row[t];
    else r = a.row[t];
    if (r.x == kNone) continue;  // dead
    const uint32_t wi = r.x >> 5;
    if (wi != cw) {
      cw = wi;
      word = nh[wi];
    }
    if (!((word >> (r.x & 31)) & 1u)) continue;
    const uint32_t w = wu_weight(a, f, t, r);
    if (!w || (unsigned long long)w != wu_dist(a, i, r.w)) continue;
    emit(n, t);
    ++n;
  }
  return n;
}

// Do the records of (m, nh) under failure i differ from set s's base records?  *n: their number.
template <bool LDS>
__device__ __forceinline__ bool wu_differs(const WuArgs& a, uint32_t i, const Fd& f, uint32_t s,
                                           unsigned long long m, const uint32_t* nh, uint32_t* n) {
  const unsigned long long bp = a.bptr[s], bn = a.bptr[s + 1] - bp;
  bool diff = false;
  *n = m == kNoRoute ? 0u : wu_walk<LDS>(a, i, f, nh, [&](uint32_t k, uint32_t t) {
    if (k >= bn || (uint32_t)a.brec[bp + k] != a.row0 + t) diff = true;
  });
  diff |= *n != bn;
  if (*n && !diff) diff = (a.brec[bp] >> 32) != m;
  return diff;
}

template <bool LDS>
__device__ __forceinline__ void wu_stage(const WuArgs& a) {
  if constexpr (LDS) {
    for (uint32_t t = threadIdx.x; t < a.n_row; t += kThreads) s_row[t] = a.row[t];
    __syncthreads();
  }
}

// every set's base records: a lane per set
template <bool FILL, bool LDS>
__global__ __launch_bounds__(kThreads) void wu_base_kernel(WuArgs a) {
  wu_stage<LDS>(a);
  const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= a.n_sets) return;
  const unsigned long long m = a.rbm[s];
  const Fd f = wu_fail(a, kNone);
  const uint32_t* nh = a.rbnh + (size_t)s * a.W;
  if constexpr (!FILL) {
    a.bcnt[s] = m == kNoRoute ? 0u : wu_walk<LDS>(a, kNone, f, nh, [](uint32_t, uint32_t) {});
  } else {
    const unsigned long long bp = a.bptr[s], bn = a.bptr[s + 1] - bp;
    if (m == kNoRoute || !bn) return;
    wu_walk<LDS>(a, kNone, f, nh, [&](uint32_t k, uint32_t t) {
      if (k < bn) a.brec[bp + k] = (unsigned long long)(a.row0 + t) | (m << 32);
      else atomicOr(a.fault, kFaultListRoom);
    });
  }
}

// The slots of src's row that failure i removes or re-weighs: visit(t) for each.
template <class F>
__device__ __forceinline__ void wu_touched_slots(const WuArgs& a, uint32_t i, F&& visit) {
  const Fd f = wu_fail(a, i);
  switch (f.kind) {
    case 0u: {
      const uint32_t t = wu_find_link(a, f.x);
      if (t != kNone) visit(t);
      break;
    }
    case SPF_WHATIF_NODE_DOWN:
      if (a.nbr_bit[f.x] != kNone)
        for (uint32_t t = 0; t < a.n_row; ++t)
          if (a.row[t].x != kNone && a.row[t].w == f.x) visit(t);
      break;
    case SPF_WHATIF_LINK_SET:
      for (uint32_t k = f.lo; k < f.hi; ++k) {
        const uint32_t t = wu_find_link(a, a.set_links[k]);
        if (t != kNone) visit(t);
      }
      break;
    case SPF_WHATIF_LINK_METRIC:
      for (uint32_t side = 0; side < 2; ++side) {  // a down link: both edges kNone
        const uint32_t e = side ? f.chg.y : f.chg.x, w = side ? f.chg.w : f.chg.z, t = e - a.row0;
        if (e != kNone && e >= a.row0 && t < a.n_row && a.row[t].x != kNone && a.row[t].y != w) visit(t);
      }
      break;
    default: break;  // a drain changes no slot
  }
}

// a lane per failure: touched failures get an index and are listed
__global__ __launch_bounds__(kThreads) void wu_touch_kernel(WuArgs a) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_fail) return;
  bool any = false;
  wu_touched_slots(a, i, [&](uint32_t) { any = true; });
  uint32_t k = kNone;
  if (any) {
    k = atomicAdd(&a.tn[0], 1u);
    a.tlist[k] = i;
    atomicAdd(reinterpret_cast<unsigned long long*>(a.tn + 2), a.rptr[i + 1] - a.rptr[i]);
  }
  a.tidx[i] = k;
}

// a lane per touched failure: its mask (zeroed before) and the words it spans
__global__ __launch_bounds__(kThreads) void wu_mask_kernel(WuArgs a) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= a.n_touch) return;
  uint32_t lo = kNone, hi = 0;
  uint32_t* T = a.tmask + (size_t)k * a.W;
  wu_touched_slots(a, a.tlist[k], [&](uint32_t t) {
    const uint32_t j = a.row[t].x, w = j >> 5;
    T[w] |= 1u << (j & 31);
    lo = w < lo ? w : lo;
    hi = w > hi ? w : hi;
  });
  a.trange[k] = make_uint2(lo, hi);
}

// A changed record sequence of failure i: counted, or its entry written at the failure's next place.
template <bool FILL>
__device__ __forceinline__ void wu_claim(const WuArgs& a, uint32_t i, uint32_t s, unsigned long long m,
                                         uint32_t from, uint32_t n) {
  if constexpr (!FILL) {
    atomicAdd(&a.cnt[i], 1u);
  } else {
    const unsigned long long at = a.uptr[i] + atomicAdd(&a.cur[i], 1u);
    if (at >= a.uptr[i + 1]) {  // more entries than were counted: dropped
      atomicOr(a.fault, kFaultListRoom);
      return;
    }
    a.uset[at] = s;
    a.umet[at] = m;
    a.usrc[at] = from;
    a.rcnt[at] = n;
  }
}

// a lane per route-list entry
template <bool FILL, bool LDS>
__global__ __launch_bounds__(kThreads) void wu_entries_kernel(WuArgs a) {
  wu_stage<LDS>(a);
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.rtotal) return;
  const uint32_t i = list_owner(a.rptr, a.n_fail, e), s = a.rset[e];
  if (!FILL && a.tidx[i] != kNone) {  // the sweep leaves this pair to this lane
    const unsigned long long key = ((unsigned long long)i << 32) | s;
    for (uint32_t h = wu_hash(key) & a.mmask;; h = (h + 1) & a.mmask) {
      const unsigned long long was = atomicCAS(&a.mkeys[h], kNoRoute, key);
      if (was == kNoRoute || was == key) break;
    }
  }
  const unsigned long long m = a.rmet[e];
  uint32_t n = 0;
  if (wu_differs<LDS>(a, i, wu_fail(a, i), s, m, a.rnh + (size_t)e * a.W, &n))
    wu_claim<FILL>(a, i, s, m, (uint32_t)e, n);
}

// The touched failures against the sets their route lists do not hold:
// workgroups stride over (touched failure, kThreads sets).
template <bool FILL>
__global__ __launch_bounds__(kThreads) void wu_sweep_kernel(WuArgs a) {
  const uint64_t chunks = ((uint64_t)a.n_sets + kThreads - 1) / kThreads, units = chunks * a.n_touch;
  for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
    const uint32_t k = (uint32_t)(u / chunks);
    const uint64_t s64 = (u % chunks) * kThreads + threadIdx.x;
    if (s64 >= a.n_sets) continue;
    const uint32_t s = (uint32_t)s64, i = a.tlist[k];
    const uint2 span = a.trange[k];
    const uint32_t* nh = a.rbnh + (size_t)s * a.W;
    bool meets = false;
    for (uint32_t w = span.x; w <= span.y && w < a.W && !meets; ++w)
      meets = (nh[w] & a.tmask[(size_t)k * a.W + w]) != 0;
    if (!meets) continue;
    const unsigned long long key = ((unsigned long long)i << 32) | s;
    bool listed = false;
    for (uint32_t h = wu_hash(key) & a.mmask;; h = (h + 1) & a.mmask) {
      const unsigned long long at = a.mkeys[h];
      listed = at == key;
      if (listed || at == kNoRoute) break;
    }
    if (listed) continue;
    const unsigned long long m = a.rbm[s];
    uint32_t n = 0;
    if (wu_differs<false>(a, i, wu_fail(a, i), s, m, nh, &n)) wu_claim<FILL>(a, i, s, m, kNone, n);
  }
}

// a lane per update entry: its records
template <bool LDS>
__global__ __launch_bounds__(kThreads) void wu_records_kernel(WuArgs a) {
  wu_stage<LDS>(a);
  const unsigned long long at = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (at >= a.utotal) return;
  const unsigned long long rp = a.urp[at], rn = a.urp[at + 1] - rp, m = a.umet[at];
  if (!rn || m == kNoRoute) return;
  const uint32_t i = list_owner(a.uptr, a.n_fail, at), s = a.uset[at], e = a.usrc[at];
  const uint32_t* nh = e != kNone ? a.rnh + (size_t)e * a.W : a.rbnh + (size_t)s * a.W;
  wu_walk<LDS>(a, i, wu_fail(a, i), nh, [&](uint32_t k, uint32_t t) {
    if (k < rn) a.urec[rp + k] = (unsigned long long)(a.row0 + t) | (m << 32);
    else atomicOr(a.fault, kFaultListRoom);
  });
}

constexpr int kPhases = 7;

}  // namespace

extern "C" {

spf_status spf_whatif_route_update(spf_whatif_plan* p, uint64_t* n_entries, uint64_t* n_records,
                                   uint64_t* pool_bytes, double* kernel_ms, void* stream) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_whatif_route_update: NULL plan");
  WiListsView v;
  whatif_lists_view(p, &v);
  spf_ctx* c = v.ctx;
  WiUpdate& U = *v.up;
  const WiRoutes& r = *v.rt;
  const WiPool& R = r.pool;
  const WiPool& L = *v.changes;
  U.ent.valid = U.rec.valid = false;  // after a failed call the plan holds no update lists
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (v.epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  if (v.exact)
    return fail(c, SPF_E_UNSUPPORTED,
                "spf_whatif_route_update: the plan runs on the exact path (a metric <= 0 or u64 labels); "
                "a record holds a 32-bit metric");
  if (!R.valid || !L.valid)
    return fail(c, SPF_E_STATE,
                "spf_whatif_route_update: the plan holds no route lists (spf_whatif_changes and "
                "spf_whatif_routes first)");
  if (R.total >> 31)
    return fail(c, SPF_E_NOMEM, "spf_whatif_route_update: %llu route-list entries, an entry indexes 2^31",
                (unsigned long long)R.total);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const uint32_t W = v.W, nf = v.n_fail, n_sets = r.n_sets;

  // host, once per call: src's row as the kernels walk it
  const UpdateRow row = update_row(c->row_ptr.data(), c->col.data(), c->wt.data(), c->link.data(),
                                   c->edge_nb.data(), v.src);
  const uint32_t n_row = (uint32_t)row.slot.size();
  const bool lds = n_row <= kLdsSlots;
  const size_t lds_bytes = sizeof(uint4) * std::max<uint32_t>(1, n_row);
  for (hipEvent_t& e : U.ev)
    if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  HIP_TRY(c, U.d_row.upload(reinterpret_cast<const uint4*>(row.slot.data()), n_row, s));
  HIP_TRY(c, U.d_row_link.upload(reinterpret_cast<const uint2*>(row.links.data()), row.links.size(), s));
  HIP_TRY(c, U.d_bcnt.alloc(std::max<uint32_t>(1, n_sets)));
  HIP_TRY(c, U.d_bptr.alloc((size_t)n_sets + 1));
  HIP_TRY(c, U.d_tidx.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, U.d_tlist.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, U.d_tn.alloc(4));
  HIP_TRY(c, U.d_cnt.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, U.d_cur.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, U.ent.ptr.alloc((size_t)nf + 1));

  // the kernels that stage the row take it in LDS when it fits
  WuArgs a{};
  const auto launch = [&](void (*staged)(WuArgs), void (*plain)(WuArgs), unsigned long long items) {
    hipLaunchKernelGGL(lds ? staged : plain, dim3(blocks_for(items, kThreads)), dim3(kThreads),
                       lds ? lds_bytes : 0, s, a);
    return hipGetLastError();
  };
  a.row = U.d_row.p;
  a.row_link = U.d_row_link.p;
  a.n_row = n_row;
  a.n_link = (uint32_t)row.links.size();
  a.row0 = row.first;
  a.kind = v.kind;
  a.n_fail = nf;
  a.n_sets = n_sets;
  a.W = W;
  a.fails = v.fails;
  a.set_links = v.set_links;
  a.met = static_cast<const uint4*>(v.met);
  a.nbr_bit = v.nbr_bit;
  a.bd = r.d_bd.p;
  a.cdist = L.val.p;
  a.keys = r.tab_mask ? r.d_keys.p : nullptr;
  a.vals = r.d_vals.p;
  a.mask = r.tab_mask;
  a.rbm = r.d_rbm.p;
  a.rbnh = r.d_rbnh.p;
  a.rptr = R.ptr.p;
  a.rset = R.key.p;
  a.rmet = R.val.p;
  a.rnh = R.rows.p;
  a.rtotal = R.total;
  a.bcnt = U.d_bcnt.p;
  a.bptr = U.d_bptr.p;
  a.tidx = U.d_tidx.p;
  a.tlist = U.d_tlist.p;
  a.tn = U.d_tn.p;
  a.cnt = U.d_cnt.p;
  a.cur = U.d_cur.p;
  a.fault = c->d_fault.p;

  // base records: count, scan, fill
  HIP_TRY(c, hipEventRecord(U.ev[0], s));
  if (n_sets) HIP_TRY(c, launch(wu_base_kernel<false, true>, wu_base_kernel<false, false>, n_sets));
  HIP_TRY(c, whatif_scan(U.d_bcnt.p, 1, n_sets, U.d_bptr.p, s));
  unsigned long long base_records = 0;
  HIP_TRY(c, hipMemcpyAsync(&base_records, U.d_bptr.p + n_sets, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (U.d_brec.alloc(std::max<size_t>(1, (size_t)base_records)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SPF_E_NOMEM, "spf_whatif_route_update: no memory for %llu base records", base_records);
  }
  a.brec = U.d_brec.p;
  if (n_sets && base_records)
    HIP_TRY(c, launch(wu_base_kernel<true, true>, wu_base_kernel<true, false>, n_sets));
  // touch: the failures that change a slot of src's row, and their masks
  HIP_TRY(c, hipEventRecord(U.ev[1], s));
  HIP_TRY(c, hipMemsetAsync(U.d_tn.p, 0, 16, s));
  if (nf) {
    hipLaunchKernelGGL(wu_touch_kernel, dim3(blocks_for(nf, kThreads)), dim3(kThreads), 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  uint32_t tn[4] = {0, 0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(tn, U.d_tn.p, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint32_t n_touch = tn[0];
  const unsigned long long marked = ((unsigned long long)tn[3] << 32) | tn[2];
  size_t mcap = 64;  // a power of two >= 2 x the pairs marked, so a probe always meets an empty slot
  while (mcap < 2 * (size_t)marked) mcap <<= 1;
  if (U.d_tmask.alloc(std::max<size_t>(1, (size_t)n_touch * W)) != hipSuccess ||
      U.d_trange.alloc(std::max<uint32_t>(1, n_touch)) != hipSuccess ||
      U.d_mkeys.alloc(mcap) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SPF_E_NOMEM, "spf_whatif_route_update: no memory for %u touched failures", n_touch);
  }
  a.tmask = U.d_tmask.p;
  a.trange = U.d_trange.p;
  a.n_touch = n_touch;
  a.mkeys = U.d_mkeys.p;
  a.mmask = (uint32_t)(mcap - 1);
  HIP_TRY(c, hipMemsetAsync(U.d_mkeys.p, 0xFF, 8 * mcap, s));
  if (n_touch) {
    HIP_TRY(c, hipMemsetAsync(U.d_tmask.p, 0, 4ull * n_touch * W, s));
    hipLaunchKernelGGL(wu_mask_kernel, dim3(blocks_for(n_touch, kThreads)), dim3(kThreads), 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  // count
  HIP_TRY(c, hipMemsetAsync(U.d_cnt.p, 0, 4ull * std::max<uint32_t>(1, nf), s));
  HIP_TRY(c, hipMemsetAsync(U.d_cur.p, 0, 4ull * std::max<uint32_t>(1, nf), s));
  HIP_TRY(c, hipEventRecord(U.ev[2], s));
  const uint64_t units = (((uint64_t)n_sets + kThreads - 1) / kThreads) * n_touch;
  const uint32_t sweep_blocks = (uint32_t)std::min<uint64_t>(units, kSweepBlocks);
  if (R.total)
    HIP_TRY(c, launch(wu_entries_kernel<false, true>, wu_entries_kernel<false, false>, R.total));
  if (sweep_blocks) {
    hipLaunchKernelGGL(wu_sweep_kernel<false>, dim3(sweep_blocks), dim3(kThreads), 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(U.ev[3], s));
  HIP_TRY(c, whatif_scan(U.d_cnt.p, 1, nf, U.ent.ptr.p, s));
  HIP_TRY(c, hipEventRecord(U.ev[4], s));
  unsigned long long total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, U.ent.ptr.p + nf, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (total >> 32)
    return fail(c, SPF_E_NOMEM, "spf_whatif_route_update: %llu entries, the scan takes 2^32", total);
  if (const spf_status st = pool_size(c, &U.ent, total, 0, "spf_whatif_route_update"); st != SPF_OK)
    return st;
  if (U.d_usrc.alloc(std::max<size_t>(1, (size_t)total)) != hipSuccess ||
      U.d_rcnt.alloc(std::max<size_t>(1, (size_t)total)) != hipSuccess ||
      U.rec.ptr.alloc((size_t)total + 1) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, SPF_E_NOMEM, "spf_whatif_route_update: no memory for %llu entries", total);
  }
  // fill
  a.uptr = U.ent.ptr.p;
  a.uset = U.ent.key.p;
  a.umet = U.ent.val.p;
  a.usrc = U.d_usrc.p;
  a.rcnt = U.d_rcnt.p;
  a.utotal = total;
  if (total) {
    // (an entry the fill drops leaves its record count at zero)
    HIP_TRY(c, hipMemsetAsync(U.d_rcnt.p, 0, 4ull * total, s));
    if (R.total)
      HIP_TRY(c, launch(wu_entries_kernel<true, true>, wu_entries_kernel<true, false>, R.total));
    if (sweep_blocks) {
      hipLaunchKernelGGL(wu_sweep_kernel<true>, dim3(sweep_blocks), dim3(kThreads), 0, s, a);
      HIP_TRY(c, hipGetLastError());
    }
  }
  HIP_TRY(c, hipEventRecord(U.ev[5], s));
  HIP_TRY(c, whatif_scan(U.d_rcnt.p, 1, (uint32_t)total, U.rec.ptr.p, s));
  HIP_TRY(c, hipEventRecord(U.ev[6], s));
  unsigned long long records = 0;
  HIP_TRY(c, hipMemcpyAsync(&records, U.rec.ptr.p + total, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (U.rec.val.alloc(std::max<size_t>(1, (size_t)records)) != hipSuccess) {
    (void)hipGetLastError();
    U.rec.val.reset();
    return fail(c, SPF_E_NOMEM, "spf_whatif_route_update: no memory for %llu records", records);
  }
  // records
  a.urp = U.rec.ptr.p;
  a.urec = U.rec.val.p;
  if (total && records) HIP_TRY(c, launch(wu_records_kernel<true>, wu_records_kernel<false>, total));
  HIP_TRY(c, hipEventRecord(U.ev[7], s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  for (int k = 0; k < kPhases; ++k) {
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, U.ev[k], U.ev[k + 1]));
    U.ms[k] = ms;
  }
  U.n_sets = n_sets;
  U.n_touch = n_touch;
  U.base_records = base_records;
  U.ent.n_owners = nf;
  U.ent.total = total;
  U.rec.n_owners = (uint32_t)total;
  U.rec.total = records;
  U.rec.W = 0;
  U.ent.valid = U.rec.valid = true;
  if (n_entries) *n_entries = total;
  if (n_records) *n_records = records;
  if (pool_bytes) *pool_bytes = 8ull * ((uint64_t)nf + 1) + 12ull * total + 8ull * (total + 1) + 8ull * records;
  if (kernel_ms) *kernel_ms = std::accumulate(U.ms, U.ms + kPhases, 0.0);
  return SPF_OK;
}

spf_status spf_whatif_route_update_timing(const spf_whatif_plan* p, double* ms) {
  if (!p || !ms) return SPF_E_INVALID;
  WiListsView v;
  if (const spf_status st = pool_held(const_cast<spf_whatif_plan*>(p), kPoolUpdate,
                                      "spf_whatif_route_update_timing", &v); st != SPF_OK)
    return st;
  for (int k = 0; k < kPhases; ++k) ms[k] = v.up->ms[k];
  return SPF_OK;
}

spf_status spf_whatif_route_update_stats(spf_whatif_plan* p, uint32_t* n_touched, uint64_t* base_records) {
  WiListsView v;
  if (const spf_status st = pool_held(p, kPoolUpdate, "spf_whatif_route_update_stats", &v); st != SPF_OK)
    return st;
  if (n_touched) *n_touched = v.up->n_touch;
  if (base_records) *base_records = v.up->base_records;
  return SPF_OK;
}

spf_status spf_whatif_route_update_buffers(spf_whatif_plan* p, const uint64_t** d_ptr,
                                           const uint32_t** d_set, const uint64_t** d_metric,
                                           const uint64_t** d_rec_ptr, const uint64_t** d_rec,
                                           uint64_t* n_entries, uint64_t* n_records) {
  if (const spf_status st = pool_buffers(p, kPoolUpdate, "spf_whatif_route_update_buffers", d_ptr, d_set,
                                         d_metric, nullptr, nullptr, nullptr, n_entries); st != SPF_OK)
    return st;
  return pool_buffers(p, kPoolUpdateRec, "spf_whatif_route_update_buffers", d_rec_ptr, nullptr, d_rec,
                      nullptr, nullptr, nullptr, n_records);
}

spf_status spf_whatif_route_update_read(spf_whatif_plan* p, uint64_t* ptr, uint32_t* set,
                                        uint64_t* min_metric, uint64_t* rec_ptr, uint64_t* rec) {
  if (const spf_status st = pool_read(p, kPoolUpdate, "spf_whatif_route_update_read", ptr, set, min_metric,
                                      nullptr); st != SPF_OK)
    return st;
  return pool_read(p, kPoolUpdateRec, "spf_whatif_route_update_read", rec_ptr, nullptr, rec, nullptr);
}

spf_status spf_whatif_route_update_base(spf_whatif_plan* p, uint64_t* rec_ptr, uint64_t* rec) {
  WiListsView v;
  if (const spf_status st = pool_held(p, kPoolUpdate, "spf_whatif_route_update_base", &v); st != SPF_OK)
    return st;
  spf_ctx* c = v.ctx;
  const WiUpdate& U = *v.up;
  HIP_TRY(c, hipSetDevice(c->device));
  if (rec_ptr) HIP_TRY(c, hipMemcpy(rec_ptr, U.d_bptr.p, 8ull * ((size_t)U.n_sets + 1), hipMemcpyDeviceToHost));
  if (rec && U.base_records)
    HIP_TRY(c, hipMemcpy(rec, U.d_brec.p, 8ull * U.base_records, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status spf_whatif_route_update_db(spf_whatif_plan* p, uint32_t i, uint32_t* set, uint64_t* min_metric,
                                      uint64_t* rec_ptr, uint64_t* rec, uint64_t cap_entries,
                                      uint64_t cap_records, uint64_t* n, uint64_t* n_rec) {
  const char* who = "spf_whatif_route_update_db";
  WiListsView v;
  if (const spf_status st = pool_held(p, kPoolUpdate, who, &v); st != SPF_OK) return st;
  spf_ctx* c = v.ctx;
  const WiPool& E = v.up->ent;
  const WiPool& Q = v.up->rec;
  if (i >= E.n_owners) return fail(c, SPF_E_INVALID, "%s: failure %u of %u", who, i, E.n_owners);
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long at[2] = {0, 0};
  HIP_TRY(c, hipMemcpy(at, E.ptr.p + i, 16, hipMemcpyDeviceToHost));
  const bool want = set || min_metric || rec_ptr || rec;
  uint64_t cnt = 0;
  bool copy = false;
  spf_status st = pool_slice(at[0], at[1], E.total, want, cap_entries, &cnt, &copy);
  if (st == SPF_E_HIP) return fail(c, st, "%s: offsets not monotone", who);
  const size_t m = (size_t)cnt;
  std::vector<unsigned long long> rp(m + 1, 0);
  HIP_TRY(c, hipMemcpy(rp.data(), Q.ptr.p + at[0], 8 * (m + 1), hipMemcpyDeviceToHost));
  uint64_t recs = 0;
  bool copy_rec = false;
  const spf_status st2 = pool_slice(rp[0], rp[m], Q.total, rec != nullptr, cap_records, &recs, &copy_rec);
  if (st2 == SPF_E_HIP) return fail(c, st2, "%s: record offsets not monotone", who);
  if (n) *n = cnt;
  if (n_rec) *n_rec = recs;
  if (st != SPF_OK || st2 != SPF_OK)
    return fail(c, SPF_E_NOMEM, "%s: %zu entries with %llu records, room for %llu and %llu", who, m,
                (unsigned long long)recs, (unsigned long long)cap_entries,
                (unsigned long long)cap_records);
  if (!copy) {
    if (rec_ptr) rec_ptr[0] = 0;
    return SPF_OK;
  }
  std::vector<uint32_t> hk(m);
  std::vector<uint64_t> hv(m), hr((size_t)recs);
  HIP_TRY(c, hipMemcpy(hk.data(), E.key.p + at[0], 4 * m, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(hv.data(), E.val.p + at[0], 8 * m, hipMemcpyDeviceToHost));
  if (recs) HIP_TRY(c, hipMemcpy(hr.data(), Q.val.p + rp[0], 8 * (size_t)recs, hipMemcpyDeviceToHost));
  const std::vector<size_t> order = pool_order(hk.data(), hv.data(), m);
  uint64_t out = 0;
  for (size_t k = 0; k < m; ++k) {
    const size_t e = order[k];
    if (set) set[k] = hk[e];
    if (min_metric) min_metric[k] = hv[e];
    if (rec_ptr) rec_ptr[k] = out;
    const uint64_t len = rp[e + 1] - rp[e];
    if (rp[e + 1] < rp[e] || out + len > recs) return fail(c, SPF_E_HIP, "%s: record offsets not monotone", who);
    if (rec && len) std::memcpy(rec + out, hr.data() + (rp[e] - rp[0]), 8 * (size_t)len);
    out += len;
  }
  if (rec_ptr) rec_ptr[m] = out;
  return SPF_OK;
}

uint32_t spf_whatif_route_update_sweep_sets(void) { return kThreads; }
uint32_t spf_whatif_route_update_lds_slots(void) { return kLdsSlots; }
uint32_t spf_whatif_scan_tile(void) { return kWhatifScanTile; }

}  // extern "C"
