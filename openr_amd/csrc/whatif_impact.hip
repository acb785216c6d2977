// ============================================================================
//  whatif_impact.hip -- what-if impact by destination: the failure-major lists
//  of a what-if plan transposed to key-major, and a summary per key.
//
//  The change lists (spf_whatif_changes) and the route lists
//  (spf_whatif_routes) answer "what does failure i change?".  This unit turns
//  the resident pools round, on the device: "which failures touch key k, which
//  cut it off, which is the worst, how narrow does its ECMP get?".  Keys are
//  nodes over the change lists (spf_whatif_by_node) and set ids over the route
//  lists (spf_whatif_by_set); one set of kernels serves both, parametrised by
//  its inputs: key[total], dist[total], nh[total][W], the owner offsets
//  (cptr / rptr) and the base (metric and row per key).
//    init     imp[k] = the base: max_metric, the row's popcount, no counts
//    count    a lane per entry: the three counts, a 64-bit max of the finite
//             metrics and a min of their popcounts, by atomics into imp[k];
//             the rows are read by the workgroup together (coalesced) and
//             summed per entry in LDS
//    scan     imp[k].n_changed -> tptr (u64), the change lists' own scan
//    fill     a lane per entry: its failure by bisecting the owner offsets
//             (list_owner, shared with whatif_routes.hip), (failure, entry) at
//             tptr[k] + a per-key cursor, and the first failure at max_metric
//    finish   min_width of the keys without a finite entry: the base's
//  No buffer is n_fail x n_keys.  Everything is device scope on one GPU.
// ============================================================================
#include "engine_internal.h"
#include "grid_ops.h"
#include "list_owner.h"

#include <cstddef>
#include <string>

using namespace spfi;

static_assert(sizeof(spf_whatif_impact) == 32 && offsetof(spf_whatif_impact, max_metric) == 16,
              "the scan strides the summaries by 8 words; the 64-bit max needs its alignment");

namespace {

constexpr unsigned long long kNoRoute = ~0ull;
constexpr uint32_t kThreads = 256;
// min_width while no finite entry has been met: the base popcount under this
// bit, so that any entry's popcount (<= 32 W < 2^31) wins the atomicMin
constexpr uint32_t kBaseWidth = 0x80000000u;

struct WiArgs {
  // the lists: entry e has key[e], dist[e], nh[e * W ..]; owner offsets ptr[n_own + 1]
  const uint32_t* key;
  const unsigned long long* dist;
  const uint32_t* nh;
  const unsigned long long* optr;
  uint32_t n_own;
  // the base per key: u32 metrics with kInf or u64 ones with ~0, rows of W
  // words (undefined where unreachable, and everywhere when no_nbr)
  const uint32_t* b32;
  const unsigned long long* b64;
  const uint32_t* bnh;
  uint32_t no_nbr;
  uint32_t n_keys, W;
  unsigned long long total;
  spf_whatif_impact* imp;
  uint32_t* cur;
  const unsigned long long* tptr;
  uint32_t* tfail;
  unsigned long long* tent;
  uint32_t* fault;
};

__device__ __forceinline__ unsigned long long base_metric(const WiArgs& a, uint32_t k) {
  if (a.b64) return a.b64[k];
  const uint32_t d = a.b32[k];
  return d == kInf ? kNoRoute : d;
}

__global__ __launch_bounds__(kThreads) void wi_init_kernel(WiArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= a.n_keys) return;
  const unsigned long long d = base_metric(a, (uint32_t)k);
  uint32_t width = 0;
  if (d != kNoRoute && !a.no_nbr)
    for (uint32_t w = 0; w < a.W; ++w) width += __popc(a.bnh[k * a.W + w]);
  spf_whatif_impact o;
  o.n_changed = o.n_unreachable = o.n_metric = 0;
  o.min_width = kBaseWidth | width;
  o.max_metric = d;
  o.max_fail = SPF_WHATIF_NONE;
  o.reserved = 0;
  a.imp[k] = o;
  a.cur[k] = 0;
}

__global__ __launch_bounds__(kThreads) void wi_count_kernel(WiArgs a) {
  __shared__ uint32_t s_width[kThreads];
  const unsigned long long e0 = (unsigned long long)blockIdx.x * kThreads;
  const unsigned long long e = e0 + threadIdx.x;
  const uint32_t W = a.W;
  s_width[threadIdx.x] = 0;
  __syncthreads();
  // the block's rows are one run of words: thread t takes words t, t + 256,
  // ...; word g belongs to entry g / W, kept as (q, r) without a division per
  // word
  const unsigned long long n_here = a.total - e0 < kThreads ? a.total - e0 : kThreads;
  const unsigned long long words = n_here * W;
  uint32_t q = threadIdx.x / W, r = threadIdx.x % W;
  const uint32_t dq = kThreads / W, dr = kThreads % W;
  for (unsigned long long g = threadIdx.x; g < words; g += kThreads) {
    const uint32_t x = a.nh[e0 * W + g];
    if (x) atomicAdd(&s_width[q], (uint32_t)__popc(x));
    q += dq;
    r += dr;
    if (r >= W) {
      r -= W;
      ++q;
    }
  }
  __syncthreads();
  if (e >= a.total) return;
  const uint32_t k = a.key[e];
  if (k >= a.n_keys) {  // not a key of this plan: nothing is touched
    atomicOr(a.fault, kFaultListRoom);
    return;
  }
  const unsigned long long d = a.dist[e], bd = base_metric(a, k);
  spf_whatif_impact* o = a.imp + k;
  atomicAdd(&o->n_changed, 1u);
  if (d != bd) atomicAdd(&o->n_metric, 1u);
  if (d == kNoRoute) {
    atomicAdd(&o->n_unreachable, 1u);
    return;
  }
  if (d > bd) atomicMax(reinterpret_cast<unsigned long long*>(&o->max_metric), d);
  atomicMin(&o->min_width, s_width[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void wi_fill_kernel(WiArgs a) {
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.total) return;
  const uint32_t k = a.key[e];
  if (k >= a.n_keys) return;  // (the count pass reported it)
  const uint32_t i = list_owner(a.optr, a.n_own, e);
  const unsigned long long lo = a.tptr[k], hi = a.tptr[k + 1];
  const unsigned long long at = lo + atomicAdd(&a.cur[k], 1u);
  if (at >= hi || hi > a.total) {  // more entries than were counted: dropped
    atomicOr(a.fault, kFaultListRoom);
    return;
  }
  a.tfail[at] = i;
  a.tent[at] = e;
  const unsigned long long d = a.dist[e];
  if (d != kNoRoute && d > base_metric(a, k) && d == a.imp[k].max_metric)
    atomicMin(&a.imp[k].max_fail, i);
}

__global__ __launch_bounds__(kThreads) void wi_finish_kernel(WiArgs a) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= a.n_keys) return;
  const uint32_t w = a.imp[k].min_width;
  if (w & kBaseWidth) a.imp[k].min_width = w & ~kBaseWidth;
}

const char* const kCall[2] = {"spf_whatif_by_node", "spf_whatif_by_set"};
WiPoolId pool_id(int which) { return WiPoolId(kPoolByNode + which); }
// spf_whatif_by_<flavour><suffix>, as the messages name the call
std::string call(int which, const char* suffix) { return std::string(kCall[which]) + suffix; }

spf_status by_key(spf_whatif_plan* p, int which, uint64_t* n_entries, uint64_t* pool_bytes,
                  double* kernel_ms, void* stream) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "%s: NULL plan", kCall[which]);
  WiListsView v;
  whatif_lists_view(p, &v);
  spf_ctx* c = v.ctx;
  WiImpact& m = *v.imp[which];
  WiPool& T = m.pool;
  T.valid = false;  // after a failed call the plan holds none
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (v.epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  if (!v.changes->valid)
    return fail(c, SPF_E_STATE, "%s: the plan holds no lists (spf_whatif_changes first)", kCall[which]);
  const bool sets = which == SPF_WHATIF_BY_SET;
  const WiRoutes& r = *v.rt;
  if (sets && !r.pool.valid)
    return fail(c, SPF_E_STATE, "%s: the plan holds no route lists (spf_whatif_routes first)",
                kCall[which]);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const WiPool& L = sets ? r.pool : *v.changes;  // the lists to transpose
  const uint32_t n_keys = sets ? r.n_sets : c->N;
  const unsigned long long total = L.total;

  for (hipEvent_t& e : m.ev)
    if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  HIP_TRY(c, T.ptr.alloc((size_t)n_keys + 1));
  HIP_TRY(c, m.d_cur.alloc(std::max<uint32_t>(1, n_keys)));
  HIP_TRY(c, m.d_imp.alloc(std::max<uint32_t>(1, n_keys)));
  if (const spf_status st = pool_size(c, &T, total, 0, kCall[which]); st != SPF_OK) return st;

  WiArgs a{};
  a.key = L.key.p;
  a.dist = L.val.p;
  a.nh = L.rows.p;
  a.optr = L.ptr.p;
  a.n_own = v.n_fail;
  if (sets) {  // base routes: u64, zero rows where there is no route
    a.b64 = r.d_rbm.p;
    a.bnh = r.d_rbnh.p;
  } else {  // what spf_whatif_base returns, read as the plan holds it
    a.b32 = v.base_d32;
    a.b64 = reinterpret_cast<const unsigned long long*>(v.base_d64);
    a.bnh = v.base_nh;
    a.no_nbr = v.no_nbr;
  }
  a.n_keys = n_keys;
  a.W = v.W;
  a.total = total;
  a.imp = m.d_imp.p;
  a.cur = m.d_cur.p;
  a.tptr = T.ptr.p;
  a.tfail = T.key.p;
  a.tent = T.val.p;
  a.fault = c->d_fault.p;

  const dim3 by_keys(blocks_for(n_keys, kThreads)), by_entries(blocks_for(total, kThreads));
  HIP_TRY(c, hipEventRecord(m.ev[0], s));
  if (n_keys) {
    hipLaunchKernelGGL(wi_init_kernel, by_keys, dim3(kThreads), 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  if (total && n_keys) {
    hipLaunchKernelGGL(wi_count_kernel, by_entries, dim3(kThreads), 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(m.ev[1], s));
  HIP_TRY(c, whatif_scan(&m.d_imp.p->n_changed, sizeof(spf_whatif_impact) / 4, n_keys, T.ptr.p, s));
  HIP_TRY(c, hipEventRecord(m.ev[2], s));
  if (total && n_keys) {
    hipLaunchKernelGGL(wi_fill_kernel, by_entries, dim3(kThreads), 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  if (n_keys) {
    hipLaunchKernelGGL(wi_finish_kernel, by_keys, dim3(kThreads), 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(m.ev[3], s));
  unsigned long long placed = 0;
  HIP_TRY(c, hipMemcpyAsync(&placed, T.ptr.p + n_keys, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  if (placed != total)
    return fail(c, SPF_E_HIP, "%s: %llu entries counted, the lists hold %llu", kCall[which], placed,
                total);
  for (int k = 0; k < 3; ++k) {
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, m.ev[k], m.ev[k + 1]));
    m.ms[k] = ms;
  }
  T.n_owners = n_keys;
  T.total = total;
  T.valid = true;
  if (n_entries) *n_entries = total;
  if (pool_bytes) *pool_bytes = spfi::pool_bytes(T) + 32ull * n_keys;
  if (kernel_ms) *kernel_ms = m.ms[0] + m.ms[1] + m.ms[2];
  return SPF_OK;
}

spf_status impact_of(spf_whatif_plan* p, int which, spf_whatif_impact* out) {
  WiListsView v;
  if (const spf_status st = pool_held(p, pool_id(which), call(which, "_impact").c_str(), &v); st != SPF_OK)
    return st;
  spf_ctx* c = v.ctx;
  const WiImpact& m = *v.imp[which];
  HIP_TRY(c, hipSetDevice(c->device));
  if (out && m.pool.n_owners)
    HIP_TRY(c, hipMemcpy(out, m.d_imp.p, sizeof(spf_whatif_impact) * m.pool.n_owners, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status read_of(spf_whatif_plan* p, int which, uint64_t* ptr, uint32_t* failure, uint64_t* ent,
                   spf_whatif_impact* imp) {
  const spf_status st = pool_read(p, pool_id(which), call(which, "_read").c_str(), ptr, failure, ent, nullptr);
  return st == SPF_OK && imp ? impact_of(p, which, imp) : st;
}

spf_status buffers_of(spf_whatif_plan* p, int which, const uint64_t** d_ptr, const uint32_t** d_fail,
                      const uint64_t** d_ent, const spf_whatif_impact** d_imp, uint32_t* n_keys,
                      uint64_t* n_entries) {
  const spf_status st = pool_buffers(p, pool_id(which), call(which, "_buffers").c_str(), d_ptr, d_fail,
                                     d_ent, nullptr, n_keys, nullptr, n_entries);
  if (st != SPF_OK || !d_imp) return st;
  WiListsView v;
  whatif_lists_view(p, &v);
  *d_imp = v.imp[which]->d_imp.p;
  return SPF_OK;
}

spf_status db_of(spf_whatif_plan* p, int which, uint32_t key, uint32_t* failure, uint64_t* ent,
                 uint64_t cap, uint64_t* n) {
  return pool_db(p, pool_id(which), call(which, "_db").c_str(), key, failure, ent, nullptr, cap, n);
}

}  // namespace

extern "C" {

spf_status spf_whatif_by_node(spf_whatif_plan* p, uint64_t* n_entries, uint64_t* pool_bytes,
                              double* kernel_ms, void* stream) {
  return by_key(p, SPF_WHATIF_BY_NODE, n_entries, pool_bytes, kernel_ms, stream);
}
spf_status spf_whatif_by_set(spf_whatif_plan* p, uint64_t* n_entries, uint64_t* pool_bytes,
                             double* kernel_ms, void* stream) {
  return by_key(p, SPF_WHATIF_BY_SET, n_entries, pool_bytes, kernel_ms, stream);
}

spf_status spf_whatif_by_node_impact(spf_whatif_plan* p, spf_whatif_impact* out) {
  return impact_of(p, SPF_WHATIF_BY_NODE, out);
}
spf_status spf_whatif_by_set_impact(spf_whatif_plan* p, spf_whatif_impact* out) {
  return impact_of(p, SPF_WHATIF_BY_SET, out);
}

spf_status spf_whatif_by_node_db(spf_whatif_plan* p, uint32_t key, uint32_t* failure, uint64_t* ent,
                                 uint64_t cap, uint64_t* n) {
  return db_of(p, SPF_WHATIF_BY_NODE, key, failure, ent, cap, n);
}
spf_status spf_whatif_by_set_db(spf_whatif_plan* p, uint32_t key, uint32_t* failure, uint64_t* ent,
                                uint64_t cap, uint64_t* n) {
  return db_of(p, SPF_WHATIF_BY_SET, key, failure, ent, cap, n);
}

spf_status spf_whatif_by_node_read(spf_whatif_plan* p, uint64_t* ptr, uint32_t* failure, uint64_t* ent,
                                   spf_whatif_impact* imp) {
  return read_of(p, SPF_WHATIF_BY_NODE, ptr, failure, ent, imp);
}
spf_status spf_whatif_by_set_read(spf_whatif_plan* p, uint64_t* ptr, uint32_t* failure, uint64_t* ent,
                                  spf_whatif_impact* imp) {
  return read_of(p, SPF_WHATIF_BY_SET, ptr, failure, ent, imp);
}

spf_status spf_whatif_by_node_buffers(spf_whatif_plan* p, const uint64_t** d_ptr, const uint32_t** d_fail,
                                      const uint64_t** d_ent, const spf_whatif_impact** d_imp,
                                      uint32_t* n_keys, uint64_t* n_entries) {
  return buffers_of(p, SPF_WHATIF_BY_NODE, d_ptr, d_fail, d_ent, d_imp, n_keys, n_entries);
}
spf_status spf_whatif_by_set_buffers(spf_whatif_plan* p, const uint64_t** d_ptr, const uint32_t** d_fail,
                                     const uint64_t** d_ent, const spf_whatif_impact** d_imp,
                                     uint32_t* n_keys, uint64_t* n_entries) {
  return buffers_of(p, SPF_WHATIF_BY_SET, d_ptr, d_fail, d_ent, d_imp, n_keys, n_entries);
}

spf_status spf_whatif_impact_timing(const spf_whatif_plan* p, uint32_t which, double* ms) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_whatif_impact_timing: NULL plan");
  WiListsView v;
  whatif_lists_view(const_cast<spf_whatif_plan*>(p), &v);
  if (which > SPF_WHATIF_BY_SET || !ms)
    return fail(v.ctx, SPF_E_INVALID, "spf_whatif_impact_timing: which = %u, ms = %p", which, (void*)ms);
  if (!v.imp[which]->pool.valid)
    return fail(v.ctx, SPF_E_STATE, "spf_whatif_impact_timing: the plan holds no impact lists (%s first)",
                kCall[which]);
  for (int k = 0; k < 3; ++k) ms[k] = v.imp[which]->ms[k];
  return SPF_OK;
}

}  // extern "C"
