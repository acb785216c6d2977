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
#include "whatif_owner.h"

#include <cstddef>
#include <numeric>

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
    atomicOr(a.fault, 64u);
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
    atomicOr(a.fault, 64u);
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

uint32_t blocks_for(unsigned long long items, uint32_t per_block) {
  return (uint32_t)((items + per_block - 1) / per_block);
}

const char* const kCall[2] = {"spf_whatif_by_node", "spf_whatif_by_set"};

// The plan's view when it holds flavour `which`, the call named as
// spf_whatif_by_<flavour><suffix> in the messages.
spf_status held(spf_whatif_plan* p, int which, const char* suffix, WiListsView* v) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "%s%s: NULL plan", kCall[which], suffix);
  whatif_lists_view(p, v);
  if (!v->imp[which]->valid)
    return fail(v->ctx, SPF_E_STATE, "%s%s: the plan holds no impact lists (%s first)", kCall[which],
                suffix, kCall[which]);
  return SPF_OK;
}

spf_status by_key(spf_whatif_plan* p, int which, uint64_t* n_entries, uint64_t* pool_bytes,
                  double* kernel_ms, void* stream) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "%s: NULL plan", kCall[which]);
  WiListsView v;
  whatif_lists_view(p, &v);
  spf_ctx* c = v.ctx;
  WiImpact& m = *v.imp[which];
  m.valid = false;  // after a failed call the plan holds none
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (v.epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  if (!v.has_lists)
    return fail(c, SPF_E_STATE, "%s: the plan holds no lists (spf_whatif_changes first)", kCall[which]);
  const bool sets = which == SPF_WHATIF_BY_SET;
  if (sets && !v.rt->valid)
    return fail(c, SPF_E_STATE, "%s: the plan holds no route lists (spf_whatif_routes first)",
                kCall[which]);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const WiRoutes& r = *v.rt;
  const uint32_t n_keys = sets ? r.n_sets : c->N;
  const unsigned long long total = sets ? r.total : v.total;

  for (hipEvent_t& e : m.ev)
    if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  const size_t room = std::max<size_t>(1, (size_t)total);
  HIP_TRY(c, m.d_tptr.alloc((size_t)n_keys + 1));
  HIP_TRY(c, m.d_cur.alloc(std::max<uint32_t>(1, n_keys)));
  HIP_TRY(c, m.d_imp.alloc(std::max<uint32_t>(1, n_keys)));
  if (m.d_tfail.alloc(room) != hipSuccess || m.d_tent.alloc(room) != hipSuccess) {
    (void)hipGetLastError();
    m.d_tfail.reset();
    m.d_tent.reset();
    return fail(c, SPF_E_NOMEM, "%s: no memory for %llu entries of 12 bytes", kCall[which], total);
  }

  WiArgs a{};
  a.key = sets ? r.d_rset.p : v.cnode;
  a.dist = sets ? r.d_rmet.p : v.cdist;
  a.nh = sets ? r.d_rnh.p : v.cnh;
  a.optr = sets ? r.d_rptr.p : v.cptr;
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
  a.tptr = m.d_tptr.p;
  a.tfail = m.d_tfail.p;
  a.tent = m.d_tent.p;
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
  HIP_TRY(c, whatif_scan(&m.d_imp.p->n_changed, sizeof(spf_whatif_impact) / 4, n_keys, m.d_tptr.p, s));
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
  HIP_TRY(c, hipMemcpyAsync(&placed, m.d_tptr.p + n_keys, 8, hipMemcpyDeviceToHost, s));
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
  m.n_keys = n_keys;
  m.total = total;
  m.valid = true;
  if (n_entries) *n_entries = total;
  if (pool_bytes) *pool_bytes = 8ull * ((uint64_t)n_keys + 1) + 12ull * total + 32ull * n_keys;
  if (kernel_ms) *kernel_ms = m.ms[0] + m.ms[1] + m.ms[2];
  return SPF_OK;
}

spf_status impact_of(spf_whatif_plan* p, int which, spf_whatif_impact* out) {
  WiListsView v;
  if (const spf_status st = held(p, which, "_impact", &v); st != SPF_OK) return st;
  spf_ctx* c = v.ctx;
  const WiImpact& m = *v.imp[which];
  HIP_TRY(c, hipSetDevice(c->device));
  if (out && m.n_keys)
    HIP_TRY(c, hipMemcpy(out, m.d_imp.p, sizeof(spf_whatif_impact) * m.n_keys, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status read_of(spf_whatif_plan* p, int which, uint64_t* ptr, uint32_t* failure, uint64_t* ent,
                   spf_whatif_impact* imp) {
  WiListsView v;
  if (const spf_status st = held(p, which, "_read", &v); st != SPF_OK) return st;
  spf_ctx* c = v.ctx;
  const WiImpact& m = *v.imp[which];
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t t = (size_t)m.total, nk = m.n_keys;
  if (ptr) HIP_TRY(c, hipMemcpy(ptr, m.d_tptr.p, 8 * (nk + 1), hipMemcpyDeviceToHost));
  if (failure && t) HIP_TRY(c, hipMemcpy(failure, m.d_tfail.p, 4 * t, hipMemcpyDeviceToHost));
  if (ent && t) HIP_TRY(c, hipMemcpy(ent, m.d_tent.p, 8 * t, hipMemcpyDeviceToHost));
  if (imp && nk) HIP_TRY(c, hipMemcpy(imp, m.d_imp.p, sizeof(spf_whatif_impact) * nk, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status buffers_of(spf_whatif_plan* p, int which, const uint64_t** d_ptr, const uint32_t** d_fail,
                      const uint64_t** d_ent, const spf_whatif_impact** d_imp, uint32_t* n_keys,
                      uint64_t* n_entries) {
  WiListsView v;
  if (const spf_status st = held(p, which, "_buffers", &v); st != SPF_OK) return st;
  const WiImpact& m = *v.imp[which];
  if (d_ptr) *d_ptr = reinterpret_cast<const uint64_t*>(m.d_tptr.p);
  if (d_fail) *d_fail = m.d_tfail.p;
  if (d_ent) *d_ent = reinterpret_cast<const uint64_t*>(m.d_tent.p);
  if (d_imp) *d_imp = m.d_imp.p;
  if (n_keys) *n_keys = m.n_keys;
  if (n_entries) *n_entries = m.total;
  return SPF_OK;
}

spf_status db_of(spf_whatif_plan* p, int which, uint32_t key, uint32_t* failure, uint64_t* ent,
                 uint64_t cap, uint64_t* n) {
  WiListsView v;
  if (const spf_status st = held(p, which, "_db", &v); st != SPF_OK) return st;
  spf_ctx* c = v.ctx;
  const WiImpact& m = *v.imp[which];
  if (key >= m.n_keys) return fail(c, SPF_E_INVALID, "%s_db: key %u of %u", kCall[which], key, m.n_keys);
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long at[2] = {0, 0};
  HIP_TRY(c, hipMemcpy(at, m.d_tptr.p + key, 16, hipMemcpyDeviceToHost));
  if (at[1] < at[0] || at[1] > m.total) return fail(c, SPF_E_HIP, "%s_db: offsets not monotone", kCall[which]);
  const size_t cnt = (size_t)(at[1] - at[0]);
  if (n) *n = cnt;
  if (!failure && !ent) return SPF_OK;
  if (cap < cnt)
    return fail(c, SPF_E_NOMEM, "%s_db: %zu entries, room for %llu", kCall[which], cnt,
                (unsigned long long)cap);
  if (!cnt) return SPF_OK;
  std::vector<uint32_t> hf(cnt);
  std::vector<uint64_t> he(cnt);
  HIP_TRY(c, hipMemcpy(hf.data(), m.d_tfail.p + at[0], 4 * cnt, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(he.data(), m.d_tent.p + at[0], 8 * cnt, hipMemcpyDeviceToHost));
  std::vector<size_t> order(cnt);  // the device order is the cursor's: ascending by failure here
  std::iota(order.begin(), order.end(), (size_t)0);
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    return hf[x] != hf[y] ? hf[x] < hf[y] : he[x] < he[y];
  });
  for (size_t k = 0; k < cnt; ++k) {
    if (failure) failure[k] = hf[order[k]];
    if (ent) ent[k] = he[order[k]];
  }
  return SPF_OK;
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
  if (!v.imp[which]->valid)
    return fail(v.ctx, SPF_E_STATE, "spf_whatif_impact_timing: the plan holds no impact lists (%s first)",
                kCall[which]);
  for (int k = 0; k < 3; ++k) ms[k] = v.imp[which]->ms[k];
  return SPF_OK;
}

}  // extern "C"
