// ============================================================================
//  ksp2_route_delta.hip -- the KSP2_ED_ECMP route databases of two generations
//  compared and the difference's payload gathered, on the device that holds
//  the pools (spf_ksp2_route_snapshot / _delta / _update, include/openr_spf.h).
//
//  Reference: DecisionRouteDb::calculateUpdate in openr/decision/Decision.cpp
//    :111-146   routes to update (new, or the entry differs) and routes to
//               delete (gone), against the previous database
//  for every source of a KSP2 plan at once, over the pools spf_ksp2_routes
//  (ksp2_routes.hip) materialised: the old generation held by an
//  spf_ksp2_snapshot, the new one by the plan.  A route's value is its
//  set of next hops, each the triple (first-hop link by value, cost, label
//  stack as a sequence).  Records name CSR edges and the CSR moves between
//  generations, so first hops compare through key[e] = link_hash[link_id[e]]
//  of their own generation.
//
//  GPU mapping.  Nearly every route of a real delta is unchanged and lies in
//  the same order in both pools, and a route has a handful of next hops, so
//  the compare is bound by reading both generations' pools once:
//    positional pass  a lane per route (source i, set p), 256 routes of one
//               source per workgroup: the lanes of a wave read consecutive
//               rptr entries of either generation (coalesced), and
//               consecutive routes' records, offsets and label words are
//               neighbours in their pools, so the wave's loads fall on a few
//               lines it uses whole.  Equal hop counts, then hop by hop an
//               equal key, cost, stack length and stack words.
//    set pass   the routes whose positional pass failed at equal hop counts
//               (their order in the pool moved, or they differ): the wave
//               ballots them and takes them one after another, the new hops
//               on the lanes (strided by 64: any number of next hops), each
//               lane searching the old hops for its own.  Either side is a
//               set of the same size, so every new hop found = equal sets.
//               c^2 / 64 hop compares per lane for c next hops; only routes
//               that moved take it.
//  The kind of every route (a byte) and the changed routes of every workgroup
//  go to memory; the label routes' deterministic scan over the workgroup
//  counts and the IP delta's fill pass (route_delta.hip) place the entries:
//  three ordinary launches, no route takes an atomic, no workgroup waits for
//  another.  The matched routes and the deletes are counted with one atomic per
//  workgroup that has any.
//
//  The payload (spf_ksp2_route_update) is two gathers, each count, scan, fill:
//  a lane per entry sizes uptr; a lane per record copies it and sizes ulptr; a
//  lane per record copies its stack.
//
//  Every index read from a pool is checked against the pool's size before it
//  is used; a violation sets the fault word and the call fails.
// ============================================================================
#include "engine_internal.h"
#include "list_owner.h"

using namespace spfi;

namespace {

constexpr uint32_t kKdThreads = 256;  // routes per workgroup (= route_delta.hip's fill geometry)
constexpr uint8_t kSame = 0, kUpdate = 1, kDelete = 2;

// One generation's pools with their sizes.
struct Gen {
  const unsigned long long* rptr;  // [n_routes + 1]
  const unsigned long long* rec;   // [hops]
  const unsigned long long* lptr;  // [hops + 1]
  const int32_t* lab;              // [words]
  const unsigned long long* key;   // [E]
  unsigned long long hops, words;
  uint32_t E;
};

struct Hop {
  unsigned long long key;
  uint32_t cost, len;
  unsigned long long at;  // first label word
  bool ok;                // every index was inside its pool
};

__device__ __forceinline__ Hop load_hop(const Gen& g, unsigned long long h) {
  Hop x{0, 0, 0, 0, false};
  if (h >= g.hops) return x;
  const unsigned long long r = g.rec[h], l0 = g.lptr[h], l1 = g.lptr[h + 1];
  const uint32_t e = (uint32_t)r;
  if (e >= g.E || l0 > l1 || l1 > g.words || l1 - l0 > 0xFFFFFFFFull) return x;
  x.key = g.key[e];
  x.cost = (uint32_t)(r >> 32);
  x.len = (uint32_t)(l1 - l0);
  x.at = l0;
  x.ok = true;
  return x;
}

__device__ __forceinline__ bool same_hop(const Gen& o, const Hop& a, const Gen& n, const Hop& b) {
  if (a.key != b.key || a.cost != b.cost || a.len != b.len) return false;
  for (uint32_t t = 0; t < a.len; ++t)
    if (o.lab[a.at + t] != n.lab[b.at + t]) return false;
  return true;
}

// kind[i * S + p] of every route and the workgroup's changed routes into
// blk[blockIdx]; cnt[1] += the routes the set pass decided, cnt[2] = 1 on an
// index outside its pool.  n_chunks workgroups per source.
__global__ __launch_bounds__(kKdThreads) void ksp2_delta_kernel(Gen o, Gen n, uint32_t S, uint32_t n_chunks,
                                                                uint8_t* __restrict__ kind,
                                                                unsigned long long* __restrict__ blk,
                                                                unsigned long long* __restrict__ cnt) {
  const uint32_t i = blockIdx.x / n_chunks, chunk = blockIdx.x % n_chunks;
  const uint32_t p = chunk * kKdThreads + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long r = (unsigned long long)i * S + p;
  uint8_t kd = kSame;
  bool match = false, bad = false;
  unsigned long long o0 = 0, n0 = 0;
  uint32_t c = 0;
  if (p < S) {
    o0 = o.rptr[r];
    n0 = n.rptr[r];
    const unsigned long long o1 = o.rptr[r + 1], n1 = n.rptr[r + 1];
    if (o0 > o1 || o1 > o.hops || n0 > n1 || n1 > n.hops || n1 - n0 > 0xFFFFFFFFull) {
      bad = true;
      kd = kUpdate;
    } else if (n1 == n0) {
      kd = o1 != o0 ? kDelete : kSame;
    } else if (o1 - o0 != n1 - n0) {
      kd = kUpdate;
    } else {
      c = (uint32_t)(n1 - n0);
      bool eq = true;
      for (uint32_t h = 0; h < c && eq; ++h) {
        const Hop a = load_hop(o, o0 + h), b = load_hop(n, n0 + h);
        bad |= !a.ok || !b.ok;
        eq = a.ok && b.ok && same_hop(o, a, n, b);
      }
      match = !eq && !bad;
      if (bad) kd = kUpdate;
    }
  }
  // ---- the set pass: the wave takes its routes that need it one by one ----
  unsigned long long todo = __ballot(match);
  uint32_t n_matched = 0;
  while (todo) {
    const int b = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const unsigned long long wo0 = __shfl(o0, b), wn0 = __shfl(n0, b);  // (64-bit shuffles)
    const uint32_t wc = __shfl(c, b);
    bool all = true, wbad = false;
    for (uint32_t base = 0; base < wc; base += 64) {
      const uint32_t j = base + lane;
      bool found = true;
      if (j < wc) {
        const Hop mine = load_hop(n, wn0 + j);
        wbad |= !mine.ok;
        found = false;
        for (uint32_t k = 0; k < wc && !found && mine.ok; ++k) {
          const Hop a = load_hop(o, wo0 + k);
          wbad |= !a.ok;
          found = a.ok && same_hop(o, a, n, mine);
        }
      }
      all &= __all(found) != 0;
      if (!all) break;  // (wave-uniform)
    }
    wbad = __any(wbad) != 0;
    if (lane == (uint32_t)b) {
      kd = all && !wbad ? kSame : kUpdate;
      bad |= wbad;
    }
    ++n_matched;
  }
  if (p < S) kind[r] = kd;
  const int changed = __syncthreads_count(kd != kSame);
  const int any_bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    blk[blockIdx.x] = (unsigned long long)changed;
    if (any_bad) cnt[2] = 1ull;
  }
  if (lane == 0 && n_matched) atomicAdd(&cnt[1], (unsigned long long)n_matched);
}

// ---- the payload -----------------------------------------------------------
// uptr[j] = entry j's records (0 for a delete), usrc[j] = its first record in
// the plan's pool; entry j of dset belongs to the source slot
// list_owner(dptr, n_src, j).
__global__ __launch_bounds__(kKdThreads) void ksp2_update_count_kernel(
    const unsigned long long* __restrict__ dptr, const uint32_t* __restrict__ dset, uint32_t n_src,
    unsigned long long entries, const unsigned long long* __restrict__ rptr, unsigned long long hops,
    uint32_t S, unsigned long long* __restrict__ uptr, unsigned long long* __restrict__ usrc,
    unsigned long long* __restrict__ cnt) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kKdThreads + threadIdx.x;
  if (j >= entries) return;
  const uint32_t v = dset[j];
  unsigned long long c = 0, at = 0;
  if (!(v & SPF_DELTA_DELETE)) {
    const uint32_t i = list_owner(dptr, n_src, j);
    if (v < S) {
      const unsigned long long r = (unsigned long long)i * S + v;
      const unsigned long long a = rptr[r], b = rptr[r + 1];
      if (a <= b && b <= hops) {
        at = a;
        c = b - a;
      } else {
        cnt[2] = 1ull;
      }
    } else {
      cnt[2] = 1ull;
    }
  }
  uptr[j] = c;
  usrc[j] = at;
}

// record k of the payload: copied, its stack's length into ulptr[k], where
// the stack starts in the plan's pool into ulsrc[k].  uptr is scanned.
__global__ __launch_bounds__(kKdThreads) void ksp2_update_records_kernel(
    const unsigned long long* __restrict__ uptr, const unsigned long long* __restrict__ usrc,
    unsigned long long entries, unsigned long long n_urec, const unsigned long long* __restrict__ rec,
    const unsigned long long* __restrict__ lptr, unsigned long long hops, unsigned long long words,
    unsigned long long* __restrict__ urec, unsigned long long* __restrict__ ulptr,
    unsigned long long* __restrict__ ulsrc, unsigned long long* __restrict__ cnt) {
  const unsigned long long k = (unsigned long long)blockIdx.x * kKdThreads + threadIdx.x;
  if (k >= n_urec) return;
  // (entries < 2^32: dset entries of n_src < 2^32 sources x n_sets < 2^31 are
  // bounded by the caller; the search runs over 64-bit positions)
  const unsigned long long lo = list_owner(uptr, entries, k);
  const unsigned long long h = usrc[lo] + (k - uptr[lo]);
  unsigned long long r = 0, l0 = 0, l1 = 0;
  if (h < hops) {
    r = rec[h];
    l0 = lptr[h];
    l1 = lptr[h + 1];
  }
  if (h >= hops || l0 > l1 || l1 > words) {
    cnt[2] = 1ull;
    l0 = l1 = 0;
  }
  urec[k] = r;
  ulptr[k] = l1 - l0;
  ulsrc[k] = l0;
}

// record k's stack into ulab at the scanned ulptr[k]
__global__ __launch_bounds__(kKdThreads) void ksp2_update_labels_kernel(
    const unsigned long long* __restrict__ ulptr, const unsigned long long* __restrict__ ulsrc,
    unsigned long long n_urec, const int32_t* __restrict__ lab, int32_t* __restrict__ ulab) {
  const unsigned long long k = (unsigned long long)blockIdx.x * kKdThreads + threadIdx.x;
  if (k >= n_urec) return;
  const unsigned long long a = ulptr[k], n = ulptr[k + 1] - a, from = ulsrc[k];
  for (unsigned long long t = 0; t < n; ++t) ulab[a + t] = lab[from + t];
}

// key[e] = link_hash[link_id[e]] over the loaded CSR
spf_status edge_keys(spf_ctx* c, const uint64_t* link_hash, uint32_t n_links, const char* who,
                     std::vector<unsigned long long>* out) {
  out->assign(std::max<uint32_t>(c->E, 1), 0ull);
  for (uint32_t e = 0; e < c->E; ++e) {
    if (c->link[e] >= n_links) return fail(c, SPF_E_INVALID, "%s: link_hash shorter than the link ids", who);
    (*out)[e] = link_hash[c->link[e]];
  }
  return SPF_OK;
}

float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

}  // namespace

spf_ksp2_snapshot::~spf_ksp2_snapshot() {
  if (!ctx) return;
  // (a delta's kernels may still read the pools)
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  auto& v = ctx->ksp2_snaps;
  v.erase(std::remove(v.begin(), v.end(), this), v.end());
}

extern "C" {

spf_status spf_ksp2_route_snapshot(spf_ksp2_plan* p, const uint64_t* link_hash, uint32_t n_links,
                                   spf_ksp2_snapshot** out) {
  if (!p || !link_hash || !out)
    return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_ksp2_route_snapshot: NULL argument");
  *out = nullptr;
  spf_ctx* c = p->ctx;
  Ksp2Routes& rt = p->rt;
  if (!rt.valid) return fail(c, SPF_E_STATE, "spf_ksp2_route_snapshot: the plan holds no routes (call spf_ksp2_routes)");
  if (!c->loaded || p->epoch != c->epoch)
    return fail(c, SPF_E_STATE, "spf_ksp2_route_snapshot: graph changed since the plan was created");
  std::vector<unsigned long long> key;
  spf_status st = edge_keys(c, link_hash, n_links, "spf_ksp2_route_snapshot", &key);
  if (st != SPF_OK) return st;
  auto sn = std::make_unique<spf_ksp2_snapshot>();
  HIP_TRY(c, hipSetDevice(c->device));
  // the keys first: nothing has moved when the upload fails
  HIP_TRY(c, sn->key.upload(key.data(), key.size(), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (`key` is this call's)
  sn->srcs = p->srcs;
  sn->n_nodes = c->N;
  sn->n_sets = rt.n_sets;
  sn->n_edges = c->E;
  sn->hops = rt.hops;
  sn->words = rt.words;
  sn->rptr.take(rt.d_rptr);
  sn->rec.take(rt.d_rec);
  sn->lptr.take(rt.d_lptr);
  sn->lab.take(rt.d_lab);
  rt.valid = false;
  ++rt.gen;
  sn->ctx = c;
  c->ksp2_snaps.push_back(sn.get());
  *out = sn.release();
  return SPF_OK;
}

void spf_ksp2_route_snapshot_destroy(spf_ksp2_snapshot* snap) { delete snap; }

uint64_t spf_ksp2_route_snapshot_bytes(const spf_ksp2_snapshot* snap) {
  if (!snap) return 0;
  return 8ull * (snap->rptr.n + snap->rec.n + snap->lptr.n + snap->key.n) + 4ull * snap->lab.n;
}

spf_status spf_ksp2_route_delta(spf_ksp2_plan* p, const spf_ksp2_snapshot* snap,
                                const uint64_t* link_hash, uint32_t n_links, uint64_t* totals,
                                double* kernel_ms) {
  if (!p || !snap || !link_hash)
    return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_ksp2_route_delta: NULL argument");
  spf_ctx* c = p->ctx;
  Ksp2Routes& rt = p->rt;
  Ksp2Delta& d = p->dl;
  d.valid = d.up_valid = false;
  if (snap->ctx != c) return fail(c, SPF_E_INVALID, "spf_ksp2_route_delta: the snapshot is another context's");
  if (!rt.valid) return fail(c, SPF_E_STATE, "spf_ksp2_route_delta: the plan holds no routes (call spf_ksp2_routes)");
  if (!c->loaded || p->epoch != c->epoch)
    return fail(c, SPF_E_STATE, "spf_ksp2_route_delta: graph changed since the routes were built");
  if (snap->srcs != p->srcs || snap->n_nodes != c->N || snap->n_sets != rt.n_sets)
    return fail(c, SPF_E_INVALID, "spf_ksp2_route_delta: srcs, n_nodes or n_sets differ from the snapshot");
  const uint32_t S = rt.n_sets, n_src = p->n_src;
  if (S >= (1u << 31)) return fail(c, SPF_E_INVALID, "spf_ksp2_route_delta: n_sets >= 2^31");
  const uint32_t n_chunks = route_delta_chunks(S);
  const uint64_t blocks = (uint64_t)n_src * n_chunks;
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "spf_ksp2_route_delta: grid too large");
  std::vector<unsigned long long> key;
  spf_status st = edge_keys(c, link_hash, n_links, "spf_ksp2_route_delta", &key);
  if (st != SPF_OK) return st;
  const uint64_t n_routes = (uint64_t)n_src * S;

  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  for (hipEvent_t& e : d.ev)
    if (!e) HIP_TRY(c, hipEventCreate(&e));
  HIP_TRY(c, d.d_key.upload(key.data(), key.size(), s));
  HIP_TRY(c, d.d_kind.alloc(std::max<uint64_t>(n_routes, 1)));
  HIP_TRY(c, d.d_blk.alloc(blocks + 1));
  HIP_TRY(c, d.d_sums.alloc(std::max<uint64_t>(label_scan_tiles(blocks), 1)));
  HIP_TRY(c, d.d_dptr.alloc((size_t)n_src + 1));
  HIP_TRY(c, d.d_cnt.alloc(3));
  HIP_TRY(c, hipMemsetAsync(d.d_cnt.p, 0, 24, s));
  HIP_TRY(c, hipMemsetAsync(d.d_dptr.p, 0, 8ull * (n_src + 1), s));  // (a pass without routes writes none)
  const Gen go{snap->rptr.p, snap->rec.p, snap->lptr.p, snap->lab.p, snap->key.p, snap->hops, snap->words,
               snap->n_edges};
  const Gen gn{rt.d_rptr.p, rt.d_rec.p, rt.d_lptr.p, rt.d_lab.p, d.d_key.p, rt.hops, rt.words, c->E};
  HIP_TRY(c, hipEventRecord(d.ev[0], s));
  if (blocks) {
    hipLaunchKernelGGL(ksp2_delta_kernel, dim3((uint32_t)blocks), dim3(kKdThreads), 0, s, go, gn, S, n_chunks,
                       d.d_kind.p, d.d_blk.p, d.d_cnt.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(d.ev[1], s));
  st = launch_label_scan(c, d.d_blk.p, blocks, d.d_sums.p, s);
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(d.ev[2], s));
  unsigned long long total = 0, cnt[3] = {0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(&total, d.d_blk.p + blocks, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));  // (`key` has been uploaded too)
  HIP_TRY(c, d.d_dset.alloc(std::max<unsigned long long>(total, 1)));
  HIP_TRY(c, hipEventRecord(d.ev[3], s));
  st = launch_delta_fill(c, d.d_kind.p, S, n_src, d.d_blk.p, nullptr, d.d_dset.p, d.d_dptr.p, d.d_cnt.p, s);
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(d.ev[4], s));
  HIP_TRY(c, hipMemcpyAsync(cnt, d.d_cnt.p, 24, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (cnt[2]) return fail(c, SPF_E_STATE, "spf_ksp2_route_delta: a pool index lies outside its pool");
  d.ms[0] = elapsed(d.ev[0], d.ev[1]);
  d.ms[1] = elapsed(d.ev[1], d.ev[2]);
  d.ms[2] = elapsed(d.ev[3], d.ev[4]);
  d.ms[3] = d.ms[4] = d.ms[5] = 0;
  d.entries = total;
  d.tot[0] = total - cnt[0];
  d.tot[1] = cnt[0];
  d.tot[2] = cnt[1];
  d.gen = rt.gen;
  d.valid = true;
  if (totals) std::copy(d.tot, d.tot + 3, totals);
  if (kernel_ms) *kernel_ms = d.ms[0] + d.ms[1] + d.ms[2];
  return SPF_OK;
}

spf_status spf_ksp2_route_delta_db(spf_ksp2_plan* p, uint32_t i, uint32_t* set, uint64_t cap, uint64_t* n) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_ksp2_route_delta_db: NULL plan");
  spf_ctx* c = p->ctx;
  Ksp2Delta& d = p->dl;
  if (!d.valid) return fail(c, SPF_E_STATE, "spf_ksp2_route_delta_db: no delta (call spf_ksp2_route_delta)");
  if (i >= p->n_src) return fail(c, SPF_E_INVALID, "spf_ksp2_route_delta_db: no such source slot %u", i);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  unsigned long long h[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(h, d.d_dptr.p + i, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t cnt = h[1] - h[0];
  if (n) *n = cnt;
  if (!set) return SPF_OK;
  if (cap < cnt)
    return fail(c, SPF_E_NOMEM, "KSP2 route delta of %llu entries, room for %llu", (unsigned long long)cnt,
                (unsigned long long)cap);
  if (cnt) HIP_TRY(c, hipMemcpyAsync(set, d.d_dset.p + h[0], 4ull * cnt, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SPF_OK;
}

spf_status spf_ksp2_route_delta_buffers(spf_ksp2_plan* p, const uint64_t** d_dptr, const uint32_t** d_dset,
                                        uint64_t* n_entries) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_ksp2_route_delta_buffers: NULL plan");
  const Ksp2Delta& d = p->dl;
  if (!d.valid) return fail(p->ctx, SPF_E_STATE, "spf_ksp2_route_delta_buffers: no delta (call spf_ksp2_route_delta)");
  if (d_dptr) *d_dptr = reinterpret_cast<const uint64_t*>(d.d_dptr.p);
  if (d_dset) *d_dset = d.d_dset.p;
  if (n_entries) *n_entries = d.entries;
  return SPF_OK;
}

spf_status spf_ksp2_route_update(spf_ksp2_plan* p, uint64_t* totals, uint64_t* pool_bytes, double* kernel_ms) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_ksp2_route_update: NULL plan");
  spf_ctx* c = p->ctx;
  Ksp2Routes& rt = p->rt;
  Ksp2Delta& d = p->dl;
  d.up_valid = false;
  if (!d.valid) return fail(c, SPF_E_STATE, "spf_ksp2_route_update: no delta (call spf_ksp2_route_delta)");
  if (!rt.valid || rt.gen != d.gen)
    return fail(c, SPF_E_STATE, "spf_ksp2_route_update: the plan's routes are not the ones the delta compared");
  const uint64_t entries = d.entries;
  const uint64_t eblocks = (entries + kKdThreads - 1) / kKdThreads;
  if (eblocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "spf_ksp2_route_update: grid too large");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  HIP_TRY(c, d.d_uptr.alloc(entries + 1));
  HIP_TRY(c, d.d_usrc.alloc(std::max<uint64_t>(entries, 1)));
  HIP_TRY(c, d.d_sums.alloc(std::max<uint64_t>(label_scan_tiles(entries), 1)));
  HIP_TRY(c, hipMemsetAsync(d.d_cnt.p + 2, 0, 8, s));
  // ---- entries -> records ----
  HIP_TRY(c, hipEventRecord(d.ev[5], s));
  if (entries) {
    hipLaunchKernelGGL(ksp2_update_count_kernel, dim3((uint32_t)eblocks), dim3(kKdThreads), 0, s, d.d_dptr.p,
                       d.d_dset.p, p->n_src, (unsigned long long)entries, rt.d_rptr.p,
                       (unsigned long long)rt.hops, rt.n_sets, d.d_uptr.p, d.d_usrc.p, d.d_cnt.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(d.ev[6], s));
  spf_status st = launch_label_scan(c, d.d_uptr.p, entries, d.d_sums.p, s);
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(d.ev[7], s));
  unsigned long long n_urec = 0, n_words = 0, bad = 0;
  HIP_TRY(c, hipMemcpyAsync(&n_urec, d.d_uptr.p + entries, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t rblocks = (n_urec + kKdThreads - 1) / kKdThreads;
  if (rblocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "spf_ksp2_route_update: grid too large");
  HIP_TRY(c, d.d_urec.alloc(std::max<unsigned long long>(n_urec, 1)));
  HIP_TRY(c, d.d_ulptr.alloc(n_urec + 1));
  HIP_TRY(c, d.d_ulsrc.alloc(std::max<unsigned long long>(n_urec, 1)));
  HIP_TRY(c, d.d_sums.alloc(std::max<uint64_t>(label_scan_tiles(n_urec), 1)));
  // ---- records -> label words ----
  HIP_TRY(c, hipEventRecord(d.ev[8], s));
  if (n_urec) {
    hipLaunchKernelGGL(ksp2_update_records_kernel, dim3((uint32_t)rblocks), dim3(kKdThreads), 0, s, d.d_uptr.p,
                       d.d_usrc.p, (unsigned long long)entries, n_urec, rt.d_rec.p, rt.d_lptr.p,
                       (unsigned long long)rt.hops, (unsigned long long)rt.words, d.d_urec.p, d.d_ulptr.p,
                       d.d_ulsrc.p, d.d_cnt.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(d.ev[9], s));
  st = launch_label_scan(c, d.d_ulptr.p, n_urec, d.d_sums.p, s);
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(d.ev[10], s));
  HIP_TRY(c, hipMemcpyAsync(&n_words, d.d_ulptr.p + n_urec, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(&bad, d.d_cnt.p + 2, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (bad) return fail(c, SPF_E_STATE, "spf_ksp2_route_update: a pool index lies outside its pool");
  HIP_TRY(c, d.d_ulab.alloc(std::max<unsigned long long>(n_words, 1)));
  HIP_TRY(c, hipEventRecord(d.ev[11], s));
  if (n_urec) {
    hipLaunchKernelGGL(ksp2_update_labels_kernel, dim3((uint32_t)rblocks), dim3(kKdThreads), 0, s, d.d_ulptr.p,
                       d.d_ulsrc.p, n_urec, rt.d_lab.p, d.d_ulab.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(d.ev[12], s));
  HIP_TRY(c, hipStreamSynchronize(s));
  d.ms[3] = elapsed(d.ev[5], d.ev[6]) + elapsed(d.ev[8], d.ev[9]);
  d.ms[4] = elapsed(d.ev[6], d.ev[7]) + elapsed(d.ev[9], d.ev[10]);
  d.ms[5] = elapsed(d.ev[11], d.ev[12]);
  d.up_tot[0] = d.tot[0];
  d.up_tot[1] = n_urec;
  d.up_tot[2] = n_words;
  d.up_valid = true;
  if (totals) std::copy(d.up_tot, d.up_tot + 3, totals);
  if (pool_bytes) *pool_bytes = 8 * (entries + 1) + 8 * n_urec + 8 * (n_urec + 1) + 4 * n_words;
  if (kernel_ms) *kernel_ms = d.ms[3] + d.ms[4] + d.ms[5];
  return SPF_OK;
}

spf_status spf_ksp2_route_delta_timing(const spf_ksp2_plan* p, double* ms) {
  if (!p || !ms) return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_ksp2_route_delta_timing: NULL argument");
  if (!p->dl.valid) return fail(p->ctx, SPF_E_STATE, "spf_ksp2_route_delta_timing: no delta (call spf_ksp2_route_delta)");
  std::copy(p->dl.ms, p->dl.ms + 6, ms);
  return SPF_OK;
}

// the update of the plan's current delta and routes, or SPF_E_STATE
static spf_status update_held(spf_ksp2_plan* p, const char* who) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "%s: NULL plan", who);
  const Ksp2Delta& d = p->dl;
  if (!d.valid || !d.up_valid || !p->rt.valid || p->rt.gen != d.gen)
    return fail(p->ctx, SPF_E_STATE, "%s: no update (call spf_ksp2_route_update)", who);
  return SPF_OK;
}

spf_status spf_ksp2_route_update_db(spf_ksp2_plan* p, uint32_t i, uint64_t* uptr, uint64_t* urec,
                                    uint64_t rec_cap, uint64_t* n_rec, uint64_t* ulptr, int32_t* ulab,
                                    uint64_t lab_cap, uint64_t* n_lab) {
  spf_status st = update_held(p, "spf_ksp2_route_update_db");
  if (st != SPF_OK) return st;
  spf_ctx* c = p->ctx;
  Ksp2Delta& d = p->dl;
  if (i >= p->n_src) return fail(c, SPF_E_INVALID, "spf_ksp2_route_update_db: no such source slot %u", i);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  unsigned long long h[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(h, d.d_dptr.p + i, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t m = h[1] - h[0];
  std::vector<uint64_t> up(m + 1);
  HIP_TRY(c, hipMemcpyAsync(up.data(), d.d_uptr.p + h[0], 8ull * (m + 1), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t cnt = up[m] - up[0];
  std::vector<uint64_t> lp(cnt + 1);
  HIP_TRY(c, hipMemcpyAsync(lp.data(), d.d_ulptr.p + up[0], 8ull * (cnt + 1), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t words = lp[cnt] - lp[0];
  if (n_rec) *n_rec = cnt;
  if (n_lab) *n_lab = words;
  if ((urec || ulptr) && rec_cap < cnt)
    return fail(c, SPF_E_NOMEM, "KSP2 route update of %llu records, room for %llu", (unsigned long long)cnt,
                (unsigned long long)rec_cap);
  if (ulab && lab_cap < words)
    return fail(c, SPF_E_NOMEM, "KSP2 route update of %llu label words, room for %llu",
                (unsigned long long)words, (unsigned long long)lab_cap);
  if (urec && cnt) HIP_TRY(c, hipMemcpyAsync(urec, d.d_urec.p + up[0], 8ull * cnt, hipMemcpyDeviceToHost, s));
  if (ulab && words) HIP_TRY(c, hipMemcpyAsync(ulab, d.d_ulab.p + lp[0], 4ull * words, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (uptr)
    for (uint64_t k = 0; k <= m; ++k) uptr[k] = up[k] - up[0];
  if (ulptr)
    for (uint64_t k = 0; k <= cnt; ++k) ulptr[k] = lp[k] - lp[0];
  return SPF_OK;
}

spf_status spf_ksp2_route_update_read(spf_ksp2_plan* p, uint64_t* n, uint64_t* dptr, uint32_t* dset,
                                      uint64_t* uptr, uint64_t* urec, uint64_t* ulptr, int32_t* ulab) {
  spf_status st = update_held(p, "spf_ksp2_route_update_read");
  if (st != SPF_OK) return st;
  spf_ctx* c = p->ctx;
  Ksp2Delta& d = p->dl;
  const uint64_t ns = p->n_src, ne = d.entries, nr = d.up_tot[1], nw = d.up_tot[2];
  if (n) {
    n[0] = ns;
    n[1] = ne;
    n[2] = nr;
    n[3] = nw;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (dptr) HIP_TRY(c, hipMemcpyAsync(dptr, d.d_dptr.p, 8 * (ns + 1), hipMemcpyDeviceToHost, s));
  if (dset && ne) HIP_TRY(c, hipMemcpyAsync(dset, d.d_dset.p, 4 * ne, hipMemcpyDeviceToHost, s));
  if (uptr) HIP_TRY(c, hipMemcpyAsync(uptr, d.d_uptr.p, 8 * (ne + 1), hipMemcpyDeviceToHost, s));
  if (urec && nr) HIP_TRY(c, hipMemcpyAsync(urec, d.d_urec.p, 8 * nr, hipMemcpyDeviceToHost, s));
  if (ulptr) HIP_TRY(c, hipMemcpyAsync(ulptr, d.d_ulptr.p, 8 * (nr + 1), hipMemcpyDeviceToHost, s));
  if (ulab && nw) HIP_TRY(c, hipMemcpyAsync(ulab, d.d_ulab.p, 4 * nw, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SPF_OK;
}

spf_status spf_ksp2_route_update_buffers(spf_ksp2_plan* p, const uint64_t** d_uptr, const uint64_t** d_urec,
                                         const uint64_t** d_ulptr, const int32_t** d_ulab,
                                         uint64_t* n_records, uint64_t* n_label_words) {
  spf_status st = update_held(p, "spf_ksp2_route_update_buffers");
  if (st != SPF_OK) return st;
  const Ksp2Delta& d = p->dl;
  if (d_uptr) *d_uptr = reinterpret_cast<const uint64_t*>(d.d_uptr.p);
  if (d_urec) *d_urec = reinterpret_cast<const uint64_t*>(d.d_urec.p);
  if (d_ulptr) *d_ulptr = reinterpret_cast<const uint64_t*>(d.d_ulptr.p);
  if (d_ulab) *d_ulab = d.d_ulab.p;
  if (n_records) *n_records = d.up_tot[1];
  if (n_label_words) *n_label_words = d.up_tot[2];
  return SPF_OK;
}

}  // extern "C"
