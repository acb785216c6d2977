// ============================================================================
//  ksp2_routes.hip -- every source's KSP2_ED_ECMP routes (SR-MPLS label
//  stacks) from the device-resident pairs and pool of a KSP2 plan
//  (spf_ksp2_routes, include/openr_spf.h).
//
//  Reference: SpfSolver::SpfSolverImpl::selectBestPathsKsp2 in
//  openr/decision/Decision.cpp:895-1018, for one area:
//    :919-929    the k = 1 paths towards every best advertiser but me
//    :934-957    the k = 2 paths that contain none of those k = 1 paths
//                (LinkState::pathAInPathB, LinkState.h:395-410)
//    :964-1007   per path its cost, its first link and the PUSH label stack
//                [prepend?, L(vk), ..., L(v2)]; the next hops go into a
//                std::unordered_set<NextHopThrift>, so equal ones collapse
//  addBestPaths (:1020-1080: the min-nexthop threshold, static next hops of a
//  self-advertised prefix), thrift formatting and the union over several areas
//  stay with the host.
//
//  GPU mapping: one wavefront per route (source slot i, destination set p),
//  four routes per workgroup, candidates on the lanes in chunks of 64.
//    * the wave enumerates the route's candidates in the reference's order --
//      per member the chained k = 1 records, then the k = 2 records -- and
//      hands candidate n of a chunk to lane n;
//    * a lane walks its record once: cost, first CSR edge, stack length and a
//      64-bit key of (first edge, cost, label sequence).  A hop is one read of
//      the per-link table (both directed CSR edges of a link id with their
//      ends and metrics), not a scan of the node's row;
//    * a k = 2 lane tests its path against every k = 1 path of the route by
//      link ids;
//    * duplicates: inside a chunk a lane compares keys with the lanes before
//      it and, on a match, walks both records again (the key never decides);
//      against earlier chunks (routes with more than 64 candidates: rare) it
//      enumerates the earlier candidates itself and walks each against its
//      own, which is quadratic in the candidates of such a route;
//    * the survivors are balloted; their ranks and the scan of their stack
//      lengths place them.
//  Three ordinary launches size the pools exactly: count (next hops and label
//  words per route), the exclusive scans (label_routes.hip's), fill (the same
//  walk, the same decisions, records and stacks written with plain stores).
//  No atomics, no workgroup waits for another.
// ============================================================================
#include "engine_internal.h"

#include <cstdlib>

using namespace spfi;

namespace {

constexpr uint32_t kRtThreads = 256;
constexpr uint32_t kRtWaves = kRtThreads / 64;  // routes per workgroup

struct RtArgs {
  const uint4* pairs;    // spf_ksp2_pair = {first[0], first[1], n_paths[0], n_paths[1]}
  const uint32_t* pool;  // [n_links, next, link ids src -> dst]
  const uint4* links;    // per link id: {e_a, tail, head, metric_a}, {e_b, metric_b, 0, 0}
  uint32_t max_link;
  const uint32_t* srcs;
  uint32_t N, n_sets;
  unsigned long long n_routes;
  const uint32_t* set_ptr;
  const uint32_t* set_nodes;
  const int32_t* prepend;  // parallel to set_nodes, -1 = none; may be null
  const int32_t* label;    // [N]
  unsigned long long* rptr;   // count: next hops per route; fill: its scan
  unsigned long long* lbase;  // count: label words per route; fill: its scan
  unsigned long long* rec;
  unsigned long long* lptr;
  int32_t* lab;
};

struct Hop {
  uint32_t edge, node, met;
};

// the link `l` walked from `cur`: the CSR edge of cur's row, its head, the
// metric cur advertises
__device__ __forceinline__ Hop hop(const RtArgs& a, uint32_t l, uint32_t cur) {
  l = min(l, a.max_link);
  const uint4 x = a.links[2ull * l], y = a.links[2ull * l + 1];
  const bool fwd = cur == x.y;
  return {fwd ? x.x : y.x, fwd ? x.z : x.y, fwd ? x.w : y.y};
}

__device__ __forceinline__ uint64_t fnv(uint64_t h, uint64_t x) { return (h ^ x) * 0x100000001b3ULL; }
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

__device__ __forceinline__ int32_t prepend_of(const RtArgs& a, uint32_t m) {
  return a.prepend ? a.prepend[m] : -1;
}

// The route's candidate records in the reference's order: for k = 0 (the
// k = 1 lists) and then k = 1 (the k = 2 lists), the members in set order,
// each member's chained records.  A member equal to me has none.
struct Cursor {
  uint32_t k = 0, m, q = 0, np = 0, at = 0, dm = 0;
  __device__ explicit Cursor(uint32_t m0) : m(m0) {}
  // the next record of the lists k <= kmax: its pool offset, its member's
  // index into set_nodes, its list
  __device__ bool next(const RtArgs& a, const uint4* row, uint32_t me, uint32_t m0, uint32_t m1,
                       uint32_t kmax, uint32_t* o_at, uint32_t* o_m, uint32_t* o_k) {
    while (q == np) {  // open the next member's list
      if (m == m1) {
        if (k == kmax) return false;
        k = 1;
        m = m0;
        q = np = 0;
        continue;
      }
      const uint32_t d = a.set_nodes[m];
      const uint4 h = row[d];
      np = d == me ? 0u : (k ? h.w : h.z);
      at = k ? h.y : h.x;
      q = 0;
      dm = m++;
    }
    *o_at = at;
    *o_m = dm;
    *o_k = k;
    at = a.pool[(size_t)at + 1];
    ++q;
    return true;
  }
};

// LinkState::pathAInPathB over every k = 1 path A of the route: the k = 2
// record at `at_b` holds one of them as a contiguous run of link ids
__device__ bool k2_dropped(const RtArgs& a, const uint4* row, uint32_t me, uint32_t m0, uint32_t m1,
                           uint32_t at_b) {
  const uint32_t lb = a.pool[at_b];
  const uint32_t* B = a.pool + (size_t)at_b + 2;
  Cursor c(m0);
  uint32_t at_a, m_a, k_a;
  while (c.next(a, row, me, m0, m1, 0, &at_a, &m_a, &k_a)) {
    const uint32_t la = a.pool[at_a];
    if (la > lb || la == 0) continue;
    const uint32_t* A = a.pool + (size_t)at_a + 2;
    const uint32_t a0 = A[0];
    for (uint32_t i = 0; i + la <= lb; ++i) {
      if (B[i] != a0) continue;
      uint32_t j = 1;
      while (j < la && A[j] == B[i + j]) ++j;
      if (j == la) return true;
    }
  }
  return false;
}

// One walk of the record at `at` (member m): first CSR edge, cost, stack
// length and the key of (first edge, cost, label sequence bottom-up).
__device__ void walk(const RtArgs& a, uint32_t me, uint32_t at, uint32_t m, uint32_t* first,
                     uint32_t* cost, uint32_t* nst, uint64_t* key) {
  const uint32_t len = a.pool[at];
  const uint32_t* L = a.pool + (size_t)at + 2;
  uint32_t cur = me, c = 0, f = 0;
  uint64_t h = 0xcbf29ce484222325ULL;
  for (uint32_t x = 0; x < len; ++x) {
    const Hop s = hop(a, L[x], cur);
    c += s.met;
    cur = s.node;
    if (x == 0) f = s.edge;
    else h = fnv(h, (uint32_t)a.label[cur]);
  }
  uint32_t n = len ? len - 1 : 0u;
  const int32_t pre = prepend_of(a, m);
  if (pre != -1) {
    h = fnv(h, (uint32_t)pre);
    ++n;
  }
  *first = f;
  *cost = c;
  *nst = n;
  *key = mix64(fnv(fnv(h, n), (uint64_t)f | ((uint64_t)c << 32)));
}

// Exact equality of two candidates' next hops (first CSR edge, cost, label
// sequence): both records walked in step, the stacks compared bottom-up --
// element t is L(v_{2+t}) while the path lasts, then the prepend label.
__device__ bool same_hop(const RtArgs& a, uint32_t me, uint32_t at_e, uint32_t m_e, uint32_t at_c,
                         uint32_t m_c) {
  const uint32_t le = a.pool[at_e], lc = a.pool[at_c];
  const uint32_t* E = a.pool + (size_t)at_e + 2;
  const uint32_t* C = a.pool + (size_t)at_c + 2;
  const int32_t pe = prepend_of(a, m_e), pc = prepend_of(a, m_c);
  if (le == 0 || lc == 0) return false;
  const uint32_t n = le - 1 + (pe != -1);
  // (a link id is one CSR edge of me's row: equal first links, equal first edges)
  if (n != lc - 1 + (pc != -1) || E[0] != C[0]) return false;
  Hop s = hop(a, E[0], me);
  uint32_t ce = s.node, cc = s.node, cost_e = s.met, cost_c = s.met, xe = 1, xc = 1;
  for (uint32_t t = 0; t < n; ++t) {
    int32_t ve = pe, vc = pc;
    if (xe < le) {
      s = hop(a, E[xe++], ce);
      cost_e += s.met;
      ce = s.node;
      ve = a.label[ce];
    }
    if (xc < lc) {
      s = hop(a, C[xc++], cc);
      cost_c += s.met;
      cc = s.node;
      vc = a.label[cc];
    }
    if (ve != vc) return false;
  }
  return cost_e == cost_c;
}

// FILL = false: route r's next hops into rptr[r], its label words into
// lbase[r] (both scanned in place afterwards).  FILL = true: the same walk;
// survivor j of the route goes to rec / lptr[rptr[r] + j], its stack to lab at
// lbase[r] + the stack lengths of the survivors before it.
template <bool FILL>
__global__ __launch_bounds__(kRtThreads) void ksp2_routes_kernel(RtArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long r = (unsigned long long)blockIdx.x * kRtWaves + (threadIdx.x >> 6);
  if (r >= a.n_routes) return;  // (the whole wave)
  const uint32_t i = (uint32_t)(r / a.n_sets), p = (uint32_t)(r % a.n_sets);
  const uint32_t me = a.srcs[i];
  const uint32_t m0 = a.set_ptr[p], m1 = a.set_ptr[p + 1];
  const uint4* row = a.pairs + (size_t)i * a.N;
  const unsigned long long hop_base = FILL ? a.rptr[r] : 0ull;
  const unsigned long long word_base = FILL ? a.lbase[r] : 0ull;
  unsigned long long n_hops = 0, n_words = 0;  // of the chunks so far (wave-uniform)
  Cursor all(m0);
  for (uint32_t base = 0;; base += 64) {
    // ---- the chunk's candidates: number n to lane n ----
    uint32_t my_at = 0, my_m = 0, my_k = 0, n = 0;
    {
      uint32_t at, m, k;
      while (n < 64 && all.next(a, row, me, m0, m1, 1, &at, &m, &k)) {
        if (lane == n) {
          my_at = at;
          my_m = m;
          my_k = k;
        }
        ++n;
      }
    }
    if (n == 0) break;
    const bool have = lane < n;
    uint32_t first = 0, cost = 0, nst = 0;
    uint64_t key = 0;
    bool valid = have;
    if (have) {
      walk(a, me, my_at, my_m, &first, &cost, &nst, &key);
      if (my_k == 1) valid = !k2_dropped(a, row, me, m0, m1, my_at);
    }
    // ---- duplicates of candidates of earlier chunks ----
    bool dup = false;
    if (base && valid) {
      Cursor c(m0);
      uint32_t at_e, m_e, k_e;
      for (uint32_t idx = 0; idx < base && c.next(a, row, me, m0, m1, 1, &at_e, &m_e, &k_e); ++idx)
        if (same_hop(a, me, at_e, m_e, my_at, my_m) &&
            !(k_e == 1 && k2_dropped(a, row, me, m0, m1, at_e))) {
          dup = true;
          break;
        }
    }
    // ---- duplicates inside the chunk: key match, then the full compare ----
    for (uint32_t j = 0; j + 1 < n; ++j) {
      const uint32_t klo = __shfl((uint32_t)key, (int)j), khi = __shfl((uint32_t)(key >> 32), (int)j);
      const uint32_t at_j = __shfl(my_at, (int)j), m_j = __shfl(my_m, (int)j);
      const bool v_j = __shfl((uint32_t)valid, (int)j) != 0;
      if (lane > j && valid && !dup && v_j && (((uint64_t)khi << 32) | klo) == key &&
          same_hop(a, me, at_j, m_j, my_at, my_m))
        dup = true;
    }
    // ---- survivors: rank among them, offset of the stack ----
    const bool surv = valid && !dup;
    const unsigned long long mask = __ballot(surv);
    const uint32_t rank = __popcll(mask & ((1ull << lane) - 1ull));
    const uint32_t w = surv ? nst : 0u;
    uint32_t inc = w;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(inc, d);
      if (lane >= d) inc += y;
    }
    const uint32_t total = __shfl(inc, 63);
    if constexpr (FILL) {
      if (surv) {
        const unsigned long long h = hop_base + n_hops + rank;
        const unsigned long long lw = word_base + n_words + (inc - w);
        a.rec[h] = (unsigned long long)first | ((unsigned long long)cost << 32);
        a.lptr[h] = lw;
        const uint32_t len = a.pool[my_at];
        const uint32_t* L = a.pool + (size_t)my_at + 2;
        uint32_t cur = me;
        for (uint32_t x = 0; x < len; ++x) {
          cur = hop(a, L[x], cur).node;
          if (x) a.lab[lw + (nst - x)] = a.label[cur];  // element t = x - 1 from the bottom
        }
        const int32_t pre = prepend_of(a, my_m);
        if (pre != -1) a.lab[lw] = pre;
      }
    }
    n_hops += (unsigned long long)__popcll(mask);
    n_words += total;
    if (n < 64) break;
  }
  if (lane == 0) {
    if constexpr (FILL) {
      // the last route closes lptr with the total
      if (r + 1 == a.n_routes) a.lptr[a.rptr[a.n_routes]] = a.lbase[a.n_routes];
    } else {
      a.rptr[r] = n_hops;
      a.lbase[r] = n_words;
    }
  }
}

}  // namespace

extern "C" {

spf_status spf_ksp2_routes(spf_ksp2_plan* p, const spf_ksp2_pair* d_pairs, const uint32_t* d_pool,
                           const uint32_t* set_ptr, const uint32_t* set_nodes, uint32_t n_sets,
                           const int32_t* set_prepend, const int32_t* node_label, uint64_t* n_hops,
                           uint64_t* n_label_words, uint64_t* pool_bytes, double* kernel_ms) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_ksp2_routes: NULL plan");
  spf_ctx* c = p->ctx;
  Ksp2Routes& rt = p->rt;
  rt.valid = false;
  ++rt.gen;  // (a delta of the previous pools has no payload to gather any more)
  if (!d_pairs || !d_pool || !set_ptr || !node_label)
    return fail(c, SPF_E_INVALID, "spf_ksp2_routes: NULL argument");
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (p->epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  for (uint32_t s = 0; s < n_sets; ++s)
    if (set_ptr[s] > set_ptr[s + 1])
      return fail(c, SPF_E_INVALID, "spf_ksp2_routes: set_ptr not monotone at set %u", s);
  const uint32_t n_members = set_ptr[n_sets];
  if (n_members && !set_nodes) return fail(c, SPF_E_INVALID, "spf_ksp2_routes: NULL set_nodes");
  for (uint32_t k = set_ptr[0]; k < n_members; ++k)
    if (set_nodes[k] >= c->N)
      return fail(c, SPF_E_INVALID, "spf_ksp2_routes: set node %u out of range", set_nodes[k]);
  // a path has at most N - 1 links: every cost fits the record's 32 bits
  uint64_t max_abs = c->max_metric;
  if (c->n_neg)
    for (uint32_t u = 0; u < c->N; ++u)
      for (uint32_t e = c->row_ptr[u]; e < c->row_ptr[u + 1]; ++e)
        if (c->col[e] != u) max_abs = std::max<uint64_t>(max_abs, (uint64_t)std::llabs((long long)c->met[e]));
  if (max_abs * (uint64_t)(c->N - 1) >= (1ull << 32))
    return fail(c, SPF_E_UNSUPPORTED, "spf_ksp2_routes: max metric %llu x %u links may exceed a 32-bit cost",
                (unsigned long long)max_abs, c->N - 1);
  const uint64_t n_routes = (uint64_t)p->n_src * n_sets;
  const uint64_t blocks = (n_routes + kRtWaves - 1) / kRtWaves;
  if (blocks >= (1ull << 31)) return fail(c, SPF_E_INVALID, "spf_ksp2_routes: grid too large");

  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  std::vector<uint32_t> tab;  // (alive until the stream has synchronised)
  if (rt.links_epoch != c->epoch || !rt.d_links.p) {
    // both directed CSR edges of every link id (dead slots -- self-loops -- are no edges)
    rt.max_link = c->max_link;
    tab.assign(8ull * ((size_t)c->max_link + 1), 0u);
    for (uint32_t u = 0; u < c->N; ++u)
      for (uint32_t e = c->row_ptr[u]; e < c->row_ptr[u + 1]; ++e) {
        if (c->col[e] == u) continue;
        uint32_t* t = &tab[8ull * c->link[e]];
        if (e < c->rev[e]) {  // {edge, tail, head, metric} of the lower edge id
          t[0] = e;
          t[1] = u;
          t[2] = c->col[e];
          t[3] = (uint32_t)c->met[e];
        } else {  // {edge, metric} of its reverse
          t[4] = e;
          t[5] = (uint32_t)c->met[e];
        }
      }
    HIP_TRY(c, rt.d_links.upload(tab.data(), tab.size(), s));
    rt.links_epoch = c->epoch;
  }
  HIP_TRY(c, rt.d_set_ptr.upload(set_ptr, (size_t)n_sets + 1, s));
  HIP_TRY(c, rt.d_set_nodes.upload(set_nodes, n_members, s));
  if (set_prepend) HIP_TRY(c, rt.d_prepend.upload(set_prepend, n_members, s));
  HIP_TRY(c, rt.d_label.upload(node_label, c->N, s));
  HIP_TRY(c, rt.d_rptr.alloc(n_routes + 1));
  HIP_TRY(c, rt.d_lbase.alloc(n_routes + 1));
  HIP_TRY(c, rt.d_sums.alloc(std::max<uint64_t>(label_scan_tiles(n_routes), 1)));
  for (hipEvent_t& e : rt.ev)
    if (!e) HIP_TRY(c, hipEventCreate(&e));

  RtArgs a{reinterpret_cast<const uint4*>(d_pairs), d_pool, reinterpret_cast<const uint4*>(rt.d_links.p),
           rt.max_link, p->d_srcs.p, c->N, n_sets, n_routes, rt.d_set_ptr.p, rt.d_set_nodes.p,
           set_prepend ? rt.d_prepend.p : nullptr, rt.d_label.p, rt.d_rptr.p, rt.d_lbase.p, nullptr,
           nullptr, nullptr};
  const dim3 grid((uint32_t)blocks), block(kRtThreads);
  HIP_TRY(c, hipEventRecord(rt.ev[0], s));
  if (n_routes) {
    hipLaunchKernelGGL(ksp2_routes_kernel<false>, grid, block, 0, s, a);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipEventRecord(rt.ev[1], s));
  spf_status st = launch_label_scan(c, rt.d_rptr.p, n_routes, rt.d_sums.p, s);
  if (st != SPF_OK) return st;
  st = launch_label_scan(c, rt.d_lbase.p, n_routes, rt.d_sums.p, s);
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(rt.ev[2], s));
  uint64_t tot[2] = {0, 0};
  HIP_TRY(c, hipMemcpyAsync(&tot[0], rt.d_rptr.p + n_routes, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(&tot[1], rt.d_lbase.p + n_routes, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  HIP_TRY(c, rt.d_rec.alloc(tot[0]));
  HIP_TRY(c, rt.d_lptr.alloc(tot[0] + 1));
  HIP_TRY(c, rt.d_lab.alloc(tot[1]));
  a.rec = rt.d_rec.p;
  a.lptr = rt.d_lptr.p;
  a.lab = rt.d_lab.p;
  HIP_TRY(c, hipEventRecord(rt.ev[3], s));
  if (n_routes) {
    hipLaunchKernelGGL(ksp2_routes_kernel<true>, grid, block, 0, s, a);
    HIP_TRY(c, hipGetLastError());
  } else {
    HIP_TRY(c, hipMemsetAsync(rt.d_lptr.p, 0, 8, s));
  }
  HIP_TRY(c, hipEventRecord(rt.ev[4], s));
  HIP_TRY(c, hipStreamSynchronize(s));
  float ms[3] = {0, 0, 0};
  HIP_TRY(c, hipEventElapsedTime(&ms[0], rt.ev[0], rt.ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&ms[1], rt.ev[1], rt.ev[2]));
  HIP_TRY(c, hipEventElapsedTime(&ms[2], rt.ev[3], rt.ev[4]));
  for (int k = 0; k < 3; ++k) rt.ms[k] = ms[k];
  rt.n_sets = n_sets;
  rt.hops = tot[0];
  rt.words = tot[1];
  rt.valid = true;
  if (n_hops) *n_hops = tot[0];
  if (n_label_words) *n_label_words = tot[1];
  if (pool_bytes) *pool_bytes = 8 * tot[0] + 8 * (n_routes + 1) + 8 * (tot[0] + 1) + 4 * tot[1];
  if (kernel_ms) *kernel_ms = rt.ms[0] + rt.ms[1] + rt.ms[2];
  return SPF_OK;
}

spf_status spf_ksp2_routes_timing(const spf_ksp2_plan* p, double* ms) {
  if (!p || !ms) return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_ksp2_routes_timing: NULL argument");
  if (!p->rt.valid) return fail(p->ctx, SPF_E_STATE, "spf_ksp2_routes_timing: no routes (call spf_ksp2_routes)");
  std::copy(p->rt.ms, p->rt.ms + 3, ms);
  return SPF_OK;
}

spf_status spf_ksp2_route_db(spf_ksp2_plan* p, uint32_t i, uint64_t* rptr, uint64_t* rec,
                             uint64_t rec_cap, uint64_t* n_rec, uint64_t* lptr, int32_t* lab,
                             uint64_t lab_cap, uint64_t* n_lab) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_ksp2_route_db: NULL plan");
  spf_ctx* c = p->ctx;
  Ksp2Routes& rt = p->rt;
  if (!rt.valid) return fail(c, SPF_E_STATE, "spf_ksp2_route_db: no routes (call spf_ksp2_routes)");
  if (i >= p->n_src) return fail(c, SPF_E_INVALID, "spf_ksp2_route_db: no such source slot %u", i);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint32_t S = rt.n_sets;
  // the source's S + 1 offsets (the next source's first one, or the total, ends them)
  std::vector<uint64_t> h((size_t)S + 1);
  HIP_TRY(c, hipMemcpyAsync(h.data(), rt.d_rptr.p + (size_t)i * S, 8ull * (S + 1), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t cnt = h[S] - h[0];
  std::vector<uint64_t> lp(cnt + 1);
  HIP_TRY(c, hipMemcpyAsync(lp.data(), rt.d_lptr.p + h[0], 8ull * (cnt + 1), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint64_t words = lp[cnt] - lp[0];
  if (n_rec) *n_rec = cnt;
  if (n_lab) *n_lab = words;
  if ((rec || lptr) && rec_cap < cnt)
    return fail(c, SPF_E_NOMEM, "KSP2 route db of %llu next hops, room for %llu", (unsigned long long)cnt,
                (unsigned long long)rec_cap);
  if (lab && lab_cap < words)
    return fail(c, SPF_E_NOMEM, "KSP2 route db of %llu label words, room for %llu",
                (unsigned long long)words, (unsigned long long)lab_cap);
  if (rec && cnt) HIP_TRY(c, hipMemcpyAsync(rec, rt.d_rec.p + h[0], 8ull * cnt, hipMemcpyDeviceToHost, s));
  if (lab && words) HIP_TRY(c, hipMemcpyAsync(lab, rt.d_lab.p + lp[0], 4ull * words, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (rptr)
    for (uint32_t k = 0; k <= S; ++k) rptr[k] = h[k] - h[0];
  if (lptr)
    for (uint64_t k = 0; k <= cnt; ++k) lptr[k] = lp[k] - lp[0];
  return SPF_OK;
}

spf_status spf_ksp2_route_buffers(spf_ksp2_plan* p, const uint64_t** d_rptr, const uint64_t** d_rec,
                                  const uint64_t** d_lptr, const int32_t** d_lab, uint64_t* n_hops,
                                  uint64_t* n_label_words) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_ksp2_route_buffers: NULL plan");
  const Ksp2Routes& rt = p->rt;
  if (!rt.valid) return fail(p->ctx, SPF_E_STATE, "spf_ksp2_route_buffers: no routes (call spf_ksp2_routes)");
  if (d_rptr) *d_rptr = reinterpret_cast<const uint64_t*>(rt.d_rptr.p);
  if (d_rec) *d_rec = reinterpret_cast<const uint64_t*>(rt.d_rec.p);
  if (d_lptr) *d_lptr = reinterpret_cast<const uint64_t*>(rt.d_lptr.p);
  if (d_lab) *d_lab = rt.d_lab.p;
  if (n_hops) *n_hops = rt.hops;
  if (n_label_words) *n_label_words = rt.words;
  return SPF_OK;
}

}  // extern "C"
