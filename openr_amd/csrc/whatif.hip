// ============================================================================
//  whatif.hip -- what-if batches: the SPF of one source re-run for every
//  single-link failure of a list, reduced to a
//  per-failure digest.
//
//  Reference semantics per failure l: runSpf(src, true, {l})
//  (openr/decision/LinkState.cpp:808-882 with linksToIgnore = {l}, the
//  primitive getKthPaths uses at :776-779), compared with runSpf(src).
//
//  Exact incremental evaluation instead of one full Dijkstra per failure:
//    * l is "cold" when neither direction is a tight edge of the unfailed
//      shortest-path DAG (tail expanded, d(tail) + w = d(head)).  Removing a
//      link that no shortest path uses changes no distance, no pathLinks and
//      so no next hop: the digest is the unfailed one.
//    * l is "hot" when a -> b is tight (one direction at most: metrics are
//      positive).  Only D = the DAG descendants of b (b included) can change:
//      a node outside D has no tight path through a -> b, keeps its distance
//      and its tight predecessors, none of which is in D.  On D:
//        - distances: seeds from in-edges leaving nodes outside D (exact,
//          unchanged) and a label-correcting sweep inside D;
//        - next hops: nh(v) = union over tight expanded predecessors u of
//          ({v} if u = src else nh(u)) -- the reference's addNextHops rule
//          (:867-872) -- iterated to its fixed point (monotone union over a
//          DAG, so the least fixed point is the Dijkstra result);
//        - the digest delta is summed over D.
//  Teams: a wave per hot failure while |D| fits its scratch (4096 nodes),
//  the rest re-done by whole 1024-thread workgroups with room for all nodes.
//
//  Node failures (spf_whatif_plan_create_nodes) run the same repairs with the
//  failure kind as a compile-time parameter (failed / drain_x below):
//    * DOWN x = runSpf(src, true, linksFromNode(x)): D = the DAG descendants
//      of x, x included (dlist[0] = x); every edge with an end at x is failed,
//      so x gets no seed and no relaxation, stays at kInf and is counted and
//      listed as unreachable.  Cold when x is unreachable in the unfailed run.
//    * DRAIN x = runSpf(src) with x overloaded: D is the same set, and x sits
//      in it (dlist[0] = x) as a node that is reached but never a transit: its
//      tight predecessors are all outside D, so its seed is its unfailed
//      distance and its row its unfailed row -- it contributes nothing to the
//      digest and is never an entry -- while nothing is relaxed out of it and
//      it is nobody's predecessor.  Cold when x is unreachable, drained
//      already, or has no tight out-edge.
//
//  Link sets (spf_whatif_plan_create_sets, shared-risk groups) are the fourth
//  kind: failure i = runSpf(src, true, S_i) for a set S_i of links.  An edge is
//  failed when its link id is a member of S_i, and D = the DAG descendants of
//  several roots, the heads of every tight member (two members with one head
//  claim it once; a root below another root is found marked by the level
//  loop).  The argument above carries over: a node outside D has no tight path
//  through any failed link.  Cold when no member is tight (an empty set, down
//  or non-tight members only).  A single link is a set of one, DOWN x the set
//  linksFromNode(x).
//
//  Link metric changes (spf_whatif_plan_create_metrics: cost-out, undrain) are
//  the fifth kind: change i = (link l, m_lo, m_hi) is runSpf(src) on the graph
//  in which l's two directions weigh m_lo (smaller CSR id -> larger) and m_hi
//  (0 keeps a direction).  Nothing is failed: what changes is what an edge
//  WEIGHS (w_fwd / w_rev below substitute the two new weights wherever a weight
//  of l's two directed edges is read).  One direction at most can matter,
//  because metrics are positive: if u -> v is tight, or becomes useful
//  (d(u) + w' <= d(v)), then d(u) < d(v), and v -> u cannot reach u at or below
//  d(u) whatever it weighs.
//    * cold: l is down; both directions kept or equal to the current metric; a
//      raised direction that is not tight; a lowered u -> v with
//      d(u) + w' > d(v), or u unreachable, or u not expanded (drained, not src).
//    * raise of a tight u -> v: D = the DAG descendants of v, the link plan's D,
//      but the edge stays: it seeds v from u at w'.
//    * lower with d(u) + w' <= d(v): delta = d(v) - d(u) - w' >= 0 (0: a new
//      ECMP tie, distances stay, next hops grow).  No node improves by more
//      than delta.  D grows from v over edges x -> c with
//      d(x) + w(x, c) <= d(c) + delta (unfailed distances on both sides; c
//      reachable and not src, which never changes): a shortest new path from v
//      to a changed node runs through changed nodes only, and each of its edges
//      has slack <= delta.  The set is closed -- a node outside it keeps its
//      distance and its tight predecessors -- and the repair is exact for any
//      D whose complement is unchanged; unchanged nodes of D add nothing to
//      the digest and are no entries.  With delta = 0 the test is the tight
//      test: raises and lowers share one loop, delta a team-uniform scalar.
//  No change alters src's neighbour set or anyone's reachability.
//
//  Digest of a result (same definition in oracle/spf_oracle.cpp):
//    n_dist_changed, n_nh_changed (a node becoming unreachable counts in both)
//    hash = sum over reachable v of mix(mix(v + 1) + d(v)) ^ fnv(nh(v) words)
//  with nh(v) a bitset over the distinct up neighbours of src in the unfailed
//  graph (ascending id).
//
//  This unit holds what every plan kind shares on the host (plan_build, execute,
//  changes, the lists' scan) and the link kind with its classify kernel.  The
//  unfailed pass is whatif_base_kernel in grid_spf.hip (run_base hands it the
//  plan's buffers), the repairs are whatif_repair.h over the primitives of
//  grid_ops.h, their one launch path whatif_plan.h; node, set and metric plans
//  instantiate theirs in whatif_nodes.hip, whatif_sets.hip and
//  whatif_metrics.hip, a code object each.
// ============================================================================
#include "whatif_plan.h"

namespace {

// ---------------------------------------------------------------------------
//  classify failures: cold -> digest now, hot -> work list (failure, edge)
// ---------------------------------------------------------------------------
__global__ void classify_kernel(WiGraph g, const uint32_t* __restrict__ dist,
                                const unsigned long long* __restrict__ H,
                                const uint32_t* __restrict__ fails, uint32_t n_fail,
                                const uint32_t* __restrict__ link_edge,
                                const uint32_t* __restrict__ sub, uint32_t wave_cap,
                                spf_whatif_digest* out, uint2* hot, uint32_t* n_hot,
                                uint2* big, uint32_t* n_big) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_fail) return;
  const uint32_t e0 = link_edge[fails[f]];
  uint32_t tight = kInf;
  if (e0 != kInf) {
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t e = k ? g.rev[e0] : e0;
      const uint32_t a = g.col[g.rev[e]], b = g.col[e];  // a -> b
      if (g.ovl[a] && a != g.src) continue;
      if (dist[a] != kInf && dist[a] + g.wt[e] == dist[b]) tight = e;
    }
  }
  if (tight == kInf) {
    out[f] = spf_whatif_digest{0u, 0u, (uint64_t)*H};
  } else if (sub[g.col[tight]] > wave_cap) {  // |D| >= subtree: a workgroup's repair
    big[atomicAdd(n_big, 1u)] = make_uint2(f, tight);
  } else {
    hot[atomicAdd(n_hot, 1u)] = make_uint2(f, tight);
  }
}

// cptr[0 .. n] = exclusive scan of the failures' entry counts, cptr[n] the
// total: one workgroup, 8 counts per thread and tile, the per-thread sums
// scanned with the DPP wave scans (a sum < 2^35 as two words of 24 and 11
// bits: 64 of either stay below 2^32), u64 offsets.  Count t is cnt[t *
// STRIDE]: 1 for the lists' own arrays, 8 for the counts inside the impact
// summaries (spfi::whatif_scan).
constexpr uint32_t kListScanPer = 8;
static_assert(1024 * kListScanPer == spfi::kWhatifScanTile, "the tile the tests cross");
template <uint32_t STRIDE>
__global__ __launch_bounds__(1024) void whatif_scan_kernel(const uint32_t* __restrict__ cnt,
                                                           uint32_t n,
                                                           unsigned long long* __restrict__ cptr) {
  __shared__ unsigned long long s_wave[16];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint64_t t0 = 0; t0 < n; t0 += 1024ull * kListScanPer) {  // block-uniform
    const uint64_t b = t0 + (uint64_t)threadIdx.x * kListScanPer;
    uint32_t x[kListScanPer];
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kListScanPer; ++j) {
      x[j] = b + j < n ? cnt[(b + j) * STRIDE] : 0u;
      sum += x[j];
    }
    uint32_t tl = 0, th = 0;
    const uint32_t el = wave_excl_scan((uint32_t)sum & 0xFFFFFFu, &tl);
    const uint32_t eh = wave_excl_scan((uint32_t)(sum >> 24), &th);
    if (lane == 0) s_wave[wv] = tl + ((unsigned long long)th << 24);
    __syncthreads();
    unsigned long long run = carry + el + ((unsigned long long)eh << 24);
    for (uint32_t w = 0; w < 16; ++w) {
      const unsigned long long t = s_wave[w];
      if (w < wv) run += t;
      carry += t;
    }
#pragma unroll
    for (uint32_t j = 0; j < kListScanPer; ++j) {
      if (b + j < n) cptr[b + j] = run;
      run += x[j];
    }
    __syncthreads();  // s_wave is rewritten by the next tile
  }
  if (threadIdx.x == 0) cptr[n] = carry;
}

__global__ void base_digest_kernel(spf_whatif_digest* o, const unsigned long long* H) {
  *o = spf_whatif_digest{0u, 0u, (uint64_t)*H};
}

}  // namespace

namespace spfi {

hipError_t whatif_scan(const uint32_t* cnt, uint32_t stride, uint32_t n, unsigned long long* ptr,
                       hipStream_t s) {
  if (stride == 1) hipLaunchKernelGGL(whatif_scan_kernel<1>, dim3(1), dim3(1024), 0, s, cnt, n, ptr);
  else if (stride == 8) hipLaunchKernelGGL(whatif_scan_kernel<8>, dim3(1), dim3(1024), 0, s, cnt, n, ptr);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

void whatif_lists_view(spf_whatif_plan* p, WiListsView* v) {
  const spf_ctx* c = p->ctx;
  v->ctx = p->ctx;
  v->rt = &p->rt;
  v->imp[SPF_WHATIF_BY_NODE] = &p->imp_node;
  v->imp[SPF_WHATIF_BY_SET] = &p->imp_set;
  v->up = &p->up;
  v->kind = p->kind;
  v->exact = p->exact != nullptr;
  v->fails = p->d_fails.p;
  v->set_links = p->d_set_links.p;
  v->met = p->d_met.p;
  v->nbr_bit = p->d_nbr_bit.p;
  v->changes = &p->lists;
  v->no_nbr = p->src + 1 < c->nb_ptr.size() && c->nb_ptr[p->src + 1] == c->nb_ptr[p->src];
  v->epoch = p->epoch;
  v->src = p->src;
  v->n_fail = p->n_fail;
  v->W = p->W;
  v->base_d32 = p->exact ? nullptr : p->d_dist.p;
  v->base_d64 = p->exact ? p->exact->base_d.p : nullptr;
  v->base_nh = p->exact ? p->exact->base_nh.p : p->d_nhb.p;
}
}  // namespace spfi

namespace {

// SPF_WHATIF_PROF: unset 0 (production instances), "global" 2 (per-event
// global read-modify-writes), anything else 1 (register counters)
int whatif_prof_mode() {
  const char* e = std::getenv("SPF_WHATIF_PROF");
  return !e ? 0 : (std::strcmp(e, "global") == 0 ? 2 : 1);
}

// 1. unfailed SPF, next hops, hash: one grid-resident launch (grid_spf.hip)
spf_status run_base(spf_whatif_plan* p, hipStream_t s) {
  BaseBufs b{p->src, p->W, p->d_nbr_bit.p, p->d_dist.p, p->d_q.p, p->d_q2.p, p->d_bm.p, p->d_ctr.p,
             p->d_bar.p, p->d_nhb.p, p->d_lvl.p, p->d_order.p, p->d_misc.p, p->d_H.p, p->d_parent.p,
             p->d_sub.p, nullptr, nullptr};
  if (p->d_prof.p) {
    b.prof = p->d_prof.p + 16ull * p->big_teams;
    b.lprof = p->d_prof.p + 16ull * (p->big_teams + 1 + p->wave_teams);
  }
  return launch_base(p->ctx, b, s);
}

// Link plans: work items (failure, tight edge), sorted by the parent subtree
// of the edge's head; the only kind with profiled instances.
struct LinkKind {
  static constexpr int kKind = kLink;
  static constexpr bool kProfiled = true;
  static constexpr const char* kDebugName = "";
  static constexpr const char* kPlanName = "a link plan (spf_whatif_plan_links)";
  static std::tuple<> table(const spf_whatif_plan*) { return {}; }
  static void classify(spf_whatif_plan* p, const WiGraph& g, spf_whatif_digest* d_out, hipStream_t s) {
    hipLaunchKernelGGL(classify_kernel, dim3((p->n_fail + 255) / 256), dim3(256), 0, s, g,
                       p->d_dist.p, p->d_H.p, p->d_fails.p, p->n_fail, p->d_link_edge.p,
                       p->d_sub.p, p->classify_cap, d_out, p->d_hot.p, p->d_cnt.p, p->d_big0.p,
                       p->d_cnt.p + 3);
  }
  using SortKey = KeySubOfHead;
  static SortKey sort_key(const spf_whatif_plan* p) { return {p->d_sub.p, p->ctx->d_col.p}; }
};

}  // namespace

namespace spfi {

const WiKindOps kLinkOps = kind_ops_of<LinkKind>();

const WiKindOps& kind_ops(uint32_t kind) {
  static const WiKindOps* const ops[] = {&kLinkOps, &kDownOps, &kDrainOps, &kSetOps, &kMetricOps};
  static_assert(kLink == 0 && sizeof ops / sizeof *ops == kMetric + 1, "indexed by the plan's kind");
  assert(kind <= (uint32_t)kMetric);  // (a plan's kind is set by its create call)
  return *ops[kind];
}

spf_status create_prologue(spf_ctx* c, spf_whatif_plan** out, uint32_t src, const char* who) {
  if (!c || !out) return fail(c, SPF_E_INVALID, "%s: NULL argument", who);
  *out = nullptr;
  if (!c->loaded) return fail(c, SPF_E_STATE, "no graph loaded");
  if (src >= c->N) return fail(c, SPF_E_INVALID, "source %u out of range", src);
  return SPF_OK;
}

std::unique_ptr<spf_whatif_plan> new_plan(spf_ctx* c, uint32_t src, uint32_t kind, uint32_t n_fail) {
  auto p = std::make_unique<spf_whatif_plan>();
  p->ctx = c;
  p->src = src;
  p->kind = kind;
  p->n_fail = n_fail;
  return p;
}

// Up links only (a dead slot is a self-loop).  The edge is the first met in
// row order, so the one out of the endpoint with the smaller CSR id: a metric
// plan names a link's two directions by it (m_lo, m_hi).
std::vector<uint32_t> link_edges(const spf_ctx* c) {
  std::vector<uint32_t> link_edge((size_t)c->max_link + 1, kInf);
  for (uint32_t u = 0; u < c->N; ++u)
    for (uint32_t e = c->row_ptr[u]; e < c->row_ptr[u + 1]; ++e)
      if (c->col[e] != u && link_edge[c->link[e]] == kInf) link_edge[c->link[e]] = e;
  return link_edge;
}

// The part of plan creation that every kind shares, from the
// source's neighbour bits to the teams' scratch: p holds ctx, src, kind and
// n_fail, `fails` its list (link ids with `link_edge`, node ids without; a set
// plan's set_ptr with `link_edge`, its members uploaded by the caller).
spf_status plan_build(spf_ctx* c, std::unique_ptr<spf_whatif_plan>& p,
                      const std::vector<uint32_t>& fails, const std::vector<uint32_t>* link_edge,
                      spf_whatif_plan** out) {
  const uint32_t N = c->N, src = p->src;
  const WiKindOps& ops = kind_ops(p->kind);
  p->prof_mode = p->kind ? 0 : whatif_prof_mode();  // only link plans have profiled instances
  // bit of each distinct up neighbour of src
  std::vector<uint32_t> nbr_bit(N, kInf);
  const uint32_t k = c->nb_ptr[src + 1] - c->nb_ptr[src];
  for (uint32_t j = 0; j < k; ++j) nbr_bit[c->nb_id[c->nb_ptr[src] + j]] = j;
  p->W = std::max<uint32_t>(1, (k + 31) / 32);
  {  // wave teams: 16 per CU within the scratch budget (failures on the
     // 1M-link graph, r02_v75 with 8 GB: 12: 17.9 ms, 16: 16.4, 20: 20.2,
     // 24: 19.6; r02_v30 before the lane-read / DPP repairs: 12 best)
     // (SPF_WHATIF_WAVES=<per CU>, a multiple of 4: A/B)
    const char* e = std::getenv("SPF_WHATIF_WAVES");
    const size_t per_cu = e ? std::max(4, atoi(e) & ~3) : 16;
    if (const char* ec = std::getenv("SPF_WHATIF_WAVECAP")) p->wave_cap = std::max(64, atoi(ec));
    p->classify_cap = p->wave_cap;
    if (const char* ec = std::getenv("SPF_WHATIF_CLASSIFY")) p->classify_cap = std::max(1, atoi(ec));
    const size_t cap = p->wave_cap;
    const size_t per_team = 4ull * (N + cap * (4ull + p->W) + cap + 1);
    const size_t fit = std::max<size_t>(4, kWaveScratch / per_team) & ~size_t(3);
    p->wave_teams = (uint32_t)std::min<size_t>(per_cu * c->n_cu, fit);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, p->d_fails.upload(fails.data(), fails.size(), c->stream));
  if (link_edge) HIP_TRY(c, p->d_link_edge.upload(link_edge->data(), link_edge->size(), c->stream));
  HIP_TRY(c, p->d_nbr_bit.upload(nbr_bit.data(), N, c->stream));
  HIP_TRY(c, p->d_dist.alloc(N));
  HIP_TRY(c, p->d_q.alloc(N));
  HIP_TRY(c, p->d_q2.alloc(N));
  HIP_TRY(c, p->d_bm.alloc((N + 31) / 32));
  HIP_TRY(c, p->d_nhb.alloc((size_t)N * p->W));
  HIP_TRY(c, p->d_ctr.alloc(4));
  HIP_TRY(c, p->d_bar.alloc(kGridBarWords));
  HIP_TRY(c, p->d_lvl.alloc(kLevelCap + 1));
  HIP_TRY(c, p->d_order.alloc(N));
  HIP_TRY(c, p->d_misc.alloc(8));
  HIP_TRY(c, p->d_H.alloc(1));
  HIP_TRY(c, p->d_hot.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_big.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_big0.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_big1.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_parent.alloc(N));
  HIP_TRY(c, p->d_sub.alloc(N));
  if (!c->side) {  // the classified big failures' workgroup teams run here
    HIP_TRY(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->side_fork, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->side_join, hipEventDisableTiming));
  }
  HIP_TRY(c, p->d_cnt.alloc(8));
  {  // workgroup teams: one per CU, two sets (b_*, c_*) within the scratch budget
    const size_t per_team = 4ull * ((size_t)N * (6 + p->W) + 1);
    p->big_teams = (uint32_t)std::max<size_t>(4, std::min<size_t>(c->n_cu, kBigScratch / 2 / per_team));
  }
  const size_t bt = p->big_teams;
  {  // group teams over the concurrent (c_*) scratch sets: G workgroups each,
     // n_cu / G teams (a multiple of 8: members share an XCD), no more teams
     // than scratch sets (SPF_WHATIF_GROUP=1: one-workgroup teams, A/B).
     // G = 8 by default: ba_whatif's failures took 9.3 ms at G = 8 against
     // 10.2 at 4 and 14.8 at 16 (profiles/r05_whatif/flat)
    const char* e = std::getenv("SPF_WHATIF_GROUP");
    uint32_t G = e ? (uint32_t)atoi(e) : 8u;
    if (G > 1) {
      while (G <= 16 && (c->n_cu / G > bt || (c->n_cu / G) % 8)) G *= 2;
      if (G <= 16 && c->n_cu % (8 * G) == 0 && c->n_cu / G >= 8) {
        p->group = G;
        p->group_teams = c->n_cu / G;
        HIP_TRY(c, p->d_ctl.alloc(sizeof(TeamCtl) * p->group_teams));
      }
    }
  }
  if (p->group) {
    // The group teams' members must all be resident while the wave teams'
    // blocks hold their CUs (launched beside them on the side stream; a
    // member that cannot be placed stalls its team at every barrier).  Per
    // SIMD: the wave teams' waves (one per 256-thread block) and the group
    // workgroup's 2 waves share 512 VGPRs (granule 8).  Fewer wave teams per
    // CU until both fit.  (Round 4's stamp pointer in the wave kernel --
    // 75 -> 80+ VGPRs at 4 waves per SIMD beside 2 x 88 -- broke this sum.)
    // Every kind launches its own instances: the sum is made with their
    // registers (kind_regs).
    int rw = 0, rg = 0;
    HIP_TRY(c, ops.regs(p.get(), rw, rg));
    const auto gran = [](int r) { return (uint32_t)((std::max(r, 1) + 7) & ~7); };
    const uint32_t per_simd_group = kGroupWg / 64 / 4;
    const uint32_t vw = gran(rw), vg = gran(rg);
    uint32_t per_simd_wave = (p->wave_teams + 4 * c->n_cu - 1) / (4 * c->n_cu);
    while (per_simd_wave > 1 && per_simd_wave * vw + per_simd_group * vg > 512) --per_simd_wave;
    p->wave_teams = std::min(p->wave_teams, per_simd_wave * 4 * c->n_cu);
    if (std::getenv("SPF_WHATIF_DEBUG"))
      std::fprintf(stderr, "whatif%s: wave kernel %d VGPRs, group<%u> %d VGPRs: %u wave teams (%u per SIMD)\n",
                   ops.debug_name, rw, p->group, rg, p->wave_teams, per_simd_wave);
  }
  const size_t wt = p->wave_teams;
  while ((1u << p->tab_log2) < 4 * p->wave_cap) ++p->tab_log2;
  {  // WiGraph::ed from the context's host CSR (the plan lives within one graph epoch)
    std::vector<uint4> ed(std::max<uint32_t>(c->E, 1));
    for (uint32_t e = 0; e < c->E; ++e) ed[e] = make_uint4(c->col[e], c->wt[e], c->link[e], c->wt[c->rev[e]]);
    HIP_TRY(c, p->d_ed.upload(ed.data(), ed.size(), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (ed is freed on return)
  }
  HIP_TRY(c, p->w_tab.alloc(wt << p->tab_log2));
  HIP_TRY(c, p->w_dlist.alloc(wt * p->wave_cap));
  HIP_TRY(c, p->w_dnew.alloc(wt * p->wave_cap));
  HIP_TRY(c, p->w_nhn.alloc(wt * p->wave_cap * p->W));
  HIP_TRY(c, p->w_lvl.alloc(wt * (p->wave_cap + 1)));
  HIP_TRY(c, p->w_ord.alloc(wt * 2 * p->wave_cap));
  HIP_TRY(c, p->b_mark.alloc(bt * N));
  HIP_TRY(c, p->b_dlist.alloc(bt * N));
  HIP_TRY(c, p->b_dnew.alloc(bt * N));
  HIP_TRY(c, p->b_nhn.alloc(bt * N * p->W));
  HIP_TRY(c, p->b_lvl.alloc(bt * (N + 1)));
  HIP_TRY(c, p->b_ord.alloc(bt * 2 * N));
  HIP_TRY(c, p->c_mark.alloc(bt * N));
  HIP_TRY(c, p->c_dlist.alloc(bt * N));
  HIP_TRY(c, p->c_dnew.alloc(bt * N));
  HIP_TRY(c, p->c_nhn.alloc(bt * N * p->W));
  HIP_TRY(c, p->c_lvl.alloc(bt * (N + 1)));
  HIP_TRY(c, p->c_ord.alloc(bt * 2 * N));
  HIP_TRY(c, hipMemsetAsync(p->c_mark.p, 0xFF, bt * N * 4, c->stream));
  // marks start (and are always left) at kInf
  HIP_TRY(c, hipMemsetAsync(p->w_tab.p, 0xFF, (wt << p->tab_log2) * 8, c->stream));
  HIP_TRY(c, hipMemsetAsync(p->b_mark.p, 0xFF, bt * N * 4, c->stream));
  if (p->prof_mode) {  // [bt teams][base][wave teams] x 16 (row bounds checked in the kernels)
    const size_t slots = 16 * (bt + 1 + p->wave_teams) + 128;  // + the base's per-level clocks
    HIP_TRY(c, p->d_prof.alloc(slots));
    HIP_TRY(c, hipMemsetAsync(p->d_prof.p, 0, slots * 8, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  p->epoch = c->epoch;
  *out = p.release();
  return SPF_OK;
}

}  // namespace spfi

extern "C" {

spf_status spf_whatif_plan_create(spf_ctx* c, uint32_t src, const uint32_t* fail_links,
                                  uint32_t n_fail, spf_whatif_plan** out) {
  if (const spf_status st = create_prologue(c, out, src, "spf_whatif_plan_create"); st != SPF_OK)
    return st;
  const std::vector<uint32_t> link_edge = link_edges(c);
  std::vector<uint32_t> fails;
  if (fail_links) {
    fails.assign(fail_links, fail_links + n_fail);
    for (uint32_t l : fails)
      if (l > c->max_link || link_edge[l] == kInf)
        return fail(c, SPF_E_INVALID, "link %u is not an up link of the graph", l);
  } else {  // every up link, ascending id
    for (uint32_t l = 0; l <= c->max_link && c->E; ++l)
      if (link_edge[l] != kInf) fails.push_back(l);
  }
  auto p = new_plan(c, src, (uint32_t)kLink, (uint32_t)fails.size());
  if (c->nonpos || c->needs64) {
    // zero / negative metrics, u64 labels: the exact kernel replays
    // runSpf(src, true, {l}) for every failure touching a pathLink
    HIP_TRY(c, hipSetDevice(c->device));
    p->exact = std::make_unique<spfi::ExactWhatIf>();
    const spf_status st = exact_whatif_prepare(c, p->exact.get(), src, fails, link_edge);
    if (st != SPF_OK) return st;
    if (!fails.empty()) HIP_TRY(c, p->d_fails.upload(fails.data(), fails.size(), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    p->W = p->exact->W;
    p->epoch = c->epoch;
    *out = p.release();
    return SPF_OK;
  }
  return plan_build(c, p, fails, &link_edge, out);
}

void spf_whatif_plan_destroy(spf_whatif_plan* p) { delete p; }
uint32_t spf_whatif_plan_failures(const spf_whatif_plan* p) { return p ? p->n_fail : 0; }

spf_status spf_whatif_plan_links(const spf_whatif_plan* p, uint32_t* links) {
  if (!p || !links) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  if (p->kind) return fail(c, SPF_E_STATE, "spf_whatif_plan_links: %s", kind_ops(p->kind).plan_name);
  HIP_TRY(c, hipMemcpy(links, p->d_fails.p, 4ull * p->n_fail, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status spf_whatif_plan_kind(const spf_whatif_plan* p, uint32_t* kind) {
  if (!p || !kind) return SPF_E_INVALID;
  *kind = p->kind;
  return SPF_OK;
}

spf_status spf_whatif_execute(spf_whatif_plan* p, spf_whatif_digest* d_out,
                              spf_whatif_digest* d_base, void* stream) {
  if (!p || !d_out) return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_whatif_execute: NULL");
  spf_ctx* c = p->ctx;
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (p->epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  p->last = s;
  hipEvent_t* ev = nullptr;
  if (p->timing_cap) {
    ev = &p->ev[3 * (p->timing_n % p->timing_cap)];
    ++p->timing_n;
    HIP_TRY(c, hipEventRecord(ev[0], s));
  }
  if (p->exact) {
    const spf_status st = exact_whatif_launch(c, p->exact.get(), d_out, d_base, s, ev ? ev[1] : nullptr);
    if (st != SPF_OK) return st;
    if (ev) HIP_TRY(c, hipEventRecord(ev[2], s));
    c->solves += 1ull + p->n_fail;
    return SPF_OK;
  }
  if (const spf_status st = run_base(p, s); st != SPF_OK) return st;
  if (ev) HIP_TRY(c, hipEventRecord(ev[1], s));
  if (const spf_status st = kind_ops(p->kind).run(p, d_out, s, nullptr); st != SPF_OK) return st;
  if (p->d_prof.p) {  // diagnostics: phase ticks (100 MHz) per team, accumulated over repairs
    const size_t bt = p->big_teams, wt = p->wave_teams;
    std::vector<unsigned long long> h(16ull * (bt + 1 + wt) + 128);
    HIP_TRY(c, hipMemcpyAsync(h.data(), p->d_prof.p, h.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    auto line = [&](const char* who, const unsigned long long* r) {
      std::fprintf(stderr, "whatif %s repairs=%llu sum|D|=%llu max|D|=%llu dial_levels=%llu gave_up=%llu "
                   "bfs=%llu seeds=%llu dial=%llu fallback=%llu digest=%llu (x10ns)\n", who, r[0], r[8],
                   r[10], r[9], r[11], r[1], r[2], r[3], r[4], r[5]);
    };
    for (size_t t = 0; t < bt; ++t) {
      const unsigned long long* r = &h[16 * t];
      if (!r[0]) continue;
      char who[32];
      std::snprintf(who, sizeof who, "team %zu", t);
      line(who, r);
    }
    std::vector<unsigned long long> sum(16, 0);  // the wave teams, summed
    unsigned long long busiest = 0;
    for (size_t t = 0; t < wt; ++t) {
      const unsigned long long* r = &h[16 * (bt + 1 + t)];
      for (int k = 0; k < 16; ++k) sum[k] = k == 10 ? std::max(sum[k], r[k]) : sum[k] + r[k];
      busiest = std::max(busiest, r[1] + r[2] + r[3] + r[4] + r[5]);
    }
    line("wave-teams(sum)", sum.data());
    std::fprintf(stderr, "whatif wave teams %zu, busiest team %llu ticks (x10ns)\n", wt, busiest);
    const unsigned long long* r = &h[16 * bt];
    std::fprintf(stderr, "whatif base sssp=%llu nh=%llu (of which subtree sizes %llu) hash=%llu (x10ns) maxd=%llu levels=%llu W=%u\n",
                 r[1] - r[0], r[2] - r[1], r[6] ? r[2] - r[6] : 0ull, r[3] - r[2], r[4], r[5], p->W);
    const unsigned long long* lv = &h[16 * (bt + 1 + wt)];
    unsigned long long prev = 0;
    std::string line2 = "whatif base levels (distance:nodes:ticks)";
    for (int d = 1; d < 64; ++d) {
      if (!lv[2 * d]) continue;
      const unsigned long long t0 = prev ? prev : lv[2 * d];
      line2 += " " + std::to_string(d) + ":" + std::to_string(lv[2 * d + 1]) + ":" +
               std::to_string(prev ? lv[2 * d] - t0 : 0ull);
      prev = lv[2 * d];
    }
    std::fprintf(stderr, "%s\n", line2.c_str());
  }
  if (d_base) {
    // the unfailed digest: nothing changed, hash = H
    hipLaunchKernelGGL(base_digest_kernel, dim3(1), dim3(1), 0, s, d_base, p->d_H.p);
    HIP_TRY(c, hipGetLastError());
  }
  if (ev) HIP_TRY(c, hipEventRecord(ev[2], s));
  c->solves += 1ull + p->n_fail;
  return SPF_OK;
}

spf_status spf_whatif_changes(spf_whatif_plan* p, spf_whatif_digest* d_out, spf_whatif_digest* d_base,
                              uint64_t* n_entries, uint64_t* pool_bytes, double* kernel_ms,
                              void* stream) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_whatif_changes: NULL plan");
  spf_ctx* c = p->ctx;
  WiPool& L = p->lists;
  L.valid = false;             // after a failed call the plan holds no lists
  p->rt.pool.valid = false;    // ... and the route lists were built from the old ones
  p->imp_node.pool.valid = p->imp_set.pool.valid = false;  // ... as were the transpositions
  p->up.ent.valid = p->up.rec.valid = false;                // ... and the route updates
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (p->epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const uint32_t nf = p->n_fail;
  HIP_TRY(c, p->l_cnt.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, L.ptr.alloc((size_t)nf + 1));
  if (!d_out) {
    HIP_TRY(c, p->l_dig.alloc(std::max<uint32_t>(1, nf)));
    d_out = p->l_dig.p;
  }
  for (hipEvent_t& e : p->l_ev)
    if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  p->last = s;
  WiEmit em;
  em.cnt = p->l_cnt.p;
  em.W = p->W;
  em.fault = c->d_fault.p;
  // one pass over the failures with the EMIT instances (count, then fill)
  auto pass = [&](bool first) -> spf_status {
    if (p->exact)
      return exact_whatif_launch(c, p->exact.get(), d_out, first ? d_base : nullptr, s, nullptr, &em,
                                 first);
    return kind_ops(p->kind).run(p, d_out, s, &em);
  };
  if (!p->exact)
    if (const spf_status st = run_base(p, s); st != SPF_OK) return st;
  // count: cnt[f] = failure f's entries (0 for cold ones: the memset)
  HIP_TRY(c, hipMemsetAsync(p->l_cnt.p, 0, 4ull * std::max<uint32_t>(1, nf), s));
  HIP_TRY(c, hipEventRecord(p->l_ev[0], s));
  if (const spf_status st = pass(true); st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(p->l_ev[1], s));
  HIP_TRY(c, whatif_scan(p->l_cnt.p, 1, nf, L.ptr.p, s));
  HIP_TRY(c, hipEventRecord(p->l_ev[2], s));
  // the pool is sized from the scan's total
  unsigned long long total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, L.ptr.p + nf, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  if (const spf_status st = pool_size(c, &L, total, p->W, "spf_whatif_changes"); st != SPF_OK) return st;
  // fill: the repairs again, entries to cptr[f] + k
  em.cptr = L.ptr.p;
  em.cnode = L.key.p;
  em.cdist = L.val.p;
  em.cnh = L.rows.p;
  if (const spf_status st = pass(false); st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(p->l_ev[3], s));
  if (d_base && !p->exact) {
    hipLaunchKernelGGL(base_digest_kernel, dim3(1), dim3(1), 0, s, d_base, p->d_H.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  for (int k = 0; k < 3; ++k) HIP_TRY(c, hipEventElapsedTime(&p->l_ms[k], p->l_ev[k], p->l_ev[k + 1]));
  L.n_owners = nf;
  L.total = total;
  L.valid = true;
  c->solves += 1ull + nf;
  if (n_entries) *n_entries = total;
  if (pool_bytes) *pool_bytes = spfi::pool_bytes(L);
  if (kernel_ms) *kernel_ms = (double)p->l_ms[0] + p->l_ms[1] + p->l_ms[2];
  return SPF_OK;
}

spf_status spf_whatif_changes_timing(const spf_whatif_plan* p, double* ms) {
  if (!p || !ms) return SPF_E_INVALID;
  WiListsView v;
  if (const spf_status st = pool_held(const_cast<spf_whatif_plan*>(p), kPoolChanges,
                                      "spf_whatif_changes_timing", &v); st != SPF_OK)
    return st;
  for (int k = 0; k < 3; ++k) ms[k] = p->l_ms[k];
  return SPF_OK;
}

spf_status spf_whatif_changes_buffers(spf_whatif_plan* p, const uint64_t** d_ptr, const uint32_t** d_node,
                                      const uint64_t** d_dist, const uint32_t** d_nh, uint32_t* W,
                                      uint64_t* n_entries) {
  return pool_buffers(p, kPoolChanges, "spf_whatif_changes_buffers", d_ptr, d_node, d_dist, d_nh, nullptr,
                      W, n_entries);
}

spf_status spf_whatif_changes_read(spf_whatif_plan* p, uint64_t* ptr, uint32_t* node, uint64_t* dist,
                                   uint32_t* nh) {
  return pool_read(p, kPoolChanges, "spf_whatif_changes_read", ptr, node, dist, nh);
}

spf_status spf_whatif_changes_db(spf_whatif_plan* p, uint32_t i, uint32_t* node, uint64_t* dist,
                                 uint32_t* nh, uint64_t cap, uint64_t* n) {
  return pool_db(p, kPoolChanges, "spf_whatif_changes_db", i, node, dist, nh, cap, n);
}

spf_status spf_whatif_base(spf_whatif_plan* p, uint64_t* dist, uint32_t* nh, uint32_t* W) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_whatif_base: NULL plan");
  spf_ctx* c = p->ctx;
  if (!p->last) return fail(c, SPF_E_STATE, "spf_whatif_base: no execute yet");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(p->last));
  const size_t N = c->N, Wp = p->W;
  if (W) *W = p->W;
  std::vector<uint64_t> d(N);
  if (p->exact) {
    HIP_TRY(c, hipMemcpy(d.data(), p->exact->base_d.p, 8 * N, hipMemcpyDeviceToHost));
  } else {
    std::vector<uint32_t> d32(N);
    HIP_TRY(c, hipMemcpy(d32.data(), p->d_dist.p, 4 * N, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < N; ++v) d[v] = d32[v] == kInf ? ~0ull : d32[v];
  }
  if (dist) std::memcpy(dist, d.data(), 8 * N);
  if (nh) {
    // rows of W words in both plans (the exact plan's Wmax is its W); an
    // unreachable node's row, and a source's without neighbours, is zero
    const uint32_t* rows = p->exact ? p->exact->base_nh.p : p->d_nhb.p;
    HIP_TRY(c, hipMemcpy(nh, rows, 4 * N * Wp, hipMemcpyDeviceToHost));
    const bool no_nbr = c->nb_ptr[p->src + 1] == c->nb_ptr[p->src];
    for (size_t v = 0; v < N; ++v)
      if (d[v] == ~0ull || no_nbr) std::memset(nh + v * Wp, 0, 4 * Wp);
  }
  return SPF_OK;
}

spf_status spf_whatif_stats(spf_whatif_plan* p, uint32_t* n_hot, uint32_t* n_big) {
  if (!p) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  uint32_t cnt[4] = {0, 0, 0, 0};
  if (!p->last) return fail(c, SPF_E_STATE, "spf_whatif_stats: no execute yet");
  if (p->exact) {  // every failure is a re-run on the exact kernel (cold ones skipped inside)
    HIP_TRY(c, hipStreamSynchronize(p->last));
    if (n_hot) *n_hot = p->n_fail;
    if (n_big) *n_big = 0;
    return SPF_OK;
  }
  // the counters are written on the execute stream (non-blocking, so the
  // null stream does not order after it): copy on that stream and wait
  HIP_TRY(c, hipMemcpyAsync(cnt, p->d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, p->last));
  HIP_TRY(c, hipStreamSynchronize(p->last));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  if (n_hot) *n_hot = cnt[0] + cnt[3];  // wave list + classified big
  if (n_big) *n_big = cnt[2] + cnt[3];  // wave overflow + classified big
  return SPF_OK;
}

spf_status spf_whatif_enable_timing(spf_whatif_plan* p, uint32_t max_executes) {
  if (!p) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
  p->ev.assign(3ull * max_executes, nullptr);
  // timing only: no system-scope fence (its L2 writeback + invalidate cost
  // ~5 us per event and left the next kernel a cold L2)
  for (auto& e : p->ev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  p->timing_cap = max_executes;
  p->timing_n = 0;
  return SPF_OK;
}

spf_status spf_whatif_timing(spf_whatif_plan* p, double* base_ms, double* fail_ms, uint32_t* n) {
  if (!p || !p->timing_cap) return SPF_E_STATE;
  spf_ctx* c = p->ctx;
  const uint32_t cnt = std::min(p->timing_n, p->timing_cap);
  double a = 0, b = 0;
  for (uint32_t i = 0; i < cnt; ++i) {
    float t0 = 0, t1 = 0;
    HIP_TRY(c, hipEventSynchronize(p->ev[3 * i + 2]));
    HIP_TRY(c, hipEventElapsedTime(&t0, p->ev[3 * i], p->ev[3 * i + 1]));
    HIP_TRY(c, hipEventElapsedTime(&t1, p->ev[3 * i + 1], p->ev[3 * i + 2]));
    a += t0;
    b += t1;
  }
  if (base_ms) *base_ms = a;
  if (fail_ms) *fail_ms = b;
  if (n) *n = cnt;
  p->timing_n = 0;
  return SPF_OK;
}

spf_status spf_whatif_solve(spf_ctx* c, uint32_t src, const uint32_t* fail_links,
                            uint32_t n_fail, spf_whatif_digest* out, spf_whatif_digest* base) {
  if (!c || !out) return fail(c, SPF_E_INVALID, "spf_whatif_solve: NULL argument");
  spf_whatif_plan* raw = nullptr;
  spf_status st = spf_whatif_plan_create(c, src, fail_links, n_fail, &raw);
  if (st != SPF_OK) return st;
  std::unique_ptr<spf_whatif_plan> p(raw);
  DevBuf<spf_whatif_digest> d_out, d_base;
  HIP_TRY(c, d_out.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, d_base.alloc(1));
  st = spf_whatif_execute(p.get(), d_out.p, d_base.p, c->stream);
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipMemcpyAsync(out, d_out.p, sizeof(spf_whatif_digest) * p->n_fail,
                            hipMemcpyDeviceToHost, c->stream));
  if (base)
    HIP_TRY(c, hipMemcpyAsync(base, d_base.p, sizeof(spf_whatif_digest), hipMemcpyDeviceToHost,
                              c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return spf_device_check(c);
}

}  // extern "C"
