// ============================================================================
//  whatif_plan.h -- the host side every what-if plan kind shares: the plan,
//  what whatif.hip builds and launches for all of them, and the one launch
//  path of a plan's failures, run_failures<K>, over a kind description K.
//  Included by the kinds' units only (whatif.hip, whatif_nodes.hip,
//  whatif_sets.hip, whatif_metrics.hip); whatif_routes.hip and
//  whatif_impact.hip read a plan through whatif_lists_view.
// ============================================================================
#ifndef OPENR_AMD_WHATIF_PLAN_H
#define OPENR_AMD_WHATIF_PLAN_H

#include "whatif_repair.h"

#include <algorithm>
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <tuple>

struct spf_whatif_plan {
  spf_ctx* ctx = nullptr;
  uint32_t src = 0, n_fail = 0, W = 0, wave_teams = 0;
  // 0: d_fails holds link ids; SPF_WHATIF_NODE_*: node ids; SPF_WHATIF_LINK_SET:
  // set_ptr [n_fail + 1], the members in d_set_links (canonical: each set
  // ascending, duplicates removed) and d_link_edge for every link id
  // SPF_WHATIF_LINK_METRIC: d_fails holds the link ids, d_met the changes as
  // the kernels read them (WiMet::chg), d_delta what classify found, m_lo /
  // m_hi the metrics as given (spf_whatif_plan_metrics)
  uint32_t kind = 0;
  DevBuf<uint32_t> d_set_links;
  DevBuf<uint4> d_met;
  DevBuf<uint32_t> d_delta;
  std::vector<uint32_t> m_lo, m_hi;
  uint64_t epoch = 0;  // graph state the plan was derived from
  DevBuf<uint32_t> d_fails, d_link_edge, d_nbr_bit, d_dist, d_q, d_q2, d_bm, d_nhb, d_ctr;
  DevBuf<uint32_t> d_bar;  // the base kernel's grid-barrier counters
  DevBuf<uint32_t> d_lvl, d_order, d_misc;
  DevBuf<unsigned long long> d_H;
  DevBuf<uint2> d_hot, d_big, d_big0, d_big1;  // d_big1: d_big0 largest first
  // [0] n_hot, [1] cursor, [2] n_big (overflow), [3] n_big0 (classified),
  // [4] group teams' cursor
  DevBuf<uint32_t> d_cnt;
  DevBuf<unsigned char> d_ctl;  // group teams' TeamCtl
  uint32_t group = 0, group_teams = 0;  // workgroups per group team (0: one-workgroup teams)
  int prof_mode = 0;                    // whatif_prof_mode() at plan creation
  DevBuf<uint32_t> d_parent, d_sub;
  uint32_t big_teams = 0;
  // |D| a wave team holds (its scratch) and the parent-subtree size past
  // which classify sends a failure to the workgroup teams (A/B:
  // SPF_WHATIF_WAVECAP, SPF_WHATIF_CLASSIFY)
  uint32_t wave_cap = kWaveCap, classify_cap = kWaveCap;
  DevBuf<unsigned long long> d_prof;  // SPF_WHATIF_PROF diagnostics
  DevBuf<uint32_t> w_dlist, w_dnew, w_nhn, w_lvl, w_ord;  // wave-team scratch
  DevBuf<unsigned long long> w_tab;  // wave-team node sets (WaveSet), 1 << tab_log2 slots each
  DevBuf<uint4> d_ed;                 // interleaved edges (WiGraph::ed)
  uint32_t tab_log2 = 0;
  DevBuf<uint32_t> b_mark, b_dlist, b_dnew, b_nhn, b_lvl, b_ord;  // workgroup-team scratch
  DevBuf<uint32_t> c_mark, c_dlist, c_dnew, c_nhn, c_lvl, c_ord;  // same, concurrent set
  std::vector<hipEvent_t> ev;
  uint32_t timing_cap = 0, timing_n = 0;
  hipStream_t last = nullptr;  // stream of the last execute (spf_whatif_stats waits on it)
  // zero / negative metrics or u64 labels: every failure on the exact kernel
  std::unique_ptr<spfi::ExactWhatIf> exact;
  // change lists of the last spf_whatif_changes: the pool and its counts, the
  // digests when the caller passes none, events around count / scan / fill
  spfi::WiPool lists;
  DevBuf<uint32_t> l_cnt;
  DevBuf<spf_whatif_digest> l_dig;
  hipEvent_t l_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  float l_ms[3] = {0, 0, 0};
  // route lists of the last spf_whatif_routes (whatif_routes.hip), a consumer
  // of the lists above: spf_whatif_changes invalidates them
  spfi::WiRoutes rt;
  // the lists transposed to destination-major with every destination's summary
  // (whatif_impact.hip): imp_node over the change lists, imp_set over the route
  // lists; spf_whatif_changes invalidates both, spf_whatif_routes imp_set
  spfi::WiImpact imp_node, imp_set;
  // the route lists at link level (whatif_route_update.hip), a consumer of
  // both lists: spf_whatif_changes and spf_whatif_routes invalidate them
  spfi::WiUpdate up;
  ~spf_whatif_plan() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : l_ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace spfi {

// (whatif.hip) What the create calls of every kind start with: their NULL,
// loaded-graph and source checks (`who` names the call in the NULL message).
spf_status create_prologue(spf_ctx* c, spf_whatif_plan** out, uint32_t src, const char* who);
std::unique_ptr<spf_whatif_plan> new_plan(spf_ctx* c, uint32_t src, uint32_t kind, uint32_t n_fail);
// (whatif.hip) link id -> one directed edge of that link, kInf for a down link.
std::vector<uint32_t> link_edges(const spf_ctx* c);
// (whatif.hip) The part of plan creation that all kinds share.
spf_status plan_build(spf_ctx* c, std::unique_ptr<spf_whatif_plan>& p,
                      const std::vector<uint32_t>& fails, const std::vector<uint32_t>* link_edge,
                      spf_whatif_plan** out);

// A plan kind's entry points; kind_ops(p->kind) is how plan_build, execute and
// changes reach them.  Each kind's unit defines its entry (kind_ops_of<K>).
struct WiKindOps {
  // the plan's failures on `s` and the context's side stream (run_failures<K>)
  spf_status (*run)(spf_whatif_plan* p, spf_whatif_digest* d_out, hipStream_t s, const WiEmit* em);
  // the most registers of the kind's wave (rw) and group (rg) kernels
  hipError_t (*regs)(const spf_whatif_plan* p, int& rw, int& rg);
  const char* debug_name;  // in the SPF_WHATIF_DEBUG line
  const char* plan_name;   // in the accessors' wrong-kind messages
};
extern const WiKindOps kLinkOps, kDownOps, kDrainOps, kSetOps, kMetricOps;
const WiKindOps& kind_ops(uint32_t kind);

}  // namespace spfi

namespace {

inline WiGraph wi_graph(const spf_whatif_plan* p) {
  spf_ctx* c = p->ctx;
  WiGraph g{c->d_row_ptr.p, c->d_col.p, c->d_wt.p, c->d_rev.p, c->d_link.p, c->d_ovl.p,
            p->d_nbr_bit.p, c->N, p->src, p->W};
  g.fault = c->d_fault.p;
  g.ed = p->d_ed.p;
  return g;
}

// launch_resident with the arguments checked against the kernel's parameter
// list: one per parameter, each converted to its parameter's type, so a wrong
// or misplaced argument does not compile.  The occupancy check is made with
// the same pointer.
template <class... P, class... A>
hipError_t launch_resident_typed(void (*kernel)(P...), uint32_t blocks, uint32_t threads,
                                 uint32_t n_cu, hipStream_t s, const A&... a) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  std::tuple<P...> v(a...);
  return std::apply(
      [&](P&... x) {
        void* args[] = {static_cast<void*>(&x)...};
        return launch_resident(reinterpret_cast<const void*>(kernel), blocks, threads, args, n_cu, s);
      },
      v);
}

// A kind description K supplies
//   kKind               the repairs' KIND
//   kProfiled           whether the PROF 1 / 2 instances exist (link plans)
//   kDebugName, kPlanName   WiKindOps' names
//   table(p)            the kernels' trailing per-plan table as a tuple: none,
//                       a WiSets or a WiMet
//   classify(p, g, d_out, s)   the classify launch
//   SortKey, sort_key(p)       sort_big_kernel's key
//
// The repair kernels of kind K: f(wave, block, group, tail...) gets the typed
// kernel pointers and the kernels' trailing arguments -- the EMIT instances
// and the WiEmit first when `em`, else the PROF instances (0 unless
// K::kProfiled), then the kind's table.  `group` is the G-workgroup instance,
// NULL when G is none of 2, 4, 8, 16.  EMIT and PROF are chosen here and
// nowhere else.
template <class K, int PROF, bool EMIT, class F, class... EM>
auto repair_kernels_as(uint32_t G, F&& f, const EM&... tail) {
  constexpr int KIND = K::kKind;
  decltype(&repair_group_kernel<2, PROF, EMIT, KIND, EM...>) group = nullptr;
  switch (G) {
    case 2: group = repair_group_kernel<2, PROF, EMIT, KIND, EM...>; break;
    case 4: group = repair_group_kernel<4, PROF, EMIT, KIND, EM...>; break;
    case 8: group = repair_group_kernel<8, PROF, EMIT, KIND, EM...>; break;
    case 16: group = repair_group_kernel<16, PROF, EMIT, KIND, EM...>; break;
  }
  return f(repair_wave_kernel<PROF, EMIT, KIND, EM...>, repair_block_kernel<PROF, EMIT, KIND, EM...>,
           group, tail...);
}
template <class K, class F>
auto repair_kernels(const spf_whatif_plan* p, uint32_t G, int prof, const WiEmit* em, F&& f) {
  return std::apply(
      [&](const auto&... table) {
        if (em) return repair_kernels_as<K, 0, true>(G, f, *em, table...);
        if constexpr (K::kProfiled) {
          if (prof == 2) return repair_kernels_as<K, 2, false>(G, f, table...);
          if (prof == 1) return repair_kernels_as<K, 1, false>(G, f, table...);
        }
        return repair_kernels_as<K, 0, false>(G, f, table...);
      },
      K::table(p));
}

// The failures of the plan's list on `s` and the context's side stream:
// digests into d_out; with `em` the EMIT instances, which also count or fill
// the change lists (one pass per call).
template <class K>
spf_status run_failures(spf_whatif_plan* p, const WiGraph& g, spf_whatif_digest* d_out,
                        hipStream_t s, const WiEmit* em) {
  spf_ctx* c = p->ctx;
  // [0] n_hot, [1] cursor, [2] n_big (overflow), [3] n_big0, [4] group cursor
  uint32_t* const cnt = p->d_cnt.p;
  HIP_TRY(c, hipMemsetAsync(cnt, 0, 32, s));
  if (p->group) HIP_TRY(c, hipMemsetAsync(p->d_ctl.p, 0, sizeof(TeamCtl) * p->group_teams, s));
  if (!p->n_fail) return SPF_OK;
  K::classify(p, g, d_out, s);
  HIP_TRY(c, hipGetLastError());
  const WiBase B{p->d_dist.p, p->d_nhb.p, p->d_H.p};
  // SPF_WHATIF_PROF (link plans; never with lists): the prof buffer's rows are
  // [block / group teams][base][wave teams]
  const int prof = em ? 0 : p->prof_mode;
  const uint32_t bt = p->big_teams;
  // failures classified big (parent subtree > classify_cap) go to workgroup
  // teams on a second stream right away, beside the wave teams; separate
  // scratch, separate list, no dependence between the two grids
  hipStream_t side = c->side ? c->side : s;
  if (c->side) {
    HIP_TRY(c, hipEventRecord(c->side_fork, s));
    HIP_TRY(c, hipStreamWaitEvent(c->side, c->side_fork, 0));
  }
  // one-workgroup teams over `list` (n_list items) with the scratch set c_*
  // (`conc`: beside the wave teams, profiled) or b_*
  const auto blocks = [&](hipStream_t on, const uint2* list, const uint32_t* n_list, bool conc) {
    uint32_t *mark = conc ? p->c_mark.p : p->b_mark.p, *dlist = conc ? p->c_dlist.p : p->b_dlist.p;
    uint32_t *dnew = conc ? p->c_dnew.p : p->b_dnew.p, *nhn = conc ? p->c_nhn.p : p->b_nhn.p;
    uint32_t *lvl = conc ? p->c_lvl.p : p->b_lvl.p, *ord = conc ? p->c_ord.p : p->b_ord.p;
    const int pm = conc ? prof : 0;
    (void)repair_kernels<K>(p, 0, pm, em, [&](auto, auto block, auto, const auto&... tail) {
      hipLaunchKernelGGL(block, dim3(bt), dim3(1024), 0, on, g, B, list, n_list, mark, dlist, dnew, nhn,
                         lvl, ord, d_out, pm ? p->d_prof.p : nullptr, pm ? bt : 0u, tail...);
      return hipSuccess;
    });
  };
  bool grouped = false;
  if (p->group) {  // largest first, to group teams: one launch, a workgroup per CU
    hipLaunchKernelGGL(sort_big_kernel<typename K::SortKey>, dim3(1), dim3(1024), 0, side, p->d_big0.p,
                       cnt + 3, K::sort_key(p), p->d_big1.p);
    HIP_TRY(c, hipGetLastError());
    if (const spf_status st = resident_order(c, side); st != SPF_OK) return st;
    grouped = repair_kernels<K>(p, p->group, prof, em, [&](auto, auto, auto group, const auto&... tail) {
      if (!group) return hipErrorInvalidValue;
      return launch_resident_typed(group, c->n_cu, kGroupWg, c->n_cu, side, g, B, p->d_big1.p, cnt + 3,
                                   cnt + 4, reinterpret_cast<TeamCtl*>(p->d_ctl.p), p->c_mark.p,
                                   p->c_dlist.p, p->c_dnew.p, p->c_nhn.p, p->c_lvl.p, p->c_ord.p, d_out,
                                   prof ? p->d_prof.p : nullptr, prof ? bt : 0u, tail...);
    }) == hipSuccess;
    if (!grouped) (void)hipGetLastError();  // fall back to one-workgroup teams
    else if (const spf_status st = resident_done(c, side); st != SPF_OK) return st;
  }
  if (!grouped) blocks(side, p->d_big0.p, cnt + 3, true);
  HIP_TRY(c, hipGetLastError());
  if (c->side) HIP_TRY(c, hipEventRecord(c->side_join, c->side));
  (void)repair_kernels<K>(p, 0, prof, em, [&](auto wave, auto, auto, const auto&... tail) {
    hipLaunchKernelGGL(wave, dim3(p->wave_teams / 4), dim3(256), 0, s, g, B, p->d_hot.p, cnt, cnt + 1,
                       p->d_big.p, cnt + 2, p->w_tab.p, p->w_dlist.p, p->w_dnew.p, p->w_nhn.p,
                       p->w_lvl.p, p->w_ord.p, d_out, p->wave_cap, p->tab_log2,
                       prof ? p->d_prof.p + 16ull * (bt + 1) : nullptr, prof ? p->wave_teams : 0u,
                       tail...);
    return hipSuccess;
  });
  HIP_TRY(c, hipGetLastError());
  // the wave teams' overflow (|D| > wave_cap), after them on `s`
  blocks(s, p->d_big.p, cnt + 2, false);
  HIP_TRY(c, hipGetLastError());
  if (c->side) HIP_TRY(c, hipStreamWaitEvent(s, c->side_join, 0));
  return SPF_OK;
}

// The registers of the kind's wave and group kernels for plan_build's
// co-residency sum: the larger of the digest and the list instance of each.
// Link plans count the instance SPF_WHATIF_PROF selects alone, as they did
// before the list instances existed (ba_whatif's wave-team count rests on it).
template <class K>
hipError_t kind_regs(const spf_whatif_plan* p, int& rw, int& rg) {
  const auto most = [](auto kernel, int& r) {
    hipFuncAttributes a{};
    const hipError_t e = kernel ? hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel))
                                : hipErrorInvalidDeviceFunction;
    r = std::max(r, a.numRegs);
    return e;
  };
  const WiEmit lists{};
  for (const bool emit : {false, true}) {
    if (emit && K::kProfiled) break;
    const hipError_t e = repair_kernels<K>(
        p, p->group, p->prof_mode, emit ? &lists : nullptr,
        [&](auto wave, auto, auto group, const auto&...) {
          const hipError_t ew = most(wave, rw);
          return ew != hipSuccess ? ew : most(group, rg);
        });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

template <class K>
spf_status run_kind(spf_whatif_plan* p, spf_whatif_digest* d_out, hipStream_t s, const WiEmit* em) {
  return run_failures<K>(p, wi_graph(p), d_out, s, em);
}
// A kind's entry.  Not constexpr, and the entries not constants: a constant
// object is emitted for the device too, where the host functions it names do
// not exist.  The entries are initialised when the library loads; kind_ops
// holds their addresses only, and they are read from API calls.
template <class K>
WiKindOps kind_ops_of() {
  return {run_kind<K>, kind_regs<K>, K::kDebugName, K::kPlanName};
}

}  // namespace

#endif  // OPENR_AMD_WHATIF_PLAN_H
