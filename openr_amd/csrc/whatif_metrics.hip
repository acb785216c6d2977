// ============================================================================
//  whatif_metrics.hip -- what-if plans whose failures are link metric changes
//  (spf_whatif_plan_create_metrics: cost-out, undrain; whatif.hip's head
//  describes the kind): their classify kernel, their instances of the repair
//  kernels and their part of the C ABI.
// ============================================================================
#include "whatif_plan.h"

namespace {

// Link metric changes: cold -> digest now, hot -> work item (change, hot edge
// u -> v) and delta[f].  A direction a -> b whose weight changes from w to w'
// (a reachable and expanded) is hot when it is raised and tight, or lowered
// with d(a) + w' <= d(b) (delta = the slack); one direction at most is
// (positive metrics: a hot direction has d(a) < d(b)).  With delta = 0, D is
// the DAG descendants of b (a raise) or holds them (a new tie), so the parent
// subtree sub[b] is a lower bound of |D| and routes the item as a link
// failure's; with delta > 0 no bound is known: the wave teams take it and
// hand it to the workgroup teams when its D overflows.
__global__ void classify_metrics_kernel(WiGraph g, const uint32_t* __restrict__ dist,
                                        const unsigned long long* __restrict__ H,
                                        const uint4* __restrict__ chg, uint32_t n_fail,
                                        const uint32_t* __restrict__ sub, uint32_t wave_cap,
                                        spf_whatif_digest* out, uint2* hot, uint32_t* n_hot,
                                        uint2* big, uint32_t* n_big, uint32_t* delta) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_fail) return;
  const uint4 m = chg[f];
  uint32_t root = kInf, dl = 0;
  if (m.x != kInf && !g.hop) {  // (hop counts: no metric is read, every change is cold)
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t e = k ? m.y : m.x, w1 = k ? m.w : m.z, w0 = g.wt[e];
      const uint32_t a = g.col[g.rev[e]], b = g.col[e];  // a -> b
      if (w1 == w0 || (g.ovl[a] && a != g.src)) continue;
      const uint32_t da = dist[a], db = dist[b];
      if (da == kInf) continue;  // (a reached and expanded over an up link: b is reached)
      if (w1 > w0 ? da + w0 == db : (uint64_t)da + w1 <= db) {
        root = e;
        dl = w1 > w0 ? 0u : db - da - w1;
      }
    }
  }
  delta[f] = dl;
  if (root == kInf) {
    out[f] = spf_whatif_digest{0u, 0u, (uint64_t)*H};
  } else if (dl == 0 && sub[g.col[root]] > wave_cap) {  // |D| >= subtree: a workgroup's repair
    big[atomicAdd(n_big, 1u)] = make_uint2(f, root);
  } else {
    hot[atomicAdd(n_hot, 1u)] = make_uint2(f, root);
  }
}

// Metric plans: work items (change, hot edge u -> v) -- the link plans' items
// and their sort key; the kernels' trailing table is the WiMet.
struct MetricKind {
  static constexpr int kKind = kMetric;
  static constexpr bool kProfiled = false;
  static constexpr const char* kDebugName = " (link metrics)";
  static constexpr const char* kPlanName = "a metric plan (spf_whatif_plan_metrics)";
  static std::tuple<WiMet> table(const spf_whatif_plan* p) {
    return {WiMet{p->d_met.p, p->d_delta.p}};
  }
  static void classify(spf_whatif_plan* p, const WiGraph& g, spf_whatif_digest* d_out, hipStream_t s) {
    hipLaunchKernelGGL(classify_metrics_kernel, dim3((p->n_fail + 255) / 256), dim3(256), 0, s, g,
                       p->d_dist.p, p->d_H.p, p->d_met.p, p->n_fail, p->d_sub.p, p->classify_cap, d_out,
                       p->d_hot.p, p->d_cnt.p, p->d_big0.p, p->d_cnt.p + 3, p->d_delta.p);
  }
  using SortKey = KeySubOfHead;
  static SortKey sort_key(const spf_whatif_plan* p) { return {p->d_sub.p, p->ctx->d_col.p}; }
};

}  // namespace

const WiKindOps spfi::kMetricOps = kind_ops_of<MetricKind>();

extern "C" {

spf_status spf_whatif_plan_create_metrics(spf_ctx* c, uint32_t src, const uint32_t* links,
                                          const uint32_t* m_lo, const uint32_t* m_hi, uint32_t n,
                                          spf_whatif_plan** out) {
  if (const spf_status st = create_prologue(c, out, src, "spf_whatif_plan_create_metrics"); st != SPF_OK)
    return st;
  if (n && (!links || !m_lo || !m_hi))
    return fail(c, SPF_E_INVALID, "spf_whatif_plan_create_metrics: NULL links, m_lo or m_hi");
  for (uint32_t i = 0; i < n; ++i) {
    if (!c->E || links[i] > c->max_link)
      return fail(c, SPF_E_INVALID, "link %u is not a link id of the graph", links[i]);
    for (const uint32_t m : {m_lo[i], m_hi[i]})
      if (spfi::metric_past_u32(m, c->N))  // the loader's bound on the largest metric
        return fail(c, SPF_E_INVALID,
                    "spf_whatif_plan_create_metrics: metric %u of change %u (link %u) x %u nodes "
                    "leaves 32-bit distances", m, i, links[i], c->N);
  }
  if (c->nonpos || c->needs64)
    return fail(c, SPF_E_UNSUPPORTED,
                "spf_whatif_plan_create_metrics: link metric changes are not supported on graphs that "
                "take the exact path (a metric <= 0 or u64 labels)");
  // (link_edges: the edge out of the endpoint with the smaller CSR id, m_lo's)
  const std::vector<uint32_t> link_edge = link_edges(c);
  auto p = new_plan(c, src, (uint32_t)kMetric, n);
  p->m_lo.assign(m_lo, m_lo + n);
  p->m_hi.assign(m_hi, m_hi + n);
  std::vector<uint32_t> fails(links, links + n);
  if (fails.empty()) fails.push_back(0u);  // (never read: no change)
  std::vector<uint4> chg(std::max<uint32_t>(n, 1), make_uint4(kInf, kInf, 0u, 0u));
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t e = link_edge[links[i]];
    if (e == kInf) continue;
    const uint32_t r = c->rev[e];
    chg[i] = make_uint4(e, r, m_lo[i] != SPF_WHATIF_METRIC_KEEP ? m_lo[i] : c->wt[e],
                        m_hi[i] != SPF_WHATIF_METRIC_KEEP ? m_hi[i] : c->wt[r]);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, p->d_met.upload(chg.data(), chg.size(), c->stream));
  HIP_TRY(c, p->d_delta.alloc(std::max<uint32_t>(n, 1)));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (chg is freed on return)
  return plan_build(c, p, fails, nullptr, out);
}

spf_status spf_whatif_plan_metrics(const spf_whatif_plan* p, uint32_t* links, uint32_t* m_lo,
                                   uint32_t* m_hi) {
  if (!p) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  if (p->kind != (uint32_t)kMetric)
    return fail(c, SPF_E_STATE,
                "spf_whatif_plan_metrics: not a metric plan (spf_whatif_plan_links / _nodes / _sets)");
  if (links && p->n_fail)
    HIP_TRY(c, hipMemcpy(links, p->d_fails.p, 4ull * p->n_fail, hipMemcpyDeviceToHost));
  if (m_lo) std::copy(p->m_lo.begin(), p->m_lo.end(), m_lo);
  if (m_hi) std::copy(p->m_hi.begin(), p->m_hi.end(), m_hi);
  return SPF_OK;
}

}  // extern "C"
