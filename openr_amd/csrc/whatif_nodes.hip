// ============================================================================
//  whatif_nodes.hip -- what-if plans whose failures are nodes, down or drained
//  (spf_whatif_plan_create_nodes; whatif.hip's head describes the two kinds):
//  their classify kernel, their instances of the repair kernels and their part
//  of the C ABI.
// ============================================================================
#include "whatif_plan.h"

namespace {

// Node failures: cold -> digest now, hot -> work item (failure, node x), to
// the workgroup teams when x's parent subtree exceeds wave_cap.  DOWN is hot
// whenever x is reachable (x itself changes); DRAIN when x is reachable, not
// drained already and the tail of a tight edge (the scan stops at the first).
template <int KIND>
__global__ void classify_nodes_kernel(WiGraph g, const uint32_t* __restrict__ dist,
                                      const unsigned long long* __restrict__ H,
                                      const uint32_t* __restrict__ fails, uint32_t n_fail,
                                      const uint32_t* __restrict__ sub, uint32_t wave_cap,
                                      spf_whatif_digest* out, uint2* hot, uint32_t* n_hot,
                                      uint2* big, uint32_t* n_big) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_fail) return;
  const uint32_t x = fails[f];  // < N, != src (checked at plan creation)
  const uint32_t dx = dist[x];
  bool is_hot = dx != kInf;
  if (is_hot && KIND == kDrain) {
    is_hot = false;
    if (!g.ovl[x])
      for (uint32_t e = g.row_ptr[x]; e < g.row_ptr[x + 1] && !is_hot; ++e)
        is_hot = g.col[e] != x && dx + g.wt[e] == dist[g.col[e]];
  }
  if (!is_hot) {
    out[f] = spf_whatif_digest{0u, 0u, (uint64_t)*H};
  } else if (sub[x] > wave_cap) {  // |D| >= subtree: a workgroup's repair
    big[atomicAdd(n_big, 1u)] = make_uint2(f, x);
  } else {
    hot[atomicAdd(n_hot, 1u)] = make_uint2(f, x);
  }
}

// Node plans: work items (failure, node), sorted by the node's parent subtree.
template <int KIND>
struct NodeKind {
  static constexpr int kKind = KIND;
  static constexpr bool kProfiled = false;
  static constexpr const char* kDebugName = KIND == kDown ? " (node down)" : " (node drain)";
  static constexpr const char* kPlanName = "a node plan (spf_whatif_plan_nodes)";
  static std::tuple<> table(const spf_whatif_plan*) { return {}; }
  static void classify(spf_whatif_plan* p, const WiGraph& g, spf_whatif_digest* d_out, hipStream_t s) {
    hipLaunchKernelGGL(classify_nodes_kernel<KIND>, dim3((p->n_fail + 255) / 256), dim3(256), 0, s, g,
                       p->d_dist.p, p->d_H.p, p->d_fails.p, p->n_fail, p->d_sub.p, p->classify_cap,
                       d_out, p->d_hot.p, p->d_cnt.p, p->d_big0.p, p->d_cnt.p + 3);
  }
  using SortKey = KeySubOfNode;
  static SortKey sort_key(const spf_whatif_plan* p) { return {p->d_sub.p}; }
};

}  // namespace

const WiKindOps spfi::kDownOps = kind_ops_of<NodeKind<kDown>>();
const WiKindOps spfi::kDrainOps = kind_ops_of<NodeKind<kDrain>>();

extern "C" {

spf_status spf_whatif_plan_create_nodes(spf_ctx* c, uint32_t src, uint32_t kind,
                                        const uint32_t* fail_nodes, uint32_t n_fail,
                                        spf_whatif_plan** out) {
  if (const spf_status st = create_prologue(c, out, src, "spf_whatif_plan_create_nodes"); st != SPF_OK)
    return st;
  if (kind != SPF_WHATIF_NODE_DOWN && kind != SPF_WHATIF_NODE_DRAIN)
    return fail(c, SPF_E_INVALID, "spf_whatif_plan_create_nodes: unknown kind %u", kind);
  std::vector<uint32_t> fails;
  if (fail_nodes) {
    fails.assign(fail_nodes, fail_nodes + n_fail);
    for (uint32_t x : fails) {
      if (x >= c->N) return fail(c, SPF_E_INVALID, "node %u out of range", x);
      if (x == src) return fail(c, SPF_E_INVALID, "node %u is the source: not a failure of this call", x);
    }
  } else {  // every node except the source, ascending id
    for (uint32_t x = 0; x < c->N; ++x)
      if (x != src) fails.push_back(x);
  }
  if (c->nonpos || c->needs64)
    return fail(c, SPF_E_UNSUPPORTED,
                "spf_whatif_plan_create_nodes: node failures are not supported on graphs that take the "
                "exact path (a metric <= 0 or u64 labels)");
  auto p = new_plan(c, src, kind, (uint32_t)fails.size());
  return plan_build(c, p, fails, nullptr, out);
}

spf_status spf_whatif_plan_nodes(const spf_whatif_plan* p, uint32_t* nodes) {
  if (!p || !nodes) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  if (p->kind != (uint32_t)kDown && p->kind != (uint32_t)kDrain)
    return fail(c, SPF_E_STATE, "spf_whatif_plan_nodes: %s", kind_ops(p->kind).plan_name);
  HIP_TRY(c, hipMemcpy(nodes, p->d_fails.p, 4ull * p->n_fail, hipMemcpyDeviceToHost));
  return SPF_OK;
}

}  // extern "C"
