// ============================================================================
//  whatif_sets.hip -- what-if plans whose failures are sets of links failing
//  together (spf_whatif_plan_create_sets, shared-risk groups; whatif.hip's head
//  describes the kind): their classify kernel, their instances of the repair
//  kernels and their part of the C ABI.
// ============================================================================
#include "whatif_plan.h"

namespace {

// Link sets: a wave per set, its lanes over the members 64 at a time (a hub's
// 167 links, a conduit's 200, do not serialise on one thread).  Cold (no tight
// member: the empty set too) -> digest now.  Hot -> work item (failure, size
// estimate): the saturating sum of sub[] over the tight members' heads.  The
// sum counts a shared head and a root nested in another root's subtree twice,
// so it can exceed |D|'s lower bound; it is right for the common case, roots
// with disjoint subtrees, where the maximum would keep a repair of several
// near-cap subtrees on a wave team only for it to overflow and be re-queued.
// Either way the result is the same: an estimate above wave_cap goes to the
// workgroup teams, a wave team that overflows hands its failure to them.
__global__ __launch_bounds__(256) void classify_sets_kernel(
    WiGraph g, const uint32_t* __restrict__ dist, const unsigned long long* __restrict__ H, WiSets ss,
    uint32_t n_fail, const uint32_t* __restrict__ sub, uint32_t wave_cap, spf_whatif_digest* out,
    uint2* hot, uint32_t* n_hot, uint2* big, uint32_t* n_big) {
  const uint32_t f = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (f >= n_fail) return;  // wave-uniform
  const uint32_t b0 = ss.ptr[f], n = ss.ptr[f + 1] - b0;
  const auto sat_add = [](uint32_t a, uint32_t b) { return a + b < a ? ~0u : a + b; };
  uint32_t est = 0;
  bool any = false;
  for (uint32_t c0 = 0; c0 < n; c0 += 64) {  // wave-uniform
    const uint32_t i = c0 + lane;
    const uint32_t head = i < n ? tight_head(g, dist, ss.link_edge[ss.links[b0 + i]]) : kInf;
    if (head != kInf) {
      any = true;
      est = sat_add(est, sub[head]);
    }
  }
  for (int d = 32; d >= 1; d >>= 1) est = sat_add(est, (uint32_t)__shfl_xor(est, d, 64));
  const bool is_hot = __ballot(any) != 0;
  if (lane != 0) return;
  if (!is_hot) {
    out[f] = spf_whatif_digest{0u, 0u, (uint64_t)*H};
  } else if (est > wave_cap) {  // a workgroup's repair
    big[atomicAdd(n_big, 1u)] = make_uint2(f, est);
  } else {
    hot[atomicAdd(n_hot, 1u)] = make_uint2(f, est);
  }
}

// Set plans: work items (failure, size estimate), sorted by the estimate; the
// kernels' trailing table is the WiSets.
struct SetKind {
  static constexpr int kKind = kSet;
  static constexpr bool kProfiled = false;
  static constexpr const char* kDebugName = " (link sets)";
  static constexpr const char* kPlanName = "a set plan (spf_whatif_plan_sets)";
  static std::tuple<WiSets> table(const spf_whatif_plan* p) {
    return {WiSets{p->d_fails.p, p->d_set_links.p, p->d_link_edge.p}};
  }
  static void classify(spf_whatif_plan* p, const WiGraph& g, spf_whatif_digest* d_out, hipStream_t s) {
    hipLaunchKernelGGL(classify_sets_kernel, dim3((p->n_fail + 3) / 4), dim3(256), 0, s, g, p->d_dist.p,
                       p->d_H.p, std::get<0>(table(p)), p->n_fail, p->d_sub.p, p->classify_cap, d_out,
                       p->d_hot.p, p->d_cnt.p, p->d_big0.p, p->d_cnt.p + 3);
  }
  using SortKey = KeyItself;
  static SortKey sort_key(const spf_whatif_plan*) { return {}; }
};

}  // namespace

const WiKindOps spfi::kSetOps = kind_ops_of<SetKind>();

extern "C" {

spf_status spf_whatif_plan_create_sets(spf_ctx* c, uint32_t src, const uint32_t* set_ptr,
                                       const uint32_t* set_links, uint32_t n_sets,
                                       spf_whatif_plan** out) {
  if (const spf_status st = create_prologue(c, out, src, "spf_whatif_plan_create_sets"); st != SPF_OK)
    return st;
  if (n_sets && !set_ptr) return fail(c, SPF_E_INVALID, "spf_whatif_plan_create_sets: NULL set_ptr");
  if (n_sets && set_ptr[0] != 0)
    return fail(c, SPF_E_INVALID, "spf_whatif_plan_create_sets: set_ptr[0] = %u, not 0", set_ptr[0]);
  for (uint32_t i = 0; i < n_sets; ++i)
    if (set_ptr[i + 1] < set_ptr[i])
      return fail(c, SPF_E_INVALID, "spf_whatif_plan_create_sets: set_ptr decreases at set %u", i);
  const uint32_t total = n_sets ? set_ptr[n_sets] : 0u;
  if (total && !set_links) return fail(c, SPF_E_INVALID, "spf_whatif_plan_create_sets: NULL set_links");
  for (uint32_t k = 0; k < total; ++k)
    if (!c->E || set_links[k] > c->max_link)
      return fail(c, SPF_E_INVALID, "link %u is not a link id of the graph", set_links[k]);
  if (c->nonpos || c->needs64)
    return fail(c, SPF_E_UNSUPPORTED,
                "spf_whatif_plan_create_sets: link sets are not supported on graphs that take the "
                "exact path (a metric <= 0 or u64 labels)");
  // canonical sets: each ascending, duplicates removed; the order of the sets kept
  std::vector<uint32_t> ptr(1, 0u), links;
  links.reserve(total);
  for (uint32_t i = 0; i < n_sets; ++i) {
    const size_t b0 = links.size();
    links.insert(links.end(), set_links + set_ptr[i], set_links + set_ptr[i + 1]);
    std::sort(links.begin() + b0, links.end());
    links.erase(std::unique(links.begin() + b0, links.end()), links.end());
    ptr.push_back((uint32_t)links.size());
  }
  const std::vector<uint32_t> link_edge = link_edges(c);
  auto p = new_plan(c, src, (uint32_t)kSet, n_sets);
  HIP_TRY(c, hipSetDevice(c->device));
  if (links.empty()) links.push_back(0u);  // (never read: every set is empty)
  HIP_TRY(c, p->d_set_links.upload(links.data(), links.size(), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (links is freed on return)
  return plan_build(c, p, ptr, &link_edge, out);
}

spf_status spf_whatif_plan_sets(const spf_whatif_plan* p, uint32_t* set_ptr, uint32_t* set_links) {
  if (!p || !set_ptr) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  if (p->kind != (uint32_t)kSet)
    return fail(c, SPF_E_STATE, "spf_whatif_plan_sets: not a set plan (spf_whatif_plan_links / _nodes)");
  HIP_TRY(c, hipMemcpy(set_ptr, p->d_fails.p, 4ull * ((size_t)p->n_fail + 1), hipMemcpyDeviceToHost));
  const uint32_t total = set_ptr[p->n_fail];
  if (total && set_links) HIP_TRY(c, hipMemcpy(set_links, p->d_set_links.p, 4ull * total, hipMemcpyDeviceToHost));
  return SPF_OK;
}

}  // extern "C"
