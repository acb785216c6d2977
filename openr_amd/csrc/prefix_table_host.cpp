// ============================================================================
//  prefix_table_host.cpp -- see prefix_table_host.h.
// ============================================================================
#include "prefix_table_host.h"

#include <algorithm>
#include <array>
#include <climits>

namespace spfi {

namespace {

using Tuple = std::array<int64_t, 3>;  // (path_preference, source_preference, -distance)

spf_status refuse(std::string* err, spf_status st, uint32_t p, const std::string& what) {
  if (err) *err = "prefix " + std::to_string(p) + ": " + what;
  return st;
}

}  // namespace

spf_status prefix_table_build(const uint32_t* pfx_ptr, const uint32_t* ent_node, const int32_t* ent_pp,
                              const int32_t* ent_sp, const int32_t* ent_dist, const int64_t* ent_min_nh,
                              uint32_t n_pfx, const uint8_t* overloaded, uint32_t n_nodes, bool all_best,
                              PrefixTable* out, std::string* err) {
  out->n_pfx = n_pfx;
  out->ptr.assign((size_t)n_pfx + 1, 0);
  out->ent.clear();
  if (n_pfx && !pfx_ptr) return refuse(err, SPF_E_INVALID, 0, "NULL pfx_ptr");
  if (n_pfx && pfx_ptr[0] != 0) return refuse(err, SPF_E_INVALID, 0, "pfx_ptr does not start at 0");
  for (uint32_t p = 0; p < n_pfx; ++p)
    if (pfx_ptr[p + 1] < pfx_ptr[p]) return refuse(err, SPF_E_INVALID, p, "pfx_ptr decreases");
  const uint32_t n_ent = n_pfx ? pfx_ptr[n_pfx] : 0;
  if (n_ent && (!ent_node || !ent_pp || !ent_sp || !ent_dist || !ent_min_nh || !overloaded))
    return refuse(err, SPF_E_INVALID, 0, "NULL entry array");
  std::vector<uint32_t> seen(n_nodes, 0);  // seen[v] = p + 1: v advertises prefix p
  std::vector<Tuple> order;
  for (uint32_t p = 0; p < n_pfx; ++p) {
    const uint32_t b = pfx_ptr[p], e = pfx_ptr[p + 1];
    if (e - b >= (1u << 24)) return refuse(err, SPF_E_UNSUPPORTED, p, "2^24 entries or more");
    const size_t first = out->ent.size();
    order.clear();
    for (uint32_t k = b; k < e; ++k) {
      const uint32_t v = ent_node[k];
      if (v >= n_nodes) return refuse(err, SPF_E_INVALID, p, "node " + std::to_string(v) + " out of range");
      if (seen[v] == p + 1) return refuse(err, SPF_E_INVALID, p, "node " + std::to_string(v) + " twice");
      seen[v] = p + 1;
      if (ent_dist[k] == INT32_MIN) return refuse(err, SPF_E_INVALID, p, "distance INT32_MIN");
      const Tuple t{ent_pp[k], ent_sp[k], -(int64_t)ent_dist[k]};
      if (!all_best && t < Tuple{0, 0, 0}) continue;  // under the floor: never selected
      const int64_t mn = ent_min_nh[k];
      const uint32_t need = mn <= 0 ? 0u : (uint32_t)std::min<int64_t>(mn, UINT32_MAX);
      out->ent.push_back({v, 0u, need, overloaded[v] ? 1u : 0u});
      order.push_back(t);
    }
    if (!all_best) {
      std::vector<Tuple> rank(order);
      std::sort(rank.begin(), rank.end());
      rank.erase(std::unique(rank.begin(), rank.end()), rank.end());
      for (size_t i = 0; i < order.size(); ++i)
        out->ent[first + i].rank = (uint32_t)(std::lower_bound(rank.begin(), rank.end(), order[i]) - rank.begin());
    }
    out->ptr[p + 1] = (uint32_t)out->ent.size();
  }
  return SPF_OK;
}

PrefixChoice prefix_select(const PrefixTable& t, uint32_t p, uint32_t me, const uint32_t* dist, bool all_best) {
  PrefixChoice c;
  const uint32_t b = t.ptr[p], e = t.ptr[p + 1];
  // 1, 2: the reachable entries of the greatest rank
  std::vector<uint32_t> b0;
  uint32_t top = 0;
  for (uint32_t k = b; k < e; ++k) {
    const PrefixEnt& x = t.ent[k];
    if (x.node != me && dist[x.node] == SPF_UNREACHABLE) continue;
    if (b0.empty() || x.rank > top) {
      top = x.rank;
      b0.clear();
    }
    if (x.rank == top) b0.push_back(k);
  }
  if (b0.empty()) {
    c.status = SPF_PREFIX_NONE;
    return c;
  }
  // 3: the best node, before the drained filter (which never moves it)
  bool mine = false;
  for (const uint32_t k : b0) {
    mine |= t.ent[k].node == me;
    c.best = std::min(c.best, t.ent[k].node);
  }
  if (mine && !all_best) c.best = me;
  // 4: without the drained ones, unless every one is drained
  std::vector<uint32_t> kept;
  for (const uint32_t k : b0)
    if (!t.ent[k].drained) kept.push_back(k);
  if (kept.empty()) kept = b0;
  c.status = SPF_PREFIX_ROUTE;
  for (const uint32_t k : kept) {
    c.B.push_back(t.ent[k].node);
    c.need = std::max(c.need, t.ent[k].min_nh);
    if (t.ent[k].node == me) c.status = SPF_PREFIX_SELF;  // 5: me in B (not B0)
  }
  return c;
}

}  // namespace spfi
