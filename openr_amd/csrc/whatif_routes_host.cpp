// whatif_routes_host.cpp -- see whatif_routes_host.h.
#include "whatif_routes_host.h"

#include <algorithm>

namespace spfi {

const char* route_sets_check(uint32_t n_nodes, const uint32_t* set_ptr, const uint32_t* set_nodes,
                             uint32_t n_sets) {
  if (n_sets == 0) return nullptr;
  if (!set_ptr) return "set_ptr is NULL";
  if (set_ptr[0] != 0) return "set_ptr[0] != 0";
  for (uint32_t s = 0; s < n_sets; ++s)
    if (set_ptr[s + 1] < set_ptr[s]) return "set_ptr decreases";
  const uint32_t m = set_ptr[n_sets];
  if (m && !set_nodes) return "set_nodes is NULL";
  for (uint32_t k = 0; k < m; ++k)
    if (set_nodes[k] >= n_nodes) return "a member is not a node of the graph";
  return nullptr;
}

SetIndex route_sets_index(uint32_t n_nodes, const uint32_t* set_ptr, const uint32_t* set_nodes,
                          uint32_t n_sets, uint32_t skip) {
  SetIndex x;
  x.ptr.assign((size_t)n_nodes + 1, 0);
  // seen[v] == s + 1: v was met in set s already (sets are visited ascending)
  std::vector<uint32_t> seen(n_nodes, 0);
  std::vector<uint8_t> out(n_sets, 0);
  for (uint32_t s = 0; s < n_sets; ++s)
    for (uint32_t k = set_ptr[s]; k < set_ptr[s + 1]; ++k)
      if (set_nodes[k] == skip) out[s] = 1;
  for (uint32_t s = 0; s < n_sets; ++s) {
    if (out[s]) continue;
    for (uint32_t k = set_ptr[s]; k < set_ptr[s + 1]; ++k) {
      const uint32_t v = set_nodes[k];
      if (seen[v] == s + 1) continue;
      seen[v] = s + 1;
      ++x.ptr[v + 1];
    }
  }
  for (uint32_t v = 0; v < n_nodes; ++v) x.ptr[v + 1] += x.ptr[v];
  x.set.resize(x.ptr[n_nodes]);
  x.pos.resize(x.ptr[n_nodes]);
  std::vector<uint32_t> at(x.ptr.begin(), x.ptr.end() - 1);
  std::fill(seen.begin(), seen.end(), 0u);
  for (uint32_t s = 0; s < n_sets; ++s) {
    if (out[s]) continue;
    for (uint32_t k = set_ptr[s]; k < set_ptr[s + 1]; ++k) {
      const uint32_t v = set_nodes[k];
      if (seen[v] == s + 1) continue;
      seen[v] = s + 1;
      x.set[at[v]] = s;
      x.pos[at[v]++] = k - set_ptr[s];
    }
  }
  return x;
}

}  // namespace spfi
