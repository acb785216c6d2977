// ============================================================================
//  whatif_routes_host.h -- the host tables of spf_whatif_routes: the check of
//  the caller's destination sets and the inverse index node -> the sets that
//  hold it.  Plain C++ with no device in it, as plan_host.h:
//  whatif_routes.hip calls these and uploads what they return;
//  tests/host/whatif_routes_host_check.cpp runs them on the CPU.
// ============================================================================
#pragma once
#include <cstdint>
#include <vector>

namespace spfi {

// NULL when the sets are well formed, else what is wrong with them:
// set_ptr[0] != 0, set_ptr decreasing, a member >= n_nodes, NULL arrays with
// members.  n_sets == 0 needs no arrays.
const char* route_sets_check(uint32_t n_nodes, const uint32_t* set_ptr, const uint32_t* set_nodes,
                             uint32_t n_sets);

// Node v is a member of sets set[ptr[v] .. ptr[v + 1]) (ascending set id, each
// set once however often it repeats v), first at position pos[] of the set's
// member order.  Sets that hold `skip` (the source: its route never changes)
// are left out altogether, as are empty ones.
struct SetIndex {
  std::vector<uint32_t> ptr, set, pos;  // [n_nodes + 1], [entries], [entries]
};
SetIndex route_sets_index(uint32_t n_nodes, const uint32_t* set_ptr, const uint32_t* set_nodes,
                          uint32_t n_sets, uint32_t skip);

}  // namespace spfi
