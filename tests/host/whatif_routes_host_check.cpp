// The host tables of spf_whatif_routes (openr_amd/csrc/whatif_routes_host.cpp)
// on the CPU: the check of the caller's sets, and the inverse index against a
// brute-force one over seeded sets (repeated members, empty sets, identical
// sets, sets that hold the skipped node).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "whatif_routes_host.h"

using namespace spfi;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

static void check_index(uint32_t n_nodes, const std::vector<std::vector<uint32_t>>& sets, uint32_t skip) {
  std::vector<uint32_t> ptr(1, 0), nodes;
  for (const auto& s : sets) {
    nodes.insert(nodes.end(), s.begin(), s.end());
    ptr.push_back((uint32_t)nodes.size());
  }
  const uint32_t n = (uint32_t)sets.size();
  CHECK(route_sets_check(n_nodes, ptr.data(), nodes.empty() ? nullptr : nodes.data(), n) == nullptr);
  const SetIndex x = route_sets_index(n_nodes, ptr.data(), nodes.data(), n, skip);
  CHECK(x.ptr.size() == (size_t)n_nodes + 1 && x.ptr[0] == 0);
  CHECK(x.set.size() == x.ptr[n_nodes] && x.pos.size() == x.set.size());
  for (uint32_t v = 0; v < n_nodes; ++v) {
    std::vector<std::pair<uint32_t, uint32_t>> want;  // brute force: every set, every member
    for (uint32_t s = 0; s < n; ++s) {
      bool skipped = false;
      uint32_t first = UINT32_MAX;
      for (uint32_t k = 0; k < sets[s].size(); ++k) {
        skipped |= sets[s][k] == skip;
        if (sets[s][k] == v && first == UINT32_MAX) first = k;
      }
      if (!skipped && first != UINT32_MAX) want.push_back({s, first});
    }
    CHECK(x.ptr[v + 1] - x.ptr[v] == want.size());
    for (size_t k = 0; k < want.size(); ++k) {
      CHECK(x.set[x.ptr[v] + k] == want[k].first);
      CHECK(x.pos[x.ptr[v] + k] == want[k].second);
    }
  }
  CHECK(x.ptr[skip + 1] == x.ptr[skip]);  // the skipped node is in no indexed set
}

int main() {
  // the check
  {
    const uint32_t ptr[] = {0, 2, 2, 3}, nodes[] = {1, 4, 0};
    CHECK(route_sets_check(5, ptr, nodes, 3) == nullptr);
    CHECK(route_sets_check(5, nullptr, nullptr, 0) == nullptr);
    CHECK(route_sets_check(4, ptr, nodes, 3) != nullptr);  // member 4 of 4 nodes
    CHECK(route_sets_check(5, ptr, nullptr, 3) != nullptr);
    CHECK(route_sets_check(5, nullptr, nodes, 3) != nullptr);
    const uint32_t from1[] = {1, 2, 2, 3}, down[] = {0, 2, 1, 3}, empty[] = {0, 0, 0};
    CHECK(route_sets_check(5, from1, nodes, 3) != nullptr);
    CHECK(route_sets_check(5, down, nodes, 3) != nullptr);
    CHECK(route_sets_check(5, empty, nullptr, 2) == nullptr);  // no members: no array needed
  }
  // hand cases
  check_index(6, {{1, 2}, {}, {2, 2, 1}, {1, 2}, {0, 3}, {5}}, 0);
  check_index(3, {}, 1);
  check_index(4, {{}, {}}, 2);
  // seeded
  std::mt19937 rng(7);
  for (int round = 0; round < 50; ++round) {
    const uint32_t n_nodes = 1 + rng() % 40;
    std::vector<std::vector<uint32_t>> sets(rng() % 30);
    for (auto& s : sets) {
      s.resize(rng() % 4 == 0 ? 0 : rng() % (2 * n_nodes));
      for (auto& v : s) v = rng() % n_nodes;
    }
    if (sets.size() > 2) sets[1] = sets[0];
    check_index(n_nodes, sets, rng() % n_nodes);
  }
  std::puts("whatif_routes_host_check: ok");
  return 0;
}
