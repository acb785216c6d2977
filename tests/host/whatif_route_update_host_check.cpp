// The host tables of spf_whatif_route_update
// (openr_amd/csrc/whatif_route_update_host.cpp) on the CPU: the source's row as
// the kernels walk it and the link -> slot index, against brute force over
// seeded multigraph rows (parallel links, dead self-loop slots, an empty row).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "whatif_route_update_host.h"

using namespace spfi;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

struct Csr {
  std::vector<uint32_t> row_ptr, col, wt, link, edge_nb;
};

// rows[u] = (head, metric, link id); a head equal to u is a dead slot
static Csr make(const std::vector<std::vector<UpdateSlot>>& rows) {
  Csr g;
  g.row_ptr.push_back(0);
  for (uint32_t u = 0; u < rows.size(); ++u) {
    std::vector<uint32_t> nb;
    for (const UpdateSlot& e : rows[u])
      if (e.head != u) nb.push_back(e.head);
    std::sort(nb.begin(), nb.end());
    nb.erase(std::unique(nb.begin(), nb.end()), nb.end());
    for (const UpdateSlot& e : rows[u]) {
      g.col.push_back(e.head);
      g.wt.push_back(e.metric);
      g.link.push_back(e.link);
      g.edge_nb.push_back(e.head == u ? UINT32_MAX
                                      : (uint32_t)(std::lower_bound(nb.begin(), nb.end(), e.head) - nb.begin()));
    }
    g.row_ptr.push_back((uint32_t)g.col.size());
  }
  return g;
}

static void check(const std::vector<std::vector<UpdateSlot>>& rows, uint32_t src, uint32_t max_link) {
  const Csr g = make(rows);
  const UpdateRow r = update_row(g.row_ptr.data(), g.col.data(), g.wt.data(), g.link.data(),
                                 g.edge_nb.data(), src);
  CHECK(r.first == g.row_ptr[src]);
  CHECK(r.slot.size() == rows[src].size());
  size_t live = 0;
  for (uint32_t t = 0; t < r.slot.size(); ++t) {
    const UpdateSlot& want = rows[src][t];
    CHECK(r.slot[t].head == want.head && r.slot[t].metric == want.metric && r.slot[t].link == want.link);
    CHECK((r.slot[t].bit == UINT32_MAX) == (want.head == src));
    if (want.head != src) {
      ++live;
      CHECK(r.slot[t].bit == g.edge_nb[r.first + t]);
    }
  }
  CHECK(r.links.size() == live);
  for (size_t k = 1; k < r.links.size(); ++k) CHECK(r.links[k - 1].link < r.links[k].link);
  for (uint32_t l = 0; l <= max_link + 1; ++l) {
    uint32_t want = UINT32_MAX;
    for (uint32_t t = 0; t < rows[src].size(); ++t)
      if (rows[src][t].head != src && rows[src][t].link == l) want = t;
    CHECK(update_row_find(r, l) == want);
  }
}

int main() {
  // a bundle of two and a heavier third to node 1, a dead slot, a single link to node 2
  // (slots as {unused, metric, link id, head})
  check({{{0, 1, 7, 1}, {0, 1, 3, 1}, {0, 3, 5, 0}, {0, 3, 9, 1}, {0, 1, 4, 2}},
         {{0, 1, 7, 0}, {0, 1, 3, 0}, {0, 3, 9, 0}},
         {{0, 1, 4, 0}}},
        0, 9);
  check({{}, {{0, 2, 0, 1}}}, 0, 1);  // an empty row
  check({{{0, 1, 0, 0}}}, 0, 1);      // only a dead slot
  std::mt19937 rng(11);
  for (int round = 0; round < 200; ++round) {
    const uint32_t n = 2 + rng() % 12;
    std::vector<std::vector<UpdateSlot>> rows(n);
    uint32_t next_link = 0;
    const uint32_t n_links = rng() % 40;
    for (uint32_t k = 0; k < n_links; ++k) {
      const uint32_t a = rng() % n, b = rng() % n, w = 1 + rng() % 4, l = next_link++;
      if (a == b || rng() % 7 == 0) {  // a link that is not up: a dead slot at either end
        rows[a].push_back({0, w, l, a});
        if (a != b) rows[b].push_back({0, w, l, b});
      } else {
        rows[a].push_back({0, w, l, b});
        rows[b].push_back({0, w, l, a});
      }
    }
    for (auto& row : rows) std::shuffle(row.begin(), row.end(), rng);
    check(rows, rng() % n, next_link);
  }
  std::puts("whatif_route_update_host_check: ok");
  return 0;
}
