// The host tables of spf_whatif_route_update (whatif_route_update_host.h).
#include "whatif_route_update_host.h"

#include <algorithm>

namespace spfi {

UpdateRow update_row(const uint32_t* row_ptr, const uint32_t* col, const uint32_t* wt,
                     const uint32_t* link, const uint32_t* edge_nb, uint32_t src) {
  UpdateRow r;
  r.first = row_ptr[src];
  const uint32_t n = row_ptr[src + 1] - r.first;
  r.slot.resize(n);
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t q = r.first + t;
    const bool dead = col[q] == src || edge_nb[q] == UINT32_MAX;
    r.slot[t] = UpdateSlot{dead ? UINT32_MAX : edge_nb[q], wt[q], link[q], col[q]};
    if (!dead) r.links.push_back(UpdateLink{link[q], t});
  }
  std::sort(r.links.begin(), r.links.end(), [](const UpdateLink& a, const UpdateLink& b) {
    return a.link != b.link ? a.link < b.link : a.slot < b.slot;
  });
  return r;
}

uint32_t update_row_find(const UpdateRow& row, uint32_t link) {
  size_t lo = 0, hi = row.links.size();
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (row.links[mid].link < link) lo = mid + 1;
    else hi = mid;
  }
  return lo < row.links.size() && row.links[lo].link == link ? row.links[lo].slot : UINT32_MAX;
}

}  // namespace spfi
