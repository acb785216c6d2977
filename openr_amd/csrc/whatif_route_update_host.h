// ============================================================================
//  whatif_route_update_host.h -- the host tables of spf_whatif_route_update:
//  the source's CSR row as the kernels walk it, and the index link id -> slot
//  of that row.  Plain C++ with no device in it, as whatif_routes_host.h:
//  whatif_route_update.hip calls these and uploads what they return;
//  tests/host/whatif_route_update_host_check.cpp runs them on the CPU.
// ============================================================================
#pragma once
#include <cstdint>
#include <vector>

namespace spfi {

// Slot t of the source's row (CSR edge row_ptr[src] + t), in row order, which
// is linksFromNode order.  bit = the head's index among the source's distinct
// up neighbours, UINT32_MAX for a dead slot (a self-loop: a link that is not
// up keeps its place that way).
struct UpdateSlot {
  uint32_t bit, metric, link, head;
};
// (link id, t) of a live slot
struct UpdateLink {
  uint32_t link, slot;
};
struct UpdateRow {
  uint32_t first = 0;             // row_ptr[src]
  std::vector<UpdateSlot> slot;   // [row_ptr[src + 1] - row_ptr[src]]
  std::vector<UpdateLink> links;  // the live slots, ascending by link id (a link has one slot in a row)
};
// edge_nb: per CSR edge its head's index among its tail's distinct neighbours,
// UINT32_MAX for a dead slot (GraphHost::edge_nb).
UpdateRow update_row(const uint32_t* row_ptr, const uint32_t* col, const uint32_t* wt,
                     const uint32_t* link, const uint32_t* edge_nb, uint32_t src);

// The slot of `link` in the row, UINT32_MAX when the source has no live slot
// of it (the kernels' own search, restated for the check).
uint32_t update_row_find(const UpdateRow& row, uint32_t link);

}  // namespace spfi
