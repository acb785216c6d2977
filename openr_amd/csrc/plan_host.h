// ============================================================================
//  plan_host.h -- every host table a plan derives from the graph for its
//  next-hop passes: the closure rows, the next-hop layout, the per-source
//  neighbour rows, the per-XCD source lists and the sliced pass's work units,
//  plus the two BFS bounds a plan's mode decisions read.  Plain C++ with no
//  device in it, as graph_host.h: build_plan (spf_engine.hip) decides the
//  modes, calls these and uploads what they return;
//  tests/host/plan_host_check.cpp runs them on the CPU.
// ============================================================================
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "graph_host.h"

namespace spfi {

// shared with the next-hop kernels (ecmp.hip) and the class-row expansion
// (class_rows.hip)
constexpr uint32_t kEcmpRunsPerXcd = 64;  // source runs dealt to each XCD
constexpr uint32_t kSlSlots = 8;     // plane slots per word of a sliced row
constexpr uint32_t kSlSat = 254;     // maxd at which the u8 copy saturates
constexpr uint32_t kSlGroup = 8;     // sources per group unit, at most
constexpr uint32_t kSlSeg = 4;  // neighbour positions per grouping segment (one uint4 of row offsets)
constexpr uint32_t kSlUnit = 512;    // neighbour-chunk matches per work unit, about

// The distance rows a request needs: closure[r] = the node of row r, row_of
// its inverse (kInf: no row).  Distinct sources come first (rows 0 .. n_src - 1
// are the request's rows: kernels that can write a row prefix straight into
// the caller's buffer do, msbfs_team_kernel), then each source and its
// non-drained neighbours in request order.  direct: the request is its own
// closure (distinct, every non-drained neighbour a source): closure == srcs.
struct PlanRows {
  bool distinct = false, direct = false;
  std::vector<uint32_t> closure, row_of, req_rows;  // [rows], [N], [n_src]
};
PlanRows plan_rows(const GraphHost& g, const uint32_t* srcs, uint32_t n_src);

// Next-hop layout: source i's bitmaps are words[i] (one per distinct up
// neighbour) x pitch / 32 words at nh_off[i]; wmax = words per node of the
// widest source (>= 1).  Depends on the CSR structure only.
struct NhLayout {
  std::vector<uint32_t> words;
  std::vector<uint64_t> nh_off;
  uint64_t nh_total = 0;
  uint32_t wmax = 1;
};
NhLayout plan_nh_layout(const GraphHost& g, const uint32_t* srcs, uint32_t n_src);

// Per-source neighbour rows of the next-hop pass: source i's list starts at
// nb_row_off[i] (a multiple of 8) and holds, per distinct neighbour, where its
// distance row starts -- row * stride (stride = the u8 row pitch, or the words
// of a sliced row), or the row itself when stride == 0 -- and `dead` for a
// drained one (rows * stride: the all-ones row behind the last; kInf when
// stride == 0).  Every list is padded with `dead` to a multiple of 8 plus 8.
struct NbRows {
  std::vector<uint32_t> nb_row, nb_row_off, nb_drained;
  uint32_t dead = kInf;
};
NbRows plan_nb_rows(const GraphHost& g, const uint32_t* srcs, uint32_t n_src,
                    const std::vector<uint32_t>& row_of, uint64_t stride, size_t rows);

// Next-hop blocks per XCD: runs of consecutive sources of about
// 1 / (8 * runs) of the work each, every run to the XCD with the least work so
// far (runs == 0: plain round-robin).  slot[t * 8 + g] = list[g][t], kInf past
// a list's end; slots = its size (a lone kInf stands in for an empty table).
struct XcdLists {
  std::vector<uint32_t> list[8];
  std::vector<uint32_t> slot;
  size_t slots = 0;
};
XcdLists plan_xcd_lists(const std::vector<uint32_t>& words, uint32_t runs);

// The sliced pass's work units, uint4 each, per XCD in unit_off[g] ..
// unit_off[g + 1]:
//   {source i, chunk_begin | chunk_end << 16, j0, j1}: neighbour positions
//     [j0, j1) of source i over those 64-word chunks;
//   {gtab offset, chunk | 1 << 31, j0, j1}: the same range for every member of
//     the group gtab[offset] = n, then its n sources, whose neighbour rows are
//     equal on [j0, j1) and none drained -- one wave loads each row once.
// Every (source, position, chunk) is in exactly one unit; j0 is a multiple of
// kSlSeg.  unit: matches per unit aimed at; group: 0 no groups, 1 sources with
// identical whole lists, 2 per segment of kSlSeg positions.  Empty tables are
// four zero words (units) and one (gtab).
struct SlicedUnits {
  std::vector<uint32_t> units, unit_off, gtab;
  uint32_t max_xcd_units = 0;
};
SlicedUnits plan_sliced_units(const std::vector<uint32_t> (&list)[8], const std::vector<uint32_t>& words,
                              const NbRows& nb, uint32_t chunks, uint32_t unit, int group);
// the unit size of a plan left to itself: about 16 units per CU, 16 .. kSlUnit
uint32_t plan_sliced_unit(const std::vector<uint32_t>& words, uint32_t chunks, uint32_t n_cu);

// Class rows (unit-metric plans on a graph whose twin-class quotient is in
// use): for a fixed source, every node of one class other than the source
// lies at the same distance, and twin sources agree outside themselves, so
// the BFS solves one row per distinct class among the closure rows and the
// expansion kernel writes the node rows from those.
//   csrc[k]: the node standing for class source k (the first closure row of
//     its class, class sources in closure order);
//   crow_of[r]: the class source of closure row r (closure[r]'s class);
//   fwd[c]: 1 when some member of class c is not drained (a class reached by
//     the BFS forwards then: twins share their neighbours).
// Needs g.qt built (graph_host_quotient) for the graph as it stands.
struct ClassRows {
  std::vector<uint32_t> csrc, crow_of;
  std::vector<uint8_t> fwd;
};
ClassRows plan_class_rows(const GraphHost& g, const std::vector<uint32_t>& closure);

// The expansion kernel's grid.  A workgroup owns whole groups of kExRows
// closure rows and sweeps them in pieces of kExPiece nodes (a wave's store of
// four nodes per lane).  resident = the workgroups the chip holds at once.
//   groups >= resident: the full width per workgroup (splits == 1), gper =
//     the rounds the chip needs, consecutive groups each, so every workgroup
//     is resident from the start and all but the last own gper groups;
//   fewer groups: one group per workgroup and the width split into `splits`
//     ranges of pps pieces, as many as the chip holds.
// Workgroup (x, y) owns groups [x * gper, min(groups, (x + 1) * gper)) over
// pieces [y * pps, min(pieces, (y + 1) * pps)).
constexpr uint32_t kExRows = 8;
constexpr uint32_t kExPiece = 256;
struct ExpandGrid {
  uint32_t groups = 0, pieces = 0;  // row groups, pieces of the width
  uint32_t wgs = 1, gper = 1;       // grid x, groups per workgroup
  uint32_t splits = 1, pps = 1;     // grid y, pieces per split
};
ExpandGrid plan_expand_grid(uint32_t rows, uint32_t span, uint32_t resident);

// What the two bounds below remember of the graph they were taken from.
struct DepthCache {
  std::vector<uint32_t> ecc;  // per-node eccentricity estimates, for ecc_epoch
  uint64_t ecc_epoch = ~0ull;
  uint32_t dbound = 0;  // hop-distance upper bound, for dbound_epoch
  uint64_t dbound_epoch = ~0ull;
  // recent bounds by (sliced-ELL structure version, drain bits): a drain bit
  // toggled back and forth (the BM_DecisionFabric publication) or a metric
  // patch (the bound counts hops) finds its bound again without a BFS
  struct Memo {
    uint64_t sell_ver;
    std::vector<uint8_t> ovl;
    uint32_t dbound;
  };
  std::vector<Memo> memo;
};
// Eccentricity estimate of every node (hop counts, drains ignored): the
// largest BFS distance from a few landmarks -- the node farthest from node
// 0, then repeatedly the node farthest from every landmark so far (on a grid:
// the corners, which makes it exact).  Cached per graph epoch.
const std::vector<uint32_t>& ecc_estimate(const GraphHost& g, DepthCache* m);
// the closure's rows by ecc of their node, deepest first, ties in row order
// (the register-plane BFS batches rows of similar depth)
std::vector<uint32_t> plan_depth_order(const std::vector<uint32_t>& closure, const std::vector<uint32_t>& ecc);
// An upper bound on every hop distance of the graph (any source, drained
// nodes expanded only as the source, LinkState.cpp:831-838): paths run
// s -> x -> ... -> y -> v with x .. y in H = the non-drained nodes, so
// d(s, v) <= 2 + d_H(x, y) <= 2 + 2 ecc_H(r) for any r of x's component of
// H.  One BFS in H per component.  Plans whose rows cannot saturate the u8
// copy (bound < 254) never need u32 rows of non-source closure rows.
uint32_t depth_bound(const GraphHost& g, DepthCache* m);

}  // namespace spfi
