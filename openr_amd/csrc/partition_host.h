// ============================================================================
//  partition_host.h -- the host arithmetic of the multi-device plans, no HIP
//  in it: the partition of a batch of sources over the members (multi.cpp:
//  spf_partition_sources, spf_mplan_create), the label groups of the
//  node-label routes (spf_label_groups) and the label union of a route delta
//  (mplan_routes.cpp: spf_mplan_route_delta).  Built on the CPU under the
//  sanitizers by tests/test_partition_host.py.
// ============================================================================
#pragma once
#include <cstdint>
#include <vector>

#include "openr_spf.h"

namespace spfi {

// a source's cost in next-hop bitmaps: its k bitmaps plus its distance rows
// (u32 + the u8 copy = 5N bytes = 40 bitmaps of N/8 bytes); the same
// constant as openr_amd/sharding.py AllSourcesLayout.ROW_COST
constexpr double kRowCost = 40.0;
// SPF_PARTITION_AUTO answers contiguous above this many nodes (the locality
// partition keeps a byte per node and part)
constexpr uint32_t kLocalityMaxNodes = 1u << 16;

// closure sizes of a partition: per part, its sources plus their neighbours
std::vector<uint32_t> closure_sizes(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                                    const uint32_t* srcs, uint32_t n_src, const uint32_t* part,
                                    uint32_t n_parts);

// contiguous blocks of the request order balanced by cost (k + kRowCost):
// block r ends at the first prefix cost above total * (r+1) / n_parts
void contiguous_parts(const uint32_t* nb_ptr, const uint32_t* srcs, uint32_t n_src, uint32_t n_parts,
                      uint32_t* part);

// the streaming locality partition (sharding.py locality_partition)
void locality_parts(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                    const uint32_t* srcs, uint32_t n_src, uint32_t n_parts, uint32_t* part);

// part[i] = part of srcs[i] under `mode` (SPF_PARTITION_*, n_parts >= 1, every
// source < n_nodes); returns the rule taken
uint32_t partition_sources(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                           const uint32_t* srcs, uint32_t n_src, uint32_t n_parts, uint32_t mode,
                           uint32_t* part);

// spf_label_groups without its argument checks: the distinct advertised
// labels ascending, each with its nodes ascending (labels / grp_nodes =
// [n_nodes], grp_ptr = [n_nodes + 1], any may be NULL); returns G
uint32_t label_groups(const int32_t* node_label, uint32_t n_nodes, int32_t* labels, uint32_t* grp_ptr,
                      uint32_t* grp_nodes);

// The labels of either generation of label routes (`old_labels`, `new_labels`:
// each ascending and distinct), ascending: lab[u], and label u's group index
// in the old / new generation, mold[u] / mnew[u] (0xFFFFFFFF: not there).
struct LabelUnion {
  std::vector<uint32_t> lab, mold, mnew;
};
LabelUnion label_union(const std::vector<int32_t>& old_labels, const std::vector<int32_t>& new_labels);

}  // namespace spfi
