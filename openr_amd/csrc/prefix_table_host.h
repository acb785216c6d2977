// ============================================================================
//  prefix_table_host.h -- the prefix table of spf_mplan_prefix_routes on the
//  host, no HIP in it: the caller's CSR of prefix entries validated and
//  reduced to what the kernel reads (prefix_routes.hip), and a plain CPU
//  restatement of the per-me selection over one distance row.  Built on the
//  CPU under the sanitizers by tests/test_prefix_table_host.py.
//
//  Reference: openr/decision/Decision.cpp createRouteForPrefix :390-554,
//  selectBestRoutes :725-752, maybeFilterDrainedNodes :771-792,
//  getMinNextHopThreshold :755-768; openr/common/Util.h
//  selectBestPrefixMetrics :541-570.
// ============================================================================
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "openr_spf.h"

namespace spfi {

// One entry as the device reads it (16 bytes, one load).
//   rank    the entry's (path_preference, source_preference, -distance) tuple
//           as its dense rank among the prefix's kept entries, 0 = the least:
//           the comparison does not depend on me, so the device only takes a
//           max of ranks over the entries me reaches.  SPF_PREFIX_ALL_BEST: 0.
//   min_nh  minNexthop saturated to u32, 0 = none (values <= 0)
//   drained overloaded[node]
struct PrefixEnt {
  uint32_t node, rank, min_nh, drained;
};

// Entries under the reference's floor -- a tuple below (0, 0, 0), Util.h:544,
// 555 -- never enter a selection and are dropped here (kept with
// SPF_PREFIX_ALL_BEST, which selects every reachable entry).
struct PrefixTable {
  uint32_t n_pfx = 0;
  std::vector<uint32_t> ptr;   // [n_pfx + 1] into ent
  std::vector<PrefixEnt> ent;  // prefix p's kept entries, in the caller's order
};

// SPF_OK and *out, or SPF_E_INVALID and *err (the prefix named in it): a
// pfx_ptr that does not start at 0 or decreases, a node id >= n_nodes, the same
// node twice in one prefix, distance == INT32_MIN (its negation is no int32).
// SPF_E_UNSUPPORTED: a prefix with 2^24 entries or more (|B| has 24 bits in
// the info word).  Arrays of a table without entries may be NULL.
spf_status prefix_table_build(const uint32_t* pfx_ptr, const uint32_t* ent_node, const int32_t* ent_pp,
                              const int32_t* ent_sp, const int32_t* ent_dist, const int64_t* ent_min_nh,
                              uint32_t n_pfx, const uint8_t* overloaded, uint32_t n_nodes, bool all_best,
                              PrefixTable* out, std::string* err);

// Steps 1-5 of the selection for one me and prefix p over me's distance row
// (dist[v] == SPF_UNREACHABLE: no path), up to the next-hop walk:
//   B       the selected advertisers, in the table's order
//   best    me when me is in B0 (not with all_best), else B0's smallest id;
//           SPF_UNREACHABLE when B0 is empty
//   status  SPF_PREFIX_NONE, SPF_PREFIX_SELF, or SPF_PREFIX_ROUTE for "walk the
//           links" (the walk decides NO_NEXTHOP / MIN_NEXTHOP / ROUTE)
//   need    the largest min_nh over B (0: none)
struct PrefixChoice {
  std::vector<uint32_t> B;
  uint32_t best = SPF_UNREACHABLE, status = 0, need = 0;
};
PrefixChoice prefix_select(const PrefixTable& t, uint32_t p, uint32_t me, const uint32_t* dist,
                           bool all_best);

}  // namespace spfi
