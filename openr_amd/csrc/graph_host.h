// ============================================================================
//  graph_host.h -- the loaded graph's host state: the CSR as given and every
//  table derived from it (reverse edges, link slots, distinct-neighbour lists,
//  sliced-ELL columns, msbfs_kernel's slice map and twin-class quotient).
//  Plain C++ with no device in it: graph.cpp uploads what these functions
//  derive; tests/host/graph_host_check.cpp runs them on the CPU.
// ============================================================================
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "openr_spf.h"

namespace spfi {

constexpr uint32_t kInf = SPF_UNREACHABLE;
constexpr uint32_t kBigDeg = 24;  // > kBigDeg: expanded by a whole wave
constexpr int kMsThreads = 1024;
constexpr int kMsMaxOwn = 16;
constexpr uint32_t kMsMaxNodes = kMsThreads * kMsMaxOwn;  // 16384 (F: 128 KiB of LDS)
constexpr uint32_t kSliceW = 64;  // nodes per sliced-ELL slice (= wave width)
constexpr uint32_t kNoSlice = 0x03FFFFFFu;  // unused slot: its nodes (kNoSlice * 64 + lane) lie past N
constexpr uint32_t kQChunk = 8;  // columns per chunk of a quotient row

// The owned-slot counts the multi-source BFS kernels are instantiated for,
// ascending, the last one kMsMaxOwn.  This list is the only place they are
// written: ms_own's bands below and the kernels' instance tables (msbfs.hip:
// one row per entry, which the launches and the LDS-limit registration both
// walk) are generated from it.
#define SPF_MS_OWNS(X) X(1) X(2) X(4) X(8) X(10) X(12) X(16)

// owned slots per thread of msbfs_kernel for an N-node graph: the smallest
// instance that holds ceil(N / kMsThreads) slots
constexpr uint32_t ms_own(uint32_t N) {
  const uint32_t own = (N + kMsThreads - 1) / kMsThreads;
#define SPF_MS_BAND(o) \
  if (own <= o) return o;
  SPF_MS_OWNS(SPF_MS_BAND)
#undef SPF_MS_BAND
  return kMsMaxOwn;
}
#define SPF_MS_OWN_ENTRY(o) o,
constexpr uint32_t kMsOwns[] = {SPF_MS_OWNS(SPF_MS_OWN_ENTRY)};
#undef SPF_MS_OWN_ENTRY
constexpr bool ms_owns_sound() {
  constexpr uint32_t n = sizeof kMsOwns / sizeof kMsOwns[0];
  for (uint32_t i = 1; i < n; ++i)
    if (kMsOwns[i - 1] >= kMsOwns[i]) return false;
  return kMsOwns[0] >= 1 && kMsOwns[n - 1] == kMsMaxOwn;
}
static_assert(ms_owns_sound(), "SPF_MS_OWNS: ascending, ending with kMsMaxOwn");

// Does a largest metric `m` on an N-node graph leave 32-bit distances (the
// bound argued at metric_flags; what-if metric changes are held to it too)
inline bool metric_past_u32(uint32_t m, uint32_t N) {
  return (uint64_t)m * (uint64_t)N >= (uint64_t)kInf;
}

struct GraphHost {
  bool loaded = false;
  uint32_t N = 0, E = 0, pitch = 0;
  uint32_t npitch = 0;  // narrow (u8) row pitch
  bool nonpos = false;
  bool needs64 = false;  // a negative metric or max metric x N >= 2^32 - 1: u64 labels
  bool unit = false;     // every up edge has metric 1
  uint32_t max_metric = 0;
  uint32_t max_link = 0;
  uint32_t big_nodes = 0;  // nodes with degree > kBigDeg
  // live directed edges with metric <= 0, < 0, and weight == max_metric: a
  // row patch updates the metric facts from these without a graph scan
  uint64_t n_nonpos = 0, n_neg = 0, n_at_max = 0;
  uint64_t shape = 0;  // bumped by a load (CSR structure)
  uint64_t epoch = 0;  // bumped by every graph change (load or in-place patch)
  // bumped when a patch changes some node's distinct-neighbour count (a
  // plan's next-hop layout); plans of the old layout fail with SPF_E_STATE
  uint64_t layout = 0;
  uint64_t sell_ver = 0;  // bumped whenever sell_ptr / sell_col change (load, row patch)
  std::vector<uint32_t> row_ptr, col, wt, rev, link;
  std::vector<int32_t> met;  // metrics as advertised (exact kernel)
  // the two CSR slots of every link id (kInf: none), kept by row patches
  std::vector<uint32_t> link_slot;
  std::vector<uint8_t> ovl;
  std::vector<uint32_t> nb_ptr, nb_id, nb_w;  // distinct up neighbours (ascending id, min metric)
  std::vector<uint32_t> edge_nb;  // per CSR edge: its head's index among the tail's distinct neighbours
  std::vector<uint32_t> sell_ptr, sell_col;  // sliced-ELL columns (64-node slices)
  std::vector<uint32_t> sell4_ptr, sell4;    // packed u16x4 columns (uint2 entries), planes BFS
  std::vector<uint32_t> ms_smap;  // msbfs_kernel: slice of (wave, slot), balanced by width
  // msbfs_kernel's twin-class quotient (graph_host_quotient: built at the first
  // BFS launch after a load or a row patch that changed a neighbour set)
  struct Quotient {
    bool stale = true;
    uint32_t n_cls = 0, n_vrow = 0;  // classes; quotient rows in chunks of kQChunk columns
    uint64_t n_edge = 0;             // directed quotient edges
    std::vector<uint16_t> cls, tab;  // class of node; [n_vrow'] rows + [kQChunk][n_vrow'] columns
  } qt;
};

// What a graph change left for the device copy to catch up with.
struct GraphDirty {
  bool all = false;      // a load: every table
  bool changed = false;  // set_overload: the drain bits; set_metric: wt, met, nb_w
  // a row patch:
  std::vector<uint32_t> nodes;                       // the touched nodes, ascending
  std::vector<std::pair<uint32_t, uint32_t>> runs;   // their edge ranges [begin, end), merged when adjacent
  std::vector<std::pair<uint32_t, uint32_t>> rev_runs;  // rev entries changed outside `runs`: (first, count)
  bool counts = false;           // a neighbour count changed: the lists moved from nodes.front() on
  std::vector<uint32_t> slices;  // the touched sliced-ELL slices, ascending
};

// Each returns SPF_OK or a status with its message in *err.  A call that does
// not return SPF_OK leaves *g as it was (a refused load: unloaded), counters
// included; epoch is the caller's to bump once the device copy has followed.
spf_status graph_host_load(GraphHost* g, const spf_graph* in, GraphDirty* dirty, std::string* err);
spf_status graph_host_set_overload(GraphHost* g, const uint32_t* nodes, const uint8_t* overloaded,
                                   uint32_t n, GraphDirty* dirty, std::string* err);
spf_status graph_host_set_metric(GraphHost* g, const uint32_t* edges, const int32_t* metric, uint32_t n,
                                 GraphDirty* dirty, std::string* err);
spf_status graph_host_patch_rows(GraphHost* g, const uint32_t* nodes, uint32_t n, const uint32_t* col,
                                 const int32_t* metric, const uint32_t* link, GraphDirty* dirty,
                                 std::string* err);
// False-twin classes: nodes whose distinct-neighbour lists (ascending ids)
// are equal share a class; classes are numbered by their first member.
uint32_t twin_classes(uint32_t N, const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t* cls);
// The quotient tables, rebuilt when stale: true when they were (upload them).
bool graph_host_quotient(GraphHost* g);

}  // namespace spfi
