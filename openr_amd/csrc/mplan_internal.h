// ============================================================================
//  mplan_internal.h -- the multi-device context, its plans and route snapshots
//  as multi.cpp (context, plan creation, execute, reads, graphs, enqueue
//  threads, timing) and mplan_routes.cpp (the route-database pipeline over the
//  resident pass) share them.  A plan's route state is grouped by the stage
//  that writes it -- selection tables, route records, label routes, prefix
//  routes, delta, update -- once per member (spf_mplan::Part) and once per plan.  Not part of
//  the C-ABI.
// ============================================================================
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "engine_internal.h"
#include "prefix_table_host.h"

// One generation of every me's route databases, moved out of the plan that
// materialised them (spf_mplan_route_snapshot): the pools per member, and by
// value what reads them once that plan and its graph are gone.
struct spf_route_snapshot {
  spf_mctx* m = nullptr;
  uint32_t n_nodes = 0, n_sets = 0, flags = 0;
  std::vector<uint32_t> me;                          // node id of request t
  std::vector<std::pair<uint32_t, uint32_t>> db_loc;  // request t -> (member, slot)
  std::vector<uint32_t> row_ptr;                     // the CSR rows as they were
  bool has_labels = false;
  uint32_t lr_flags = 0, lr_groups = 0;
  std::vector<int32_t> labels;                        // labels[g], ascending
  std::vector<std::pair<uint32_t, uint32_t>> lr_loc;  // request t -> (member, slot)
  struct Part {
    struct {
      spfi::DevBuf<unsigned long long> hdr, pool;
      std::vector<unsigned long long> h_base;  // per slot: its region's start in pool
    } db;  // the route records
    struct {
      spfi::DevBuf<uint32_t> owner;
      spfi::DevBuf<unsigned long long> ptr, rec;
    } lr;  // the label routes
    spfi::DevBuf<unsigned long long> key;
    uint64_t bytes = 0;  // device memory held (allocations' sizes)
  };
  std::unique_ptr<Part[]> parts;
  uint32_t n_parts = 0;
  ~spf_route_snapshot();
};

struct spf_mctx {
  std::vector<spf_ctx*> members;
  std::vector<hipStream_t> exec;  // per member: its device's execute stream (shared by repeats)
  std::string err;
  std::vector<spf_route_snapshot*> snaps;  // live route snapshots (they unlist themselves)
  ~spf_mctx() {
    while (!snaps.empty()) delete snaps.back();
    for (spf_ctx* c : members) spf_ctx_destroy(c);
  }
};

struct spf_mplan {
  using Loc = std::vector<std::pair<uint32_t, uint32_t>>;  // request t -> (member, slot)
  spf_mctx* m = nullptr;
  uint32_t n_src = 0, flags = 0, mode = 0;
  std::vector<uint32_t> srcs, owner, row;  // per request index: member, row in its plan
  struct Part {
    spf_plan* plan = nullptr;
    std::vector<uint32_t> req;  // request indices in plan order
    std::vector<uint64_t> nh_off;
    std::vector<uint32_t> words;
    spfi::DevBuf<uint32_t> dist, nh;
    spfi::DevBuf<unsigned long long> dig;
    hipGraphExec_t gexec = nullptr;
    hipGraph_t graph = nullptr;
    uint64_t g_epoch = ~0ull;  // graph epoch the captured executes belong to
    bool g_team_off = false;   // ... and the context's team switch
    std::vector<hipEvent_t> ev;  // timing: [2 * cap] start / end per execute
    // route selection over the resident pass (route_prepare): every resident
    // row's device address, the request's sets, the call's me list and the
    // outputs of spf_mplan_route_digests / spf_mplan_routes on this member's
    // device
    struct Select {
      spfi::DevBuf<unsigned long long> rowp, nhp, lh;
      spfi::DevBuf<unsigned long long> nrowp;  // every resident node's exact u8 row (u8 LFA loads), or none
      spfi::DevBuf<uint32_t> rsp, rsn, me;
      std::vector<uint32_t> h_rsp, h_rsn;  // host copies of the uploaded sets (re-upload only on change)
      std::vector<uint64_t> h_lh;
      uint64_t epoch = ~0ull;  // execute count the address tables belong to
      spfi::DevBuf<unsigned long long> dig, min, metric;
      spfi::DevBuf<uint32_t> cnt, edge;
    } sel;
    // materialised route databases (spf_mplan_route_records): per me slot
    // [n_sets] headers, its region of the record pool, reservation cursors
    struct Records {
      spfi::DevBuf<unsigned long long> hdr, pool, base;
      spfi::DevBuf<uint32_t> cnt, flags;
      std::vector<uint32_t> me, h_cnt;
      std::vector<unsigned long long> h_base;
      uint64_t tiles = 0;  // sets rounded up to whole 256-set tiles
      // the exactly sized layout (SPF_ROUTE_COMPACT): the scan's tile sums, every
      // block's first record; compact: pool / base hold that layout
      spfi::DevBuf<unsigned long long> sums, start;
      bool compact = false;
    } db;
    // node-label MPLS routes (spf_mplan_label_routes): per (me slot, label
    // group) the owner and the u64 offset of its records (CSR form), the
    // exactly sized record pool, the scan's tile sums
    struct Labels {
      spfi::DevBuf<uint32_t> owner, gptr, gnodes, me, flags;
      spfi::DevBuf<unsigned long long> ptr, rec, sums;
      std::vector<uint32_t> req;  // per me slot: its index t in the call's me list
      uint64_t records = 0;
    } lr;
    // prefix routes (spf_mplan_prefix_routes): the uploaded prefix table, per
    // (me slot, prefix) the info word and the u64 offset of its records (CSR
    // form), the exactly sized record pool, the scan's tile sums
    struct Prefixes {
      spfi::DevBuf<uint32_t> pptr, me, flags;
      spfi::DevBuf<spfi::PrefixEnt> ent;
      spfi::DevBuf<unsigned long long> info, ptr, rec, sums;
      std::vector<uint32_t> req;  // per me slot: its index t in the call's me list
      uint64_t records = 0;
    } px;
    // route-database delta (spf_mplan_route_delta): per me slot where its old
    // database lives, the kind bytes and scanned block counts of the IP ([0])
    // and label ([1]) passes, the lists
    struct Delta {
      spfi::DevBuf<unsigned long long> ohdr, opool, oown, optr, orec, key, tot;
      spfi::DevBuf<unsigned long long> blk[2], sums[2], ptr[2];
      spfi::DevBuf<uint32_t> e0, deg, same, mold, mnew, lab, set[2];
      spfi::DevBuf<uint8_t> kind[2];
      std::vector<uint32_t> req;  // per me slot: its index t in the records call's me list
      uint64_t n[2] = {0, 0};      // entries of the IP / label lists
    } dl;
    // the delta's payload (spf_mplan_route_update), parallel to dl.set[w]: the
    // records' u64 offsets, the exactly sized record pools, the new owners of
    // the label entries; src / sums: the passes' scratch
    struct Update {
      spfi::DevBuf<unsigned long long> ptr[2], rec[2], src[2], sums[2];
      spfi::DevBuf<uint32_t> owner;
      uint64_t nrec[2] = {0, 0};
    } up;
  };
  // The same stages per plan.  Selection: the address tables (host; uploads
  // read them).
  struct Select {
    std::vector<unsigned long long> h_rowp, h_nhp;
    std::vector<unsigned long long> h_nrowp;  // u8 rows, when every member's are exact (else empty)
    int peer = -1;  // 1: every member can read every other member's HBM
  } sel;
  // What the last spf_mplan_route_records was asked (a snapshot keeps it; a
  // delta checks it): node id of request t, route flags, sets, its layout
  // (SPF_ROUTE_COMPACT or tiled), and of a compact call the count / scan /
  // fill ms (slowest member each).  moved: a snapshot took the pools.
  struct Records {
    Loc loc;
    std::vector<uint32_t> nodes;
    uint32_t flags = 0, sets = 0;
    bool compact = false, moved = false;
    double ms[3] = {0, 0, 0};
  } db;
  // ... the last spf_mplan_label_routes: also its labels and groups
  struct Labels {
    Loc loc;
    std::vector<uint32_t> nodes, gptr, gnodes;
    std::vector<int32_t> labels;
    uint32_t rflags = 0, groups = 0;
    bool moved = false;
  } lr;
  // ... the last spf_mplan_prefix_routes: its prefixes, and the count / scan /
  // fill ms (slowest member each).  have: the plan holds a prefix database.
  struct Prefixes {
    Loc loc;
    bool have = false;
    uint32_t n_pfx = 0;
    double ms[3] = {0, 0, 0};
  } px;
  // The last spf_mplan_route_delta.  gen: db_gen as it was then (the update
  // resolves the delta's lists in those same databases); labels / uni / tot:
  // whether it had label routes, its label union's size, its totals.
  struct Delta {
    Loc loc;
    uint64_t gen = 0;
    bool labels = false;
    uint32_t uni = 0;
    uint64_t tot[5] = {0, 0, 0, 0, 0};
  } dl;
  // The last spf_mplan_route_update: its count / scan / fill ms (slowest member each)
  struct Update {
    bool done = false;
    double ms[3] = {0, 0, 0};
  } up;
  // db_gen counts the calls that replace or move the plan's databases
  // (spf_mplan_route_records, spf_mplan_label_routes, spf_mplan_route_snapshot)
  uint64_t db_gen = 0;
  // "the plan holds a generation of X": what the readers and the later stages ask
  bool has_records() const { return !db.loc.empty() && !db.moved; }
  bool has_label_routes() const { return !lr.loc.empty() && !lr.moved; }
  bool has_prefix_routes() const { return px.have; }
  bool has_delta() const { return !dl.loc.empty(); }
  bool has_update() const { return has_delta() && up.done; }
  std::unique_ptr<Part[]> parts;  // [n_parts]
  uint32_t n_parts = 0;
  bool graphs = false;
  uint32_t timing_cap = 0, timing_n = 0;
  uint64_t executes = 0;   // bumps on every spf_mplan_execute (route tables follow it)
  // host enqueue: per member, ns from the execute's start until its launches
  // were enqueued (the last execute; spf_mplan_enqueue_ns)
  std::vector<uint64_t> enq_ns;
  // per-member enqueue threads (spf_mplan_set_enqueue_threads): each member's
  // launches issued from its own host thread, so the last GPU does not start
  // n_members - 1 enqueues after the first
  struct Pool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<uint64_t> gen{0};
    std::atomic<uint32_t> pending{0};
    std::atomic<bool> stop{false};
    std::vector<spf_status> st;
    std::chrono::steady_clock::time_point t0;
  };
  std::unique_ptr<Pool> pool;
  int threads_mode = -1;  // -1: automatic (distinct devices), 0 off, 1 on
  void stop_pool();
  ~spf_mplan();
};

namespace spfi {

// the error text into the context (NULL: none) and g_err; returns st.  Member
// errors may come from the enqueue threads: one mutex, in multi.cpp.
spf_status mfail(spf_mctx* m, spf_status st, const char* fmt, ...);
spf_status member_fail(spf_mctx* m, uint32_t i, spf_status st);

#define M_HIP(m, expr)                                                                   \
  do {                                                                                   \
    const hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                                \
      return mfail(m, e_ == hipErrorOutOfMemory ? SPF_E_NOMEM : SPF_E_HIP, "%s: %s (%s:%d)", \
                   #expr, hipGetErrorString(e_), __FILE__, __LINE__);                     \
  } while (0)

// Streams a route call has queued work on (copies into the caller's or the
// call's own host memory): on every return, early ones too, they are drained
// before that memory goes away -- so a guard is declared after the host
// buffers its streams copy into.
struct IssuedGuard {
  spf_mctx* m;
  std::vector<uint32_t> members;
  void drain() {
    for (uint32_t r : members) {
      (void)hipSetDevice(m->members[r]->device);
      (void)hipStreamSynchronize(m->exec[r]);
    }
    members.clear();
  }
  ~IssuedGuard() { drain(); }
};

}  // namespace spfi
