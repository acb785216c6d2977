// ============================================================================
//  multi.cpp -- several GPUs behind one C-ABI context (include/openr_spf.h,
//  "multi-device context").
//
//  Open/R's Decision is one process on one event-base thread
//  (openr/decision/Decision.cpp:1484): the LinkState it owns must reach every
//  GPU of the node from that thread, not through a process per GPU.  An
//  spf_mctx holds one engine context (spf_ctx) per listed device, each with
//  its own replica of the graph (the CSR is small and
//  replicated); an spf_mplan splits a batch of sources over the members --
//  the locality partition (a source's next hops need its neighbours' rows,
//  so a member solves its sources' neighbours too: keep that closure small)
//  or contiguous blocks -- and keeps every member's distance rows and
//  next-hop bitmaps resident in that member's HBM.  Queries
//  (spf_mplan_read / spf_mplan_preds / spf_mplan_digest) are answered by the
//  owning member: the way Decision::getDecisionRouteDb(node) for every node
//  (Decision.cpp:1480-1500) reads an all-sources pass.
//
//  Device ids may repeat (one GPU holding several members, e.g. for tests on
//  a one-GPU machine): members of one device share that device's execute
//  stream, so their executes run one after another there, exactly as they
//  would run side by side on separate GPUs.
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <numeric>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine_internal.h"

using namespace spfi;

namespace {

// a source's cost in next-hop bitmaps: its k bitmaps plus its distance rows
// (u32 + the u8 copy = 5N bytes = 40 bitmaps of N/8 bytes); the same
// constant as openr_amd/sharding.py AllSourcesLayout.ROW_COST
constexpr double kRowCost = 40.0;
constexpr uint32_t kLocalityMaxNodes = 1u << 16;

// closure sizes of a partition: per part, its sources plus their neighbours
std::vector<uint32_t> closure_sizes(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                                    const uint32_t* srcs, uint32_t n_src, const uint32_t* part,
                                    uint32_t n_parts) {
  std::vector<uint32_t> out(n_parts, 0);
  std::vector<uint32_t> mark(n_nodes, 0xFFFFFFFFu);
  for (uint32_t r = 0; r < n_parts; ++r) {
    uint32_t cnt = 0;
    auto add = [&](uint32_t x) {
      if (mark[x] != r) mark[x] = r, ++cnt;
    };
    for (uint32_t i = 0; i < n_src; ++i) {
      if (part[i] != r) continue;
      add(srcs[i]);
      for (uint32_t e = nb_ptr[srcs[i]]; e < nb_ptr[srcs[i] + 1]; ++e) add(nb_id[e]);
    }
    out[r] = cnt;
  }
  return out;
}

// contiguous blocks of the request order balanced by cost (k + kRowCost):
// block r ends at the first prefix cost above total * (r+1) / n_parts
void contiguous_parts(const uint32_t* nb_ptr, const uint32_t* srcs, uint32_t n_src,
                      uint32_t n_parts, uint32_t* part) {
  std::vector<double> cum(n_src);
  double acc = 0;
  for (uint32_t i = 0; i < n_src; ++i) {
    acc += (double)(nb_ptr[srcs[i] + 1] - nb_ptr[srcs[i]]) + kRowCost;
    cum[i] = acc;
  }
  std::vector<uint32_t> bounds(n_parts + 1, 0);
  bounds[n_parts] = n_src;
  for (uint32_t r = 1; r < n_parts; ++r)
    bounds[r] = (uint32_t)(std::upper_bound(cum.begin(), cum.end(), acc * r / n_parts) - cum.begin());
  for (uint32_t r = 0; r < n_parts; ++r)
    for (uint32_t i = bounds[r]; i < std::max(bounds[r], bounds[r + 1]); ++i) part[i] = r;
}

// One-pass streaming partition (linear deterministic greedy): sources in
// ascending (degree, position), each to the part whose closure it grows
// least among the parts whose cost stays within 3 % of the mean, ties to
// the least loaded, then the lowest part.  Low-degree nodes first: a
// fabric's rack switches gather by pod, the fabric switches follow their
// pod, a plane's spines land together.  Same rule as sharding.py
// locality_partition (tests/test_partition.py checks they agree).
void locality_parts(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                    const uint32_t* srcs, uint32_t n_src, uint32_t n_parts, uint32_t* part) {
  std::vector<uint32_t> order(n_src);
  std::iota(order.begin(), order.end(), 0u);
  auto deg = [&](uint32_t i) { return nb_ptr[srcs[i] + 1] - nb_ptr[srcs[i]]; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return deg(a) < deg(b); });
  double total = 0;
  for (uint32_t i = 0; i < n_src; ++i) total += (double)deg(i) + kRowCost;
  const double cap = total / n_parts * (1.0 + 0.03);  // sharding.py: sum / world * (1 + slack)
  std::vector<uint8_t> clo((size_t)n_parts * n_nodes, 0);
  std::vector<double> load(n_parts, 0.0);
  std::vector<double> grow(n_parts);
  for (uint32_t i : order) {
    const uint32_t v = srcs[i];
    const double cost = (double)deg(i) + kRowCost;
    bool any_ok = false;
    for (uint32_t r = 0; r < n_parts; ++r) any_ok |= load[r] + cost <= cap;
    for (uint32_t r = 0; r < n_parts; ++r) {
      if (any_ok && !(load[r] + cost <= cap)) {
        grow[r] = std::numeric_limits<double>::infinity();
        continue;
      }
      const uint8_t* c = clo.data() + (size_t)r * n_nodes;
      uint32_t g = c[v] ? 0u : 1u;
      for (uint32_t e = nb_ptr[v]; e < nb_ptr[v + 1]; ++e) g += c[nb_id[e]] ? 0u : 1u;
      grow[r] = g;
    }
    const double best = *std::min_element(grow.begin(), grow.end());
    uint32_t pick = n_parts;
    for (uint32_t r = 0; r < n_parts; ++r)
      if (grow[r] == best && (pick == n_parts || load[r] < load[pick])) pick = r;
    part[i] = pick;
    uint8_t* c = clo.data() + (size_t)pick * n_nodes;
    c[v] = 1;
    for (uint32_t e = nb_ptr[v]; e < nb_ptr[v + 1]; ++e) c[nb_id[e]] = 1;
    load[pick] += cost;
  }
}

uint32_t partition(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                   const uint32_t* srcs, uint32_t n_src, uint32_t n_parts, uint32_t mode,
                   uint32_t* part) {
  contiguous_parts(nb_ptr, srcs, n_src, n_parts, part);
  if (mode == SPF_PARTITION_CONTIGUOUS || n_parts <= 1) return SPF_PARTITION_CONTIGUOUS;
  if (mode == SPF_PARTITION_AUTO && n_nodes > kLocalityMaxNodes) return SPF_PARTITION_CONTIGUOUS;
  std::vector<uint32_t> loc(n_src);
  locality_parts(nb_ptr, nb_id, n_nodes, srcs, n_src, n_parts, loc.data());
  if (mode == SPF_PARTITION_AUTO) {
    const auto a = closure_sizes(nb_ptr, nb_id, n_nodes, srcs, n_src, part, n_parts);
    const auto b = closure_sizes(nb_ptr, nb_id, n_nodes, srcs, n_src, loc.data(), n_parts);
    if (*std::max_element(b.begin(), b.end()) >= *std::max_element(a.begin(), a.end()))
      return SPF_PARTITION_CONTIGUOUS;
  }
  std::copy(loc.begin(), loc.end(), part);
  return SPF_PARTITION_LOCALITY;
}

}  // namespace

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
    DevBuf<unsigned long long> dbhdr, dbpool, lr_ptr, lr_rec, key;
    DevBuf<uint32_t> lr_owner;
    std::vector<unsigned long long> h_dbbase;  // per slot: its region's start in dbpool
    uint64_t bytes = 0;                        // device memory held (allocations' sizes)
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

spf_route_snapshot::~spf_route_snapshot() {
  if (!m) return;
  // (a delta's kernels may still read the pools)
  for (uint32_t r = 0; r < n_parts && r < m->members.size(); ++r) {
    (void)hipSetDevice(m->members[r]->device);
    (void)hipStreamSynchronize(m->exec[r]);
  }
  m->snaps.erase(std::remove(m->snaps.begin(), m->snaps.end(), this), m->snaps.end());
}

struct spf_mplan {
  spf_mctx* m = nullptr;
  uint32_t n_src = 0, flags = 0, mode = 0;
  std::vector<uint32_t> srcs, owner, row;  // per request index: member, row in its plan
  struct Part {
    spf_plan* plan = nullptr;
    std::vector<uint32_t> req;  // request indices in plan order
    std::vector<uint64_t> nh_off;
    std::vector<uint32_t> words;
    DevBuf<uint32_t> dist, nh;
    DevBuf<unsigned long long> dig;
    hipGraphExec_t gexec = nullptr;
    hipGraph_t graph = nullptr;
    uint64_t g_epoch = ~0ull;  // graph epoch the captured executes belong to
    bool g_team_off = false;   // ... and the context's team switch
    std::vector<hipEvent_t> ev;  // timing: [2 * cap] start / end per execute
    // route selection over the resident pass (spf_mplan_route_digests /
    // spf_mplan_routes): every resident row's device address, the request's
    // sets, its me list and outputs on this member's device
    DevBuf<unsigned long long> rowp, nhp, lh, rdig, rmin, rmetric;
    DevBuf<unsigned long long> nrowp;  // every resident node's exact u8 row (u8 LFA loads), or none
    DevBuf<uint32_t> rsp, rsn, rme, rcnt, redge;
    std::vector<uint32_t> h_rsp, h_rsn;  // host copies of the uploaded sets (re-upload only on change)
    std::vector<uint64_t> h_lh;
    uint64_t r_epoch = ~0ull;  // execute count the address tables belong to
    // materialised route databases (spf_mplan_route_records): per me slot
    // [n_sets] headers, its region of the record pool, reservation cursors
    DevBuf<unsigned long long> dbhdr, dbpool, dbbase;
    DevBuf<uint32_t> dbcnt, dbflags;
    std::vector<uint32_t> db_me, h_dbcnt;
    std::vector<unsigned long long> h_dbbase;
    uint64_t db_tiles = 0;  // sets rounded up to whole 256-set tiles
    // the exactly sized layout (SPF_ROUTE_COMPACT): the scan's tile sums, every
    // block's first record; db_compact: dbpool / dbbase hold that layout
    DevBuf<unsigned long long> dbsums, dbstart;
    bool db_compact = false;
    // node-label MPLS routes (spf_mplan_label_routes): per (me slot, label
    // group) the owner and the u64 offset of its records (CSR form), the
    // exactly sized record pool, the scan's tile sums
    DevBuf<uint32_t> lr_owner, lr_gptr, lr_gnodes, lr_me, lr_flags;
    DevBuf<unsigned long long> lr_ptr, lr_rec, lr_sums;
    std::vector<uint32_t> lr_req;  // per me slot: its index t in the call's me list
    uint64_t lr_records = 0;
    // route-database delta (spf_mplan_route_delta): per me slot where its old
    // database lives, the kind bytes and scanned block counts of the IP ([0])
    // and label ([1]) passes, the lists
    DevBuf<unsigned long long> dl_ohdr, dl_opool, dl_oown, dl_optr, dl_orec, dl_key, dl_tot;
    DevBuf<unsigned long long> dl_blk[2], dl_sums[2], dl_ptr[2];
    DevBuf<uint32_t> dl_e0, dl_deg, dl_same, dl_mold, dl_mnew, dl_lab, dl_set[2];
    DevBuf<uint8_t> dl_kind[2];
    std::vector<uint32_t> dl_req;  // per me slot: its index t in the records call's me list
    uint64_t dl_n[2] = {0, 0};      // entries of the IP / label lists
    // the delta's payload (spf_mplan_route_update), parallel to dl_set[w]: the
    // records' u64 offsets, the exactly sized record pools, the new owners of
    // the label entries; up_src / up_sums: the passes' scratch
    DevBuf<unsigned long long> up_ptr[2], up_rec[2], up_src[2], up_sums[2];
    DevBuf<uint32_t> up_owner;
    uint64_t up_nrec[2] = {0, 0};
  };
  // the last spf_mplan_route_delta: request t -> (member, slot)
  std::vector<std::pair<uint32_t, uint32_t>> dl_loc;
  // db_gen counts the calls that replace or move the plan's databases
  // (spf_mplan_route_records, spf_mplan_label_routes, spf_mplan_route_snapshot);
  // dl_gen: its value at the last delta, whose lists spf_mplan_route_update
  // resolves in those same databases.  dl_labels / dl_union / dl_tot: whether
  // that delta had label routes, its label union's size, its totals.
  uint64_t db_gen = 0, dl_gen = 0;
  bool dl_labels = false, up_done = false;
  uint32_t dl_union = 0;
  uint64_t dl_tot[5] = {0, 0, 0, 0, 0};
  double up_ms[3] = {0, 0, 0};  // the last update's count / scan / fill (slowest member each)
  // what the last materialising calls were asked (a snapshot keeps them; a
  // delta checks them): node id of request t, route flags, the labels; *_moved:
  // a snapshot took the pools
  std::vector<uint32_t> db_nodes, lr_nodes;
  std::vector<int32_t> lr_labels;
  uint32_t db_flags = 0, lr_rflags = 0;
  bool db_moved = false, lr_moved = false;
  // the last spf_mplan_label_routes: request t -> (member, slot), its groups
  std::vector<std::pair<uint32_t, uint32_t>> lr_loc;
  std::vector<uint32_t> lr_gptr, lr_gnodes;
  uint32_t lr_groups = 0;
  // the last spf_mplan_route_records: request t -> (member, slot), sets
  std::vector<std::pair<uint32_t, uint32_t>> db_loc;
  uint32_t db_sets = 0;
  // ... its layout (SPF_ROUTE_COMPACT or tiled), and of a compact call the
  // count / scan / fill ms (slowest member each)
  bool db_compact = false;
  double db_ms[3] = {0, 0, 0};
  std::vector<unsigned long long> h_rowp, h_nhp;  // the address tables (host; uploads read them)
  std::vector<unsigned long long> h_nrowp;  // u8 rows, when every member's are exact (else empty)
  std::unique_ptr<Part[]> parts;  // [n_parts]
  uint32_t n_parts = 0;
  bool graphs = false;
  uint32_t timing_cap = 0, timing_n = 0;
  uint64_t executes = 0;   // bumps on every spf_mplan_execute (route tables follow it)
  int peer = -1;           // 1: every member can read every other member's HBM
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
  void stop_pool() {
    if (!pool) return;
    {
      std::lock_guard<std::mutex> lk(pool->mu);
      pool->stop = true;
    }
    pool->cv.notify_all();
    for (auto& t : pool->th) t.join();
    pool.reset();
  }
  ~spf_mplan() {
    stop_pool();
    for (size_t i = 0; i < n_parts; ++i) {
      Part& p = parts[i];
      if (!p.plan) continue;
      (void)hipSetDevice(m->members[i]->device);
      (void)hipStreamSynchronize(m->exec[i]);
      if (p.gexec) (void)hipGraphExecDestroy(p.gexec);
      if (p.graph) (void)hipGraphDestroy(p.graph);
      for (hipEvent_t e : p.ev) (void)hipEventDestroy(e);
      spf_plan_destroy(p.plan);
      p.dist.reset();
      p.nh.reset();
      p.dig.reset();
    }
  }
};

namespace {

std::mutex g_err_mu;  // member errors may come from the enqueue threads

spf_status mfail(spf_mctx* m, spf_status st, const char* fmt, ...) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (m) m->err = buf;
  g_err = buf;
  return st;
}

spf_status member_fail(spf_mctx* m, uint32_t i, spf_status st) {
  return mfail(m, st, "member %u (device %d): %s", i, m->members[i]->device,
               spf_last_error(m->members[i]));
}

#define M_HIP(m, expr)                                                                   \
  do {                                                                                   \
    const hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                                \
      return mfail(m, e_ == hipErrorOutOfMemory ? SPF_E_NOMEM : SPF_E_HIP, "%s: %s (%s:%d)", \
                   #expr, hipGetErrorString(e_), __FILE__, __LINE__);                     \
  } while (0)

// One member's execute on its device's stream: a replay of the captured
// graph when one matches the member's graph epoch, else the plan's execute
// (which re-derives the plan after an in-place patch) -- captured then for
// the next call when graphs are on.
spf_status run_part(spf_mplan* mp, uint32_t i) {
  spf_mctx* m = mp->m;
  spf_ctx* c = m->members[i];
  spf_mplan::Part& p = mp->parts[i];
  const hipStream_t s = m->exec[i];
  M_HIP(m, hipSetDevice(c->device));
  hipEvent_t* ev = nullptr;
  if (mp->timing_cap) {
    ev = &p.ev[2 * (mp->timing_n % mp->timing_cap)];
    M_HIP(m, hipEventRecord(ev[0], s));
  }
  // (a capture made before a team timeout turned teams off is stale too)
  if (p.gexec && p.g_epoch == spf_graph_epoch(c) && p.g_team_off == c->team_off) {
    // A replay bypasses the plan's own resident_order / resident_done (they
    // skip a capturing stream): a plan with grid-resident launches (team BFS,
    // big-graph kernel) orders the replay itself, so it never splits the CUs
    // with another context's resident launch on this device.
    const bool resident = p.plan->tm_G || p.plan->big;
    if (resident) {
      const spf_status st = resident_order(c, s);
      if (st != SPF_OK) return member_fail(m, i, st);
    }
    M_HIP(m, hipGraphLaunch(p.gexec, s));
    if (resident) {
      const spf_status st = resident_done(c, s);
      if (st != SPF_OK) return member_fail(m, i, st);
    }
  } else {
    if (p.gexec) {
      (void)hipGraphExecDestroy(p.gexec);
      (void)hipGraphDestroy(p.graph);
      p.gexec = nullptr;
      p.graph = nullptr;
    }
    // A re-derive (graph patched, teams turned off) rebuilds the plan's
    // tables on the member's own stream; a member whose execute runs on a
    // shared stream (repeated device id) waits for what is in flight there
    // first, so the rebuild never overwrites tables a queued kernel reads.
    if (s != c->stream && (p.plan->epoch != c->epoch || (p.plan->tm_G && c->team_off)))
      M_HIP(m, hipStreamSynchronize(s));
    spf_status st = spf_plan_execute(p.plan, p.dist.p, p.nh.p, s);
    if (st != SPF_OK) return member_fail(m, i, st);
    if (mp->graphs) {  // the plan is derived for this epoch now: capture its launches
      M_HIP(m, hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
      st = spf_plan_execute(p.plan, p.dist.p, p.nh.p, s);
      hipGraph_t g = nullptr;
      const hipError_t e = hipStreamEndCapture(s, &g);
      if (st != SPF_OK) {
        if (g) (void)hipGraphDestroy(g);
        return member_fail(m, i, st);
      }
      M_HIP(m, e);
      M_HIP(m, hipGraphInstantiate(&p.gexec, g, nullptr, nullptr, 0));
      p.graph = g;
      p.g_epoch = spf_graph_epoch(c);
      p.g_team_off = c->team_off;
    }
  }
  if (ev) M_HIP(m, hipEventRecord(ev[1], s));
  return SPF_OK;
}

}  // namespace

extern "C" {

spf_status spf_partition_sources(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                                 const uint32_t* srcs, uint32_t n_src, uint32_t n_parts,
                                 uint32_t mode, uint32_t* part_out, uint32_t* mode_used) {
  if (!nb_ptr || (n_src && (!srcs || !part_out)) || n_parts == 0 || mode > SPF_PARTITION_LOCALITY)
    return mfail(nullptr, SPF_E_INVALID, "spf_partition_sources: bad argument");
  if (nb_ptr[n_nodes] && !nb_id) return mfail(nullptr, SPF_E_INVALID, "spf_partition_sources: nb_id NULL");
  for (uint32_t i = 0; i < n_src; ++i)
    if (srcs[i] >= n_nodes) return mfail(nullptr, SPF_E_INVALID, "source %u out of range", srcs[i]);
  const uint32_t used = partition(nb_ptr, nb_id, n_nodes, srcs, n_src, n_parts, mode, part_out);
  if (mode_used) *mode_used = used;
  return SPF_OK;
}

spf_status spf_label_groups(const int32_t* node_label, uint32_t n_nodes, int32_t* labels,
                            uint32_t* grp_ptr, uint32_t* grp_nodes, uint32_t* n_groups) {
  if ((n_nodes && !node_label) || !n_groups)
    return mfail(nullptr, SPF_E_INVALID, "spf_label_groups: NULL argument");
  // buildRouteDb (Decision.cpp:592-603): label 0 = none advertised, a label
  // outside the 20-bit space (isMplsLabelValid) is skipped
  std::vector<std::pair<int32_t, uint32_t>> adv;
  for (uint32_t v = 0; v < n_nodes; ++v)
    if (node_label[v] > 0 && node_label[v] <= (1 << 20) - 1) adv.emplace_back(node_label[v], v);
  std::sort(adv.begin(), adv.end());
  uint32_t g = 0;
  for (size_t i = 0; i < adv.size(); ++i) {
    if (i == 0 || adv[i].first != adv[i - 1].first) {
      if (labels) labels[g] = adv[i].first;
      if (grp_ptr) grp_ptr[g] = (uint32_t)i;
      ++g;
    }
    if (grp_nodes) grp_nodes[i] = adv[i].second;
  }
  if (grp_ptr) grp_ptr[g] = (uint32_t)adv.size();
  *n_groups = g;
  return SPF_OK;
}

spf_status spf_mctx_create(const int* gpu_ids, uint32_t n, spf_mctx** out) {
  if (!out || !gpu_ids || n == 0) return mfail(nullptr, SPF_E_INVALID, "spf_mctx_create: bad argument");
  *out = nullptr;
  auto m = std::make_unique<spf_mctx>();
  std::map<int, hipStream_t> dev_stream;
  for (uint32_t i = 0; i < n; ++i) {
    spf_ctx* c = nullptr;
    const spf_status st = spf_ctx_create(gpu_ids[i], &c);
    if (st != SPF_OK) return mfail(nullptr, st, "member %u: %s", i, spf_global_error());
    m->members.push_back(c);
    auto it = dev_stream.find(gpu_ids[i]);
    if (it == dev_stream.end()) it = dev_stream.emplace(gpu_ids[i], c->stream).first;
    m->exec.push_back(it->second);
  }
  *out = m.release();
  return SPF_OK;
}

void spf_mctx_destroy(spf_mctx* m) { delete m; }
const char* spf_mctx_last_error(const spf_mctx* m) { return m ? m->err.c_str() : g_err.c_str(); }
uint32_t spf_mctx_size(const spf_mctx* m) { return m ? (uint32_t)m->members.size() : 0; }
spf_ctx* spf_mctx_member(spf_mctx* m, uint32_t i) {
  return m && i < m->members.size() ? m->members[i] : nullptr;
}
int spf_mctx_device(const spf_mctx* m, uint32_t i) {
  return m && i < m->members.size() ? m->members[i]->device : -1;
}

// Patches upload on each member's own stream, while a member of a repeated
// device id executes on that device's shared stream: wait for every execute
// stream first, so a patch never rewrites the drain bytes / metrics a queued
// execute still reads (spf_mplan_execute returns before its kernels run).
static spf_status drain_exec(spf_mctx* m) {
  for (uint32_t i = 0; i < m->members.size(); ++i) {
    M_HIP(m, hipSetDevice(m->members[i]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[i]));
  }
  return SPF_OK;
}

spf_status spf_mctx_graph_load(spf_mctx* m, const spf_graph* g) {
  if (!m || !g) return mfail(m, SPF_E_INVALID, "spf_mctx_graph_load: NULL argument");
  if (const spf_status st = drain_exec(m); st != SPF_OK) return st;
  for (uint32_t i = 0; i < m->members.size(); ++i) {
    const spf_status st = spf_graph_load(m->members[i], g);
    if (st != SPF_OK) return member_fail(m, i, st);
  }
  return SPF_OK;
}

spf_status spf_mctx_graph_set_overload(spf_mctx* m, const uint32_t* nodes, const uint8_t* overloaded,
                                       uint32_t n) {
  if (!m) return mfail(m, SPF_E_INVALID, "spf_mctx_graph_set_overload: NULL context");
  if (const spf_status st = drain_exec(m); st != SPF_OK) return st;
  for (uint32_t i = 0; i < m->members.size(); ++i) {
    const spf_status st = spf_graph_set_overload(m->members[i], nodes, overloaded, n);
    if (st != SPF_OK) return member_fail(m, i, st);
  }
  return SPF_OK;
}

spf_status spf_mctx_graph_set_metric(spf_mctx* m, const uint32_t* edges, const int32_t* metric,
                                     uint32_t n) {
  if (!m) return mfail(m, SPF_E_INVALID, "spf_mctx_graph_set_metric: NULL context");
  if (const spf_status st = drain_exec(m); st != SPF_OK) return st;
  for (uint32_t i = 0; i < m->members.size(); ++i) {
    const spf_status st = spf_graph_set_metric(m->members[i], edges, metric, n);
    if (st != SPF_OK) return member_fail(m, i, st);
  }
  return SPF_OK;
}

spf_status spf_mctx_graph_patch_rows(spf_mctx* m, const uint32_t* nodes, uint32_t n,
                                     const uint32_t* col, const int32_t* metric, const uint32_t* link) {
  if (!m) return mfail(m, SPF_E_INVALID, "spf_mctx_graph_patch_rows: NULL context");
  if (const spf_status st = drain_exec(m); st != SPF_OK) return st;
  // every member holds the same graph (spf_mplan_create relies on it) and a
  // member refuses a patch before it changes anything: what member 0 refuses
  // has changed no member
  for (uint32_t i = 0; i < m->members.size(); ++i) {
    const spf_status st = spf_graph_patch_rows(m->members[i], nodes, n, col, metric, link);
    if (st != SPF_OK) return member_fail(m, i, st);
  }
  return SPF_OK;
}

spf_status spf_mplan_create(spf_mctx* m, const uint32_t* srcs, uint32_t n_src, uint32_t flags,
                            uint32_t mode, spf_mplan** out) {
  if (!m || !out || !srcs || n_src == 0 || mode > SPF_PARTITION_LOCALITY)
    return mfail(m, SPF_E_INVALID, "spf_mplan_create: bad argument");
  *out = nullptr;
  spf_ctx* c0 = m->members[0];
  for (spf_ctx* c : m->members)
    if (!c->loaded || c->shape == 0 || c->N != c0->N)
      return mfail(m, SPF_E_STATE, "spf_mplan_create: load the graph with spf_mctx_graph_load first");
  for (uint32_t i = 0; i < n_src; ++i)
    if (srcs[i] >= c0->N) return mfail(m, SPF_E_INVALID, "source %u out of range", srcs[i]);
  const uint32_t P = (uint32_t)m->members.size();
  auto mp = std::make_unique<spf_mplan>();
  mp->m = m;
  mp->n_src = n_src;
  mp->flags = flags;
  mp->srcs.assign(srcs, srcs + n_src);
  mp->owner.resize(n_src);
  mp->row.resize(n_src);
  mp->mode = partition(c0->nb_ptr.data(), c0->nb_id.data(), c0->N, srcs, n_src, P, mode,
                       mp->owner.data());
  mp->parts.reset(new spf_mplan::Part[P]);
  mp->n_parts = P;
  for (uint32_t i = 0; i < n_src; ++i) {
    spf_mplan::Part& p = mp->parts[mp->owner[i]];
    mp->row[i] = (uint32_t)p.req.size();
    p.req.push_back(i);
  }
  const uint32_t pitch = c0->pitch;
  const size_t lab = (flags & SPF_FLAG_DIST64) ? 2 : 1;
  for (uint32_t r = 0; r < P; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (p.req.empty()) continue;
    spf_ctx* c = m->members[r];
    std::vector<uint32_t> ps(p.req.size());
    for (size_t t = 0; t < ps.size(); ++t) ps[t] = srcs[p.req[t]];
    spf_status st = spf_plan_create(c, ps.data(), (uint32_t)ps.size(), flags, &p.plan);
    if (st != SPF_OK) return member_fail(m, r, st);
    p.nh_off.resize(ps.size());
    p.words.resize(ps.size());
    spf_plan_nh_layout(p.plan, p.nh_off.data(), p.words.data());
    M_HIP(m, hipSetDevice(c->device));
    M_HIP(m, p.dist.alloc(ps.size() * pitch * lab));
    M_HIP(m, p.nh.alloc(std::max<uint64_t>(spf_plan_nh_words(p.plan), 1)));
    M_HIP(m, p.dig.alloc(ps.size()));
  }
  *out = mp.release();
  return SPF_OK;
}

void spf_mplan_destroy(spf_mplan* mp) { delete mp; }

uint32_t spf_mplan_partition(const spf_mplan* mp) { return mp ? mp->mode : 0; }

spf_status spf_mplan_owner(const spf_mplan* mp, uint32_t i, uint32_t* member, uint32_t* row) {
  if (!mp || i >= mp->n_src) return SPF_E_INVALID;
  if (member) *member = mp->owner[i];
  if (row) *row = mp->row[i];
  return SPF_OK;
}

spf_status spf_mplan_shard(spf_mplan* mp, uint32_t member, uint32_t* n_src, spf_plan** plan,
                           void** d_dist, uint32_t** d_nh) {
  if (!mp || member >= mp->n_parts) return SPF_E_INVALID;
  spf_mplan::Part& p = mp->parts[member];
  if (n_src) *n_src = (uint32_t)p.req.size();
  if (plan) *plan = p.plan;
  if (d_dist) *d_dist = p.dist.p;
  if (d_nh) *d_nh = p.nh.p;
  return SPF_OK;
}

spf_status spf_mplan_set_graphs(spf_mplan* mp, int enable) {
  if (!mp) return SPF_E_INVALID;
  mp->graphs = enable != 0;
  return SPF_OK;
}

namespace {

// enqueue threads wanted: on when asked, or -- automatically -- when the
// members with work sit on two or more distinct devices (members of one
// device share its stream: nothing to overlap)
bool want_threads(const spf_mplan* mp) {
  if (mp->threads_mode >= 0) return mp->threads_mode == 1;
  std::vector<int> devs;
  for (uint32_t i = 0; i < mp->n_parts; ++i)
    if (mp->parts[i].plan) devs.push_back(mp->m->members[i]->device);
  std::sort(devs.begin(), devs.end());
  return std::unique(devs.begin(), devs.end()) - devs.begin() > 1;
}

void enqueue_worker(spf_mplan* mp, uint32_t i) {
  spf_mplan::Pool& P = *mp->pool;
  uint64_t seen = 0;
  for (;;) {
    // spin briefly (back-to-back executes), then sleep until the next one
    uint64_t g = P.gen.load(std::memory_order_acquire);
    for (int k = 0; g == seen && k < 20000 && !P.stop.load(std::memory_order_relaxed); ++k) {
      __builtin_ia32_pause();
      g = P.gen.load(std::memory_order_acquire);
    }
    if (g == seen) {
      std::unique_lock<std::mutex> lk(P.mu);
      P.cv.wait(lk, [&] { return P.stop || P.gen.load(std::memory_order_acquire) != seen; });
      if (P.stop) return;
      g = P.gen.load(std::memory_order_acquire);
    }
    if (P.stop) return;
    seen = g;
    if (mp->parts[i].plan) {
      P.st[i] = run_part(mp, i);
      mp->enq_ns[i] = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now() - P.t0).count();
    }
    P.pending.fetch_sub(1, std::memory_order_acq_rel);
  }
}

}  // namespace

spf_status spf_mplan_set_enqueue_threads(spf_mplan* mp, int mode) {
  if (!mp || mode < -1 || mode > 1) return SPF_E_INVALID;
  mp->threads_mode = mode;
  if (!want_threads(mp)) mp->stop_pool();
  return SPF_OK;
}

spf_status spf_mplan_enqueue_ns(const spf_mplan* mp, uint64_t* out, uint32_t n, int* threaded) {
  if (!mp || (n && !out)) return SPF_E_INVALID;
  for (uint32_t i = 0; i < n && i < mp->n_parts; ++i) out[i] = i < mp->enq_ns.size() ? mp->enq_ns[i] : 0;
  if (threaded) *threaded = mp->pool ? 1 : 0;
  return SPF_OK;
}

spf_status spf_mplan_execute(spf_mplan* mp) {
  if (!mp) return mfail(nullptr, SPF_E_INVALID, "spf_mplan_execute: NULL plan");
  mp->enq_ns.assign(mp->n_parts, 0);
  const auto t0 = std::chrono::steady_clock::now();
  if (want_threads(mp)) {
    if (!mp->pool) {
      mp->pool = std::make_unique<spf_mplan::Pool>();
      mp->pool->st.assign(mp->n_parts, SPF_OK);
      for (uint32_t i = 0; i < mp->n_parts; ++i) mp->pool->th.emplace_back(enqueue_worker, mp, i);
    }
    spf_mplan::Pool& P = *mp->pool;
    P.t0 = t0;
    P.pending.store(mp->n_parts, std::memory_order_release);
    {
      std::lock_guard<std::mutex> lk(P.mu);
      P.gen.fetch_add(1, std::memory_order_acq_rel);
    }
    P.cv.notify_all();
    while (P.pending.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
    for (uint32_t i = 0; i < mp->n_parts; ++i)
      if (P.st[i] != SPF_OK) return P.st[i];
  } else {
    for (uint32_t i = 0; i < mp->n_parts; ++i) {
      if (!mp->parts[i].plan) continue;
      const spf_status st = run_part(mp, i);
      if (st != SPF_OK) return st;
      mp->enq_ns[i] = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now() - t0).count();
    }
  }
  if (mp->timing_cap) ++mp->timing_n;
  ++mp->executes;
  return SPF_OK;
}

spf_status spf_mplan_synchronize(spf_mplan* mp) {
  if (!mp) return mfail(nullptr, SPF_E_INVALID, "spf_mplan_synchronize: NULL plan");
  spf_mctx* m = mp->m;
  for (uint32_t i = 0; i < mp->n_parts; ++i) {
    if (!mp->parts[i].plan) continue;
    M_HIP(m, hipSetDevice(m->members[i]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[i]));
    const spf_status st = spf_device_check(m->members[i]);
    if (st != SPF_OK) return member_fail(m, i, st);
  }
  return SPF_OK;
}

spf_status spf_mplan_digest(spf_mplan* mp, uint64_t* out) {
  if (!mp || !out) return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_digest: NULL argument");
  spf_mctx* m = mp->m;
  std::vector<std::vector<uint64_t>> h(mp->n_parts);
  for (uint32_t i = 0; i < mp->n_parts; ++i) {
    spf_mplan::Part& p = mp->parts[i];
    if (!p.plan) continue;
    M_HIP(m, hipSetDevice(m->members[i]->device));
    spf_status st = spf_plan_digest(p.plan, p.dist.p, p.nh.p, reinterpret_cast<uint64_t*>(p.dig.p),
                                    m->exec[i]);
    if (st != SPF_OK) return member_fail(m, i, st);
    h[i].resize(p.req.size());
    M_HIP(m, hipMemcpyAsync(h[i].data(), p.dig.p, 8 * p.req.size(), hipMemcpyDeviceToHost, m->exec[i]));
  }
  const spf_status st = spf_mplan_synchronize(mp);
  if (st != SPF_OK) return st;
  for (uint32_t i = 0; i < mp->n_parts; ++i)
    for (size_t t = 0; t < mp->parts[i].req.size(); ++t) out[mp->parts[i].req[t]] = h[i][t];
  return SPF_OK;
}

spf_status spf_mplan_read(spf_mplan* mp, uint32_t i, void* dist, uint32_t* nh) {
  if (!mp || i >= mp->n_src) return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_read: bad argument");
  spf_mctx* m = mp->m;
  const uint32_t r = mp->owner[i], row = mp->row[i];
  spf_mplan::Part& p = mp->parts[r];
  spf_ctx* c = m->members[r];
  const size_t lab = (mp->flags & SPF_FLAG_DIST64) ? 8 : 4;
  M_HIP(m, hipSetDevice(c->device));
  if (dist)
    M_HIP(m, hipMemcpyAsync(dist, reinterpret_cast<const uint8_t*>(p.dist.p) + (size_t)row * c->pitch * lab,
                            (size_t)c->N * lab, hipMemcpyDeviceToHost, m->exec[r]));
  const uint64_t words = (uint64_t)p.words[row] * (c->pitch / 32);
  if (nh && words)
    M_HIP(m, hipMemcpyAsync(nh, p.nh.p + p.nh_off[row], 4 * words, hipMemcpyDeviceToHost, m->exec[r]));
  M_HIP(m, hipStreamSynchronize(m->exec[r]));
  return SPF_OK;
}

spf_status spf_mplan_preds(spf_mplan* mp, uint32_t i, uint32_t* pred_ptr, uint32_t* pred_edge,
                           uint32_t cap, uint32_t* n_preds) {
  if (!mp || i >= mp->n_src || !pred_ptr || !n_preds)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_preds: bad argument");
  spf_mctx* m = mp->m;
  const uint32_t r = mp->owner[i];
  spf_ctx* c = m->members[r];
  const bool hop = (mp->flags & SPF_FLAG_HOP_COUNT) != 0;
  if ((mp->flags & SPF_FLAG_DIST64) || (!hop && c->nonpos))
    return mfail(m, SPF_E_UNSUPPORTED, "spf_mplan_preds: zero / negative metrics and u64 rows "
                                       "order pathLinks by pop rank (spf_solve_exact)");
  const uint32_t* d_row = mp->parts[r].dist.p + (size_t)mp->row[i] * c->pitch;
  const spf_status st = preds_from_row(c, mp->srcs[i], hop, nullptr, d_row, pred_ptr, pred_edge,
                                       cap, n_preds, m->exec[r]);
  return st == SPF_OK ? SPF_OK : member_fail(m, r, st);
}

// ---- route selection over the resident pass ------------------------------
namespace {

// Every member's table of each resident row's (and bitmap set's) device
// address, plus the sets, on that member's device.  Rows of another device
// are read through peer access (xGMI): enabled here once, required for LFA
// (neighbours' rows) when the members span devices.
// Streams a route call has queued work on (copies into the caller's or the
// call's own host memory, timing events): on any early return they are
// drained and the events destroyed before that memory goes away.
struct IssuedGuard {
  spf_mctx* m;
  std::vector<uint32_t> members;
  std::vector<hipEvent_t>* ev = nullptr;
  ~IssuedGuard() {
    for (uint32_t r : members) {
      (void)hipSetDevice(m->members[r]->device);
      (void)hipStreamSynchronize(m->exec[r]);
    }
    if (ev)
      for (hipEvent_t e : *ev)
        if (e) (void)hipEventDestroy(e);
  }
};

spf_status route_prepare(spf_mplan* mp, const uint32_t* set_ptr, const uint32_t* set_nodes,
                         uint32_t n_sets, bool lfa, const uint64_t* link_hash, uint32_t n_links,
                         const uint32_t* me_req, uint32_t n_me) {
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  const uint32_t N = c0->N;
  if (mp->flags & SPF_FLAG_DIST64)
    return mfail(m, SPF_E_UNSUPPORTED, "route selection reads u32 rows (SPF_FLAG_DIST64 plan)");
  if (mp->flags & SPF_FLAG_HOP_COUNT)
    return mfail(m, SPF_E_UNSUPPORTED, "route selection needs link-metric rows (useLinkMetric)");
  // (set_ptr NULL: a call without destination sets -- spf_mplan_label_routes
  // brings its label groups itself and leaves the uploaded sets alone)
  for (uint32_t i = 0; set_ptr && i < set_ptr[n_sets]; ++i)
    if (set_nodes[i] >= N) return mfail(m, SPF_E_INVALID, "set member %u out of range", set_nodes[i]);
  if (mp->peer < 0) {
    mp->peer = 1;
    for (uint32_t a = 0; a < mp->n_parts; ++a)
      for (uint32_t b = 0; b < mp->n_parts; ++b) {
        const int da = m->members[a]->device, db = m->members[b]->device;
        if (da == db) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, da, db) != hipSuccess || !can) {
          mp->peer = 0;
          continue;
        }
        M_HIP(m, hipSetDevice(da));
        const hipError_t e = hipDeviceEnablePeerAccess(db, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) mp->peer = 0;
        (void)hipGetLastError();
      }
  }
  bool stale = false;
  for (uint32_t r = 0; r < mp->n_parts; ++r) stale |= mp->parts[r].plan && mp->parts[r].r_epoch != mp->executes;
  std::vector<unsigned long long>& rowp = mp->h_rowp;
  std::vector<unsigned long long>& nhp = mp->h_nhp;
  std::vector<int> dev_of(N, -1);
  if (stale) {  // no upload of the old tables may still be reading them
    for (uint32_t r = 0; r < mp->n_parts; ++r)
      if (mp->parts[r].plan) {
        M_HIP(m, hipSetDevice(m->members[r]->device));
        M_HIP(m, hipStreamSynchronize(m->exec[r]));
      }
    rowp.assign(N, 0);
    nhp.assign(N, 0);
    // the members' u8 row copies (the BFS's narrow rows, closure order) are
    // exact distances when every metric is 1 and no row reached 254: the
    // records kernel's LFA then loads 4 bytes for 4 destinations instead of
    // 16 (it is bound by HBM bytes: 3.94 -> 3.77 ms on fabric_full,
    // profiles/r06_routes/u8lfa).  SPF_ROUTE_U8=0: u32 loads (A/B)
    mp->h_nrowp.clear();
    const char* ue = std::getenv("SPF_ROUTE_U8");
    bool u8 = c0->unit && !(ue && ue[0] == '0');
    for (uint32_t r = 0; r < mp->n_parts && u8; ++r) {
      const spf_plan* pl = mp->parts[r].plan;
      if (!pl) continue;
      u8 = pl->narrow && pl->sliced && !pl->sdirect && !pl->expand && plan_has_narrow(pl) && pl->d_maxd.p;
      if (!u8) break;
      uint32_t md = ~0u;
      M_HIP(m, hipSetDevice(m->members[r]->device));
      M_HIP(m, hipMemcpy(&md, pl->d_maxd.p, 4, hipMemcpyDeviceToHost));
      u8 = md < 254;
    }
    if (u8) {
      mp->h_nrowp.assign(N, 0);
      for (uint32_t r = 0; r < mp->n_parts; ++r) {
        spf_plan* pl = mp->parts[r].plan;
        if (!pl) continue;
        // (class plans fill their u8 rows on the first request)
        M_HIP(m, hipSetDevice(m->members[r]->device));
        if (plan_ensure_narrow(pl, m->exec[r]) != SPF_OK)
          return mfail(m, SPF_E_HIP, "%s", spf_last_error(m->members[r]));
        M_HIP(m, hipStreamSynchronize(m->exec[r]));
        const uint32_t np = m->members[r]->npitch;
        for (size_t ci = 0; ci < pl->closure.size(); ++ci)
          mp->h_nrowp[pl->closure[ci]] = (unsigned long long)(uintptr_t)(pl->d_Dn.p + ci * np);
      }
    }
  }
  for (uint32_t i = 0; i < mp->n_src; ++i) {
    const uint32_t v = mp->srcs[i], r = mp->owner[i], row = mp->row[i];
    const spf_mplan::Part& p = mp->parts[r];
    if (stale) {
      rowp[v] = (unsigned long long)(uintptr_t)(p.dist.p + (size_t)row * c0->pitch);
      nhp[v] = (unsigned long long)(uintptr_t)(p.nh.p + p.nh_off[row]);
    }
    dev_of[v] = m->members[r]->device;
  }
  if (lfa) {
    // LFA reads every neighbour's row: a partial plan without one of them
    // would silently drop that neighbour's LFA candidates
    for (uint32_t t = 0; t < n_me; ++t) {
      const uint32_t v = mp->srcs[me_req[t]];
      for (uint32_t e = c0->nb_ptr[v]; e < c0->nb_ptr[v + 1]; ++e)
        if (!rowp[c0->nb_id[e]])
          return mfail(m, SPF_E_UNSUPPORTED,
                       "LFA route selection for node %u needs its neighbour %u resident in the plan",
                       v, c0->nb_id[e]);
    }
  }
  if (lfa && !mp->peer) {
    // members on distinct devices without peer access: every neighbour of a
    // member's me must then live on that member's device
    for (uint32_t i = 0; i < mp->n_src; ++i) {
      const uint32_t v = mp->srcs[i];
      for (uint32_t e = c0->nb_ptr[v]; e < c0->nb_ptr[v + 1]; ++e)
        if (dev_of[c0->nb_id[e]] != dev_of[v])
          return mfail(m, SPF_E_UNSUPPORTED, "LFA route selection across devices needs peer access");
    }
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (!p.plan) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    if (p.r_epoch != mp->executes) {
      M_HIP(m, p.rowp.upload(rowp.data(), N, s));
      M_HIP(m, p.nhp.upload(nhp.data(), N, s));
      if (!mp->h_nrowp.empty()) M_HIP(m, p.nrowp.upload(mp->h_nrowp.data(), N, s));
      p.r_epoch = mp->executes;
    }
    if (!set_ptr) continue;
    // the sets and link hashes of a call are usually the previous call's
    // (every route build of a node list): uploaded only when they changed
    const uint32_t n_mem = std::max<uint32_t>(1, set_ptr[n_sets]);
    auto same = [](const auto& v, const auto* x, size_t n) {
      return v.size() == n && std::equal(v.begin(), v.end(), x);
    };
    const bool up = !same(p.h_rsp, set_ptr, n_sets + 1) || !same(p.h_rsn, set_nodes, n_mem) ||
                    (link_hash && !same(p.h_lh, link_hash, std::max<uint32_t>(1, n_links)));
    if (up) M_HIP(m, hipStreamSynchronize(s));  // no upload still reads the host copies
    if (!same(p.h_rsp, set_ptr, n_sets + 1)) {
      p.h_rsp.assign(set_ptr, set_ptr + n_sets + 1);
      M_HIP(m, p.rsp.upload(p.h_rsp.data(), n_sets + 1, s));
    }
    if (!same(p.h_rsn, set_nodes, n_mem)) {
      p.h_rsn.assign(set_nodes, set_nodes + n_mem);
      M_HIP(m, p.rsn.upload(p.h_rsn.data(), n_mem, s));
    }
    if (link_hash && !same(p.h_lh, link_hash, std::max<uint32_t>(1, n_links))) {
      p.h_lh.assign(link_hash, link_hash + std::max<uint32_t>(1, n_links));
      M_HIP(m, p.lh.upload(reinterpret_cast<const unsigned long long*>(p.h_lh.data()), p.h_lh.size(), s));
    }
    // (uploads read the host copies, which outlive the call)
  }
  return SPF_OK;
}

}  // namespace

spf_status spf_mplan_route_digests(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* set_ptr, const uint32_t* set_nodes, uint32_t n_sets,
                                   uint32_t flags, const uint64_t* link_hash, uint32_t n_links,
                                   uint64_t* digests, double* kernel_ms) {
  if (!mp || (n_me && (!me_req || !digests)) || !set_ptr || !link_hash)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_digests: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  for (uint32_t t = 0; t < n_me; ++t)
    if (me_req[t] >= mp->n_src) return mfail(m, SPF_E_INVALID, "me %u is not a request index", me_req[t]);
  for (uint32_t e = 0; e < c0->E; ++e)
    if (c0->link[e] >= n_links) return mfail(m, SPF_E_INVALID, "link_hash shorter than the link ids");
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0;
  if (const spf_status st = route_prepare(mp, set_ptr, set_nodes, n_sets, lfa, link_hash, n_links,
                                         me_req, n_me);
      st != SPF_OK)
    return st;
  std::vector<std::vector<uint32_t>> mine(mp->n_parts), slot(mp->n_parts);
  for (uint32_t t = 0; t < n_me; ++t) {
    const uint32_t r = mp->owner[me_req[t]];
    mine[r].push_back(mp->srcs[me_req[t]]);
    slot[r].push_back(t);
  }
  std::vector<hipEvent_t> ev(2 * mp->n_parts, nullptr);
  std::vector<std::vector<uint64_t>> got(mp->n_parts);
  IssuedGuard guard{m, {}, &ev};  // declared after got: drains before got is freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    guard.members.push_back(r);
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)mine[r].size();
    M_HIP(m, p.rme.upload(mine[r].data(), n, s));
    M_HIP(m, p.rdig.alloc(n));
    M_HIP(m, hipMemsetAsync(p.rdig.p, 0, 8ull * n, s));
    if (kernel_ms) {
      M_HIP(m, hipEventCreate(&ev[2 * r]));
      M_HIP(m, hipEventCreate(&ev[2 * r + 1]));
      M_HIP(m, hipEventRecord(ev[2 * r], s));
    }
    const spf_status st = launch_route_sets(c, p.rowp.p, p.nhp.p, p.rme.p, n, p.rsp.p, p.rsn.p, n_sets,
                                            lfa, p.lh.p, p.rdig.p, nullptr, nullptr, nullptr, nullptr, s);
    // (u8 LFA loads only for the records kernel: the digest kernel is
    // VALU-bound and the byte unpacking made it slower, 2.33 -> 2.42 ms)
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[2 * r + 1], s));
    got[r].resize(n);
    M_HIP(m, hipMemcpyAsync(got[r].data(), p.rdig.p, 8ull * n, hipMemcpyDeviceToHost, s));
  }
  double worst = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    if (kernel_ms) {
      float t = 0;
      M_HIP(m, hipEventElapsedTime(&t, ev[2 * r], ev[2 * r + 1]));
      worst = std::max(worst, (double)t);
    }
    for (size_t q = 0; q < got[r].size(); ++q) digests[slot[r][q]] = got[r][q];
  }
  if (kernel_ms) *kernel_ms = worst;
  return SPF_OK;
}

// spf_mplan_route_records with SPF_ROUTE_COMPACT, after its checks and
// route_prepare: mine[r] = member r's me (node ids, slot order).  Per member a
// count walk, the scan of the counts and every block's start, then -- the
// pool allocated from the scan's total in between, on the host -- the fill
// walk (routes.hip kRsCount / kRsFill).  Nothing here is sized by tiles x deg.
static spf_status route_records_compact(spf_mplan* mp, const std::vector<std::vector<uint32_t>>& mine,
                                        uint32_t n_sets, bool lfa, uint64_t* n_records,
                                        double* kernel_ms) {
  spf_mctx* m = mp->m;
  const uint32_t ts = route_db_tile_sets();
  const uint32_t n_chunks = (n_sets + ts - 1) / ts;
  // per member with work: [0] before the count, [1] after it, [2] after the
  // scan and the block starts, [3] before the fill, [4] after it
  std::vector<hipEvent_t> ev(5 * mp->n_parts, nullptr);
  std::vector<std::vector<unsigned long long>> bs(mp->n_parts);
  std::vector<uint32_t> fl(mp->n_parts, 0);
  IssuedGuard guard{m, {}, &ev};  // declared after bs / fl: drains before they are freed
  // (a call that fails from here on leaves no database to read: the headers
  // hold counts or offsets until the fill has run)
  struct Drop {
    spf_mplan* mp;
    bool keep = false;
    ~Drop() {
      if (!keep) mp->db_loc.clear();
    }
  } drop{mp};
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    guard.members.push_back(r);
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)mine[r].size();
    const uint64_t cells = (uint64_t)n * n_sets, blocks = (uint64_t)n * n_chunks;
    M_HIP(m, hipStreamSynchronize(s));  // no queued upload still reads the host tables
    if (!p.db_compact) p.dbpool.reset();  // (the other layout's pool is not this one's size)
    p.db_compact = true;
    p.db_tiles = 0;
    p.db_me = mine[r];
    M_HIP(m, p.rme.upload(p.db_me.data(), n, s));
    M_HIP(m, p.dbhdr.alloc(cells + 1));
    M_HIP(m, p.dbsums.alloc(std::max<uint64_t>(label_scan_tiles(cells), 1)));
    M_HIP(m, p.dbstart.alloc(blocks + 1));
    M_HIP(m, p.dbflags.alloc(1));
    M_HIP(m, hipMemsetAsync(p.dbflags.p, 0, 4, s));
    if (kernel_ms) {
      for (uint32_t k = 0; k < 5; ++k) M_HIP(m, hipEventCreate(&ev[5 * r + k]));
      M_HIP(m, hipEventRecord(ev[5 * r], s));
    }
    RouteDbOut db;
    db.hdr = p.dbhdr.p;
    db.flags = p.dbflags.p;
    db.pass = 1;
    spf_status st = launch_route_sets(c, p.rowp.p, p.nhp.p, p.rme.p, n, p.rsp.p, p.rsn.p, n_sets, lfa, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, s, &db,
                                      mp->h_nrowp.empty() ? nullptr : p.nrowp.p);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 1], s));
    st = launch_label_scan(c, p.dbhdr.p, cells, p.dbsums.p, s);
    if (st == SPF_OK) st = launch_route_block_starts(c, p.dbhdr.p, n, n_sets, p.dbstart.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 2], s));
    bs[r].resize(blocks + 1);
    M_HIP(m, hipMemcpyAsync(bs[r].data(), p.dbstart.p, 8ull * (blocks + 1), hipMemcpyDeviceToHost, s));
    M_HIP(m, hipMemcpyAsync(&fl[r], p.dbflags.p, 4, hipMemcpyDeviceToHost, s));
  }
  uint64_t total = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scan's total and the starts
    if (fl[r] & 2u) return mfail(m, SPF_E_UNSUPPORTED, "a next-hop metric exceeds 2^32 - 1");
    const uint32_t n = (uint32_t)mine[r].size();
    p.h_dbbase.assign(n, 0);
    p.h_dbcnt.assign(n, 0);
    for (uint32_t k = 0; k < n; ++k) {
      const unsigned long long b = bs[r][(size_t)k * n_chunks], e = bs[r][(size_t)(k + 1) * n_chunks];
      if (e - b >= (1ull << 32))
        return mfail(m, SPF_E_UNSUPPORTED, "route database of node %u: %llu records (2^32 max)", mine[r][k],
                     e - b);
      p.h_dbbase[k] = b;
      p.h_dbcnt[k] = (uint32_t)(e - b);
    }
    const unsigned long long tot = bs[r].back();
    total += tot;
    // the record pool: exactly the total (kept when the previous compact one is large enough)
    M_HIP(m, p.dbpool.alloc(std::max<unsigned long long>(tot, 1)));
    M_HIP(m, p.dbbase.upload(p.h_dbbase.data(), n, s));
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 3], s));
    RouteDbOut db;
    db.hdr = p.dbhdr.p;
    db.pool = p.dbpool.p;
    db.flags = p.dbflags.p;
    db.pass = 2;
    db.bstart = p.dbstart.p;
    db.stage = route_compact_stage();
    if (const char* nte = std::getenv("SPF_ROUTE_COMPACT_NT")) db.nt = nte[0] == '1' ? 1u : 0u;  // (A/B)
    const spf_status st = launch_route_sets(c, p.rowp.p, p.nhp.p, p.rme.p, n, p.rsp.p, p.rsn.p, n_sets, lfa,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s, &db,
                                            mp->h_nrowp.empty() ? nullptr : p.nrowp.p);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 4], s));
  }
  double ms[3] = {0, 0, 0}, worst = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    if (kernel_ms) {
      const uint32_t from[3] = {0, 1, 3};
      double sum = 0;
      for (uint32_t k = 0; k < 3; ++k) {
        float t = 0;
        M_HIP(m, hipEventElapsedTime(&t, ev[5 * r + from[k]], ev[5 * r + from[k] + 1]));
        ms[k] = std::max(ms[k], (double)t);
        sum += t;
      }
      worst = std::max(worst, sum);
    }
  }
  drop.keep = true;
  mp->db_moved = false;
  if (kernel_ms) std::copy(ms, ms + 3, mp->db_ms);
  if (n_records) *n_records = total;
  if (kernel_ms) *kernel_ms = worst;
  return SPF_OK;
}

spf_status spf_mplan_route_records(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* set_ptr, const uint32_t* set_nodes, uint32_t n_sets,
                                   uint32_t flags, uint64_t* n_records, double* kernel_ms) {
  if (!mp || (n_me && !me_req) || !set_ptr)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_records: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  for (uint32_t t = 0; t < n_me; ++t)
    if (me_req[t] >= mp->n_src) return mfail(m, SPF_E_INVALID, "me %u is not a request index", me_req[t]);
  // a header's count field has 16 bits (offset | count << 32 | stride << 48,
  // read back in spf_mplan_route_db) and a route keeps at most one next hop
  // per slot of me's row: refused here, before anything is uploaded or
  // launched (the region limit below is per member and tile size)
  for (uint32_t t = 0; t < n_me; ++t) {
    const uint32_t v = mp->srcs[me_req[t]], slots = c0->row_ptr[v + 1] - c0->row_ptr[v];
    if (slots >= (1u << 16))
      return mfail(m, SPF_E_UNSUPPORTED, "route database of node %u: %u link slots (65535 max per node)", v,
                   slots);
  }
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0;
  ++mp->db_gen;  // (the databases a delta compared are overwritten from here on)
  if (const spf_status st = route_prepare(mp, set_ptr, set_nodes, n_sets, lfa, nullptr, 0, me_req, n_me);
      st != SPF_OK)
    return st;
  mp->db_loc.assign(n_me, {0u, 0u});
  mp->db_sets = n_sets;
  mp->db_flags = flags & SPF_ROUTE_LFA;
  mp->db_nodes.resize(n_me);
  std::vector<std::vector<uint32_t>> mine(mp->n_parts);
  for (uint32_t t = 0; t < n_me; ++t) {
    const uint32_t r = mp->owner[me_req[t]];
    mp->db_loc[t] = {r, (uint32_t)mine[r].size()};
    mine[r].push_back(mp->srcs[me_req[t]]);
    mp->db_nodes[t] = mp->srcs[me_req[t]];
  }
  mp->db_compact = (flags & SPF_ROUTE_COMPACT) != 0;
  if (mp->db_compact) return route_records_compact(mp, mine, n_sets, lfa, n_records, kernel_ms);
  // me's region: one [deg(me)][ts] tile per chunk of ts sets (route_quads_kernel<kRsDb>)
  const uint64_t ts = route_db_tile_sets();
  const uint64_t tiles = ((uint64_t)n_sets + ts - 1) / ts * ts;
  std::vector<hipEvent_t> ev(2 * mp->n_parts, nullptr);
  std::vector<std::vector<uint32_t>> fl(mp->n_parts);
  IssuedGuard guard{m, {}, &ev};  // declared after fl: drains before it is freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    guard.members.push_back(r);
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)mine[r].size();
    if (p.db_me != mine[r] || p.db_tiles != tiles || p.db_compact) {
      M_HIP(m, hipStreamSynchronize(s));  // no queued upload still reads the host tables
      if (p.db_compact) p.dbpool.reset();  // (the other layout's pool is not this one's size)
      p.db_compact = false;
      p.db_me = mine[r];
      p.db_tiles = tiles;
      p.h_dbbase.assign(n, 0);
      unsigned long long tot = 0;
      for (uint32_t k = 0; k < n; ++k) {
        const uint32_t v = mine[r][k];
        const uint64_t region = tiles * (c0->row_ptr[v + 1] - c0->row_ptr[v]);
        if (region >= (1ull << 32))
          return mfail(m, SPF_E_UNSUPPORTED, "route database of node %u: %llu record slots (2^32 max)", v,
                       (unsigned long long)region);
        p.h_dbbase[k] = tot;
        tot += region;
      }
      M_HIP(m, p.dbpool.alloc(std::max<unsigned long long>(tot, 1)));
      M_HIP(m, p.dbbase.upload(p.h_dbbase.data(), n, s));
    }
    M_HIP(m, p.rme.upload(p.db_me.data(), n, s));
    M_HIP(m, p.dbhdr.alloc(std::max<size_t>(1, (size_t)n * n_sets)));
    M_HIP(m, p.dbcnt.alloc(n));
    M_HIP(m, p.dbflags.alloc(1));
    M_HIP(m, hipMemsetAsync(p.dbcnt.p, 0, 4ull * n, s));
    M_HIP(m, hipMemsetAsync(p.dbflags.p, 0, 4, s));
    if (kernel_ms) {
      M_HIP(m, hipEventCreate(&ev[2 * r]));
      M_HIP(m, hipEventCreate(&ev[2 * r + 1]));
      M_HIP(m, hipEventRecord(ev[2 * r], s));
    }
    RouteDbOut db;
    db.hdr = p.dbhdr.p;
    db.pool = p.dbpool.p;
    db.base = p.dbbase.p;
    db.count = p.dbcnt.p;
    db.flags = p.dbflags.p;
    const spf_status st = launch_route_sets(c, p.rowp.p, p.nhp.p, p.rme.p, n, p.rsp.p, p.rsn.p, n_sets, lfa,
                                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s, &db,
                                            mp->h_nrowp.empty() ? nullptr : p.nrowp.p);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[2 * r + 1], s));
    fl[r].resize(n + 1);
    M_HIP(m, hipMemcpyAsync(fl[r].data(), p.dbcnt.p, 4ull * n, hipMemcpyDeviceToHost, s));
    M_HIP(m, hipMemcpyAsync(fl[r].data() + n, p.dbflags.p, 4, hipMemcpyDeviceToHost, s));
  }
  double worst = 0;
  uint64_t total = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    const uint32_t n = (uint32_t)mine[r].size();
    if (fl[r][n] & 2u) return mfail(m, SPF_E_UNSUPPORTED, "a next-hop metric exceeds 2^32 - 1");
    p.h_dbcnt.assign(fl[r].begin(), fl[r].begin() + n);
    for (uint32_t k = 0; k < n; ++k) total += p.h_dbcnt[k];
    if (kernel_ms) {
      float t = 0;
      M_HIP(m, hipEventElapsedTime(&t, ev[2 * r], ev[2 * r + 1]));
      worst = std::max(worst, (double)t);
    }
  }
  mp->db_moved = false;  // (only now: a call that failed after a snapshot leaves SPF_E_STATE standing)
  if (n_records) *n_records = total;
  if (kernel_ms) *kernel_ms = worst;
  return SPF_OK;
}

spf_status spf_mplan_route_db(spf_mplan* mp, uint32_t t, uint64_t* hdr, uint64_t* rec, uint64_t cap,
                              uint64_t* n) {
  if (mp && mp->db_moved)
    return mfail(mp->m, SPF_E_STATE, "spf_mplan_route_db: a snapshot took the databases (call spf_mplan_route_records)");
  if (!mp || t >= mp->db_loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_db: no such me (call spf_mplan_route_records)");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->db_loc[t];
  spf_mplan::Part& p = mp->parts[r];
  const uint32_t cnt = p.h_dbcnt[k];
  if (n) *n = cnt;
  if (!hdr && !rec) return SPF_OK;
  if (rec && cap < cnt)
    return mfail(m, SPF_E_NOMEM, "route db of %u records, room for %llu", cnt, (unsigned long long)cap);
  // the device headers and me's tiled region, compacted here: route p's
  // records contiguous from its header's offset, in set order
  const uint32_t S = mp->db_sets;
  std::vector<uint64_t> h(S);
  const uint32_t me = p.db_me[k];
  // (the compact layout's region is me's records themselves, stride 1)
  const uint64_t region =
      p.db_compact ? cnt : p.db_tiles * (mp->m->members[r]->row_ptr[me + 1] - mp->m->members[r]->row_ptr[me]);
  std::vector<uint64_t> tile(std::max<uint64_t>(region, 1));
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  if (S) M_HIP(m, hipMemcpyAsync(h.data(), p.dbhdr.p + (size_t)k * S, 8ull * S, hipMemcpyDeviceToHost, s));
  if (rec && region)
    M_HIP(m, hipMemcpyAsync(tile.data(), p.dbpool.p + p.h_dbbase[k], 8ull * region, hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  uint64_t at = 0;
  for (uint32_t q = 0; q < S; ++q) {
    const uint64_t off = h[q] & 0xFFFFFFFFull, c = (h[q] >> 32) & 0xFFFFull, stride = h[q] >> 48;
    if (rec)
      for (uint64_t j = 0; j < c; ++j) rec[at + j] = tile[off + j * stride];
    if (hdr) hdr[q] = at | (c << 32);
    at += c;
  }
  return SPF_OK;
}

spf_status spf_mplan_route_record_pool(spf_mplan* mp, uint32_t* layout, uint64_t* pool_bytes,
                                       uint64_t* record_bytes) {
  if (!mp) return mfail(nullptr, SPF_E_INVALID, "spf_mplan_route_record_pool: NULL argument");
  if (mp->db_loc.empty() || mp->db_moved)
    return mfail(mp->m, SPF_E_STATE,
                 "spf_mplan_route_record_pool: the plan holds no route records (call spf_mplan_route_records)");
  std::vector<uint8_t> used(mp->n_parts, 0);
  for (const auto& loc : mp->db_loc) used[loc.first] = 1;
  uint64_t bytes = 0, rec = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (!used[r]) continue;
    bytes += 8ull * mp->parts[r].dbpool.n;
    for (const uint32_t c : mp->parts[r].h_dbcnt) rec += c;
  }
  if (layout) *layout = mp->db_compact ? 1u : 0u;
  if (pool_bytes) *pool_bytes = bytes;
  if (record_bytes) *record_bytes = 8 * rec;
  return SPF_OK;
}

uint32_t spf_route_compact_stage(void) { return route_compact_stage(); }

spf_status spf_mplan_route_records_timing(const spf_mplan* mp, double* ms) {
  if (!mp || !ms) return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_records_timing: NULL argument");
  std::copy(mp->db_ms, mp->db_ms + 3, ms);
  return SPF_OK;
}

spf_status spf_mplan_route_record_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_hdr,
                                          const uint64_t** d_base, const uint64_t** d_pool,
                                          uint64_t* n_records, uint32_t* slots, uint32_t cap,
                                          uint32_t* n_slots) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_record_buffers: bad argument");
  const spf_mplan::Part& p = mp->parts[member];
  // (a member without a me of the last call holds nothing of it)
  uint32_t k = 0;
  if (!mp->db_moved)
    for (const auto& loc : mp->db_loc) k += loc.first == member;
  const bool has = k != 0;
  uint64_t rec = 0;
  if (has)
    for (const uint32_t c : p.h_dbcnt) rec += c;
  if (n_slots) *n_slots = k;
  if (d_hdr) *d_hdr = has ? reinterpret_cast<const uint64_t*>(p.dbhdr.p) : nullptr;
  if (d_base) *d_base = has ? reinterpret_cast<const uint64_t*>(p.dbbase.p) : nullptr;
  if (d_pool) *d_pool = has ? reinterpret_cast<const uint64_t*>(p.dbpool.p) : nullptr;
  if (n_records) *n_records = rec;
  if (slots) {
    if (cap < k) return mfail(mp->m, SPF_E_NOMEM, "%u me slots, room for %u", k, cap);
    for (uint32_t t = 0; t < mp->db_loc.size() && has; ++t)
      if (mp->db_loc[t].first == member) slots[mp->db_loc[t].second] = t;
  }
  return SPF_OK;
}

spf_status spf_mplan_label_routes(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                  const int32_t* node_label, uint32_t flags, uint32_t* n_labels,
                                  uint64_t* n_records, uint64_t* pool_bytes, double* kernel_ms) {
  if (!mp || (n_me && !me_req) || !node_label)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_label_routes: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  for (uint32_t t = 0; t < n_me; ++t)
    if (me_req[t] >= mp->n_src) return mfail(m, SPF_E_INVALID, "me %u is not a request index", me_req[t]);
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0;
  ++mp->db_gen;
  if (const spf_status st = route_prepare(mp, nullptr, nullptr, 0, lfa, nullptr, 0, me_req, n_me);
      st != SPF_OK)
    return st;
  mp->lr_loc.clear();  // (the previous call's databases are overwritten from here on)
  const uint32_t N = c0->N;
  mp->lr_gptr.assign((size_t)N + 1, 0);
  mp->lr_gnodes.assign(std::max<uint32_t>(N, 1), 0);
  mp->lr_labels.assign(std::max<uint32_t>(N, 1), 0);
  uint32_t G = 0;
  if (const spf_status st = spf_label_groups(node_label, N, mp->lr_labels.data(), mp->lr_gptr.data(),
                                             mp->lr_gnodes.data(), &G);
      st != SPF_OK)
    return st;
  std::vector<std::pair<uint32_t, uint32_t>> loc(n_me);
  std::vector<std::vector<uint32_t>> mine(mp->n_parts);
  for (uint32_t r = 0; r < mp->n_parts; ++r) mp->parts[r].lr_req.clear();
  for (uint32_t t = 0; t < n_me; ++t) {
    const uint32_t r = mp->owner[me_req[t]];
    loc[t] = {r, (uint32_t)mine[r].size()};
    mine[r].push_back(mp->srcs[me_req[t]]);
    mp->parts[r].lr_req.push_back(t);
  }
  // per member with work: [0] before the count, [1] after the scan, [2]
  // before the fill, [3] after it (the pool is allocated in between, on the
  // host, from the scan's total)
  std::vector<hipEvent_t> ev(4 * mp->n_parts, nullptr);
  std::vector<unsigned long long> tot(mp->n_parts, 0);
  std::vector<uint32_t> fl(mp->n_parts, 0);
  IssuedGuard guard{m, {}, &ev};  // declared after mine / tot / fl: drains before they are freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    guard.members.push_back(r);
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)mine[r].size();
    const uint64_t cells = (uint64_t)n * G;
    M_HIP(m, p.lr_me.upload(mine[r].data(), n, s));
    M_HIP(m, p.lr_gptr.upload(mp->lr_gptr.data(), (size_t)G + 1, s));
    M_HIP(m, p.lr_gnodes.upload(mp->lr_gnodes.data(), std::max<uint32_t>(1, mp->lr_gptr[G]), s));
    M_HIP(m, p.lr_owner.alloc(std::max<uint64_t>(cells, 1)));
    M_HIP(m, p.lr_ptr.alloc(cells + 1));
    M_HIP(m, p.lr_sums.alloc(std::max<uint64_t>(label_scan_tiles(cells), 1)));
    M_HIP(m, p.lr_flags.alloc(1));
    M_HIP(m, hipMemsetAsync(p.lr_flags.p, 0, 4, s));
    if (kernel_ms) {
      for (uint32_t k = 0; k < 4; ++k) M_HIP(m, hipEventCreate(&ev[4 * r + k]));
      M_HIP(m, hipEventRecord(ev[4 * r], s));
    }
    spf_status st = launch_label_routes(c, false, p.rowp.p, p.nhp.p, p.lr_me.p, n, p.lr_gptr.p,
                                        p.lr_gnodes.p, G, lfa, p.lr_owner.p, p.lr_ptr.p, nullptr,
                                        p.lr_flags.p, s);
    if (st == SPF_OK) st = launch_label_scan(c, p.lr_ptr.p, cells, p.lr_sums.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[4 * r + 1], s));
    M_HIP(m, hipMemcpyAsync(&tot[r], p.lr_ptr.p + cells, 8, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scan's total
    // the record pool: exactly the total (kept when the previous one is large enough)
    M_HIP(m, p.lr_rec.alloc(std::max<unsigned long long>(tot[r], 1)));
    p.lr_records = tot[r];
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[4 * r + 2], s));
    const spf_status st = launch_label_routes(c, true, p.rowp.p, p.nhp.p, p.lr_me.p, (uint32_t)mine[r].size(),
                                              p.lr_gptr.p, p.lr_gnodes.p, G, lfa, p.lr_owner.p,
                                              p.lr_ptr.p, p.lr_rec.p, p.lr_flags.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[4 * r + 3], s));
    M_HIP(m, hipMemcpyAsync(&fl[r], p.lr_flags.p, 4, hipMemcpyDeviceToHost, s));
  }
  double worst = 0;
  uint64_t total = 0, bytes = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    if (fl[r] & 2u) return mfail(m, SPF_E_UNSUPPORTED, "a next-hop metric exceeds 2^32 - 1");
    const uint64_t cells = (uint64_t)mine[r].size() * G;
    total += tot[r];
    bytes += 8 * tot[r] + 8 * (cells + 1) + 4 * cells;
    if (kernel_ms) {
      float a = 0, b = 0;
      M_HIP(m, hipEventElapsedTime(&a, ev[4 * r], ev[4 * r + 1]));
      M_HIP(m, hipEventElapsedTime(&b, ev[4 * r + 2], ev[4 * r + 3]));
      worst = std::max(worst, (double)a + (double)b);
    }
  }
  mp->lr_loc = std::move(loc);
  mp->lr_moved = false;
  mp->lr_groups = G;
  mp->lr_labels.resize(G);
  mp->lr_rflags = flags & SPF_ROUTE_LFA;
  mp->lr_nodes.resize(n_me);
  for (uint32_t t = 0; t < n_me; ++t) mp->lr_nodes[t] = mp->srcs[me_req[t]];
  if (n_labels) *n_labels = G;
  if (n_records) *n_records = total;
  if (pool_bytes) *pool_bytes = bytes;
  if (kernel_ms) *kernel_ms = worst;
  return SPF_OK;
}

spf_status spf_mplan_label_route_db(spf_mplan* mp, uint32_t t, uint32_t* owner, uint64_t* ptr,
                                    uint64_t* rec, uint64_t cap, uint64_t* n) {
  if (mp && mp->lr_moved)
    return mfail(mp->m, SPF_E_STATE,
                 "spf_mplan_label_route_db: a snapshot took the databases (call spf_mplan_label_routes)");
  if (!mp || t >= mp->lr_loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID,
                 "spf_mplan_label_route_db: no such me (call spf_mplan_label_routes)");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->lr_loc[t];
  spf_mplan::Part& p = mp->parts[r];
  const uint32_t G = mp->lr_groups;
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  // me's G + 1 offsets (the next slot's first one, or the total, ends them)
  std::vector<uint64_t> h((size_t)G + 1);
  M_HIP(m, hipMemcpyAsync(h.data(), p.lr_ptr.p + (size_t)k * G, 8ull * (G + 1), hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  const uint64_t cnt = h[G] - h[0];
  if (n) *n = cnt;
  if (rec && cap < cnt)
    return mfail(m, SPF_E_NOMEM, "label route db of %llu records, room for %llu", (unsigned long long)cnt,
                 (unsigned long long)cap);
  if (owner && G)
    M_HIP(m, hipMemcpyAsync(owner, p.lr_owner.p + (size_t)k * G, 4ull * G, hipMemcpyDeviceToHost, s));
  if (rec && cnt)
    M_HIP(m, hipMemcpyAsync(rec, p.lr_rec.p + h[0], 8ull * cnt, hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  if (ptr)
    for (uint32_t g = 0; g <= G; ++g) ptr[g] = h[g] - h[0];
  return SPF_OK;
}

spf_status spf_mplan_label_route_buffers(spf_mplan* mp, uint32_t member, const uint32_t** d_owner,
                                         const uint64_t** d_ptr, const uint64_t** d_rec,
                                         uint64_t* n_records, uint32_t* slots, uint32_t cap,
                                         uint32_t* n_slots) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_label_route_buffers: bad argument");
  const spf_mplan::Part& p = mp->parts[member];
  // (a member without a me of the last call holds nothing of it)
  const bool has = !mp->lr_loc.empty() && !p.lr_req.empty();
  const uint32_t k = has ? (uint32_t)p.lr_req.size() : 0u;
  if (n_slots) *n_slots = k;
  if (d_owner) *d_owner = has ? p.lr_owner.p : nullptr;
  if (d_ptr) *d_ptr = has ? reinterpret_cast<const uint64_t*>(p.lr_ptr.p) : nullptr;
  if (d_rec) *d_rec = has ? reinterpret_cast<const uint64_t*>(p.lr_rec.p) : nullptr;
  if (n_records) *n_records = has ? p.lr_records : 0;
  if (slots) {
    if (cap < k) return mfail(mp->m, SPF_E_NOMEM, "%u me slots, room for %u", k, cap);
    std::copy(p.lr_req.begin(), p.lr_req.begin() + k, slots);
  }
  return SPF_OK;
}

// ---- route-database delta between two passes -------------------------------
namespace {

// key[e] = link_hash[link_id[e]] over the member's CSR as it is now
spf_status edge_keys(spf_mctx* m, const spf_ctx* c, const uint64_t* link_hash, uint32_t n_links,
                     std::vector<unsigned long long>* out) {
  out->assign(std::max<uint32_t>(c->E, 1), 0ull);
  for (uint32_t e = 0; e < c->E; ++e) {
    if (c->link[e] >= n_links) return mfail(m, SPF_E_INVALID, "link_hash shorter than the link ids");
    (*out)[e] = link_hash[c->link[e]];
  }
  return SPF_OK;
}

}  // namespace

spf_status spf_mplan_route_snapshot(spf_mplan* mp, const uint64_t* link_hash, uint32_t n_links,
                                    spf_route_snapshot** out) {
  if (!mp || !link_hash || !out)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_snapshot: NULL argument");
  *out = nullptr;
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  if (mp->db_loc.empty() || mp->db_moved)
    return mfail(m, SPF_E_STATE, "spf_mplan_route_snapshot: the plan holds no route records");
  const bool labels = !mp->lr_loc.empty() && !mp->lr_moved;
  if (labels && mp->lr_nodes != mp->db_nodes)
    return mfail(m, SPF_E_INVALID, "spf_mplan_route_snapshot: label routes and route records of different me lists");
  std::vector<unsigned long long> key;
  if (const spf_status st = edge_keys(m, c0, link_hash, n_links, &key); st != SPF_OK) return st;
  auto sn = std::make_unique<spf_route_snapshot>();
  sn->n_nodes = c0->N;
  sn->n_sets = mp->db_sets;
  sn->flags = mp->db_flags;
  sn->me = mp->db_nodes;
  sn->db_loc = mp->db_loc;
  sn->row_ptr = c0->row_ptr;
  sn->parts.reset(new spf_route_snapshot::Part[mp->n_parts]);
  sn->n_parts = mp->n_parts;
  // the keys first, to every member (the next plan may place a me anywhere):
  // nothing has moved when an upload fails
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, sn->parts[r].key.upload(key.data(), key.size(), m->exec[r]));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));  // (`key` is this call's; the databases are complete)
  }
  // the members the last call placed a me on (an earlier call's pools on
  // another member are stale: they stay with the plan)
  std::vector<uint8_t> used(mp->n_parts, 0);
  for (const auto& loc : mp->db_loc) used[loc.first] = 1;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    spf_route_snapshot::Part& q = sn->parts[r];
    q.bytes = 8 * q.key.n;
    if (!used[r]) continue;
    q.dbhdr.take(p.dbhdr);
    q.dbpool.take(p.dbpool);
    q.h_dbbase = p.h_dbbase;
    q.bytes += 8 * (q.dbhdr.n + q.dbpool.n);
    p.db_me.clear();  // the next spf_mplan_route_records allocates afresh
    p.db_tiles = 0;
    if (labels) {
      q.lr_owner.take(p.lr_owner);
      q.lr_ptr.take(p.lr_ptr);
      q.lr_rec.take(p.lr_rec);
      q.bytes += 4 * q.lr_owner.n + 8 * (q.lr_ptr.n + q.lr_rec.n);
      p.lr_records = 0;
    }
  }
  mp->db_loc.clear();
  mp->db_moved = true;
  ++mp->db_gen;
  if (labels) {
    sn->has_labels = true;
    sn->lr_flags = mp->lr_rflags;
    sn->lr_groups = mp->lr_groups;
    sn->labels = mp->lr_labels;
    sn->lr_loc = mp->lr_loc;
    mp->lr_loc.clear();
    mp->lr_moved = true;
  }
  sn->m = m;
  m->snaps.push_back(sn.get());
  *out = sn.release();
  return SPF_OK;
}

void spf_route_snapshot_destroy(spf_route_snapshot* snap) { delete snap; }

uint64_t spf_route_snapshot_bytes(const spf_route_snapshot* snap) {
  uint64_t b = 0;
  for (uint32_t r = 0; snap && r < snap->n_parts; ++r) b += snap->parts[r].bytes;
  return b;
}

spf_status spf_mplan_route_delta(spf_mplan* mp, const spf_route_snapshot* snap, const uint64_t* link_hash,
                                 uint32_t n_links, uint64_t* totals, double* kernel_ms) {
  if (!mp || !snap || !link_hash)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_delta: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  if (mp->flags & (SPF_FLAG_DIST64 | SPF_FLAG_HOP_COUNT))
    return mfail(m, SPF_E_UNSUPPORTED, "route databases need u32 link-metric rows");
  if (snap->m != m) return mfail(m, SPF_E_INVALID, "spf_mplan_route_delta: the snapshot is another context's");
  if (mp->db_loc.empty() || mp->db_moved)
    return mfail(m, SPF_E_STATE, "spf_mplan_route_delta: the plan holds no databases (call spf_mplan_route_records)");
  const bool labels = !mp->lr_loc.empty() && !mp->lr_moved;
  if (snap->n_nodes != c0->N || snap->n_sets != mp->db_sets || snap->flags != mp->db_flags ||
      snap->me != mp->db_nodes)
    return mfail(m, SPF_E_INVALID, "spf_mplan_route_delta: me list, n_nodes, n_sets or route flags differ from the snapshot");
  if (labels != snap->has_labels || (labels && (mp->lr_nodes != mp->db_nodes || mp->lr_rflags != snap->lr_flags)))
    return mfail(m, SPF_E_INVALID, "spf_mplan_route_delta: label routes (presence, me list or flags) differ from the snapshot");
  std::vector<unsigned long long> key;
  if (const spf_status st = edge_keys(m, c0, link_hash, n_links, &key); st != SPF_OK) return st;
  const uint32_t n_me = (uint32_t)mp->db_nodes.size(), S = mp->db_sets;
  // an old database on another device is read over peer access
  // (route_prepare of the materialising call tried to enable it)
  for (uint32_t t = 0; t < n_me; ++t) {
    const int dn = m->members[mp->db_loc[t].first]->device, dold = m->members[snap->db_loc[t].first]->device;
    if (dn != dold && mp->peer != 1)
      return mfail(m, SPF_E_UNSUPPORTED, "route delta across devices needs peer access");
  }
  // labels of either generation, ascending, and each one's group index there
  std::vector<uint32_t> lab, mold, mnew;
  if (labels) {
    size_t i = 0, j = 0;
    const auto& a = snap->labels;
    const auto& b = mp->lr_labels;
    while (i < a.size() || j < b.size()) {
      const bool ta = j == b.size() || (i < a.size() && a[i] <= b[j]);
      const bool tb = i == a.size() || (j < b.size() && b[j] <= a[i]);
      lab.push_back((uint32_t)(ta ? a[i] : b[j]));
      mold.push_back(ta ? (uint32_t)i : 0xFFFFFFFFu);
      mnew.push_back(tb ? (uint32_t)j : 0xFFFFFFFFu);
      i += ta;
      j += tb;
    }
  }
  const uint32_t U = (uint32_t)lab.size(), Gn = mp->lr_groups, Go = snap->lr_groups;
  const uint32_t cells[2] = {S, U};
  mp->dl_loc.clear();
  mp->up_done = false;
  // per member with work: [0] before the counts, [1] after the scans, [2]
  // before the fills, [3] after them (the lists are allocated in between, on
  // the host, from the scans' totals)
  std::vector<hipEvent_t> ev(4 * mp->n_parts, nullptr);
  struct Host {
    std::vector<unsigned long long> ohdr, opool, oown, optr, orec;
    std::vector<uint32_t> e0, deg, same;
    unsigned long long tot[2] = {0, 0}, del[2] = {0, 0};
  };
  std::vector<Host> host(mp->n_parts);
  IssuedGuard guard{m, {}, &ev};  // declared after key / host / lab ...: drains before they are freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) mp->parts[r].dl_req.clear();
  for (uint32_t t = 0; t < n_me; ++t) mp->parts[mp->db_loc[t].first].dl_req.push_back(t);
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    const uint32_t n = (uint32_t)p.dl_req.size();
    if (!n) continue;
    spf_ctx* c = m->members[r];
    Host& h = host[r];
    for (uint32_t k = 0; k < n; ++k) {  // (slot k of the records call is its k-th me of this member)
      const uint32_t t = p.dl_req[k], v = mp->db_nodes[t];
      const auto [ro, ko] = snap->db_loc[t];
      const spf_route_snapshot::Part& q = snap->parts[ro];
      h.ohdr.push_back((unsigned long long)(uintptr_t)(q.dbhdr.p + (size_t)ko * S));
      h.opool.push_back((unsigned long long)(uintptr_t)(q.dbpool.p + q.h_dbbase[ko]));
      h.e0.push_back(snap->row_ptr[v]);
      h.deg.push_back(snap->row_ptr[v + 1] - snap->row_ptr[v]);
      if (labels) {
        const auto [rl, kl] = snap->lr_loc[t];
        const spf_route_snapshot::Part& ql = snap->parts[rl];
        h.oown.push_back((unsigned long long)(uintptr_t)(ql.lr_owner.p + (size_t)kl * Go));
        h.optr.push_back((unsigned long long)(uintptr_t)(ql.lr_ptr.p + (size_t)kl * Go));
        h.orec.push_back((unsigned long long)(uintptr_t)ql.lr_rec.p);
      }
    }
    M_HIP(m, hipSetDevice(c->device));
    guard.members.push_back(r);
    const hipStream_t s = m->exec[r];
    M_HIP(m, p.rme.upload(p.db_me.data(), n, s));
    M_HIP(m, p.dl_ohdr.upload(h.ohdr.data(), n, s));
    M_HIP(m, p.dl_opool.upload(h.opool.data(), n, s));
    M_HIP(m, p.dl_e0.upload(h.e0.data(), n, s));
    M_HIP(m, p.dl_deg.upload(h.deg.data(), n, s));
    M_HIP(m, p.dl_key.upload(key.data(), key.size(), s));
    M_HIP(m, p.dl_same.alloc(n));
    M_HIP(m, p.dl_tot.alloc(2));
    M_HIP(m, hipMemsetAsync(p.dl_tot.p, 0, 16, s));
    if (labels) {
      M_HIP(m, p.dl_oown.upload(h.oown.data(), n, s));
      M_HIP(m, p.dl_optr.upload(h.optr.data(), n, s));
      M_HIP(m, p.dl_orec.upload(h.orec.data(), n, s));
      M_HIP(m, p.dl_mold.upload(mold.data(), U, s));
      M_HIP(m, p.dl_mnew.upload(mnew.data(), U, s));
      M_HIP(m, p.dl_lab.upload(lab.data(), U, s));
    }
    for (uint32_t w = 0; w < 2; ++w) {
      const uint64_t nb = (uint64_t)n * route_delta_chunks(cells[w]);
      M_HIP(m, p.dl_kind[w].alloc(std::max<uint64_t>((uint64_t)n * cells[w], 1)));
      M_HIP(m, p.dl_blk[w].alloc(nb + 1));
      M_HIP(m, p.dl_sums[w].alloc(std::max<uint64_t>(label_scan_tiles(nb), 1)));
      M_HIP(m, p.dl_ptr[w].alloc((size_t)n + 1));
      M_HIP(m, hipMemsetAsync(p.dl_ptr[w].p, 0, 8ull * (n + 1), s));  // (a pass without cells writes none)
    }
    if (kernel_ms) {
      for (uint32_t k = 0; k < 4; ++k) M_HIP(m, hipEventCreate(&ev[4 * r + k]));
      M_HIP(m, hipEventRecord(ev[4 * r], s));
    }
    RouteDeltaIn in;
    in.me = p.rme.p;
    in.old_e0 = p.dl_e0.p;
    in.old_deg = p.dl_deg.p;
    in.key_old = snap->parts[r].key.p;
    in.key_new = p.dl_key.p;
    in.same = p.dl_same.p;
    spf_status st = launch_delta_rows(c, in, n, s);
    if (st == SPF_OK)
      st = launch_delta_ip(c, in, n, S, p.dbhdr.p, p.dbpool.p, p.dbbase.p, p.dl_ohdr.p, p.dl_opool.p,
                           p.dl_kind[0].p, p.dl_blk[0].p, s);
    if (st == SPF_OK) st = launch_label_scan(c, p.dl_blk[0].p, (uint64_t)n * route_delta_chunks(S), p.dl_sums[0].p, s);
    if (st == SPF_OK && labels)
      st = launch_delta_labels(c, in, n, U, p.lr_owner.p, p.lr_ptr.p, p.lr_rec.p, Gn, p.dl_oown.p,
                               p.dl_optr.p, p.dl_orec.p, p.dl_mold.p, p.dl_mnew.p, p.dl_kind[1].p,
                               p.dl_blk[1].p, s);
    if (st == SPF_OK) st = launch_label_scan(c, p.dl_blk[1].p, (uint64_t)n * route_delta_chunks(U), p.dl_sums[1].p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[4 * r + 1], s));
    for (uint32_t w = 0; w < 2; ++w)
      M_HIP(m, hipMemcpyAsync(&h.tot[w], p.dl_blk[w].p + (uint64_t)n * route_delta_chunks(cells[w]), 8,
                              hipMemcpyDeviceToHost, s));
    h.same.resize(n);
    M_HIP(m, hipMemcpyAsync(h.same.data(), p.dl_same.p, 4ull * n, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    const uint32_t n = (uint32_t)p.dl_req.size();
    if (!n) continue;
    spf_ctx* c = m->members[r];
    Host& h = host[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scans' totals
    for (uint32_t w = 0; w < 2; ++w) {
      M_HIP(m, p.dl_set[w].alloc(std::max<unsigned long long>(h.tot[w], 1)));
      p.dl_n[w] = h.tot[w];
    }
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[4 * r + 2], s));
    spf_status st = launch_delta_fill(c, p.dl_kind[0].p, S, n, p.dl_blk[0].p, nullptr, p.dl_set[0].p,
                                      p.dl_ptr[0].p, p.dl_tot.p, s);
    if (st == SPF_OK && labels)
      st = launch_delta_fill(c, p.dl_kind[1].p, U, n, p.dl_blk[1].p, p.dl_lab.p, p.dl_set[1].p, p.dl_ptr[1].p,
                             p.dl_tot.p + 1, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[4 * r + 3], s));
    M_HIP(m, hipMemcpyAsync(h.del, p.dl_tot.p, 16, hipMemcpyDeviceToHost, s));
  }
  double worst = 0;
  uint64_t out[5] = {0, 0, 0, 0, 0};
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (mp->parts[r].dl_req.empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    const Host& h = host[r];
    for (uint32_t w = 0; w < 2; ++w) {
      out[2 * w] += h.tot[w] - h.del[w];
      out[2 * w + 1] += h.del[w];
    }
    for (uint32_t x : h.same) out[4] += x ? 0u : 1u;
    if (kernel_ms) {
      float a = 0, b = 0;
      M_HIP(m, hipEventElapsedTime(&a, ev[4 * r], ev[4 * r + 1]));
      M_HIP(m, hipEventElapsedTime(&b, ev[4 * r + 2], ev[4 * r + 3]));
      worst = std::max(worst, (double)a + (double)b);
    }
  }
  mp->dl_loc = mp->db_loc;
  mp->dl_gen = mp->db_gen;
  mp->dl_labels = labels;
  mp->dl_union = U;
  std::copy(out, out + 5, mp->dl_tot);
  if (totals) std::copy(out, out + 5, totals);
  if (kernel_ms) *kernel_ms = worst;
  return SPF_OK;
}

spf_status spf_mplan_route_delta_db(spf_mplan* mp, uint32_t t, uint32_t* ip, uint64_t ip_cap,
                                    uint64_t* n_ip, uint32_t* label, uint64_t label_cap,
                                    uint64_t* n_label) {
  if (!mp || t >= mp->dl_loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID,
                 "spf_mplan_route_delta_db: no such me (call spf_mplan_route_delta)");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->dl_loc[t];
  spf_mplan::Part& p = mp->parts[r];
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  uint64_t h[2][2];
  for (uint32_t w = 0; w < 2; ++w)
    M_HIP(m, hipMemcpyAsync(h[w], p.dl_ptr[w].p + k, 16, hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  uint32_t* const dst[2] = {ip, label};
  const uint64_t cap[2] = {ip_cap, label_cap};
  uint64_t* const cnt[2] = {n_ip, n_label};
  for (uint32_t w = 0; w < 2; ++w) {
    const uint64_t c = h[w][1] - h[w][0];
    if (cnt[w]) *cnt[w] = c;
    if (dst[w] && cap[w] < c)
      return mfail(m, SPF_E_NOMEM, "route delta of %llu entries, room for %llu", (unsigned long long)c,
                   (unsigned long long)cap[w]);
    if (dst[w] && c)
      M_HIP(m, hipMemcpyAsync(dst[w], p.dl_set[w].p + h[w][0], 4 * c, hipMemcpyDeviceToHost, s));
  }
  M_HIP(m, hipStreamSynchronize(s));
  return SPF_OK;
}

spf_status spf_mplan_route_delta_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_ip_ptr,
                                         const uint32_t** d_ip_set, const uint64_t** d_label_ptr,
                                         const uint32_t** d_label_set, uint32_t* slots, uint32_t cap,
                                         uint32_t* n_slots) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_delta_buffers: bad argument");
  const spf_mplan::Part& p = mp->parts[member];
  const bool has = !mp->dl_loc.empty() && !p.dl_req.empty();
  const uint32_t k = has ? (uint32_t)p.dl_req.size() : 0u;
  if (n_slots) *n_slots = k;
  if (d_ip_ptr) *d_ip_ptr = has ? reinterpret_cast<const uint64_t*>(p.dl_ptr[0].p) : nullptr;
  if (d_ip_set) *d_ip_set = has ? p.dl_set[0].p : nullptr;
  if (d_label_ptr) *d_label_ptr = has ? reinterpret_cast<const uint64_t*>(p.dl_ptr[1].p) : nullptr;
  if (d_label_set) *d_label_set = has ? p.dl_set[1].p : nullptr;
  if (slots) {
    if (cap < k) return mfail(mp->m, SPF_E_NOMEM, "%u me slots, room for %u", k, cap);
    std::copy(p.dl_req.begin(), p.dl_req.begin() + k, slots);
  }
  return SPF_OK;
}

// ---- the delta's payload: updated routes with their next hops ----------------
spf_status spf_mplan_route_update(spf_mplan* mp, uint64_t* totals, uint64_t* pool_bytes, double* kernel_ms) {
  if (!mp) return mfail(nullptr, SPF_E_INVALID, "spf_mplan_route_update: NULL argument");
  spf_mctx* m = mp->m;
  if (mp->dl_loc.empty())
    return mfail(m, SPF_E_STATE, "spf_mplan_route_update: no delta (call spf_mplan_route_delta)");
  if (mp->dl_gen != mp->db_gen || mp->db_moved || mp->db_loc.empty())
    return mfail(m, SPF_E_STATE,
                 "spf_mplan_route_update: the plan's databases are not the ones the delta compared "
                 "(call spf_mplan_route_delta again)");
  const bool labels = mp->dl_labels;
  const uint32_t S = mp->db_sets, U = mp->dl_union, G = mp->lr_groups;
  mp->up_done = false;
  // per member with work: [0] before the counts, [1] after them, [2] after the
  // scans, [3] before the fills, [4] after them (the pools are allocated in
  // between, on the host, from the scans' totals)
  std::vector<hipEvent_t> ev(5 * mp->n_parts, nullptr);
  std::vector<unsigned long long> tot(2 * mp->n_parts, 0);
  IssuedGuard guard{m, {}, &ev};  // declared after tot: drains before it is freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    const uint32_t n = (uint32_t)p.dl_req.size();
    if (!n) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    guard.members.push_back(r);
    const hipStream_t s = m->exec[r];
    for (uint32_t w = 0; w < 2; ++w) {
      M_HIP(m, p.up_ptr[w].alloc(p.dl_n[w] + 1));
      M_HIP(m, p.up_src[w].alloc(std::max<uint64_t>(p.dl_n[w], 1)));
      M_HIP(m, p.up_sums[w].alloc(std::max<uint64_t>(label_scan_tiles(p.dl_n[w]), 1)));
    }
    M_HIP(m, p.up_owner.alloc(std::max<uint64_t>(p.dl_n[1], 1)));
    if (kernel_ms) {
      for (uint32_t k = 0; k < 5; ++k) M_HIP(m, hipEventCreate(&ev[5 * r + k]));
      M_HIP(m, hipEventRecord(ev[5 * r], s));
    }
    spf_status st = launch_update_count_ip(c, p.dl_ptr[0].p, p.dl_set[0].p, n, p.dl_n[0], p.dbhdr.p, p.dbbase.p,
                                           S, p.up_ptr[0].p, p.up_src[0].p, s);
    if (st == SPF_OK && labels)
      st = launch_update_count_labels(c, p.dl_ptr[1].p, p.dl_set[1].p, n, p.dl_n[1], p.dl_lab.p, p.dl_mnew.p, U,
                                      p.lr_owner.p, p.lr_ptr.p, G, p.up_ptr[1].p, p.up_src[1].p,
                                      p.up_owner.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 1], s));
    for (uint32_t w = 0; w < 2 && st == SPF_OK; ++w)
      st = launch_label_scan(c, p.up_ptr[w].p, p.dl_n[w], p.up_sums[w].p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 2], s));
    for (uint32_t w = 0; w < 2; ++w)
      M_HIP(m, hipMemcpyAsync(&tot[2 * r + w], p.up_ptr[w].p + p.dl_n[w], 8, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    if (p.dl_req.empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scans' totals
    // the record pools: exactly the totals (kept when the previous ones are large enough)
    for (uint32_t w = 0; w < 2; ++w) {
      M_HIP(m, p.up_rec[w].alloc(std::max<unsigned long long>(tot[2 * r + w], 1)));
      p.up_nrec[w] = tot[2 * r + w];
    }
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 3], s));
    spf_status st = launch_update_fill(c, p.up_ptr[0].p, p.up_src[0].p, p.dl_n[0], p.dbpool.p, p.up_rec[0].p, s);
    if (st == SPF_OK && labels)
      st = launch_update_fill(c, p.up_ptr[1].p, p.up_src[1].p, p.dl_n[1], p.lr_rec.p, p.up_rec[1].p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    if (kernel_ms) M_HIP(m, hipEventRecord(ev[5 * r + 4], s));
  }
  double ms[3] = {0, 0, 0};
  uint64_t out[4] = {mp->dl_tot[0], 0, mp->dl_tot[2], 0}, bytes = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part& p = mp->parts[r];
    if (p.dl_req.empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    out[1] += p.up_nrec[0];
    out[3] += p.up_nrec[1];
    bytes += 8 * p.up_nrec[0] + 8 * (p.dl_n[0] + 1) + 8 * p.up_nrec[1] + 8 * (p.dl_n[1] + 1) + 4 * p.dl_n[1];
    if (kernel_ms) {
      const uint32_t from[3] = {0, 1, 3};
      for (uint32_t k = 0; k < 3; ++k) {
        float t = 0;
        M_HIP(m, hipEventElapsedTime(&t, ev[5 * r + from[k]], ev[5 * r + from[k] + 1]));
        ms[k] = std::max(ms[k], (double)t);
      }
    }
  }
  mp->up_done = true;
  if (kernel_ms) std::copy(ms, ms + 3, mp->up_ms);
  if (totals) std::copy(out, out + 4, totals);
  if (pool_bytes) *pool_bytes = bytes;
  if (kernel_ms) *kernel_ms = ms[0] + ms[1] + ms[2];
  return SPF_OK;
}

spf_status spf_mplan_route_update_timing(const spf_mplan* mp, double* ms) {
  if (!mp || !ms) return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_update_timing: NULL argument");
  std::copy(mp->up_ms, mp->up_ms + 3, ms);
  return SPF_OK;
}

spf_status spf_mplan_route_update_db(spf_mplan* mp, uint32_t t, uint64_t* ip_ptr, uint64_t* ip_rec,
                                     uint64_t ip_cap, uint64_t* n_ip_rec, uint32_t* label_owner,
                                     uint64_t* label_ptr, uint64_t* label_rec, uint64_t label_cap,
                                     uint64_t* n_label_rec) {
  if (mp && (mp->dl_loc.empty() || !mp->up_done))
    return mfail(mp->m, SPF_E_STATE, "spf_mplan_route_update_db: no update (call spf_mplan_route_update)");
  if (!mp || t >= mp->dl_loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_update_db: no such me");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->dl_loc[t];
  spf_mplan::Part& p = mp->parts[r];
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  uint64_t e[2][2];  // me's entries [e[w][0], e[w][1]) of either list
  for (uint32_t w = 0; w < 2; ++w) M_HIP(m, hipMemcpyAsync(e[w], p.dl_ptr[w].p + k, 16, hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  uint64_t* const optr[2] = {ip_ptr, label_ptr};
  uint64_t* const orec[2] = {ip_rec, label_rec};
  const uint64_t cap[2] = {ip_cap, label_cap};
  uint64_t* const cnt[2] = {n_ip_rec, n_label_rec};
  std::vector<uint64_t> h[2];
  for (uint32_t w = 0; w < 2; ++w) {  // the entries' offsets (the next entry's, or the total, ends the last)
    h[w].resize(e[w][1] - e[w][0] + 1);
    M_HIP(m, hipMemcpyAsync(h[w].data(), p.up_ptr[w].p + e[w][0], 8 * h[w].size(), hipMemcpyDeviceToHost, s));
  }
  M_HIP(m, hipStreamSynchronize(s));
  for (uint32_t w = 0; w < 2; ++w) {
    const uint64_t c = h[w].back() - h[w][0];
    if (cnt[w]) *cnt[w] = c;
    if (orec[w] && cap[w] < c)
      return mfail(m, SPF_E_NOMEM, "route update of %llu records, room for %llu", (unsigned long long)c,
                   (unsigned long long)cap[w]);
  }
  for (uint32_t w = 0; w < 2; ++w) {
    const uint64_t c = h[w].back() - h[w][0];
    if (orec[w] && c)
      M_HIP(m, hipMemcpyAsync(orec[w], p.up_rec[w].p + h[w][0], 8 * c, hipMemcpyDeviceToHost, s));
    if (optr[w])
      for (size_t j = 0; j < h[w].size(); ++j) optr[w][j] = h[w][j] - h[w][0];
  }
  if (label_owner && e[1][1] > e[1][0])
    M_HIP(m, hipMemcpyAsync(label_owner, p.up_owner.p + e[1][0], 4 * (e[1][1] - e[1][0]), hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  return SPF_OK;
}

spf_status spf_mplan_route_update_read(spf_mplan* mp, uint32_t member, uint64_t* n, uint64_t* ip_dptr,
                                       uint32_t* ip_dset, uint64_t* ip_uptr, uint64_t* ip_urec,
                                       uint64_t* label_dptr, uint32_t* label_dset, uint32_t* label_uowner,
                                       uint64_t* label_uptr, uint64_t* label_urec) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_update_read: bad argument");
  spf_mctx* m = mp->m;
  if (mp->dl_loc.empty() || !mp->up_done)
    return mfail(m, SPF_E_STATE, "spf_mplan_route_update_read: no update (call spf_mplan_route_update)");
  spf_mplan::Part& p = mp->parts[member];
  const uint64_t slots = p.dl_req.size();
  const uint64_t size[5] = {slots, slots ? p.dl_n[0] : 0, slots ? p.up_nrec[0] : 0, slots ? p.dl_n[1] : 0,
                            slots ? p.up_nrec[1] : 0};
  if (n) std::copy(size, size + 5, n);
  if (!slots) return SPF_OK;
  M_HIP(m, hipSetDevice(m->members[member]->device));
  const hipStream_t s = m->exec[member];
  uint64_t* const dptr[2] = {ip_dptr, label_dptr};
  uint32_t* const dset[2] = {ip_dset, label_dset};
  uint64_t* const uptr[2] = {ip_uptr, label_uptr};
  uint64_t* const urec[2] = {ip_urec, label_urec};
  for (uint32_t w = 0; w < 2; ++w) {
    const uint64_t e = p.dl_n[w], r = p.up_nrec[w];
    if (dptr[w]) M_HIP(m, hipMemcpyAsync(dptr[w], p.dl_ptr[w].p, 8 * (slots + 1), hipMemcpyDeviceToHost, s));
    if (dset[w] && e) M_HIP(m, hipMemcpyAsync(dset[w], p.dl_set[w].p, 4 * e, hipMemcpyDeviceToHost, s));
    if (uptr[w]) M_HIP(m, hipMemcpyAsync(uptr[w], p.up_ptr[w].p, 8 * (e + 1), hipMemcpyDeviceToHost, s));
    if (urec[w] && r) M_HIP(m, hipMemcpyAsync(urec[w], p.up_rec[w].p, 8 * r, hipMemcpyDeviceToHost, s));
  }
  if (label_uowner && p.dl_n[1])
    M_HIP(m, hipMemcpyAsync(label_uowner, p.up_owner.p, 4 * p.dl_n[1], hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  return SPF_OK;
}

spf_status spf_mplan_route_update_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_ip_uptr,
                                          const uint64_t** d_ip_urec, const uint32_t** d_label_uowner,
                                          const uint64_t** d_label_uptr, const uint64_t** d_label_urec,
                                          uint64_t* n_ip_rec, uint64_t* n_label_rec) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_update_buffers: bad argument");
  if (mp->dl_loc.empty() || !mp->up_done)
    return mfail(mp->m, SPF_E_STATE, "spf_mplan_route_update_buffers: no update (call spf_mplan_route_update)");
  const spf_mplan::Part& p = mp->parts[member];
  const bool has = !p.dl_req.empty();  // (a member without a me of the delta holds nothing of it)
  if (d_ip_uptr) *d_ip_uptr = has ? reinterpret_cast<const uint64_t*>(p.up_ptr[0].p) : nullptr;
  if (d_ip_urec) *d_ip_urec = has ? reinterpret_cast<const uint64_t*>(p.up_rec[0].p) : nullptr;
  if (d_label_uowner) *d_label_uowner = has ? p.up_owner.p : nullptr;
  if (d_label_uptr) *d_label_uptr = has ? reinterpret_cast<const uint64_t*>(p.up_ptr[1].p) : nullptr;
  if (d_label_urec) *d_label_urec = has ? reinterpret_cast<const uint64_t*>(p.up_rec[1].p) : nullptr;
  if (n_ip_rec) *n_ip_rec = has ? p.up_nrec[0] : 0;
  if (n_label_rec) *n_label_rec = has ? p.up_nrec[1] : 0;
  return SPF_OK;
}

spf_status spf_mplan_routes(spf_mplan* mp, uint32_t me_req, const uint32_t* set_ptr,
                            const uint32_t* set_nodes, uint32_t n_sets, uint32_t flags,
                            uint64_t* min_metric, uint32_t* nh_count, uint32_t* nh_edge,
                            uint64_t* nh_metric) {
  if (!mp || !set_ptr || !min_metric || !nh_count || !nh_edge || !nh_metric)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_routes: NULL argument");
  spf_mctx* m = mp->m;
  if (me_req >= mp->n_src) return mfail(m, SPF_E_INVALID, "me %u is not a request index", me_req);
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0;
  if (const spf_status st = route_prepare(mp, set_ptr, set_nodes, n_sets, lfa, nullptr, 0, &me_req, 1);
      st != SPF_OK)
    return st;
  const uint32_t r = mp->owner[me_req];
  spf_mplan::Part& p = mp->parts[r];
  spf_ctx* c = m->members[r];
  const uint32_t me = mp->srcs[me_req];
  const uint32_t deg = c->row_ptr[me + 1] - c->row_ptr[me];
  const size_t cap = (size_t)n_sets * std::max<uint32_t>(1, deg);
  M_HIP(m, hipSetDevice(c->device));
  const hipStream_t s = m->exec[r];
  IssuedGuard guard{m, {r}};  // &me and the caller's outputs outlive every queued copy
  M_HIP(m, p.rme.upload(&me, 1, s));
  M_HIP(m, p.rmin.alloc(std::max<uint32_t>(1, n_sets)));
  M_HIP(m, p.rcnt.alloc(std::max<uint32_t>(1, n_sets)));
  M_HIP(m, p.redge.alloc(cap));
  M_HIP(m, p.rmetric.alloc(cap));
  const spf_status st = launch_route_sets(c, p.rowp.p, p.nhp.p, p.rme.p, 1, p.rsp.p, p.rsn.p, n_sets, lfa,
                                          nullptr, nullptr, reinterpret_cast<uint64_t*>(p.rmin.p),
                                          p.rcnt.p, p.redge.p, reinterpret_cast<uint64_t*>(p.rmetric.p), s);
  if (st != SPF_OK) return member_fail(m, r, st);
  if (n_sets) {
    M_HIP(m, hipMemcpyAsync(min_metric, p.rmin.p, 8ull * n_sets, hipMemcpyDeviceToHost, s));
    M_HIP(m, hipMemcpyAsync(nh_count, p.rcnt.p, 4ull * n_sets, hipMemcpyDeviceToHost, s));
    if (deg) {
      M_HIP(m, hipMemcpyAsync(nh_edge, p.redge.p, 4ull * cap, hipMemcpyDeviceToHost, s));
      M_HIP(m, hipMemcpyAsync(nh_metric, p.rmetric.p, 8ull * cap, hipMemcpyDeviceToHost, s));
    }
  }
  M_HIP(m, hipStreamSynchronize(s));
  return SPF_OK;
}

uint32_t spf_mplan_closure_rows(const spf_mplan* mp, uint32_t member) {
  if (!mp || member >= mp->n_parts || !mp->parts[member].plan) return 0;
  return spf_plan_closure_rows(mp->parts[member].plan);
}

spf_status spf_mplan_enable_timing(spf_mplan* mp, uint32_t max_executes) {
  if (!mp) return SPF_E_INVALID;
  spf_mctx* m = mp->m;
  for (uint32_t i = 0; i < mp->n_parts; ++i) {
    spf_mplan::Part& p = mp->parts[i];
    if (!p.plan) continue;
    M_HIP(m, hipSetDevice(m->members[i]->device));
    for (hipEvent_t e : p.ev) (void)hipEventDestroy(e);
    p.ev.assign(2ull * max_executes, nullptr);
    for (auto& e : p.ev) M_HIP(m, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  }
  mp->timing_cap = max_executes;
  mp->timing_n = 0;
  return SPF_OK;
}

// per member: summed milliseconds of its executes (start to end on its
// stream), and the number of executes
spf_status spf_mplan_timing(spf_mplan* mp, double* ms, uint32_t* n) {
  if (!mp || !mp->timing_cap || !ms) return SPF_E_STATE;
  spf_mctx* m = mp->m;
  const uint32_t cnt = std::min(mp->timing_n, mp->timing_cap);
  for (uint32_t i = 0; i < mp->n_parts; ++i) {
    ms[i] = 0;
    spf_mplan::Part& p = mp->parts[i];
    if (!p.plan) continue;
    M_HIP(m, hipSetDevice(m->members[i]->device));
    for (uint32_t k = 0; k < cnt; ++k) {
      float t = 0;
      M_HIP(m, hipEventSynchronize(p.ev[2 * k + 1]));
      M_HIP(m, hipEventElapsedTime(&t, p.ev[2 * k], p.ev[2 * k + 1]));
      ms[i] += t;
    }
  }
  if (n) *n = cnt;
  mp->timing_n = 0;
  return SPF_OK;
}

}  // extern "C"
