// ============================================================================
//  engine_internal.h -- state shared by the engine's translation units: the
//  context (the graph's host state of graph_host.h plus its device copy and
//  the kernels' scratch), the plans (their host tables derived by
//  plan_host.h), and the launch functions each unit offers the others
//  (graph.cpp: the spf_graph_* calls; engine_ctx.cpp: the context;
//  spf_engine.hip: SPF/ECMP plans over the kernel units of spf_units.h;
//  ksp2.hip: batched KSP2; ...).  Not part of the C-ABI:
//  include/openr_spf.h is the boundary.
// ============================================================================
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "graph_host.h"
#include "openr_spf.h"
#include "plan_host.h"

namespace spfi {

// diagnostics buffer (SPF_STAMPS): 16 waves x 64 phase stamps of one block,
// the block selector, then a start / end s_memrealtime pair per block
constexpr uint32_t kStampBlocks = 1024;
constexpr uint32_t kStampWords = 64 * 16 + 1 + 2 * kStampBlocks;

extern thread_local std::string g_err;

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  // o's allocation moved here (nothing copied); o is left empty
  void take(DevBuf& o) {
    reset();
    p = o.p;
    n = o.n;
    o.p = nullptr;
    o.n = 0;
  }
  hipError_t alloc(size_t count) {
    if (count <= n && p) return hipSuccess;
    reset();
    const hipError_t e = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  hipError_t upload(const T* h, size_t count, hipStream_t s) {
    hipError_t e = alloc(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s);
  }
  // h[off, off + count) into the allocated buffer at the same offset
  hipError_t upload_at(const T* h, size_t off, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    if (!p || off + count > n) return hipErrorInvalidValue;
    return hipMemcpyAsync(p + off, h + off, count * sizeof(T), hipMemcpyHostToDevice, s);
  }
};

// Pinned host staging (hipHostMalloc): device-to-host copies at PCIe rate
// instead of the runtime's chunked pageable path.
template <typename T>
struct PinBuf {
  T* p = nullptr;
  size_t n = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { reset(); }
  void reset() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
  }
  hipError_t alloc(size_t count) {
    if (count <= n && p) return hipSuccess;
    reset();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T),
                                       hipHostMallocDefault);
    if (e == hipSuccess) n = count;
    return e;
  }
};

// exact_spf_kernel scratch (exact.hip): per-wave heap, labels, next hops.
struct ExactScratch {
  DevBuf<uint8_t> buf;
  DevBuf<uint32_t> ctr;  // next source
  uint64_t per_wave = 0;
  uint32_t waves = 0, wmax = 0;
};

// What-if batches on the exact kernel (zero / negative metrics, u64): one
// replayed runSpf per failure that touches a pathLink, digests vs the
// unfailed run (exact.hip).
// Change lists of a what-if batch (spf_whatif_changes; the EMIT instances of
// the repair kernels and of exact_whatif_kernel).  Count pass (cnode NULL): a
// team writes cnt[f] = the entries of failure f.  Fill pass: failure f's
// entries go to cptr[f] .. cptr[f + 1]; an entry past cptr[f + 1] sets kFaultListRoom
// of the context's fault word and is dropped.
struct WiEmit {
  uint32_t* cnt = nullptr;                    // [n_fail], zeroed before the count pass
  const unsigned long long* cptr = nullptr;   // [n_fail + 1] scanned counts
  uint32_t* cnode = nullptr;                  // [total]
  unsigned long long* cdist = nullptr;        // [total] (~0: now unreachable)
  uint32_t* cnh = nullptr;                    // [total][W]
  uint32_t W = 1;                             // words per entry
  uint32_t* fault = nullptr;
};

struct ExactWhatIf {
  ExactScratch xs;
  DevBuf<uint32_t> fails, link_edge, base_pop, base_nh;
  DevBuf<uint64_t> base_d;
  DevBuf<spf_whatif_digest> base_dig;
  uint32_t src = 0, n_fail = 0, W = 1;
};

// A list product of a what-if plan (whatif_pool.cpp): owner o holds entries
// ptr[o] .. ptr[o + 1] of key / val / rows, in the order the fill pass's
// atomics left them.  Built by count, scan (whatif_scan), pool_size from the
// scan's total, and fill; the arrays are kept while they are large enough.
//   change lists   owner = failure, key = node, val = metric, rows = next hops
//   route lists    owner = failure, key = set,  val = min metric, rows = next hops
//   impact lists   owner = node or set, key = failure, val = entry index, no rows
struct WiPool {
  bool valid = false;  // the call that builds it succeeded; nothing it reads was rebuilt since
  uint32_t n_owners = 0, W = 0;  // W: words per row (0: no row column)
  uint64_t total = 0;
  DevBuf<unsigned long long> ptr, val;  // [n_owners + 1], [total] (~0: unreachable / withdrawn)
  DevBuf<uint32_t> key, rows;           // [total], [total][W]
};

// Route lists of a what-if batch (spf_whatif_routes, whatif_routes.hip): the
// caller's sets and their inverse index on the device, the base in the lists'
// layout, every set's base route, the lookup table over the change lists'
// entries and the pool (all kept while they are large enough).
struct WiRoutes {
  WiPool pool;  // invalid after spf_whatif_changes or a failed call
  uint32_t n_sets = 0;
  double ms[4] = {0, 0, 0, 0};  // base + index, count, scan, fill of the last call
  DevBuf<uint32_t> d_set_ptr, d_set_nodes, d_inv_ptr, d_inv_set, d_inv_pos;
  DevBuf<unsigned long long> d_bd;  // [N] base metrics, ~0: unreachable
  DevBuf<uint32_t> d_bnh;           // [N][W] base rows, zero where unreachable
  DevBuf<unsigned long long> d_rbm;  // [n_sets] base routes
  DevBuf<uint32_t> d_rbnh;           // [n_sets][W]
  DevBuf<unsigned long long> d_keys;  // (failure << 32 | node), ~0: empty
  DevBuf<uint32_t> d_vals, d_efail;   // entry index per slot; failure per entry
  DevBuf<uint32_t> d_cnt, d_cur;      // [n_fail] counts, fill cursors
  // the table as the last successful call left it, for spf_whatif_route_update:
  // slots - 1, 0 when the call built none (no list entry, or no set to list)
  uint32_t tab_mask = 0;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~WiRoutes() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Impact by destination (spf_whatif_by_node / spf_whatif_by_set,
// whatif_impact.hip): the change or route lists transposed to key-major and
// every key's summary (kept while they are large enough).  A plan holds one
// per flavour.
struct WiImpact {
  WiPool pool;  // owners: the keys; invalid once its lists were rebuilt or a call failed
  double ms[3] = {0, 0, 0};  // count (with init), scan, fill of the last call
  DevBuf<uint32_t> d_cur;           // [n_keys] fill cursors
  DevBuf<spf_whatif_impact> d_imp;  // [n_keys]
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~WiImpact() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Route updates of a what-if batch (spf_whatif_route_update,
// whatif_route_update.hip): every failure's sets whose link-level records
// change, as two pools -- `ent` (owner = failure, key = set, val = min metric,
// no rows) and `rec` (owner = entry, val = record, no key and no rows) -- the
// source's row table, every set's base records and the pass's scratch (all
// kept while they are large enough).
struct WiUpdate {
  WiPool ent, rec;  // valid together: ent.valid says so
  uint32_t n_sets = 0, n_touch = 0;  // n_touch: failures that change a slot of src's row
  uint64_t base_records = 0;
  // base records, touch, count, scan, fill, the records' scan, records of the last call
  double ms[7] = {0, 0, 0, 0, 0, 0, 0};
  DevBuf<uint4> d_row;               // [slots of src] {neighbour bit, metric, link id, head}
  DevBuf<uint2> d_row_link;          // the live slots' (link id, slot in row), ascending link id
  DevBuf<unsigned long long> d_bptr, d_brec;  // [n_sets + 1], [base_records]
  DevBuf<uint32_t> d_bcnt;                    // [n_sets]
  DevBuf<uint32_t> d_tidx, d_tlist, d_tmask, d_tn;  // [n_fail], [n_touch], [n_touch][W], counters
  DevBuf<uint2> d_trange;                     // [n_touch] first and last non-zero word of the mask
  DevBuf<unsigned long long> d_mkeys;         // (failure << 32 | set) of the touched failures' route entries
  DevBuf<uint32_t> d_cnt, d_cur, d_usrc, d_rcnt;  // [n_fail] x 2, [entries] x 2
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~WiUpdate() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// What whatif_routes.hip, whatif_impact.hip and whatif_route_update.hip read
// of a plan (whatif.hip owns spf_whatif_plan): the change lists of the last
// spf_whatif_changes, the unfailed result as the plan holds it (u32 metrics
// with kInf and rows that are undefined where unreachable, or the exact
// plan's u64 ones), the plan's route lists, its two transpositions and its
// route updates, and the failures as the plan's kind describes them.
// kPoolByNode + SPF_WHATIF_BY_*
enum WiPoolId { kPoolChanges, kPoolRoutes, kPoolByNode, kPoolBySet, kPoolUpdate, kPoolUpdateRec };
struct WiListsView {
  spf_ctx* ctx = nullptr;
  const WiPool* changes = nullptr;
  WiRoutes* rt = nullptr;
  WiImpact* imp[2] = {nullptr, nullptr};  // SPF_WHATIF_BY_NODE, SPF_WHATIF_BY_SET
  WiUpdate* up = nullptr;
  const WiPool* pool(WiPoolId id) const {
    return id == kPoolChanges    ? changes
           : id == kPoolRoutes   ? &rt->pool
           : id == kPoolUpdate   ? &up->ent
           : id == kPoolUpdateRec ? &up->rec
                                  : &imp[id - kPoolByNode]->pool;
  }
  // the failures: kind 0 / SPF_WHATIF_LINK_METRIC: fails = link ids;
  // SPF_WHATIF_NODE_*: node ids; SPF_WHATIF_LINK_SET: fails = set_ptr
  // [n_fail + 1] into set_links; met = the metric plan's uint4 changes
  // {edge, reverse edge, their metrics under the change}
  uint32_t kind = 0;
  bool exact = false;  // the plan runs on the exact path
  const uint32_t* fails = nullptr;
  const uint32_t* set_links = nullptr;
  const void* met = nullptr;
  const uint32_t* nbr_bit = nullptr;  // [N] j if v is src's j-th distinct neighbour, else kInf
  bool no_nbr = false;  // src has no up neighbour (rows undefined)
  uint64_t epoch = 0;
  uint32_t src = 0, n_fail = 0, W = 1;
  const uint32_t* base_d32 = nullptr;  // one of the two
  const uint64_t* base_d64 = nullptr;
  const uint32_t* base_nh = nullptr;  // [N][W]
};

// KSP2 on the exact kernel: the sources' runs (labels, pop ranks), then a
// wave per pair tracing k = 1 and replaying k = 2 (exact.hip).
struct ExactKsp2 {
  ExactScratch xs_a, xs_b;
  DevBuf<uint32_t> srcs, POP;
  DevBuf<uint64_t> D;
  uint32_t n_src = 0, lw = 0;
};

}  // namespace spfi

// The graph itself (CSR, derived tables, versions) is the GraphHost base; here
// are its device copy and everything the kernels keep per context.
struct spf_ctx : spfi::GraphHost {
  int device = 0;
  uint32_t n_cu = 256;  // compute units (BFS batch sizing)
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;  // what-if workgroup teams (lazily created, lives with the ctx)
  hipEvent_t side_fork = nullptr, side_join = nullptr;
  // barrier-timeout word of this context's grid-resident / team launches
  // (spf_device_check reads and clears it)
  spfi::DevBuf<uint32_t> d_fault;
  bool team_off = false;  // a team barrier timed out: plans keep msbfs_kernel
  std::string err;
  uint64_t solves = 0;
  spfi::DevBuf<int32_t> d_met;
  spfi::ExactScratch exact1;  // spf_solve_exact (synchronous one-shot solves) only
  // msbfs_team_prepare's graph-derived tables for one team size (slices to
  // members, finalize slots, column streams, frontier slices each member
  // reads): valid while sell_ver holds, shared by every plan of the context
  struct TeamTables {
    uint64_t ver = ~0ull;
    uint32_t G = 0, own = 0, n_acc = 0, need_words = 0;
    bool full_copy = false;
    std::vector<uint32_t> fin, mptr, meta, need;
  } tm_tab;
  spfi::DevBuf<uint32_t> d_sell_ptr, d_sell_col;
  spfi::DevBuf<uint32_t> d_ms_smap;
  spfi::DevBuf<uint16_t> d_qcls, d_qtab;  // qt.cls, qt.tab (spfi::quotient_prepare)
  spfi::DevBuf<uint32_t> d_sell4_ptr, d_sell4;
  spfi::DevBuf<uint32_t> d_row_ptr, d_col, d_wt, d_rev, d_nb_ptr, d_nb_id, d_nb_w;
  spfi::DevBuf<uint32_t> d_edge_nb;
  spfi::DevBuf<uint8_t> d_ovl;
  // scratch for spf_preds
  spfi::DevBuf<uint32_t> d_pred_cnt, d_pred_edge, d_link, d_ign, d_one_src, d_row;
  spfi::DevBuf<unsigned long long> d_pred_key;
  spfi::DevBuf<uint32_t> d_gq, d_gq2, d_gbm, d_gctr;  // global-memory SSSP scratch
  spfi::DevBuf<uint32_t> d_gbar;  // its grid-barrier counters (grid_ops.h XGrid)
  // ecc_estimate's and depth_bound's memory of the graph (plan_host.h)
  spfi::DepthCache depth;
  // mssp_kernel tables (mssp.hip), valid for graph epoch mp_epoch
  spfi::DevBuf<uint32_t> d_mp_ell, d_mp_smap;
  spfi::DevBuf<uint32_t> d_mp_dep;  // per slice: the slices its nodes' out-edges reach (CSR)
  spfi::DevBuf<uint32_t> d_mp_cls;  // per wave: first slot of each width class (phased first sweep)
  uint32_t mp_ncls = 0;
  uint32_t mp_slots = 0, mp_ovf_at = 0;
  bool mp_redo = true;
  bool mp_u8 = false;  // u8 labels (four sources per LDS word)
  uint64_t mp_epoch = ~0ull;
  spfi::DevBuf<unsigned long long> d_stamps;  // BFS kernel phase stamps (SPF_STAMPS=1)
  // spf_plan_preds' pinned staging: lives with the context (the facade makes
  // a plan per query; pinning per plan cost more than it saved)
  spfi::PinBuf<uint32_t> pin_preds;
  // plan builds' host-to-device uploads (spfi::stage_upload): one pinned
  // buffer, copies queued on `stream`, reused once `stream` has synchronised
  spfi::PinBuf<uint8_t> stage;
  size_t stage_used = 0;
  // the open spf_ksp2_snapshot of this context (destroyed with it at the latest)
  std::vector<spf_ksp2_snapshot*> ksp2_snaps;
  // spf_routes' (routes.hip) last plan, kept while its sources and the graph
  // shape hold (executes re-derive it after in-place patches), and its
  // buffers, which only grow: a route build per publication allocates nothing
  struct RouteCache {
    spf_plan* plan = nullptr;
    std::vector<uint32_t> srcs;
    uint64_t shape = ~0ull;
    spfi::DevBuf<uint32_t> dist, nh, ecol, ew, ej, sp, sn, cnt, edge;
    spfi::DevBuf<uint64_t> mn, metric;
  } rt;
};

namespace spfi {
// A plan build's uploads (build_plan, msbfs_team_prepare) through the
// context's pinned stage: a pageable hipMemcpyAsync is a blocking staged copy
// (~35 us each on MI355X boxes, a dozen per build_plan), a pinned one is only
// queued.  Copies go on c->stream; the stage is reused after that stream has
// synchronised (here when it runs full, and stage_done after a build's final
// synchronize).  Payloads above kStageMax take the plain path.
constexpr size_t kStageMax = 8u << 20;
// bytes from host memory to device memory through the stage (queued on c->stream)
inline hipError_t stage_copy(spf_ctx* c, void* dst, const void* h, size_t bytes) {
  if (bytes == 0) return hipSuccess;
  if (bytes > kStageMax) return hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, c->stream);
  size_t at = (c->stage_used + 255) & ~(size_t)255;
  if (!c->stage.p || at + bytes > c->stage.n) {
    if (c->stage_used) {
      const hipError_t e = hipStreamSynchronize(c->stream);  // every copy out of the stage has landed
      if (e != hipSuccess) return e;
    }
    c->stage_used = at = 0;
    if (bytes > c->stage.n || !c->stage.p) {
      const hipError_t e = c->stage.alloc(std::max<size_t>(std::max<size_t>(bytes, 2 * c->stage.n), 1u << 20));
      if (e != hipSuccess) return e;
    }
  }
  std::memcpy(c->stage.p + at, h, bytes);
  c->stage_used = at + bytes;
  return hipMemcpyAsync(dst, c->stage.p + at, bytes, hipMemcpyHostToDevice, c->stream);
}
template <typename T>
hipError_t stage_upload(spf_ctx* c, DevBuf<T>& d, const T* h, size_t count) {
  const hipError_t e = d.alloc(count);
  if (e != hipSuccess || count == 0) return e;
  return stage_copy(c, d.p, h, count * sizeof(T));
}
// h[off, off + count) into the allocated buffer at the same offset
template <typename T>
hipError_t stage_upload_at(spf_ctx* c, DevBuf<T>& d, const T* h, size_t off, size_t count) {
  if (count == 0) return hipSuccess;
  if (!d.p || off + count > d.n) return hipErrorInvalidValue;
  return stage_copy(c, d.p + off, h + off, count * sizeof(T));
}
// after a synchronize of c->stream: the stage's copies are done
inline void stage_done(spf_ctx* c) { c->stage_used = 0; }
}  // namespace spfi

struct spf_plan {
  spf_ctx* ctx = nullptr;
  uint32_t n_src = 0, flags = 0;
  uint64_t shape = 0, epoch = 0;  // graph state the plan was derived from
  uint64_t layout = 0;             // c->layout its next-hop layout was taken at
  std::vector<uint32_t> srcs, closure;
  std::vector<uint64_t> nh_off;
  std::vector<uint32_t> words;
  uint64_t nh_total = 0;
  bool direct = false;  // closure == srcs: D is the caller's dist buffer
  bool prefix = false;  // closure[i] == srcs[i] for i < n_src (distinct sources)
  bool ms = false;      // unit metrics: multi-source BFS
  bool narrow = false;  // ... writing the u8 narrow copy for the next-hop pass
  bool sliced = false;  // ... and the next-hop pass on its bit-sliced form
  bool expand = false;  // ... the u32 rows expanded from the u8 ones (BFS stores bytes only)
  bool exact = false;   // exact_spf_kernel (exact.hip): zero/negative metrics, u64, any size
  bool mp = false;      // weighted: mssp_kernel (mssp.hip), S sources per workgroup
  bool pl_order = false;  // planes BFS: rows batched deepest-first (d_pl_order)
  bool sdirect = false;   // team plan writing the sliced rows itself (kTeamPlanes planes, no u8 rows)
  // msbfs_team_kernel (msbfs_team.hip): G workgroups per batch when the plan
  // has too few batches to fill the chip (tm_G == 0: msbfs_kernel)
  uint32_t tm_G = 0, tm_own = 0, tm_teams = 0, tm_bs = 0, tm_nacc = 0;
  uint32_t tm_rptr_at = 0, tm_runs_at = 0;  // d_tm_map = finalize slots | stream ranges | streams
  uint32_t tm_need_at = 0, tm_need_words = 0;  // ... | per-member frontier slice masks
  uint32_t tm_drained_at = 0, tm_n_drained = 0;  // ... | the drained nodes
  uint32_t tm_push_at = 0, tm_push_n = 0;  // ... | batch push offsets [tm_push_n] | push lists
  spfi::DevBuf<uint32_t> d_tm_map, d_tm_F, d_tm_bar;
  spfi::DevBuf<uint32_t> d_pl_order;
  spfi::DevBuf<uint32_t> d_redo;  // mp: rows whose u16 labels may have overflowed
  uint32_t wmax = 0;    // exact: max next-hop words per node over the plan's sources
  spfi::ExactScratch xs;  // exact: the kernel's scratch, reserved by build_plan
  spfi::DevBuf<uint32_t> d_srcs, d_closure, d_row_of, d_req_rows, d_D;
  spfi::DevBuf<uint8_t> d_Dn;
  spfi::DevBuf<uint32_t> d_S, d_maxd;  // sliced rows (+ dead row); deepest BFS level + 8 counters
  spfi::DevBuf<uint32_t> d_units, d_unit_off;  // sliced pass: uint4 work units per XCD
  spfi::DevBuf<uint32_t> d_gtab;  // sliced pass: source groups ([n, sources...] each)
  uint32_t max_xcd_units = 0;
  // class rows (ms plans on a quotient graph, plan_host.h ClassRows):
  // class_bfs_kernel solves cls_k class sources into d_Dc[cls_k][cls_pitch]
  // (u16), expand_rows_kernel writes the u32 rows and the bit planes from
  // them.  The u8 rows exist only once someone asked (plan_ensure_narrow):
  // keep_narrow then has every execute's expansion write them too.
  bool cls = false, keep_narrow = false;
  bool cls_ready = false;  // d_Dc holds the class rows of an execute on the current tables
  uint32_t cls_k = 0, cls_pitch = 0;
  spfi::DevBuf<uint32_t> d_csrc, d_crow_of;
  spfi::DevBuf<uint8_t> d_cfwd;
  spfi::DevBuf<uint16_t> d_Dc;
  bool big = false;  // spf_big_kernel (grid_spf.hip): graphs beyond the LDS kernels
  spfi::DevBuf<uint32_t> b_q, b_q2, b_bm, b_ctr, b_nbr_bit, b_nhb, b_lvl, b_order, b_misc, b_parent;
  spfi::DevBuf<uint32_t> b_bar;  // spf_big_kernel's grid-barrier counters
  spfi::DevBuf<uint64_t> d_nh_off;
  spfi::DevBuf<uint32_t> d_words;  // [n_src] next-hop bitmaps per source (spf_plan_digest)
  spfi::DevBuf<uint32_t> d_nb_row, d_nb_row_off, d_nb_drained;  // next-hop pass inputs
  uint32_t dead = 0;  // nb_row value of a drained neighbour
  spfi::DevBuf<uint32_t> d_slot_src;  // next-hop blocks: source per (slot, XCD)
  spfi::DevBuf<uint32_t> h_dist, h_nh;  // spf_plan_execute_host staging
  uint64_t h_epoch = ~0ull;              // graph epoch of the rows in h_dist
  spfi::DevBuf<uint32_t> h_pcnt, h_pedge;  // spf_plan_preds scratch
  spfi::DevBuf<unsigned long long> h_pkey;  // ... its sort keys
  size_t slots = 0;
  size_t lds_bytes = 0;
  bool q16 = true;
  // optional per-kernel timing: 4 events per execute (before the distance
  // kernel, after it, after the row slicing, after ECMP), ring of
  // `timing_cap` executes
  std::vector<hipEvent_t> ev;
  uint32_t timing_cap = 0, timing_n = 0;
  ~spf_plan() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

// A KSP2 source batch (ksp2.hip) and, once spf_ksp2_routes ran on it, every
// source's KSP2_ED_ECMP routes (ksp2_routes.hip).
namespace spfi {
constexpr uint32_t kKsp2Chunk = 64;  // sources per KSP2 workgroup (default)
constexpr uint32_t kKsp2Grab = 256;  // pool words a KSP2 wave reserves at a time

// spf_ksp2_routes' state: inputs staged on the device, the exactly sized
// pools (kept while they are large enough) and the last call's totals.
struct Ksp2Routes {
  bool valid = false;  // a call succeeded and nothing failed since
  uint64_t gen = 0;    // bumped by every spf_ksp2_routes and by a snapshot: which pools a delta compared
  uint32_t n_sets = 0;
  uint64_t hops = 0, words = 0;
  double ms[3] = {0, 0, 0};  // count, scan, fill of the last call
  uint64_t links_epoch = ~0ull;  // graph epoch d_links was built for
  uint32_t max_link = 0;
  DevBuf<uint32_t> d_links;  // per link id 8 words: both directed CSR edges (Ksp2LinkEnds)
  DevBuf<uint32_t> d_set_ptr, d_set_nodes;
  DevBuf<int32_t> d_prepend, d_label;
  DevBuf<unsigned long long> d_rptr, d_lbase, d_sums, d_rec, d_lptr;
  DevBuf<int32_t> d_lab;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Ksp2Routes() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// spf_ksp2_route_delta's and spf_ksp2_route_update's state
// (ksp2_route_delta.hip): the lists and the payload pools of the last calls
// (kept while they are large enough) and their scratch.
struct Ksp2Delta {
  bool valid = false;     // a delta succeeded and nothing failed since
  bool up_valid = false;  // ... and an update of that delta
  uint64_t gen = 0;       // Ksp2Routes::gen of the pools the delta compared
  uint64_t entries = 0, tot[3] = {0, 0, 0};  // delta: updates, deletes, routes matched as sets
  uint64_t up_tot[3] = {0, 0, 0};            // update: update entries, records, label words
  double ms[6] = {0, 0, 0, 0, 0, 0};         // count, scan, fill of the delta, then of the update
  DevBuf<unsigned long long> d_key;   // [E] key_new
  DevBuf<uint8_t> d_kind;             // [n_routes]
  DevBuf<unsigned long long> d_blk, d_sums, d_dptr, d_cnt;  // block counts, scan scratch, [n_src + 1], {deletes, matched, fault}
  DevBuf<uint32_t> d_dset;            // [entries]
  DevBuf<unsigned long long> d_uptr, d_usrc, d_urec, d_ulptr, d_ulsrc;  // [entries + 1], [entries], [records], [records + 1], [records]
  DevBuf<int32_t> d_ulab;             // [label words]
  hipEvent_t ev[13] = {};  // 0-4: the delta's marks; 5-12: the update's
  ~Ksp2Delta() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
}  // namespace spfi

// A generation of KSP2 routes moved out of its plan (spf_ksp2_route_snapshot,
// ksp2_route_delta.hip): the pools, their sizes, what the plan was over, and
// key_old[e] = link_hash[link_id[e]] of the graph as it was.
struct spf_ksp2_snapshot {
  spf_ctx* ctx = nullptr;
  std::vector<uint32_t> srcs;
  uint32_t n_nodes = 0, n_sets = 0, n_edges = 0;
  uint64_t hops = 0, words = 0;
  spfi::DevBuf<unsigned long long> rptr, rec, lptr, key;
  spfi::DevBuf<int32_t> lab;
  ~spf_ksp2_snapshot();
};

struct spf_ksp2_plan {
  spf_ctx* ctx = nullptr;
  uint32_t n_src = 0, lw = 0;
  uint32_t delta = 0;  // bucket width of the k = 2 SPF (KspArgs::delta)
  uint32_t chunk = spfi::kKsp2Chunk;  // sources per workgroup
  uint32_t grab = spfi::kKsp2Grab;    // pool words per wave reservation
  uint64_t epoch = 0;  // graph state the plan was derived from
  std::vector<uint32_t> srcs;
  spfi::DevBuf<uint32_t> d_srcs, d_D, d_H, d_all, d_wt_rev;
  spfi::DevBuf<uint8_t> d_no_drain;
  spfi::DevBuf<unsigned long long> d_prof;  // SPF_KSP2_PROF diagnostics
  size_t lds = 0;
  uint32_t lds_waves = 0;  // > 0: the staged-graph kernel with this many waves
  bool compact = false;     // ... with u16 labels, and the u32 redo pass behind it
  uint32_t lw_links = 0, redo_waves = 0;
  size_t redo_lds = 0;
  spfi::DevBuf<unsigned long long> d_redo;  // [n_src * N] pairs handed to the redo pass
  std::vector<hipEvent_t> ev;
  uint32_t timing_cap = 0, timing_n = 0;
  // outside the batched kernel's envelope (metrics <= 0, u64 labels, more
  // than 65535 nodes or a working set past the LDS): the exact kernel
  std::unique_ptr<spfi::ExactKsp2> exact;
  spfi::Ksp2Routes rt;  // spf_ksp2_routes (ksp2_routes.hip)
  spfi::Ksp2Delta dl;   // spf_ksp2_route_delta / _update (ksp2_route_delta.hip)
  ~spf_ksp2_plan() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

namespace spfi {

spf_status fail(spf_ctx* c, spf_status st, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                   \
  do {                                                                       \
    const hipError_t e_ = (expr);                                            \
    if (e_ != hipSuccess)                                                    \
      return fail(ctx, e_ == hipErrorOutOfMemory ? SPF_E_NOMEM : SPF_E_HIP,   \
                  "%s: %s (%s:%d)", #expr,                                   \
                  hipGetErrorString(e_), __FILE__, __LINE__);                \
  } while (0)

// Upload an ignore set (undirected link ids) as a device bitmap; NULL if empty.
spf_status upload_ignore(spf_ctx* c, const uint32_t* ignore, uint32_t n_ignore,
                         const uint32_t** dev);

// Launch the per-source SSSP kernel (distances only) over `rows` sources
// (device list rows_src), writing rows [rows][pitch] of D.
// wt / ovl override the graph's metrics / drain bits (e.g. transposed
// metrics and no drains for distances TO the rows' nodes).
spf_status launch_sssp(spf_ctx* c, const uint32_t* rows_src, uint32_t rows, bool hop,
                       const uint32_t* ign, uint32_t* D, hipStream_t s,
                       const uint32_t* wt = nullptr, const uint8_t* ovl = nullptr,
                       uint8_t* Dn = nullptr, const uint32_t* redo = nullptr);
// Multi-source weighted distances (mssp.hip): mssp_words() = LDS words per
// node (0: does not apply), mssp_prepare() builds its tables for the current
// graph epoch (plan build), launch_mssp() enqueues it (+ the overflow redo
// pass over `redo` = [1 + rows] words of plan scratch).
uint32_t mssp_words(const spf_ctx* c);
uint32_t mssp_sources(const spf_ctx* c);
// Team BFS (msbfs_team.hip): the team size for a unit plan of `rows` rows
// (0: not used), its tables, its launch, its barrier-timeout flag.
uint32_t msbfs_team_size(const spf_ctx* c, uint32_t rows);
spf_status msbfs_team_prepare(spf_ctx* c, spf_plan* p, uint32_t G);
spf_status launch_msbfs_team(spf_ctx* c, spf_plan* p, const uint32_t* rows_src, uint32_t rows,
                             uint32_t* D, uint8_t* Dn, uint32_t* maxd, hipStream_t s,
                             uint32_t d_rows,  // u32 rows written: closure rows < d_rows
                             uint32_t* S = nullptr, uint32_t s_stride = 0);  // sdirect planes
// planes per word of the rows msbfs_team_kernel slices itself (sdirect plans)
constexpr uint32_t kTeamPlanes = 4;
spf_status mssp_prepare(spf_ctx* c);
spf_status mssp_set_lds_limits(spf_ctx* c);
spf_status launch_mssp(spf_ctx* c, const uint32_t* rows_src, uint32_t rows, uint32_t* D,
                       uint8_t* Dn, uint32_t* redo, hipStream_t s, uint32_t* maxd = nullptr);
// Single-source SSSP in global memory, one grid-resident launch (any graph
// size, grid_spf.hip); scratch lives in the context.  dist = [N].
spf_status launch_gsssp(spf_ctx* c, uint32_t src, bool hop, const uint32_t* ign, uint32_t* dist,
                        hipStream_t s);
// The exact kernel (exact.hip) over n_src sources: dist rows (u32 or u64,
// pitch entries), planar next-hop bitmaps at nh_off, optional pop ranks.
spf_status exact_reserve(spf_ctx* c, ExactScratch* x, uint32_t n_src, uint32_t Wmax,
                         uint64_t extra = 0);
spf_status exact_whatif_prepare(spf_ctx* c, ExactWhatIf* x, uint32_t src,
                                const std::vector<uint32_t>& fails,
                                const std::vector<uint32_t>& link_edge);
// em (change lists): the EMIT instance, one pass (count or fill) per call;
// base_run false skips the unfailed run (the fill pass: base_* are there).
spf_status exact_whatif_launch(spf_ctx* c, ExactWhatIf* x, spf_whatif_digest* d_out,
                               spf_whatif_digest* d_base, hipStream_t s, hipEvent_t mid,
                               const WiEmit* em = nullptr, bool base_run = true);
spf_status exact_ksp2_prepare(spf_ctx* c, ExactKsp2* x, const std::vector<uint32_t>& srcs);
spf_status exact_ksp2_launch(spf_ctx* c, ExactKsp2* x, spf_ksp2_pair* d_pairs, uint32_t* d_pool,
                             uint64_t pool_words, uint64_t* d_counters, hipStream_t s,
                             hipEvent_t mid);
spf_status launch_exact(spf_ctx* c, ExactScratch* x, const uint32_t* d_srcs, uint32_t n_src,
                        const uint64_t* d_nh_off, uint32_t Wmax, bool hop, bool dist64,
                        const uint32_t* ign, void* d_dist, uint32_t* d_nh, uint32_t* d_pop,
                        hipStream_t s);
// A what-if plan's lists, base, route-list and impact state (whatif.hip), for
// spf_whatif_routes (whatif_routes.hip) and spf_whatif_by_node / _by_set
// (whatif_impact.hip); p is not NULL.
void whatif_lists_view(spf_whatif_plan* p, WiListsView* v);
// Every pool's scan (whatif_scan_kernel, whatif.hip) on `s`: ptr[0 .. n] = the
// exclusive scan of cnt[0], cnt[stride], ... (n counts) and the total.
// stride is 1 (a plain array) or 8 (spf_whatif_impact::n_changed).
hipError_t whatif_scan(const uint32_t* cnt, uint32_t stride, uint32_t n, unsigned long long* ptr,
                       hipStream_t s);
constexpr uint32_t kWhatifScanTile = 8192;  // counts the scan's workgroup takes per round
// What the pools share on the host (whatif_pool.cpp).  `who` is the C call's
// name, in front of every message.
// v = the view of plan p when it holds pool `id`; else "NULL plan" (p NULL) or
// "the plan holds no <lists>".
spf_status pool_held(spf_whatif_plan* p, WiPoolId id, const char* who, WiListsView* v);
// key / val / rows for `total` entries of W words, exactly (at least one);
// all three freed and SPF_E_NOMEM when the device has no room.  Sets q->W.
spf_status pool_size(spf_ctx* c, WiPool* q, uint64_t total, uint32_t W, const char* who);
uint64_t pool_bytes(const WiPool& q);  // offsets and entries
// The _read, _buffers and _db calls of pool `id` (any output may be NULL;
// rows are left alone in a pool without a row column).  _db: the owner's
// entries ascending by (key, val), *n their number, SPF_E_NOMEM past `cap`.
spf_status pool_read(spf_whatif_plan* p, WiPoolId id, const char* who, uint64_t* ptr, uint32_t* key,
                     uint64_t* val, uint32_t* rows);
spf_status pool_buffers(spf_whatif_plan* p, WiPoolId id, const char* who, const uint64_t** d_ptr,
                        const uint32_t** d_key, const uint64_t** d_val, const uint32_t** d_rows,
                        uint32_t* n_owners, uint32_t* W, uint64_t* n_entries);
spf_status pool_db(spf_whatif_plan* p, WiPoolId id, const char* who, uint32_t owner, uint32_t* key,
                   uint64_t* val, uint32_t* rows, uint64_t cap, uint64_t* n);
// spf_big_kernel (grid_spf.hip): the plan's sources one after another on the
// whole chip -- frontier SSSP into the dist rows, next hops in distance
// order, transposed into the plan's bitmaps.  Positive metrics or hop counts.
spf_status launch_big(spf_ctx* c, spf_plan* p, uint32_t* d_dist, uint32_t* d_nh, bool hop,
                      hipStream_t s);
// The launch rule of every kernel whose blocks meet at barriers (grid_spf.hip):
// launch_resident is a regular launch checked for co-residency, coop_blocks the
// grid of a 512-thread grid-barrier kernel at `per_cu` blocks per CU.
hipError_t launch_resident(const void* kernel, uint32_t blocks, uint32_t threads, void** args,
                           uint32_t n_cu, hipStream_t s);
uint32_t coop_blocks(spf_ctx* c, const void* kernel, uint32_t per_cu);
// whatif_base_kernel (grid_spf.hip), the unfailed pass of a what-if batch --
// SPF of `src`, next-hop rows of W words, parent subtree sizes, result hash --
// over a plan's buffers (whatif.hip fills this from spf_whatif_plan).
constexpr uint32_t kLevelCap = 1u << 16;  // distance values bucketed directly (lvl's size - 1)
#pragma GCC visibility push(hidden)
struct BaseBufs {
  uint32_t src, W;
  const uint32_t* nbr_bit;  // [N] j if v is src's j-th distinct neighbour, else kInf
  uint32_t *dist, *q, *q2, *bm, *ctr;  // [N] x 3, [ceil(N / 32)], [4]
  uint32_t* bar;                       // [kGridBarWords]
  uint32_t *nhb, *lvl, *order, *misc;  // [N][W], [kLevelCap + 1], [N], [8]
  unsigned long long* H;
  uint32_t *parent, *sub;              // [N] x 2
  unsigned long long *prof, *lprof;    // SPF_WHATIF_PROF: [16] phase clocks, [2 x 64] per level; or NULL
};
spf_status launch_base(spf_ctx* c, const BaseBufs& b, hipStream_t s);
#pragma GCC visibility pop
// Raise the dynamic-LDS limit of the engine's LDS-resident kernels (once per
// process; each unit registers its own, spf_units.h).
spf_status set_lds_limits(spf_ctx* c);
// msbfs_kernel's twin-class quotient: its tables rebuilt and uploaded when
// stale (graph.cpp); whether the BFS sweeps it, and whether the register-plane
// BFS runs instead (msbfs.hip, with the kernels)
spf_status quotient_prepare(spf_ctx* c);
bool use_quotient(const spf_ctx* c);
bool use_planes(const spf_ctx* c);
// The u8 rows of a plan (closure order, npitch bytes each, the dead row behind
// them) for readers outside the step: true when the plan can provide them;
// plan_ensure_narrow makes p->d_Dn hold the last execute's (class plans fill
// them on the first call, on stream s, and keep them from then on).
bool plan_has_narrow(const spf_plan* p);
spf_status plan_ensure_narrow(spf_plan* p, hipStream_t s);
// Order a launch whose workgroups wait on each other (grid barriers, team
// BFS) on stream s after the previous such launch of this process on the
// same device, whatever context or stream that was on: two of them running
// at once could each hold part of the CUs the other's members need (each
// waits for members that cannot become resident until it exits).  Call
// before the launch, then resident_done(c, s) after it.
spf_status resident_order(spf_ctx* c, hipStream_t s);
spf_status resident_done(spf_ctx* c, hipStream_t s);
void resident_forget(const spf_ctx* c);
// Materialised route databases of many `me` (routes.hip kRsDb): per me slot
// its headers (n_sets words), where its region of the record pool starts
// (n_chunks x 256 x deg(me) records), its record count (zeroed before the
// launch, added to) and the error flags.
// The exactly sized layout (SPF_ROUTE_COMPACT; kRsCount / kRsFill) takes two
// launches, pass = 1 then 2, with launch_label_scan over hdr[n_me * n_sets]
// (+ 1 for the total) and launch_route_block_starts in between: pass 1 leaves
// each route's count in hdr, pass 2 reads the scanned hdr and bstart, writes
// the records into pool and the headers over hdr; base and count are unused.
struct RouteDbOut {
  unsigned long long* hdr = nullptr;
  unsigned long long* pool = nullptr;
  const unsigned long long* base = nullptr;
  uint32_t* count = nullptr;
  uint32_t* flags = nullptr;
  uint32_t pass = 0;                           // 0: tiled (kRsDb); 1: count; 2: fill
  const unsigned long long* bstart = nullptr;  // (fill) per block its first record, the total last
  uint32_t stage = 0;                          // (fill) records a block may assemble in LDS
  uint32_t nt = 0;                             // (fill) streaming stores for the spans stored directly
};
// sets per kRsDb tile (the [deg][sets] tiles of a route database region) =
// routes per block of the count and fill passes
uint32_t route_db_tile_sets();
// records a fill block assembles in LDS before it stores them (longer spans
// are stored directly, with plain stores or, SPF_ROUTE_COMPACT_NT=1, streaming
// ones; SPF_ROUTE_STAGE=records: A/B, 0 = never)
uint32_t route_compact_stage();
// bstart[slot * n_chunks + chunk] = scanned[slot * n_sets + chunk *
// route_db_tile_sets()], bstart[n_me * n_chunks] = scanned[n_me * n_sets];
// n_chunks = ceil(n_sets / route_db_tile_sets())
spf_status launch_route_block_starts(spf_ctx* c, const unsigned long long* d_scanned, uint32_t n_me,
                                     uint32_t n_sets, unsigned long long* d_bstart, hipStream_t s);
// Route selection over resident rows for many `me` (routes.hip): digests per
// me (d_digest, n_me slots, added to), their route databases (db), or
// spf_routes' records of ONE me.
spf_status launch_route_sets(spf_ctx* c, const unsigned long long* d_rowp,
                             const unsigned long long* d_nhp, const uint32_t* d_me, uint32_t n_me,
                             const uint32_t* d_set_ptr, const uint32_t* d_set_nodes, uint32_t n_sets,
                             bool lfa, const unsigned long long* d_link_hash,
                             unsigned long long* d_digest, uint64_t* d_min, uint32_t* d_cnt,
                             uint32_t* d_edge, uint64_t* d_metric, hipStream_t s,
                             const RouteDbOut* db = nullptr,
                             const unsigned long long* d_nrowp = nullptr);
// Node-label MPLS routes of many `me` over resident rows (label_routes.hip):
// the count pass (fill = false: d_owner[n_me * G], the counts into d_ptr) or
// the fill pass (d_rec at the scanned d_ptr; d_flags bit 1: a metric past
// 2^32 - 1).  Label group g = d_grp_nodes[d_grp_ptr[g] .. d_grp_ptr[g + 1]).
spf_status launch_label_routes(spf_ctx* c, bool fill, const unsigned long long* d_rowp,
                               const unsigned long long* d_nhp, const uint32_t* d_me, uint32_t n_me,
                               const uint32_t* d_grp_ptr, const uint32_t* d_grp_nodes, uint32_t G,
                               bool lfa, uint32_t* d_owner, unsigned long long* d_ptr,
                               unsigned long long* d_rec, uint32_t* d_flags, hipStream_t s);
// d_ptr[0 .. n) -> its exclusive scan in place, d_ptr[n] = the total; d_sums =
// label_scan_tiles(n) words of scratch.  Deterministic.
uint64_t label_scan_tiles(uint64_t n);
uint32_t label_scan_tile();  // entries per tile
spf_status launch_label_scan(spf_ctx* c, unsigned long long* d_ptr, uint64_t n,
                             unsigned long long* d_sums, hipStream_t s);
// Prefix routes of many `me` over resident rows (prefix_routes.hip): the count
// pass (fill = false: d_info[n_me * P] = best | |B| << 32 | status << 56, the
// counts into d_ptr) or the fill pass (d_rec at the scanned d_ptr); d_flags bit
// 1: a metric past 2^32 - 1.  Prefix p = d_ent[d_pfx_ptr[p] .. d_pfx_ptr[p + 1])
// (prefix_table_host.h).  prefix_routes_threads / _links: the prefixes of a
// block, the links it stages at a time.
struct PrefixEnt;
spf_status launch_prefix_routes(spf_ctx* c, bool fill, const unsigned long long* d_rowp,
                                const unsigned long long* d_nhp, const uint32_t* d_me, uint32_t n_me,
                                const uint32_t* d_pfx_ptr, const PrefixEnt* d_ent, uint32_t P, bool lfa,
                                bool all_best, unsigned long long* d_info, unsigned long long* d_ptr,
                                unsigned long long* d_rec, uint32_t* d_flags, hipStream_t s);
uint32_t prefix_routes_threads();
uint32_t prefix_routes_links();
// Route-database delta between two generations (route_delta.hip), per member:
// its me slots' node ids, where each me's OLD row started and how long it was,
// key[e] = link_hash[link_id[e]] over the old and the new CSR, and same[slot]
// (written by launch_delta_rows: me's row has one key sequence in both).
struct RouteDeltaIn {
  const uint32_t* me = nullptr;
  const uint32_t* old_e0 = nullptr;
  const uint32_t* old_deg = nullptr;
  const unsigned long long* key_old = nullptr;
  const unsigned long long* key_new = nullptr;
  uint32_t* same = nullptr;
};
// blocks per me of the count / fill passes over `cells` routes per me
uint32_t route_delta_chunks(uint32_t cells);
spf_status launch_delta_rows(spf_ctx* c, const RouteDeltaIn& in, uint32_t n_me, hipStream_t s);
// count passes: kind[n_me * cells] (0 unchanged, 1 update, 2 delete) and the
// changed routes of every block into blk[n_me * route_delta_chunks(cells)].
// old_*: per me slot the device address of its old headers / region (IP), of
// its old owner and offset rows and the old record pool (labels); map_old /
// map_new[u]: label u of the union's group index in its generation.
spf_status launch_delta_ip(spf_ctx* c, const RouteDeltaIn& in, uint32_t n_me, uint32_t S,
                           const unsigned long long* new_hdr, const unsigned long long* new_pool,
                           const unsigned long long* new_base, const unsigned long long* old_hdr,
                           const unsigned long long* old_pool, uint8_t* kind, unsigned long long* blk,
                           hipStream_t s);
spf_status launch_delta_labels(spf_ctx* c, const RouteDeltaIn& in, uint32_t n_me, uint32_t U,
                               const uint32_t* new_owner, const unsigned long long* new_ptr,
                               const unsigned long long* new_rec, uint32_t Gn,
                               const unsigned long long* old_owner, const unsigned long long* old_ptr,
                               const unsigned long long* old_rec, const uint32_t* map_old,
                               const uint32_t* map_new, uint8_t* kind, unsigned long long* blk,
                               hipStream_t s);
// fill pass over the scanned blk: entries (vals[cell] or the cell index, |
// SPF_DELTA_DELETE) into dset, dptr[n_me + 1], *deletes += the deleted routes
spf_status launch_delta_fill(spf_ctx* c, const uint8_t* kind, uint32_t cells, uint32_t n_me,
                             const unsigned long long* blk, const uint32_t* vals, uint32_t* dset,
                             unsigned long long* dptr, unsigned long long* deletes, hipStream_t s);
// The delta's payload (route_update.hip), per member and kind over its delta
// lists dptr[n_me + 1] / dset[entries].  Count passes: entry j's records into
// uptr[j] (scanned in place afterwards with launch_label_scan), its first source
// record | stride << 48 into src[j]; IP from the headers and region starts of
// the current database, labels (dset holds label values: searched in the
// delta's union lab[U], mapped by map_new to the new generation's group) from
// its owner / offset arrays, with the new owner into uowner[j].  Fill: entry j's
// records from pool into urec[uptr[j] .. uptr[j + 1]), route_update_group()
// lanes per entry.
uint32_t route_update_group();
spf_status launch_update_count_ip(spf_ctx* c, const unsigned long long* dptr, const uint32_t* dset,
                                  uint32_t n_me, uint64_t entries, const unsigned long long* hdr,
                                  const unsigned long long* base, uint32_t S, unsigned long long* uptr,
                                  unsigned long long* src, hipStream_t s);
spf_status launch_update_count_labels(spf_ctx* c, const unsigned long long* dptr, const uint32_t* dset,
                                      uint32_t n_me, uint64_t entries, const uint32_t* lab,
                                      const uint32_t* map_new, uint32_t U, const uint32_t* owner,
                                      const unsigned long long* ptr, uint32_t G, unsigned long long* uptr,
                                      unsigned long long* src, uint32_t* uowner, hipStream_t s);
spf_status launch_update_fill(spf_ctx* c, const unsigned long long* uptr, const unsigned long long* src,
                              uint64_t entries, const unsigned long long* pool, unsigned long long* urec,
                              hipStream_t s);
// pathLinks of `src` from its u32 distance row on the device (spf_preds
// without the upload; spf_mplan_preds reads a resident row).
spf_status preds_from_row(spf_ctx* c, uint32_t src, bool hop, const uint32_t* ign,
                          const uint32_t* d_row, uint32_t* pred_ptr, uint32_t* pred_edge,
                          uint32_t cap, uint32_t* n_preds, hipStream_t s);

}  // namespace spfi
