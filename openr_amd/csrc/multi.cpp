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
//
//  Here: the context, plan creation, execute (graphs, enqueue threads,
//  timing) and the reads of the resident pass.  The types are in
//  mplan_internal.h, the partition's arithmetic in partition_host.cpp, the
//  route-database pipeline over the resident pass in mplan_routes.cpp.
// ============================================================================
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <map>

#include "mplan_internal.h"
#include "partition_host.h"

using namespace spfi;

void spf_mplan::stop_pool() {
  if (!pool) return;
  {
    std::lock_guard<std::mutex> lk(pool->mu);
    pool->stop = true;
  }
  pool->cv.notify_all();
  for (auto& t : pool->th) t.join();
  pool.reset();
}

spf_mplan::~spf_mplan() {
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

namespace spfi {

static std::mutex g_err_mu;  // member errors may come from the enqueue threads

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

}  // namespace spfi

namespace {

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
  const uint32_t used = partition_sources(nb_ptr, nb_id, n_nodes, srcs, n_src, n_parts, mode, part_out);
  if (mode_used) *mode_used = used;
  return SPF_OK;
}

spf_status spf_label_groups(const int32_t* node_label, uint32_t n_nodes, int32_t* labels,
                            uint32_t* grp_ptr, uint32_t* grp_nodes, uint32_t* n_groups) {
  if ((n_nodes && !node_label) || !n_groups)
    return mfail(nullptr, SPF_E_INVALID, "spf_label_groups: NULL argument");
  *n_groups = label_groups(node_label, n_nodes, labels, grp_ptr, grp_nodes);
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
  mp->mode = partition_sources(c0->nb_ptr.data(), c0->nb_id.data(), c0->N, srcs, n_src, P, mode,
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
