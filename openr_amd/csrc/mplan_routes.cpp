// ============================================================================
//  mplan_routes.cpp -- the route-database pipeline of a multi-device plan
//  (include/openr_spf.h, "route selection over the resident pass"): every
//  stage reads the rows and next-hop bitmaps spf_mplan_execute left resident
//  in the members' HBM.
//
//    route_prepare            the selection tables every stage launches with
//    spf_mplan_route_digests  every me's route digests
//    spf_mplan_routes         one me's routes, on the host
//    spf_mplan_route_records  every me's route database (tiled or compact)
//    spf_mplan_label_routes   ... and its node-label MPLS routes
//    spf_mplan_route_snapshot those two moved out of the plan
//    spf_mplan_route_delta    what changed between a snapshot and the plan
//    spf_mplan_route_update   the delta's entries with their next hops
//
//  Each stage's state is one sub-struct of spf_mplan::Part (per member) and of
//  spf_mplan (per plan), mplan_internal.h.  What the stages share is written
//  once below: the request mapping (ReqMap) and the stage events with the
//  drain of every stream a call queued work on (StageEvents).
// ============================================================================
#include <algorithm>
#include <cstdlib>
#include <initializer_list>

#include "mplan_internal.h"
#include "mplan_stage.h"
#include "partition_host.h"

using namespace spfi;

// (route_prepare and edge_keys have always had C names in the library's symbol
// list, from an unnamed namespace opened inside extern "C": kept)
extern "C" {
namespace {

// Every member's table of each resident row's (and bitmap set's) device
// address, plus the sets, on that member's device.  Rows of another device
// are read through peer access (xGMI): enabled here once, required for LFA
// (neighbours' rows) when the members span devices.
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
  int& peer = mp->sel.peer;
  if (peer < 0) {
    peer = 1;
    for (uint32_t a = 0; a < mp->n_parts; ++a)
      for (uint32_t b = 0; b < mp->n_parts; ++b) {
        const int da = m->members[a]->device, db = m->members[b]->device;
        if (da == db) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, da, db) != hipSuccess || !can) {
          peer = 0;
          continue;
        }
        M_HIP(m, hipSetDevice(da));
        const hipError_t e = hipDeviceEnablePeerAccess(db, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) peer = 0;
        (void)hipGetLastError();
      }
  }
  bool stale = false;
  for (uint32_t r = 0; r < mp->n_parts; ++r) stale |= mp->parts[r].plan && mp->parts[r].sel.epoch != mp->executes;
  std::vector<unsigned long long>& rowp = mp->sel.h_rowp;
  std::vector<unsigned long long>& nhp = mp->sel.h_nhp;
  std::vector<unsigned long long>& nrowp = mp->sel.h_nrowp;
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
    nrowp.clear();
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
      nrowp.assign(N, 0);
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
          nrowp[pl->closure[ci]] = (unsigned long long)(uintptr_t)(pl->d_Dn.p + ci * np);
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
  if (lfa && !peer) {
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
    if (!mp->parts[r].plan) continue;
    spf_mplan::Part::Select& p = mp->parts[r].sel;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    if (p.epoch != mp->executes) {
      M_HIP(m, p.rowp.upload(rowp.data(), N, s));
      M_HIP(m, p.nhp.upload(nhp.data(), N, s));
      if (!nrowp.empty()) M_HIP(m, p.nrowp.upload(nrowp.data(), N, s));
      p.epoch = mp->executes;
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
}  // extern "C"

spf_status spfi::route_prepare_rows(spf_mplan* mp, bool lfa, const uint32_t* me_req, uint32_t n_me) {
  return route_prepare(mp, nullptr, nullptr, 0, lfa, nullptr, 0, me_req, n_me);
}

namespace {

// member r's u8 rows for the records kernel's LFA loads, or none
const unsigned long long* nrowp_of(const spf_mplan* mp, uint32_t r) {
  return mp->sel.h_nrowp.empty() ? nullptr : mp->parts[r].sel.nrowp.p;
}

// spf_mplan_route_records with SPF_ROUTE_COMPACT, after its checks and
// route_prepare.  Per member a count walk, the scan of the counts and every
// block's start, then -- the pool allocated from the scan's total in
// between, on the host -- the fill walk (routes.hip kRsCount / kRsFill).
// Nothing here is sized by tiles x deg.
spf_status route_records_compact(spf_mplan* mp, const ReqMap& q, uint32_t n_sets, bool lfa,
                                 uint64_t* n_records, double* kernel_ms) {
  spf_mctx* m = mp->m;
  const uint32_t ts = route_db_tile_sets();
  const uint32_t n_chunks = (n_sets + ts - 1) / ts;
  std::vector<std::vector<unsigned long long>> bs(mp->n_parts);
  std::vector<uint32_t> fl(mp->n_parts, 0);
  // marks: [0] before the count, [1] after it, [2] after the scan and the
  // block starts, [3] before the fill, [4] after it
  StageEvents ev(m, mp->n_parts, 5, kernel_ms != nullptr);  // after bs / fl: drains before they are freed
  // (a call that fails from here on leaves no database to read: the headers
  // hold counts or offsets until the fill has run)
  struct Drop {
    spf_mplan* mp;
    bool keep = false;
    ~Drop() {
      if (!keep) mp->db.loc.clear();
    }
  } drop{mp};
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part::Select& sel = mp->parts[r].sel;
    spf_mplan::Part::Records& p = mp->parts[r].db;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_TRY(ev.open(r));
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)q.mine[r].size();
    const uint64_t cells = (uint64_t)n * n_sets, blocks = (uint64_t)n * n_chunks;
    M_HIP(m, hipStreamSynchronize(s));  // no queued upload still reads the host tables
    if (!p.compact) p.pool.reset();  // (the other layout's pool is not this one's size)
    p.compact = true;
    p.tiles = 0;
    p.me = q.mine[r];
    M_HIP(m, sel.me.upload(p.me.data(), n, s));
    M_HIP(m, p.hdr.alloc(cells + 1));
    M_HIP(m, p.sums.alloc(std::max<uint64_t>(label_scan_tiles(cells), 1)));
    M_HIP(m, p.start.alloc(blocks + 1));
    M_HIP(m, p.flags.alloc(1));
    M_HIP(m, hipMemsetAsync(p.flags.p, 0, 4, s));
    M_TRY(ev.mark(r, 0));
    RouteDbOut db;
    db.hdr = p.hdr.p;
    db.flags = p.flags.p;
    db.pass = 1;
    spf_status st = launch_route_sets(c, sel.rowp.p, sel.nhp.p, sel.me.p, n, sel.rsp.p, sel.rsn.p, n_sets, lfa,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s, &db,
                                      nrowp_of(mp, r));
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 1));
    st = launch_label_scan(c, p.hdr.p, cells, p.sums.p, s);
    if (st == SPF_OK) st = launch_route_block_starts(c, p.hdr.p, n, n_sets, p.start.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 2));
    bs[r].resize(blocks + 1);
    M_HIP(m, hipMemcpyAsync(bs[r].data(), p.start.p, 8ull * (blocks + 1), hipMemcpyDeviceToHost, s));
    M_HIP(m, hipMemcpyAsync(&fl[r], p.flags.p, 4, hipMemcpyDeviceToHost, s));
  }
  uint64_t total = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part::Select& sel = mp->parts[r].sel;
    spf_mplan::Part::Records& p = mp->parts[r].db;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scan's total and the starts
    if (fl[r] & 2u) return mfail(m, SPF_E_UNSUPPORTED, "a next-hop metric exceeds 2^32 - 1");
    const uint32_t n = (uint32_t)q.mine[r].size();
    p.h_base.assign(n, 0);
    p.h_cnt.assign(n, 0);
    for (uint32_t k = 0; k < n; ++k) {
      const unsigned long long b = bs[r][(size_t)k * n_chunks], e = bs[r][(size_t)(k + 1) * n_chunks];
      if (e - b >= (1ull << 32))
        return mfail(m, SPF_E_UNSUPPORTED, "route database of node %u: %llu records (2^32 max)", q.mine[r][k],
                     e - b);
      p.h_base[k] = b;
      p.h_cnt[k] = (uint32_t)(e - b);
    }
    const unsigned long long tot = bs[r].back();
    total += tot;
    // the record pool: exactly the total (kept when the previous compact one is large enough)
    M_HIP(m, p.pool.alloc(std::max<unsigned long long>(tot, 1)));
    M_HIP(m, p.base.upload(p.h_base.data(), n, s));
    M_TRY(ev.mark(r, 3));
    RouteDbOut db;
    db.hdr = p.hdr.p;
    db.pool = p.pool.p;
    db.flags = p.flags.p;
    db.pass = 2;
    db.bstart = p.start.p;
    db.stage = route_compact_stage();
    if (const char* nte = std::getenv("SPF_ROUTE_COMPACT_NT")) db.nt = nte[0] == '1' ? 1u : 0u;  // (A/B)
    const spf_status st = launch_route_sets(c, sel.rowp.p, sel.nhp.p, sel.me.p, n, sel.rsp.p, sel.rsn.p, n_sets,
                                            lfa, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s, &db,
                                            nrowp_of(mp, r));
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 4));
  }
  double ms[3] = {0, 0, 0};
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (q.mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    M_TRY(ev.slowest(r, {0, 1, 3}, ms));
  }
  drop.keep = true;
  mp->db.moved = false;
  if (kernel_ms) std::copy(ms, ms + 3, mp->db.ms);
  if (n_records) *n_records = total;
  if (kernel_ms) *kernel_ms = ev.worst;
  return SPF_OK;
}

}  // namespace

spf_route_snapshot::~spf_route_snapshot() {
  if (!m) return;
  // (a delta's kernels may still read the pools)
  for (uint32_t r = 0; r < n_parts && r < m->members.size(); ++r) {
    (void)hipSetDevice(m->members[r]->device);
    (void)hipStreamSynchronize(m->exec[r]);
  }
  m->snaps.erase(std::remove(m->snaps.begin(), m->snaps.end(), this), m->snaps.end());
}

extern "C" {

// ---- route selection over the resident pass ------------------------------
spf_status spf_mplan_route_digests(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* set_ptr, const uint32_t* set_nodes, uint32_t n_sets,
                                   uint32_t flags, const uint64_t* link_hash, uint32_t n_links,
                                   uint64_t* digests, double* kernel_ms) {
  if (!mp || (n_me && (!me_req || !digests)) || !set_ptr || !link_hash)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_digests: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  M_TRY(me_check(mp, me_req, n_me));
  for (uint32_t e = 0; e < c0->E; ++e)
    if (c0->link[e] >= n_links) return mfail(m, SPF_E_INVALID, "link_hash shorter than the link ids");
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0;
  M_TRY(route_prepare(mp, set_ptr, set_nodes, n_sets, lfa, link_hash, n_links, me_req, n_me));
  const ReqMap q(mp, me_req, n_me);
  std::vector<std::vector<uint64_t>> got(mp->n_parts);
  StageEvents ev(m, mp->n_parts, 2, kernel_ms != nullptr);  // after q / got: drains before they are freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part::Select& p = mp->parts[r].sel;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_TRY(ev.open(r));
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)q.mine[r].size();
    M_HIP(m, p.me.upload(q.mine[r].data(), n, s));
    M_HIP(m, p.dig.alloc(n));
    M_HIP(m, hipMemsetAsync(p.dig.p, 0, 8ull * n, s));
    M_TRY(ev.mark(r, 0));
    const spf_status st = launch_route_sets(c, p.rowp.p, p.nhp.p, p.me.p, n, p.rsp.p, p.rsn.p, n_sets,
                                            lfa, p.lh.p, p.dig.p, nullptr, nullptr, nullptr, nullptr, s);
    // (u8 LFA loads only for the records kernel: the digest kernel is
    // VALU-bound and the byte unpacking made it slower, 2.33 -> 2.42 ms)
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 1));
    got[r].resize(n);
    M_HIP(m, hipMemcpyAsync(got[r].data(), p.dig.p, 8ull * n, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (q.mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    M_TRY(ev.slowest(r, {0}));
    for (size_t k = 0; k < got[r].size(); ++k) digests[q.req[r][k]] = got[r][k];
  }
  if (kernel_ms) *kernel_ms = ev.worst;
  return SPF_OK;
}

spf_status spf_mplan_routes(spf_mplan* mp, uint32_t me_req, const uint32_t* set_ptr,
                            const uint32_t* set_nodes, uint32_t n_sets, uint32_t flags,
                            uint64_t* min_metric, uint32_t* nh_count, uint32_t* nh_edge,
                            uint64_t* nh_metric) {
  if (!mp || !set_ptr || !min_metric || !nh_count || !nh_edge || !nh_metric)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_routes: NULL argument");
  spf_mctx* m = mp->m;
  M_TRY(me_check(mp, &me_req, 1));
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0;
  M_TRY(route_prepare(mp, set_ptr, set_nodes, n_sets, lfa, nullptr, 0, &me_req, 1));
  const ReqMap q(mp, &me_req, 1);
  const uint32_t r = q.loc[0].first, me = q.nodes[0];
  spf_mplan::Part::Select& p = mp->parts[r].sel;
  spf_ctx* c = m->members[r];
  const uint32_t deg = c->row_ptr[me + 1] - c->row_ptr[me];
  const size_t cap = (size_t)n_sets * std::max<uint32_t>(1, deg);
  M_HIP(m, hipSetDevice(c->device));
  const hipStream_t s = m->exec[r];
  IssuedGuard guard{m, {r}};  // q and the caller's outputs outlive every queued copy
  M_HIP(m, p.me.upload(q.mine[r].data(), 1, s));
  M_HIP(m, p.min.alloc(std::max<uint32_t>(1, n_sets)));
  M_HIP(m, p.cnt.alloc(std::max<uint32_t>(1, n_sets)));
  M_HIP(m, p.edge.alloc(cap));
  M_HIP(m, p.metric.alloc(cap));
  const spf_status st = launch_route_sets(c, p.rowp.p, p.nhp.p, p.me.p, 1, p.rsp.p, p.rsn.p, n_sets, lfa,
                                          nullptr, nullptr, reinterpret_cast<uint64_t*>(p.min.p),
                                          p.cnt.p, p.edge.p, reinterpret_cast<uint64_t*>(p.metric.p), s);
  if (st != SPF_OK) return member_fail(m, r, st);
  if (n_sets) {
    M_HIP(m, hipMemcpyAsync(min_metric, p.min.p, 8ull * n_sets, hipMemcpyDeviceToHost, s));
    M_HIP(m, hipMemcpyAsync(nh_count, p.cnt.p, 4ull * n_sets, hipMemcpyDeviceToHost, s));
    if (deg) {
      M_HIP(m, hipMemcpyAsync(nh_edge, p.edge.p, 4ull * cap, hipMemcpyDeviceToHost, s));
      M_HIP(m, hipMemcpyAsync(nh_metric, p.metric.p, 8ull * cap, hipMemcpyDeviceToHost, s));
    }
  }
  M_HIP(m, hipStreamSynchronize(s));
  return SPF_OK;
}

// ---- route records ----------------------------------------------------------
spf_status spf_mplan_route_records(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* set_ptr, const uint32_t* set_nodes, uint32_t n_sets,
                                   uint32_t flags, uint64_t* n_records, double* kernel_ms) {
  if (!mp || (n_me && !me_req) || !set_ptr)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_records: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  M_TRY(me_check(mp, me_req, n_me));
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
  M_TRY(route_prepare(mp, set_ptr, set_nodes, n_sets, lfa, nullptr, 0, me_req, n_me));
  const ReqMap q(mp, me_req, n_me);
  mp->db.loc = q.loc;
  mp->db.nodes = q.nodes;
  mp->db.sets = n_sets;
  mp->db.flags = flags & SPF_ROUTE_LFA;
  mp->db.compact = (flags & SPF_ROUTE_COMPACT) != 0;
  if (mp->db.compact) return route_records_compact(mp, q, n_sets, lfa, n_records, kernel_ms);
  // me's region: one [deg(me)][ts] tile per chunk of ts sets (route_quads_kernel<kRsDb>)
  const uint64_t ts = route_db_tile_sets();
  const uint64_t tiles = ((uint64_t)n_sets + ts - 1) / ts * ts;
  std::vector<std::vector<uint32_t>> fl(mp->n_parts);
  StageEvents ev(m, mp->n_parts, 2, kernel_ms != nullptr);  // after fl: drains before it is freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part::Select& sel = mp->parts[r].sel;
    spf_mplan::Part::Records& p = mp->parts[r].db;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_TRY(ev.open(r));
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)q.mine[r].size();
    if (p.me != q.mine[r] || p.tiles != tiles || p.compact) {
      M_HIP(m, hipStreamSynchronize(s));  // no queued upload still reads the host tables
      if (p.compact) p.pool.reset();  // (the other layout's pool is not this one's size)
      p.compact = false;
      p.me = q.mine[r];
      p.tiles = tiles;
      p.h_base.assign(n, 0);
      unsigned long long tot = 0;
      for (uint32_t k = 0; k < n; ++k) {
        const uint32_t v = q.mine[r][k];
        const uint64_t region = tiles * (c0->row_ptr[v + 1] - c0->row_ptr[v]);
        if (region >= (1ull << 32))
          return mfail(m, SPF_E_UNSUPPORTED, "route database of node %u: %llu record slots (2^32 max)", v,
                       (unsigned long long)region);
        p.h_base[k] = tot;
        tot += region;
      }
      M_HIP(m, p.pool.alloc(std::max<unsigned long long>(tot, 1)));
      M_HIP(m, p.base.upload(p.h_base.data(), n, s));
    }
    M_HIP(m, sel.me.upload(p.me.data(), n, s));
    M_HIP(m, p.hdr.alloc(std::max<size_t>(1, (size_t)n * n_sets)));
    M_HIP(m, p.cnt.alloc(n));
    M_HIP(m, p.flags.alloc(1));
    M_HIP(m, hipMemsetAsync(p.cnt.p, 0, 4ull * n, s));
    M_HIP(m, hipMemsetAsync(p.flags.p, 0, 4, s));
    M_TRY(ev.mark(r, 0));
    RouteDbOut db;
    db.hdr = p.hdr.p;
    db.pool = p.pool.p;
    db.base = p.base.p;
    db.count = p.cnt.p;
    db.flags = p.flags.p;
    const spf_status st = launch_route_sets(c, sel.rowp.p, sel.nhp.p, sel.me.p, n, sel.rsp.p, sel.rsn.p, n_sets,
                                            lfa, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s, &db,
                                            nrowp_of(mp, r));
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 1));
    fl[r].resize(n + 1);
    M_HIP(m, hipMemcpyAsync(fl[r].data(), p.cnt.p, 4ull * n, hipMemcpyDeviceToHost, s));
    M_HIP(m, hipMemcpyAsync(fl[r].data() + n, p.flags.p, 4, hipMemcpyDeviceToHost, s));
  }
  uint64_t total = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part::Records& p = mp->parts[r].db;
    if (q.mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    const uint32_t n = (uint32_t)q.mine[r].size();
    if (fl[r][n] & 2u) return mfail(m, SPF_E_UNSUPPORTED, "a next-hop metric exceeds 2^32 - 1");
    p.h_cnt.assign(fl[r].begin(), fl[r].begin() + n);
    for (uint32_t k = 0; k < n; ++k) total += p.h_cnt[k];
    M_TRY(ev.slowest(r, {0}));
  }
  mp->db.moved = false;  // (only now: a call that failed after a snapshot leaves SPF_E_STATE standing)
  if (n_records) *n_records = total;
  if (kernel_ms) *kernel_ms = ev.worst;
  return SPF_OK;
}

spf_status spf_mplan_route_db(spf_mplan* mp, uint32_t t, uint64_t* hdr, uint64_t* rec, uint64_t cap,
                              uint64_t* n) {
  if (mp && mp->db.moved)
    return mfail(mp->m, SPF_E_STATE, "spf_mplan_route_db: a snapshot took the databases (call spf_mplan_route_records)");
  if (!mp || t >= mp->db.loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_db: no such me (call spf_mplan_route_records)");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->db.loc[t];
  spf_mplan::Part::Records& p = mp->parts[r].db;
  const uint32_t cnt = p.h_cnt[k];
  if (n) *n = cnt;
  if (!hdr && !rec) return SPF_OK;
  if (rec && cap < cnt)
    return mfail(m, SPF_E_NOMEM, "route db of %u records, room for %llu", cnt, (unsigned long long)cap);
  // the device headers and me's tiled region, compacted here: route p's
  // records contiguous from its header's offset, in set order
  const uint32_t S = mp->db.sets;
  std::vector<uint64_t> h(S);
  const uint32_t me = p.me[k];
  // (the compact layout's region is me's records themselves, stride 1)
  const uint64_t region =
      p.compact ? cnt : p.tiles * (m->members[r]->row_ptr[me + 1] - m->members[r]->row_ptr[me]);
  std::vector<uint64_t> tile(std::max<uint64_t>(region, 1));
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  if (S) M_HIP(m, hipMemcpyAsync(h.data(), p.hdr.p + (size_t)k * S, 8ull * S, hipMemcpyDeviceToHost, s));
  if (rec && region)
    M_HIP(m, hipMemcpyAsync(tile.data(), p.pool.p + p.h_base[k], 8ull * region, hipMemcpyDeviceToHost, s));
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
  if (!mp->has_records())
    return mfail(mp->m, SPF_E_STATE,
                 "spf_mplan_route_record_pool: the plan holds no route records (call spf_mplan_route_records)");
  std::vector<uint8_t> used(mp->n_parts, 0);
  for (const auto& loc : mp->db.loc) used[loc.first] = 1;
  uint64_t bytes = 0, rec = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (!used[r]) continue;
    bytes += 8ull * mp->parts[r].db.pool.n;
    for (const uint32_t c : mp->parts[r].db.h_cnt) rec += c;
  }
  if (layout) *layout = mp->db.compact ? 1u : 0u;
  if (pool_bytes) *pool_bytes = bytes;
  if (record_bytes) *record_bytes = 8 * rec;
  return SPF_OK;
}

uint32_t spf_route_compact_stage(void) { return route_compact_stage(); }

spf_status spf_mplan_route_records_timing(const spf_mplan* mp, double* ms) {
  if (!mp || !ms) return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_records_timing: NULL argument");
  std::copy(mp->db.ms, mp->db.ms + 3, ms);
  return SPF_OK;
}

spf_status spf_mplan_route_record_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_hdr,
                                          const uint64_t** d_base, const uint64_t** d_pool,
                                          uint64_t* n_records, uint32_t* slots, uint32_t cap,
                                          uint32_t* n_slots) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_record_buffers: bad argument");
  const spf_mplan::Part::Records& p = mp->parts[member].db;
  // (a member without a me of the last call holds nothing of it)
  uint32_t k = 0;
  if (mp->has_records())
    for (const auto& loc : mp->db.loc) k += loc.first == member;
  const bool has = k != 0;
  uint64_t rec = 0;
  if (has)
    for (const uint32_t c : p.h_cnt) rec += c;
  if (n_slots) *n_slots = k;
  if (d_hdr) *d_hdr = has ? reinterpret_cast<const uint64_t*>(p.hdr.p) : nullptr;
  if (d_base) *d_base = has ? reinterpret_cast<const uint64_t*>(p.base.p) : nullptr;
  if (d_pool) *d_pool = has ? reinterpret_cast<const uint64_t*>(p.pool.p) : nullptr;
  if (n_records) *n_records = rec;
  if (slots) {
    if (cap < k) return mfail(mp->m, SPF_E_NOMEM, "%u me slots, room for %u", k, cap);
    for (uint32_t t = 0; t < mp->db.loc.size() && has; ++t)
      if (mp->db.loc[t].first == member) slots[mp->db.loc[t].second] = t;
  }
  return SPF_OK;
}

// ---- node-label MPLS routes -------------------------------------------------
spf_status spf_mplan_label_routes(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                  const int32_t* node_label, uint32_t flags, uint32_t* n_labels,
                                  uint64_t* n_records, uint64_t* pool_bytes, double* kernel_ms) {
  if (!mp || (n_me && !me_req) || !node_label)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_label_routes: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  M_TRY(me_check(mp, me_req, n_me));
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0;
  ++mp->db_gen;
  M_TRY(route_prepare(mp, nullptr, nullptr, 0, lfa, nullptr, 0, me_req, n_me));
  spf_mplan::Labels& L = mp->lr;
  L.loc.clear();  // (the previous call's databases are overwritten from here on)
  const uint32_t N = c0->N;
  L.gptr.assign((size_t)N + 1, 0);
  L.gnodes.assign(std::max<uint32_t>(N, 1), 0);
  L.labels.assign(std::max<uint32_t>(N, 1), 0);
  uint32_t G = 0;
  M_TRY(spf_label_groups(node_label, N, L.labels.data(), L.gptr.data(), L.gnodes.data(), &G));
  ReqMap q(mp, me_req, n_me);
  for (uint32_t r = 0; r < mp->n_parts; ++r) mp->parts[r].lr.req = q.req[r];
  std::vector<unsigned long long> tot(mp->n_parts, 0);
  std::vector<uint32_t> fl(mp->n_parts, 0);
  // marks: [0] before the count, [1] after the scan, [2] before the fill, [3]
  // after it (the pool is allocated in between, on the host, from the scan's total)
  StageEvents ev(m, mp->n_parts, 4, kernel_ms != nullptr);  // after q / tot / fl: drains before they are freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part::Select& sel = mp->parts[r].sel;
    spf_mplan::Part::Labels& p = mp->parts[r].lr;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_TRY(ev.open(r));
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)q.mine[r].size();
    const uint64_t cells = (uint64_t)n * G;
    M_HIP(m, p.me.upload(q.mine[r].data(), n, s));
    M_HIP(m, p.gptr.upload(L.gptr.data(), (size_t)G + 1, s));
    M_HIP(m, p.gnodes.upload(L.gnodes.data(), std::max<uint32_t>(1, L.gptr[G]), s));
    M_HIP(m, p.owner.alloc(std::max<uint64_t>(cells, 1)));
    M_HIP(m, p.ptr.alloc(cells + 1));
    M_HIP(m, p.sums.alloc(std::max<uint64_t>(label_scan_tiles(cells), 1)));
    M_HIP(m, p.flags.alloc(1));
    M_HIP(m, hipMemsetAsync(p.flags.p, 0, 4, s));
    M_TRY(ev.mark(r, 0));
    spf_status st = launch_label_routes(c, false, sel.rowp.p, sel.nhp.p, p.me.p, n, p.gptr.p, p.gnodes.p, G, lfa,
                                        p.owner.p, p.ptr.p, nullptr, p.flags.p, s);
    if (st == SPF_OK) st = launch_label_scan(c, p.ptr.p, cells, p.sums.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 1));
    M_HIP(m, hipMemcpyAsync(&tot[r], p.ptr.p + cells, 8, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part::Select& sel = mp->parts[r].sel;
    spf_mplan::Part::Labels& p = mp->parts[r].lr;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scan's total
    // the record pool: exactly the total (kept when the previous one is large enough)
    M_HIP(m, p.rec.alloc(std::max<unsigned long long>(tot[r], 1)));
    p.records = tot[r];
    M_TRY(ev.mark(r, 2));
    const spf_status st = launch_label_routes(c, true, sel.rowp.p, sel.nhp.p, p.me.p, (uint32_t)q.mine[r].size(),
                                              p.gptr.p, p.gnodes.p, G, lfa, p.owner.p, p.ptr.p, p.rec.p,
                                              p.flags.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 3));
    M_HIP(m, hipMemcpyAsync(&fl[r], p.flags.p, 4, hipMemcpyDeviceToHost, s));
  }
  uint64_t total = 0, bytes = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (q.mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    if (fl[r] & 2u) return mfail(m, SPF_E_UNSUPPORTED, "a next-hop metric exceeds 2^32 - 1");
    const uint64_t cells = (uint64_t)q.mine[r].size() * G;
    total += tot[r];
    bytes += 8 * tot[r] + 8 * (cells + 1) + 4 * cells;
    M_TRY(ev.slowest(r, {0, 2}));
  }
  L.loc = std::move(q.loc);
  L.moved = false;
  L.groups = G;
  L.labels.resize(G);
  L.rflags = flags & SPF_ROUTE_LFA;
  L.nodes = std::move(q.nodes);
  if (n_labels) *n_labels = G;
  if (n_records) *n_records = total;
  if (pool_bytes) *pool_bytes = bytes;
  if (kernel_ms) *kernel_ms = ev.worst;
  return SPF_OK;
}

spf_status spf_mplan_label_route_db(spf_mplan* mp, uint32_t t, uint32_t* owner, uint64_t* ptr,
                                    uint64_t* rec, uint64_t cap, uint64_t* n) {
  if (mp && mp->lr.moved)
    return mfail(mp->m, SPF_E_STATE,
                 "spf_mplan_label_route_db: a snapshot took the databases (call spf_mplan_label_routes)");
  if (!mp || t >= mp->lr.loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID,
                 "spf_mplan_label_route_db: no such me (call spf_mplan_label_routes)");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->lr.loc[t];
  spf_mplan::Part::Labels& p = mp->parts[r].lr;
  const uint32_t G = mp->lr.groups;
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  // me's G + 1 offsets (the next slot's first one, or the total, ends them)
  std::vector<uint64_t> h((size_t)G + 1);
  M_HIP(m, hipMemcpyAsync(h.data(), p.ptr.p + (size_t)k * G, 8ull * (G + 1), hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  const uint64_t cnt = h[G] - h[0];
  if (n) *n = cnt;
  if (rec && cap < cnt)
    return mfail(m, SPF_E_NOMEM, "label route db of %llu records, room for %llu", (unsigned long long)cnt,
                 (unsigned long long)cap);
  if (owner && G)
    M_HIP(m, hipMemcpyAsync(owner, p.owner.p + (size_t)k * G, 4ull * G, hipMemcpyDeviceToHost, s));
  if (rec && cnt)
    M_HIP(m, hipMemcpyAsync(rec, p.rec.p + h[0], 8ull * cnt, hipMemcpyDeviceToHost, s));
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
  const spf_mplan::Part::Labels& p = mp->parts[member].lr;
  // (a member without a me of the last call holds nothing of it)
  const bool has = mp->has_label_routes() && !p.req.empty();
  const uint32_t k = has ? (uint32_t)p.req.size() : 0u;
  if (n_slots) *n_slots = k;
  if (d_owner) *d_owner = has ? p.owner.p : nullptr;
  if (d_ptr) *d_ptr = has ? reinterpret_cast<const uint64_t*>(p.ptr.p) : nullptr;
  if (d_rec) *d_rec = has ? reinterpret_cast<const uint64_t*>(p.rec.p) : nullptr;
  if (n_records) *n_records = has ? p.records : 0;
  if (slots) {
    if (cap < k) return mfail(mp->m, SPF_E_NOMEM, "%u me slots, room for %u", k, cap);
    std::copy(p.req.begin(), p.req.begin() + k, slots);
  }
  return SPF_OK;
}

// ---- a generation moved out of the plan --------------------------------------
spf_status spf_mplan_route_snapshot(spf_mplan* mp, const uint64_t* link_hash, uint32_t n_links,
                                    spf_route_snapshot** out) {
  if (!mp || !link_hash || !out)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_snapshot: NULL argument");
  *out = nullptr;
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  if (!mp->has_records())
    return mfail(m, SPF_E_STATE, "spf_mplan_route_snapshot: the plan holds no route records");
  const bool labels = mp->has_label_routes();
  if (labels && mp->lr.nodes != mp->db.nodes)
    return mfail(m, SPF_E_INVALID, "spf_mplan_route_snapshot: label routes and route records of different me lists");
  std::vector<unsigned long long> key;
  M_TRY(edge_keys(m, c0, link_hash, n_links, &key));
  auto sn = std::make_unique<spf_route_snapshot>();
  sn->n_nodes = c0->N;
  sn->n_sets = mp->db.sets;
  sn->flags = mp->db.flags;
  sn->me = mp->db.nodes;
  sn->db_loc = mp->db.loc;
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
  for (const auto& loc : mp->db.loc) used[loc.first] = 1;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    spf_route_snapshot::Part& q = sn->parts[r];
    q.bytes = 8 * q.key.n;
    if (!used[r]) continue;
    q.db.hdr.take(p.db.hdr);
    q.db.pool.take(p.db.pool);
    q.db.h_base = p.db.h_base;
    q.bytes += 8 * (q.db.hdr.n + q.db.pool.n);
    p.db.me.clear();  // the next spf_mplan_route_records allocates afresh
    p.db.tiles = 0;
    if (labels) {
      q.lr.owner.take(p.lr.owner);
      q.lr.ptr.take(p.lr.ptr);
      q.lr.rec.take(p.lr.rec);
      q.bytes += 4 * q.lr.owner.n + 8 * (q.lr.ptr.n + q.lr.rec.n);
      p.lr.records = 0;
    }
  }
  mp->db.loc.clear();
  mp->db.moved = true;
  ++mp->db_gen;
  if (labels) {
    sn->has_labels = true;
    sn->lr_flags = mp->lr.rflags;
    sn->lr_groups = mp->lr.groups;
    sn->labels = mp->lr.labels;
    sn->lr_loc = mp->lr.loc;
    mp->lr.loc.clear();
    mp->lr.moved = true;
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

// ---- route-database delta between two passes -------------------------------
spf_status spf_mplan_route_delta(spf_mplan* mp, const spf_route_snapshot* snap, const uint64_t* link_hash,
                                 uint32_t n_links, uint64_t* totals, double* kernel_ms) {
  if (!mp || !snap || !link_hash)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_delta: NULL argument");
  spf_mctx* m = mp->m;
  spf_ctx* c0 = m->members[0];
  if (mp->flags & (SPF_FLAG_DIST64 | SPF_FLAG_HOP_COUNT))
    return mfail(m, SPF_E_UNSUPPORTED, "route databases need u32 link-metric rows");
  if (snap->m != m) return mfail(m, SPF_E_INVALID, "spf_mplan_route_delta: the snapshot is another context's");
  if (!mp->has_records())
    return mfail(m, SPF_E_STATE, "spf_mplan_route_delta: the plan holds no databases (call spf_mplan_route_records)");
  const bool labels = mp->has_label_routes();
  if (snap->n_nodes != c0->N || snap->n_sets != mp->db.sets || snap->flags != mp->db.flags ||
      snap->me != mp->db.nodes)
    return mfail(m, SPF_E_INVALID, "spf_mplan_route_delta: me list, n_nodes, n_sets or route flags differ from the snapshot");
  if (labels != snap->has_labels || (labels && (mp->lr.nodes != mp->db.nodes || mp->lr.rflags != snap->lr_flags)))
    return mfail(m, SPF_E_INVALID, "spf_mplan_route_delta: label routes (presence, me list or flags) differ from the snapshot");
  std::vector<unsigned long long> key;
  M_TRY(edge_keys(m, c0, link_hash, n_links, &key));
  const uint32_t n_me = (uint32_t)mp->db.nodes.size(), S = mp->db.sets;
  // an old database on another device is read over peer access
  // (route_prepare of the materialising call tried to enable it)
  for (uint32_t t = 0; t < n_me; ++t) {
    const int dn = m->members[mp->db.loc[t].first]->device, dold = m->members[snap->db_loc[t].first]->device;
    if (dn != dold && mp->sel.peer != 1)
      return mfail(m, SPF_E_UNSUPPORTED, "route delta across devices needs peer access");
  }
  // labels of either generation, ascending, and each one's group index there
  const LabelUnion lu = labels ? label_union(snap->labels, mp->lr.labels) : LabelUnion{};
  const uint32_t U = (uint32_t)lu.lab.size(), Gn = mp->lr.groups, Go = snap->lr_groups;
  const uint32_t cells[2] = {S, U};
  mp->dl.loc.clear();
  mp->up.done = false;
  struct Host {
    std::vector<unsigned long long> ohdr, opool, oown, optr, orec;
    std::vector<uint32_t> e0, deg, same;
    unsigned long long tot[2] = {0, 0}, del[2] = {0, 0};
  };
  std::vector<Host> host(mp->n_parts);
  // marks: [0] before the counts, [1] after the scans, [2] before the fills,
  // [3] after them (the lists are allocated in between, on the host, from the
  // scans' totals)
  StageEvents ev(m, mp->n_parts, 4, kernel_ms != nullptr);  // after key / host / lu: drains before they are freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) mp->parts[r].dl.req.clear();
  for (uint32_t t = 0; t < n_me; ++t) mp->parts[mp->db.loc[t].first].dl.req.push_back(t);
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part& p = mp->parts[r];
    spf_mplan::Part::Delta& d = p.dl;
    const uint32_t n = (uint32_t)d.req.size();
    if (!n) continue;
    spf_ctx* c = m->members[r];
    Host& h = host[r];
    for (uint32_t k = 0; k < n; ++k) {  // (slot k of the records call is its k-th me of this member)
      const uint32_t t = d.req[k], v = mp->db.nodes[t];
      const auto [ro, ko] = snap->db_loc[t];
      const spf_route_snapshot::Part& q = snap->parts[ro];
      h.ohdr.push_back((unsigned long long)(uintptr_t)(q.db.hdr.p + (size_t)ko * S));
      h.opool.push_back((unsigned long long)(uintptr_t)(q.db.pool.p + q.db.h_base[ko]));
      h.e0.push_back(snap->row_ptr[v]);
      h.deg.push_back(snap->row_ptr[v + 1] - snap->row_ptr[v]);
      if (labels) {
        const auto [rl, kl] = snap->lr_loc[t];
        const spf_route_snapshot::Part& ql = snap->parts[rl];
        h.oown.push_back((unsigned long long)(uintptr_t)(ql.lr.owner.p + (size_t)kl * Go));
        h.optr.push_back((unsigned long long)(uintptr_t)(ql.lr.ptr.p + (size_t)kl * Go));
        h.orec.push_back((unsigned long long)(uintptr_t)ql.lr.rec.p);
      }
    }
    M_TRY(ev.open(r));
    const hipStream_t s = m->exec[r];
    M_HIP(m, p.sel.me.upload(p.db.me.data(), n, s));
    M_HIP(m, d.ohdr.upload(h.ohdr.data(), n, s));
    M_HIP(m, d.opool.upload(h.opool.data(), n, s));
    M_HIP(m, d.e0.upload(h.e0.data(), n, s));
    M_HIP(m, d.deg.upload(h.deg.data(), n, s));
    M_HIP(m, d.key.upload(key.data(), key.size(), s));
    M_HIP(m, d.same.alloc(n));
    M_HIP(m, d.tot.alloc(2));
    M_HIP(m, hipMemsetAsync(d.tot.p, 0, 16, s));
    if (labels) {
      M_HIP(m, d.oown.upload(h.oown.data(), n, s));
      M_HIP(m, d.optr.upload(h.optr.data(), n, s));
      M_HIP(m, d.orec.upload(h.orec.data(), n, s));
      M_HIP(m, d.mold.upload(lu.mold.data(), U, s));
      M_HIP(m, d.mnew.upload(lu.mnew.data(), U, s));
      M_HIP(m, d.lab.upload(lu.lab.data(), U, s));
    }
    for (uint32_t w = 0; w < 2; ++w) {
      const uint64_t nb = (uint64_t)n * route_delta_chunks(cells[w]);
      M_HIP(m, d.kind[w].alloc(std::max<uint64_t>((uint64_t)n * cells[w], 1)));
      M_HIP(m, d.blk[w].alloc(nb + 1));
      M_HIP(m, d.sums[w].alloc(std::max<uint64_t>(label_scan_tiles(nb), 1)));
      M_HIP(m, d.ptr[w].alloc((size_t)n + 1));
      M_HIP(m, hipMemsetAsync(d.ptr[w].p, 0, 8ull * (n + 1), s));  // (a pass without cells writes none)
    }
    M_TRY(ev.mark(r, 0));
    RouteDeltaIn in;
    in.me = p.sel.me.p;
    in.old_e0 = d.e0.p;
    in.old_deg = d.deg.p;
    in.key_old = snap->parts[r].key.p;
    in.key_new = d.key.p;
    in.same = d.same.p;
    spf_status st = launch_delta_rows(c, in, n, s);
    if (st == SPF_OK)
      st = launch_delta_ip(c, in, n, S, p.db.hdr.p, p.db.pool.p, p.db.base.p, d.ohdr.p, d.opool.p, d.kind[0].p,
                           d.blk[0].p, s);
    if (st == SPF_OK) st = launch_label_scan(c, d.blk[0].p, (uint64_t)n * route_delta_chunks(S), d.sums[0].p, s);
    if (st == SPF_OK && labels)
      st = launch_delta_labels(c, in, n, U, p.lr.owner.p, p.lr.ptr.p, p.lr.rec.p, Gn, d.oown.p, d.optr.p,
                               d.orec.p, d.mold.p, d.mnew.p, d.kind[1].p, d.blk[1].p, s);
    if (st == SPF_OK) st = launch_label_scan(c, d.blk[1].p, (uint64_t)n * route_delta_chunks(U), d.sums[1].p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 1));
    for (uint32_t w = 0; w < 2; ++w)
      M_HIP(m, hipMemcpyAsync(&h.tot[w], d.blk[w].p + (uint64_t)n * route_delta_chunks(cells[w]), 8,
                              hipMemcpyDeviceToHost, s));
    h.same.resize(n);
    M_HIP(m, hipMemcpyAsync(h.same.data(), d.same.p, 4ull * n, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    spf_mplan::Part::Delta& d = mp->parts[r].dl;
    const uint32_t n = (uint32_t)d.req.size();
    if (!n) continue;
    spf_ctx* c = m->members[r];
    Host& h = host[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scans' totals
    for (uint32_t w = 0; w < 2; ++w) {
      M_HIP(m, d.set[w].alloc(std::max<unsigned long long>(h.tot[w], 1)));
      d.n[w] = h.tot[w];
    }
    M_TRY(ev.mark(r, 2));
    spf_status st = launch_delta_fill(c, d.kind[0].p, S, n, d.blk[0].p, nullptr, d.set[0].p, d.ptr[0].p, d.tot.p, s);
    if (st == SPF_OK && labels)
      st = launch_delta_fill(c, d.kind[1].p, U, n, d.blk[1].p, d.lab.p, d.set[1].p, d.ptr[1].p, d.tot.p + 1, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 3));
    M_HIP(m, hipMemcpyAsync(h.del, d.tot.p, 16, hipMemcpyDeviceToHost, s));
  }
  uint64_t out[5] = {0, 0, 0, 0, 0};
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (mp->parts[r].dl.req.empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    const Host& h = host[r];
    for (uint32_t w = 0; w < 2; ++w) {
      out[2 * w] += h.tot[w] - h.del[w];
      out[2 * w + 1] += h.del[w];
    }
    for (uint32_t x : h.same) out[4] += x ? 0u : 1u;
    M_TRY(ev.slowest(r, {0, 2}));
  }
  mp->dl.loc = mp->db.loc;
  mp->dl.gen = mp->db_gen;
  mp->dl.labels = labels;
  mp->dl.uni = U;
  std::copy(out, out + 5, mp->dl.tot);
  if (totals) std::copy(out, out + 5, totals);
  if (kernel_ms) *kernel_ms = ev.worst;
  return SPF_OK;
}

spf_status spf_mplan_route_delta_db(spf_mplan* mp, uint32_t t, uint32_t* ip, uint64_t ip_cap,
                                    uint64_t* n_ip, uint32_t* label, uint64_t label_cap,
                                    uint64_t* n_label) {
  if (!mp || t >= mp->dl.loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID,
                 "spf_mplan_route_delta_db: no such me (call spf_mplan_route_delta)");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->dl.loc[t];
  spf_mplan::Part::Delta& p = mp->parts[r].dl;
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  uint64_t h[2][2];
  for (uint32_t w = 0; w < 2; ++w)
    M_HIP(m, hipMemcpyAsync(h[w], p.ptr[w].p + k, 16, hipMemcpyDeviceToHost, s));
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
      M_HIP(m, hipMemcpyAsync(dst[w], p.set[w].p + h[w][0], 4 * c, hipMemcpyDeviceToHost, s));
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
  const spf_mplan::Part::Delta& p = mp->parts[member].dl;
  const bool has = mp->has_delta() && !p.req.empty();
  const uint32_t k = has ? (uint32_t)p.req.size() : 0u;
  if (n_slots) *n_slots = k;
  if (d_ip_ptr) *d_ip_ptr = has ? reinterpret_cast<const uint64_t*>(p.ptr[0].p) : nullptr;
  if (d_ip_set) *d_ip_set = has ? p.set[0].p : nullptr;
  if (d_label_ptr) *d_label_ptr = has ? reinterpret_cast<const uint64_t*>(p.ptr[1].p) : nullptr;
  if (d_label_set) *d_label_set = has ? p.set[1].p : nullptr;
  if (slots) {
    if (cap < k) return mfail(mp->m, SPF_E_NOMEM, "%u me slots, room for %u", k, cap);
    std::copy(p.req.begin(), p.req.begin() + k, slots);
  }
  return SPF_OK;
}

// ---- the delta's payload: updated routes with their next hops ----------------
spf_status spf_mplan_route_update(spf_mplan* mp, uint64_t* totals, uint64_t* pool_bytes, double* kernel_ms) {
  if (!mp) return mfail(nullptr, SPF_E_INVALID, "spf_mplan_route_update: NULL argument");
  spf_mctx* m = mp->m;
  if (!mp->has_delta())
    return mfail(m, SPF_E_STATE, "spf_mplan_route_update: no delta (call spf_mplan_route_delta)");
  if (mp->dl.gen != mp->db_gen || !mp->has_records())
    return mfail(m, SPF_E_STATE,
                 "spf_mplan_route_update: the plan's databases are not the ones the delta compared "
                 "(call spf_mplan_route_delta again)");
  const bool labels = mp->dl.labels;
  const uint32_t S = mp->db.sets, U = mp->dl.uni, G = mp->lr.groups;
  mp->up.done = false;
  std::vector<unsigned long long> tot(2 * mp->n_parts, 0);
  // marks: [0] before the counts, [1] after them, [2] after the scans, [3]
  // before the fills, [4] after them (the pools are allocated in between, on
  // the host, from the scans' totals)
  StageEvents ev(m, mp->n_parts, 5, kernel_ms != nullptr);  // after tot: drains before it is freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part& p = mp->parts[r];
    const spf_mplan::Part::Delta& d = p.dl;
    spf_mplan::Part::Update& u = mp->parts[r].up;
    const uint32_t n = (uint32_t)d.req.size();
    if (!n) continue;
    spf_ctx* c = m->members[r];
    M_TRY(ev.open(r));
    const hipStream_t s = m->exec[r];
    for (uint32_t w = 0; w < 2; ++w) {
      M_HIP(m, u.ptr[w].alloc(d.n[w] + 1));
      M_HIP(m, u.src[w].alloc(std::max<uint64_t>(d.n[w], 1)));
      M_HIP(m, u.sums[w].alloc(std::max<uint64_t>(label_scan_tiles(d.n[w]), 1)));
    }
    M_HIP(m, u.owner.alloc(std::max<uint64_t>(d.n[1], 1)));
    M_TRY(ev.mark(r, 0));
    spf_status st = launch_update_count_ip(c, d.ptr[0].p, d.set[0].p, n, d.n[0], p.db.hdr.p, p.db.base.p, S,
                                           u.ptr[0].p, u.src[0].p, s);
    if (st == SPF_OK && labels)
      st = launch_update_count_labels(c, d.ptr[1].p, d.set[1].p, n, d.n[1], d.lab.p, d.mnew.p, U, p.lr.owner.p,
                                      p.lr.ptr.p, G, u.ptr[1].p, u.src[1].p, u.owner.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 1));
    for (uint32_t w = 0; w < 2 && st == SPF_OK; ++w) st = launch_label_scan(c, u.ptr[w].p, d.n[w], u.sums[w].p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 2));
    for (uint32_t w = 0; w < 2; ++w)
      M_HIP(m, hipMemcpyAsync(&tot[2 * r + w], u.ptr[w].p + d.n[w], 8, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part& p = mp->parts[r];
    const spf_mplan::Part::Delta& d = p.dl;
    spf_mplan::Part::Update& u = mp->parts[r].up;
    if (d.req.empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scans' totals
    // the record pools: exactly the totals (kept when the previous ones are large enough)
    for (uint32_t w = 0; w < 2; ++w) {
      M_HIP(m, u.rec[w].alloc(std::max<unsigned long long>(tot[2 * r + w], 1)));
      u.nrec[w] = tot[2 * r + w];
    }
    M_TRY(ev.mark(r, 3));
    spf_status st = launch_update_fill(c, u.ptr[0].p, u.src[0].p, d.n[0], p.db.pool.p, u.rec[0].p, s);
    if (st == SPF_OK && labels) st = launch_update_fill(c, u.ptr[1].p, u.src[1].p, d.n[1], p.lr.rec.p, u.rec[1].p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 4));
  }
  double ms[3] = {0, 0, 0};
  uint64_t out[4] = {mp->dl.tot[0], 0, mp->dl.tot[2], 0}, bytes = 0;
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part::Delta& d = mp->parts[r].dl;
    const spf_mplan::Part::Update& u = mp->parts[r].up;
    if (d.req.empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    out[1] += u.nrec[0];
    out[3] += u.nrec[1];
    bytes += 8 * u.nrec[0] + 8 * (d.n[0] + 1) + 8 * u.nrec[1] + 8 * (d.n[1] + 1) + 4 * d.n[1];
    M_TRY(ev.slowest(r, {0, 1, 3}, ms));
  }
  mp->up.done = true;
  if (kernel_ms) std::copy(ms, ms + 3, mp->up.ms);
  if (totals) std::copy(out, out + 4, totals);
  if (pool_bytes) *pool_bytes = bytes;
  if (kernel_ms) *kernel_ms = ms[0] + ms[1] + ms[2];
  return SPF_OK;
}

spf_status spf_mplan_route_update_timing(const spf_mplan* mp, double* ms) {
  if (!mp || !ms) return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_update_timing: NULL argument");
  std::copy(mp->up.ms, mp->up.ms + 3, ms);
  return SPF_OK;
}

spf_status spf_mplan_route_update_db(spf_mplan* mp, uint32_t t, uint64_t* ip_ptr, uint64_t* ip_rec,
                                     uint64_t ip_cap, uint64_t* n_ip_rec, uint32_t* label_owner,
                                     uint64_t* label_ptr, uint64_t* label_rec, uint64_t label_cap,
                                     uint64_t* n_label_rec) {
  if (mp && !mp->has_update())
    return mfail(mp->m, SPF_E_STATE, "spf_mplan_route_update_db: no update (call spf_mplan_route_update)");
  if (!mp || t >= mp->dl.loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_update_db: no such me");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->dl.loc[t];
  const spf_mplan::Part::Delta& d = mp->parts[r].dl;
  const spf_mplan::Part::Update& u = mp->parts[r].up;
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  uint64_t e[2][2];  // me's entries [e[w][0], e[w][1]) of either list
  for (uint32_t w = 0; w < 2; ++w) M_HIP(m, hipMemcpyAsync(e[w], d.ptr[w].p + k, 16, hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  uint64_t* const optr[2] = {ip_ptr, label_ptr};
  uint64_t* const orec[2] = {ip_rec, label_rec};
  const uint64_t cap[2] = {ip_cap, label_cap};
  uint64_t* const cnt[2] = {n_ip_rec, n_label_rec};
  std::vector<uint64_t> h[2];
  for (uint32_t w = 0; w < 2; ++w) {  // the entries' offsets (the next entry's, or the total, ends the last)
    h[w].resize(e[w][1] - e[w][0] + 1);
    M_HIP(m, hipMemcpyAsync(h[w].data(), u.ptr[w].p + e[w][0], 8 * h[w].size(), hipMemcpyDeviceToHost, s));
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
      M_HIP(m, hipMemcpyAsync(orec[w], u.rec[w].p + h[w][0], 8 * c, hipMemcpyDeviceToHost, s));
    if (optr[w])
      for (size_t j = 0; j < h[w].size(); ++j) optr[w][j] = h[w][j] - h[w][0];
  }
  if (label_owner && e[1][1] > e[1][0])
    M_HIP(m, hipMemcpyAsync(label_owner, u.owner.p + e[1][0], 4 * (e[1][1] - e[1][0]), hipMemcpyDeviceToHost, s));
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
  if (!mp->has_update())
    return mfail(m, SPF_E_STATE, "spf_mplan_route_update_read: no update (call spf_mplan_route_update)");
  const spf_mplan::Part::Delta& d = mp->parts[member].dl;
  const spf_mplan::Part::Update& u = mp->parts[member].up;
  const uint64_t slots = d.req.size();
  const uint64_t size[5] = {slots, slots ? d.n[0] : 0, slots ? u.nrec[0] : 0, slots ? d.n[1] : 0,
                            slots ? u.nrec[1] : 0};
  if (n) std::copy(size, size + 5, n);
  if (!slots) return SPF_OK;
  M_HIP(m, hipSetDevice(m->members[member]->device));
  const hipStream_t s = m->exec[member];
  uint64_t* const dptr[2] = {ip_dptr, label_dptr};
  uint32_t* const dset[2] = {ip_dset, label_dset};
  uint64_t* const uptr[2] = {ip_uptr, label_uptr};
  uint64_t* const urec[2] = {ip_urec, label_urec};
  for (uint32_t w = 0; w < 2; ++w) {
    const uint64_t e = d.n[w], r = u.nrec[w];
    if (dptr[w]) M_HIP(m, hipMemcpyAsync(dptr[w], d.ptr[w].p, 8 * (slots + 1), hipMemcpyDeviceToHost, s));
    if (dset[w] && e) M_HIP(m, hipMemcpyAsync(dset[w], d.set[w].p, 4 * e, hipMemcpyDeviceToHost, s));
    if (uptr[w]) M_HIP(m, hipMemcpyAsync(uptr[w], u.ptr[w].p, 8 * (e + 1), hipMemcpyDeviceToHost, s));
    if (urec[w] && r) M_HIP(m, hipMemcpyAsync(urec[w], u.rec[w].p, 8 * r, hipMemcpyDeviceToHost, s));
  }
  if (label_uowner && d.n[1])
    M_HIP(m, hipMemcpyAsync(label_uowner, u.owner.p, 4 * d.n[1], hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  return SPF_OK;
}

spf_status spf_mplan_route_update_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_ip_uptr,
                                          const uint64_t** d_ip_urec, const uint32_t** d_label_uowner,
                                          const uint64_t** d_label_uptr, const uint64_t** d_label_urec,
                                          uint64_t* n_ip_rec, uint64_t* n_label_rec) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_route_update_buffers: bad argument");
  if (!mp->has_update())
    return mfail(mp->m, SPF_E_STATE, "spf_mplan_route_update_buffers: no update (call spf_mplan_route_update)");
  const spf_mplan::Part::Update& u = mp->parts[member].up;
  const bool has = !mp->parts[member].dl.req.empty();  // (a member without a me of the delta holds nothing of it)
  if (d_ip_uptr) *d_ip_uptr = has ? reinterpret_cast<const uint64_t*>(u.ptr[0].p) : nullptr;
  if (d_ip_urec) *d_ip_urec = has ? reinterpret_cast<const uint64_t*>(u.rec[0].p) : nullptr;
  if (d_label_uowner) *d_label_uowner = has ? u.owner.p : nullptr;
  if (d_label_uptr) *d_label_uptr = has ? reinterpret_cast<const uint64_t*>(u.ptr[1].p) : nullptr;
  if (d_label_urec) *d_label_urec = has ? reinterpret_cast<const uint64_t*>(u.rec[1].p) : nullptr;
  if (n_ip_rec) *n_ip_rec = has ? u.nrec[0] : 0;
  if (n_label_rec) *n_label_rec = has ? u.nrec[1] : 0;
  return SPF_OK;
}

}  // extern "C"
