// ============================================================================
//  mplan_prefix_routes.cpp -- the prefix-routes stage of a multi-device plan
//  (include/openr_spf.h, "prefix routes"): every me's unicast route decision
//  from prefix entries, over the rows and next-hop bitmaps spf_mplan_execute
//  left resident in the members' HBM.
//
//  The stage has its own state (spf_mplan::Part::Prefixes per member,
//  spf_mplan::Prefixes per plan, mplan_internal.h) and touches no other
//  stage's: route records, label routes, snapshots and deltas read back
//  unchanged after a call.  The table is validated and reduced on the host
//  (prefix_table_host.cpp) before anything is uploaded or launched; the
//  kernels are prefix_routes.hip's, the scan is label_routes.hip's.
// ============================================================================
#include <algorithm>

#include "mplan_stage.h"
#include "prefix_table_host.h"

using namespace spfi;

extern "C" {

spf_status spf_mplan_prefix_routes(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* pfx_ptr, const uint32_t* ent_node, const int32_t* ent_pp,
                                   const int32_t* ent_sp, const int32_t* ent_dist, const int64_t* ent_min_nh,
                                   uint32_t n_pfx, const uint8_t* overloaded, uint32_t flags,
                                   uint64_t* n_records, uint64_t* pool_bytes, double* kernel_ms) {
  if (!mp || (n_me && !me_req) || (n_pfx && !pfx_ptr))
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_prefix_routes: NULL argument");
  spf_mctx* m = mp->m;
  spf_mplan::Prefixes& X = mp->px;
  X.have = false;  // (a failed call leaves no prefix database)
  X.loc.clear();
  M_TRY(me_check(mp, me_req, n_me));
  const bool lfa = (flags & SPF_ROUTE_LFA) != 0, all_best = (flags & SPF_PREFIX_ALL_BEST) != 0;
  PrefixTable tab;
  std::string err;
  const spf_status ts = prefix_table_build(pfx_ptr, ent_node, ent_pp, ent_sp, ent_dist, ent_min_nh, n_pfx,
                                           overloaded, m->members[0]->N, all_best, &tab, &err);
  if (ts != SPF_OK) return mfail(m, ts, "spf_mplan_prefix_routes: %s", err.c_str());
  M_TRY(route_prepare_rows(mp, lfa, me_req, n_me));
  const uint32_t P = n_pfx;
  ReqMap q(mp, me_req, n_me);
  for (uint32_t r = 0; r < mp->n_parts; ++r) mp->parts[r].px.req = q.req[r];
  std::vector<unsigned long long> tot(mp->n_parts, 0);
  std::vector<uint32_t> fl(mp->n_parts, 0);
  // marks: [0] before the count, [1] after it, [2] after the scan, [3] before
  // the fill, [4] after it (the pool is allocated in between, on the host,
  // from the scan's total)
  StageEvents ev(m, mp->n_parts, 5, kernel_ms != nullptr);  // after tab / q / tot / fl: drains before they are freed
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part::Select& sel = mp->parts[r].sel;
    spf_mplan::Part::Prefixes& p = mp->parts[r].px;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_TRY(ev.open(r));
    const hipStream_t s = m->exec[r];
    const uint32_t n = (uint32_t)q.mine[r].size();
    const uint64_t cells = (uint64_t)n * P;
    M_HIP(m, p.me.upload(q.mine[r].data(), n, s));
    M_HIP(m, p.pptr.upload(tab.ptr.data(), (size_t)P + 1, s));
    M_HIP(m, p.ent.upload(tab.ent.data(), tab.ent.size(), s));
    M_HIP(m, p.info.alloc(std::max<uint64_t>(cells, 1)));
    M_HIP(m, p.ptr.alloc(cells + 1));
    M_HIP(m, p.sums.alloc(std::max<uint64_t>(label_scan_tiles(cells), 1)));
    M_HIP(m, p.flags.alloc(1));
    M_HIP(m, hipMemsetAsync(p.flags.p, 0, 4, s));
    M_TRY(ev.mark(r, 0));
    spf_status st = launch_prefix_routes(c, false, sel.rowp.p, sel.nhp.p, p.me.p, n, p.pptr.p, p.ent.p, P, lfa,
                                         all_best, p.info.p, p.ptr.p, nullptr, p.flags.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 1));
    st = launch_label_scan(c, p.ptr.p, cells, p.sums.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 2));
    M_HIP(m, hipMemcpyAsync(&tot[r], p.ptr.p + cells, 8, hipMemcpyDeviceToHost, s));
  }
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    const spf_mplan::Part::Select& sel = mp->parts[r].sel;
    spf_mplan::Part::Prefixes& p = mp->parts[r].px;
    if (q.mine[r].empty()) continue;
    spf_ctx* c = m->members[r];
    M_HIP(m, hipSetDevice(c->device));
    const hipStream_t s = m->exec[r];
    M_HIP(m, hipStreamSynchronize(s));  // the scan's total
    // the record pool: exactly the total (kept when the previous one is large enough)
    M_HIP(m, p.rec.alloc(std::max<unsigned long long>(tot[r], 1)));
    p.records = tot[r];
    M_TRY(ev.mark(r, 3));
    const spf_status st = launch_prefix_routes(c, true, sel.rowp.p, sel.nhp.p, p.me.p, (uint32_t)q.mine[r].size(),
                                               p.pptr.p, p.ent.p, P, lfa, all_best, p.info.p, p.ptr.p, p.rec.p,
                                               p.flags.p, s);
    if (st != SPF_OK) return member_fail(m, r, st);
    M_TRY(ev.mark(r, 4));
    M_HIP(m, hipMemcpyAsync(&fl[r], p.flags.p, 4, hipMemcpyDeviceToHost, s));
  }
  uint64_t total = 0, bytes = 0;
  double ms[3] = {0, 0, 0};
  for (uint32_t r = 0; r < mp->n_parts; ++r) {
    if (q.mine[r].empty()) continue;
    M_HIP(m, hipSetDevice(m->members[r]->device));
    M_HIP(m, hipStreamSynchronize(m->exec[r]));
    if (fl[r] & 2u) return mfail(m, SPF_E_UNSUPPORTED, "a next-hop metric exceeds 2^32 - 1");
    const uint64_t cells = (uint64_t)q.mine[r].size() * P;
    total += tot[r];
    bytes += 8 * tot[r] + 8 * (cells + 1) + 8 * cells;
    M_TRY(ev.slowest(r, {0, 1, 3}, ms));
  }
  X.loc = std::move(q.loc);
  X.n_pfx = P;
  std::copy(ms, ms + 3, X.ms);
  X.have = true;
  if (n_records) *n_records = total;
  if (pool_bytes) *pool_bytes = bytes;
  if (kernel_ms) *kernel_ms = ev.worst;
  return SPF_OK;
}

spf_status spf_mplan_prefix_route_db(spf_mplan* mp, uint32_t t, uint64_t* info, uint64_t* ptr, uint64_t* rec,
                                     uint64_t cap, uint64_t* n) {
  if (!mp || !mp->has_prefix_routes() || t >= mp->px.loc.size())
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID,
                 "spf_mplan_prefix_route_db: no such me (call spf_mplan_prefix_routes)");
  spf_mctx* m = mp->m;
  const auto [r, k] = mp->px.loc[t];
  spf_mplan::Part::Prefixes& p = mp->parts[r].px;
  const uint32_t P = mp->px.n_pfx;
  M_HIP(m, hipSetDevice(m->members[r]->device));
  const hipStream_t s = m->exec[r];
  // me's P + 1 offsets (the next slot's first one, or the total, ends them)
  std::vector<uint64_t> h((size_t)P + 1);
  M_HIP(m, hipMemcpyAsync(h.data(), p.ptr.p + (size_t)k * P, 8ull * (P + 1), hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  const uint64_t cnt = h[P] - h[0];
  if (n) *n = cnt;
  if (rec && cap < cnt)
    return mfail(m, SPF_E_NOMEM, "prefix route db of %llu records, room for %llu", (unsigned long long)cnt,
                 (unsigned long long)cap);
  if (info && P) M_HIP(m, hipMemcpyAsync(info, p.info.p + (size_t)k * P, 8ull * P, hipMemcpyDeviceToHost, s));
  if (rec && cnt) M_HIP(m, hipMemcpyAsync(rec, p.rec.p + h[0], 8ull * cnt, hipMemcpyDeviceToHost, s));
  M_HIP(m, hipStreamSynchronize(s));
  if (ptr)
    for (uint32_t g = 0; g <= P; ++g) ptr[g] = h[g] - h[0];
  return SPF_OK;
}

spf_status spf_mplan_prefix_route_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_info,
                                          const uint64_t** d_ptr, const uint64_t** d_rec, uint64_t* n_records,
                                          uint32_t* slots, uint32_t cap, uint32_t* n_slots) {
  if (!mp || member >= mp->n_parts)
    return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_prefix_route_buffers: bad argument");
  const spf_mplan::Part::Prefixes& p = mp->parts[member].px;
  // (a member without a me of the last call holds nothing of it)
  const bool has = mp->has_prefix_routes() && !p.req.empty();
  const uint32_t k = has ? (uint32_t)p.req.size() : 0u;
  if (n_slots) *n_slots = k;
  if (d_info) *d_info = has ? reinterpret_cast<const uint64_t*>(p.info.p) : nullptr;
  if (d_ptr) *d_ptr = has ? reinterpret_cast<const uint64_t*>(p.ptr.p) : nullptr;
  if (d_rec) *d_rec = has ? reinterpret_cast<const uint64_t*>(p.rec.p) : nullptr;
  if (n_records) *n_records = has ? p.records : 0;
  if (slots) {
    if (cap < k) return mfail(mp->m, SPF_E_NOMEM, "%u me slots, room for %u", k, cap);
    std::copy(p.req.begin(), p.req.begin() + k, slots);
  }
  return SPF_OK;
}

spf_status spf_mplan_prefix_routes_timing(const spf_mplan* mp, double* ms) {
  if (!mp || !ms) return mfail(mp ? mp->m : nullptr, SPF_E_INVALID, "spf_mplan_prefix_routes_timing: NULL argument");
  if (!mp->has_prefix_routes())
    return mfail(mp->m, SPF_E_STATE, "spf_mplan_prefix_routes_timing: no prefix database");
  std::copy(mp->px.ms, mp->px.ms + 3, ms);
  return SPF_OK;
}

uint32_t spf_prefix_routes_threads(void) { return prefix_routes_threads(); }
uint32_t spf_prefix_routes_links(void) { return prefix_routes_links(); }
uint32_t spf_prefix_routes_scan_tile(void) { return label_scan_tile(); }

}  // extern "C"
