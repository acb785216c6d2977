// ============================================================================
//  whatif_pool.cpp -- what every list product of a what-if plan (WiPool,
//  engine_internal.h) shares on the host: sizing the arrays from the scan's
//  total, and the _read / _buffers / _db calls of the change lists
//  (whatif.hip), the route lists (whatif_routes.hip) and the impact lists
//  (whatif_impact.hip), which forward here with their own names.
// ============================================================================
#include "engine_internal.h"
#include "whatif_pool_host.h"

namespace spfi {

spf_status pool_held(spf_whatif_plan* p, WiPoolId id, const char* who, WiListsView* v) {
  static const char* const kWhat[] = {"lists", "route lists",
                                      "impact lists (spf_whatif_by_node first)",
                                      "impact lists (spf_whatif_by_set first)",
                                      "route updates (spf_whatif_route_update first)",
                                      "route updates (spf_whatif_route_update first)"};
  if (!p) return fail(nullptr, SPF_E_INVALID, "%s: NULL plan", who);
  whatif_lists_view(p, v);
  if (!v->pool(id)->valid) return fail(v->ctx, SPF_E_STATE, "%s: the plan holds no %s", who, kWhat[id]);
  return SPF_OK;
}

spf_status pool_size(spf_ctx* c, WiPool* q, uint64_t total, uint32_t W, const char* who) {
  const size_t room = std::max<size_t>(1, (size_t)total);
  if (q->key.alloc(room) != hipSuccess || q->val.alloc(room) != hipSuccess ||
      (W && q->rows.alloc(room * W) != hipSuccess)) {  // (kept while they are large enough)
    (void)hipGetLastError();
    q->key.reset();
    q->val.reset();
    q->rows.reset();
    return fail(c, SPF_E_NOMEM, "%s: no memory for %llu entries of %u bytes", who,
                (unsigned long long)total, 12u + 4u * W);
  }
  q->W = W;
  return SPF_OK;
}

uint64_t pool_bytes(const WiPool& q) {
  return 8ull * ((uint64_t)q.n_owners + 1) + q.total * (12ull + 4ull * q.W);
}

spf_status pool_read(spf_whatif_plan* p, WiPoolId id, const char* who, uint64_t* ptr, uint32_t* key,
                     uint64_t* val, uint32_t* rows) {
  WiListsView v;
  if (const spf_status st = pool_held(p, id, who, &v); st != SPF_OK) return st;
  spf_ctx* c = v.ctx;
  const WiPool& q = *v.pool(id);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t t = (size_t)q.total;
  if (ptr) HIP_TRY(c, hipMemcpy(ptr, q.ptr.p, 8ull * ((size_t)q.n_owners + 1), hipMemcpyDeviceToHost));
  if (key && t) HIP_TRY(c, hipMemcpy(key, q.key.p, 4ull * t, hipMemcpyDeviceToHost));
  if (val && t) HIP_TRY(c, hipMemcpy(val, q.val.p, 8ull * t, hipMemcpyDeviceToHost));
  if (rows && t && q.W) HIP_TRY(c, hipMemcpy(rows, q.rows.p, 4ull * t * q.W, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status pool_buffers(spf_whatif_plan* p, WiPoolId id, const char* who, const uint64_t** d_ptr,
                        const uint32_t** d_key, const uint64_t** d_val, const uint32_t** d_rows,
                        uint32_t* n_owners, uint32_t* W, uint64_t* n_entries) {
  WiListsView v;
  if (const spf_status st = pool_held(p, id, who, &v); st != SPF_OK) return st;
  const WiPool& q = *v.pool(id);
  if (d_ptr) *d_ptr = reinterpret_cast<const uint64_t*>(q.ptr.p);
  if (d_key) *d_key = q.key.p;
  if (d_val) *d_val = reinterpret_cast<const uint64_t*>(q.val.p);
  if (d_rows) *d_rows = q.rows.p;
  if (n_owners) *n_owners = q.n_owners;
  if (W) *W = q.W;
  if (n_entries) *n_entries = q.total;
  return SPF_OK;
}

spf_status pool_db(spf_whatif_plan* p, WiPoolId id, const char* who, uint32_t owner, uint32_t* key,
                   uint64_t* val, uint32_t* rows, uint64_t cap, uint64_t* n) {
  WiListsView v;
  if (const spf_status st = pool_held(p, id, who, &v); st != SPF_OK) return st;
  spf_ctx* c = v.ctx;
  const WiPool& q = *v.pool(id);
  if (owner >= q.n_owners)
    return fail(c, SPF_E_INVALID, "%s: %s %u of %u", who, id < kPoolByNode ? "failure" : "key", owner,
                q.n_owners);
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long at[2] = {0, 0};
  HIP_TRY(c, hipMemcpy(at, q.ptr.p + owner, 16, hipMemcpyDeviceToHost));
  uint64_t cnt = 0;
  bool copy = false;
  const spf_status st = pool_slice(at[0], at[1], q.total, key || val || rows, cap, &cnt, &copy);
  if (st == SPF_E_HIP) return fail(c, st, "%s: offsets not monotone", who);
  if (n) *n = cnt;
  const size_t m = (size_t)cnt, W = q.W;
  if (st != SPF_OK)
    return fail(c, st, "%s: %zu entries, room for %llu", who, m, (unsigned long long)cap);
  if (!copy) return SPF_OK;
  std::vector<uint32_t> hk(m), hw(m * W);
  std::vector<uint64_t> hv(m);
  HIP_TRY(c, hipMemcpy(hk.data(), q.key.p + at[0], 4 * m, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(hv.data(), q.val.p + at[0], 8 * m, hipMemcpyDeviceToHost));
  if (W) HIP_TRY(c, hipMemcpy(hw.data(), q.rows.p + at[0] * W, 4 * m * W, hipMemcpyDeviceToHost));
  const std::vector<size_t> order = pool_order(hk.data(), hv.data(), m);
  for (size_t k = 0; k < m; ++k) {
    const size_t e = order[k];
    if (key) key[k] = hk[e];
    if (val) val[k] = hv[e];
    if (rows && W) std::memcpy(rows + k * W, hw.data() + e * W, 4 * W);
  }
  return SPF_OK;
}

}  // namespace spfi
