// ============================================================================
//  preds.hip -- pathLinks: the predecessor lists of a source from its distance
//  row (tight in-edges of expanded predecessors, in (dist, node, edge) =
//  Dijkstra pop order).  preds_kernel, preds_from_row (one row on the device),
//  spf_preds and spf_plan_preds.
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"
#include "wave_ops.h"

using namespace spfi;

namespace {

// ---------------------------------------------------------------------------
//  3. predecessor lists (pathLinks) of one source
// ---------------------------------------------------------------------------
// pass 0: count, pass 1: fill sorted by (dist[u], edge id) -- edge ids of one
// tail are contiguous in CSR order and tails appear in id (= name) order, so
// this is the reference's (pop order, linksFromNode order).
template <int PASS>
__global__ void preds_kernel(const uint32_t* __restrict__ dist0,  // [n_src][pitch]
                             uint32_t pitch,
                             const uint32_t* __restrict__ row_ptr,
                             const uint32_t* __restrict__ col,
                             const uint32_t* __restrict__ wt,
                             const uint32_t* __restrict__ rev,
                             const uint8_t* __restrict__ ovl,
                             const uint32_t* __restrict__ link,
                             const uint32_t* __restrict__ ign,
                             const uint32_t* __restrict__ srcs,  // [n_src] (blockIdx.y)
                             uint32_t N, uint32_t hop,
                             uint32_t* __restrict__ cnt_or_ptr0,  // [n_src][N + 1]
                             uint32_t* __restrict__ pred_edge,
                             unsigned long long* __restrict__ pred_key /* PASS 1: sort keys */) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= N) return;
  const uint32_t* dist = dist0 + (size_t)blockIdx.y * pitch;
  uint32_t* cnt_or_ptr = cnt_or_ptr0 + (size_t)blockIdx.y * (N + 1);
  const uint32_t src = srcs[blockIdx.y];
  const uint32_t dv = dist[v];
  uint32_t n = 0;
  uint32_t base = PASS ? cnt_or_ptr[v] : 0;
  if (dv != kInf && v != src) {
    for (uint32_t e = row_ptr[v]; e < row_ptr[v + 1]; ++e) {
      const uint32_t u = col[e];
      const uint32_t r = rev[e];  // the directed edge u -> v
      if (ovl[u] && u != src) continue;
      if (ign && link_ignored(ign, link[e])) continue;
      const uint32_t du = dist[u];
      if (du == kInf) continue;
      if (du + (hop ? 1u : wt[r]) != dv) continue;
      if (PASS) {
        // insertion into the sorted segment [base, base+n) by (dist of the
        // tail, edge id), the keys kept beside the edges (one load per step
        // where re-deriving a key was three dependent loads)
        const unsigned long long key = ((unsigned long long)du << 32) | r;
        uint32_t p = base + n;
        while (p > base) {
          const unsigned long long pk = pred_key[p - 1];
          if (pk < key) break;
          pred_key[p] = pk;
          pred_edge[p] = (uint32_t)pk;
          --p;
        }
        pred_key[p] = key;
        pred_edge[p] = r;
      }
      ++n;
    }
  }
  if (!PASS) cnt_or_ptr[v] = n;
}

}  // namespace

namespace spfi {

// pathLinks of one source from its distance row already on the device
// (d_row = [N] u32, positive metrics or hop counts): counts, host prefix
// sum, then the ordered lists (the batch form is spf_plan_preds).
spf_status preds_from_row(spf_ctx* c, uint32_t src, bool hop, const uint32_t* ign,
                          const uint32_t* d_row, uint32_t* pred_ptr, uint32_t* pred_edge,
                          uint32_t cap, uint32_t* n_preds, hipStream_t s) {
  const uint32_t N = c->N;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->d_pred_cnt.alloc(N + 1));
  const dim3 g((N + 255) / 256), b(256);
  HIP_TRY(c, c->d_one_src.upload(&src, 1, s));
  hipLaunchKernelGGL((preds_kernel<0>), g, b, 0, s, d_row, N, c->d_row_ptr.p, c->d_col.p,
                     c->d_wt.p, c->d_rev.p, c->d_ovl.p, c->d_link.p, ign, c->d_one_src.p, N,
                     hop ? 1u : 0u, c->d_pred_cnt.p, (uint32_t*)nullptr,
                     (unsigned long long*)nullptr);
  HIP_TRY(c, hipGetLastError());
  std::vector<uint32_t> cnt(N);
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->d_pred_cnt.p, 4ull * N, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  pred_ptr[0] = 0;
  for (uint32_t v = 0; v < N; ++v) pred_ptr[v + 1] = pred_ptr[v] + cnt[v];
  *n_preds = pred_ptr[N];
  if (!pred_edge) return SPF_OK;
  if (cap < pred_ptr[N]) return fail(c, SPF_E_INVALID, "pred_edge capacity %u < %u", cap, pred_ptr[N]);
  HIP_TRY(c, hipMemcpyAsync(c->d_pred_cnt.p, pred_ptr, 4ull * N, hipMemcpyHostToDevice, s));
  HIP_TRY(c, c->d_pred_edge.alloc(std::max<uint32_t>(pred_ptr[N], 1)));
  HIP_TRY(c, c->d_pred_key.alloc(std::max<uint32_t>(pred_ptr[N], 1)));
  hipLaunchKernelGGL((preds_kernel<1>), g, b, 0, s, d_row, N, c->d_row_ptr.p, c->d_col.p,
                     c->d_wt.p, c->d_rev.p, c->d_ovl.p, c->d_link.p, ign, c->d_one_src.p, N,
                     hop ? 1u : 0u, c->d_pred_cnt.p, c->d_pred_edge.p, c->d_pred_key.p);
  HIP_TRY(c, hipGetLastError());
  if (pred_ptr[N])
    HIP_TRY(c, hipMemcpyAsync(pred_edge, c->d_pred_edge.p, 4ull * pred_ptr[N], hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SPF_OK;
}

}  // namespace spfi

extern "C" {

spf_status spf_preds(spf_ctx* c, uint32_t src, uint32_t flags, const uint32_t* ignore_links,
                     uint32_t n_ignore, const uint32_t* dist, uint32_t* pred_ptr,
                     uint32_t* pred_edge, uint32_t cap, uint32_t* n_preds) {
  if (!c || !dist || !pred_ptr || !n_preds) return fail(c, SPF_E_INVALID, "spf_preds: NULL argument");
  if (!c->loaded) return fail(c, SPF_E_STATE, "no graph loaded");
  if (src >= c->N) return fail(c, SPF_E_INVALID, "source %u out of range", src);
  const uint32_t* ign = nullptr;
  spf_status st = upload_ignore(c, ignore_links, n_ignore, &ign);
  if (st != SPF_OK) return st;
  HIP_TRY(c, c->d_row.upload(dist, c->N, c->stream));
  return preds_from_row(c, src, (flags & SPF_FLAG_HOP_COUNT) != 0, ign, c->d_row.p, pred_ptr,
                        pred_edge, cap, n_preds, c->stream);
}

spf_status spf_plan_preds(spf_plan* p, uint32_t* pred_ptr, uint32_t* pred_edge, uint64_t cap,
                          uint64_t* n_preds) {
  if (!p || !pred_ptr || !n_preds) return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_plan_preds: NULL argument");
  spf_ctx* c = p->ctx;
  // positive metrics (or hop counts) with u32 rows: pathLinks follow from the
  // distance row alone, whichever kernel wrote it -- big plans
  // and exact plans of large positive-metric graphs included.  Zero /
  // negative metrics and u64 rows need the pop order (spf_solve_exact).
  const bool hop_only = (p->flags & SPF_FLAG_HOP_COUNT) != 0;
  if ((p->flags & SPF_FLAG_DIST64) || (!hop_only && c->nonpos))
    return fail(c, SPF_E_UNSUPPORTED, "spf_plan_preds: zero / negative metrics and u64 rows order "
                                      "pathLinks by pop rank (spf_solve_exact)");
  if (!p->h_dist.p || p->h_epoch != c->epoch)
    return fail(c, SPF_E_STATE, "spf_plan_preds: no spf_plan_execute_host on the current graph");
  const uint32_t N = c->N, n = p->n_src;
  const bool hop = (p->flags & SPF_FLAG_HOP_COUNT) != 0;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t slots = (size_t)n * (N + 1);
  HIP_TRY(c, p->h_pcnt.alloc(slots));
  const dim3 g((N + 255) / 256, n), b(256);
  hipLaunchKernelGGL((preds_kernel<0>), g, b, 0, c->stream, p->h_dist.p, c->pitch, c->d_row_ptr.p,
                     c->d_col.p, c->d_wt.p, c->d_rev.p, c->d_ovl.p, c->d_link.p, nullptr,
                     p->d_srcs.p, N, hop ? 1u : 0u, p->h_pcnt.p, (uint32_t*)nullptr,
                     (unsigned long long*)nullptr);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, c->pin_preds.alloc(slots));
  HIP_TRY(c, hipMemcpyAsync(c->pin_preds.p, p->h_pcnt.p, 4ull * slots, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::memcpy(pred_ptr, c->pin_preds.p, 4ull * slots);
  // counts -> absolute offsets: source i's list of v starts at pred_ptr[i*(N+1) + v],
  // pred_ptr[i*(N+1) + N] = the end of source i's lists
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t* pp = pred_ptr + (size_t)i * (N + 1);
    for (uint32_t v = 0; v < N; ++v) {
      const uint32_t cnt = pp[v];
      if (at + cnt > 0xFFFFFFFFull) return fail(c, SPF_E_UNSUPPORTED, "spf_plan_preds: > 2^32 entries");
      pp[v] = (uint32_t)at;
      at += cnt;
    }
    pp[N] = (uint32_t)at;
  }
  *n_preds = at;
  if (!pred_edge) return SPF_OK;
  if (cap < at) return fail(c, SPF_E_NOMEM, "spf_plan_preds: capacity %llu < %llu",
                            (unsigned long long)cap, (unsigned long long)at);
  // one staging buffer for the upload and the edges (sized before either copy)
  HIP_TRY(c, c->pin_preds.alloc(std::max<uint64_t>(slots, at)));
  std::memcpy(c->pin_preds.p, pred_ptr, 4ull * slots);
  HIP_TRY(c, hipMemcpyAsync(p->h_pcnt.p, c->pin_preds.p, 4ull * slots, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, p->h_pedge.alloc(std::max<uint64_t>(at, 1)));
  HIP_TRY(c, p->h_pkey.alloc(std::max<uint64_t>(at, 1)));
  hipLaunchKernelGGL((preds_kernel<1>), g, b, 0, c->stream, p->h_dist.p, c->pitch, c->d_row_ptr.p,
                     c->d_col.p, c->d_wt.p, c->d_rev.p, c->d_ovl.p, c->d_link.p, nullptr,
                     p->d_srcs.p, N, hop ? 1u : 0u, p->h_pcnt.p, p->h_pedge.p, p->h_pkey.p);
  HIP_TRY(c, hipGetLastError());
  if (at)
    HIP_TRY(c, hipMemcpyAsync(c->pin_preds.p, p->h_pedge.p, 4ull * at, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (at) std::memcpy(pred_edge, c->pin_preds.p, 4ull * at);
  return SPF_OK;
}

}  // extern "C"
