// ============================================================================
//  graph.cpp -- the spf_graph_* C-ABI (include/openr_spf.h): each call checks
//  its arguments, changes the host state (graph_host.cpp), uploads what that
//  left dirty, synchronises and bumps the epoch.
// ============================================================================
#include "engine_internal.h"

using namespace spfi;

namespace {

// A HIP failure after the host state changed leaves the device copy behind
// it: the context is unloaded, so the next call must reload.
spf_status uploaded(spf_ctx* c, spf_status st) {
  if (st == SPF_OK) ++c->epoch;
  else c->loaded = false;
  return st;
}

spf_status upload_graph(spf_ctx* c) {
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->d_row_ptr.upload(c->row_ptr.data(), c->N + 1, c->stream));
  HIP_TRY(c, c->d_col.upload(c->col.data(), c->E, c->stream));
  HIP_TRY(c, c->d_wt.upload(c->wt.data(), c->E, c->stream));
  HIP_TRY(c, c->d_met.upload(c->met.data(), c->E, c->stream));
  HIP_TRY(c, c->d_rev.upload(c->rev.data(), c->E, c->stream));
  HIP_TRY(c, c->d_link.upload(c->link.data(), c->E, c->stream));
  HIP_TRY(c, c->d_ovl.upload(c->ovl.data(), c->N, c->stream));
  HIP_TRY(c, c->d_nb_ptr.upload(c->nb_ptr.data(), c->N + 1, c->stream));
  HIP_TRY(c, c->d_nb_id.upload(c->nb_id.data(), c->nb_id.size(), c->stream));
  HIP_TRY(c, c->d_nb_w.upload(c->nb_w.data(), c->nb_w.size(), c->stream));
  HIP_TRY(c, c->d_edge_nb.upload(c->edge_nb.data(), c->edge_nb.size(), c->stream));
  HIP_TRY(c, c->d_sell_ptr.upload(c->sell_ptr.data(), c->sell_ptr.size(), c->stream));
  HIP_TRY(c, c->d_sell_col.upload(c->sell_col.data(), c->sell_col.size(), c->stream));
  if (!c->ms_smap.empty()) HIP_TRY(c, c->d_ms_smap.upload(c->ms_smap.data(), c->ms_smap.size(), c->stream));
  if (!c->sell4.empty()) {
    HIP_TRY(c, c->d_sell4_ptr.upload(c->sell4_ptr.data(), c->sell4_ptr.size(), c->stream));
    HIP_TRY(c, c->d_sell4.upload(c->sell4.data(), c->sell4.size(), c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SPF_OK;
}

// the drain bits (metrics = false) or wt, met and nb_w
spf_status upload_attributes(spf_ctx* c, bool metrics) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (metrics) {
    HIP_TRY(c, stage_upload(c, c->d_wt, c->wt.data(), c->E));
    HIP_TRY(c, stage_upload(c, c->d_met, c->met.data(), c->E));
    HIP_TRY(c, stage_upload(c, c->d_nb_w, c->nb_w.data(), c->nb_w.size()));
  } else {
    HIP_TRY(c, stage_upload(c, c->d_ovl, c->ovl.data(), c->N));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  stage_done(c);
  return SPF_OK;
}

// the changed ranges only, through the pinned stage (queued, not a blocking
// pageable copy each)
spf_status upload_rows(spf_ctx* c, const GraphDirty& d) {
  HIP_TRY(c, hipSetDevice(c->device));
  for (const auto& r : d.runs) {
    const size_t b = r.first, k = r.second - r.first;
    HIP_TRY(c, stage_upload_at(c, c->d_col, c->col.data(), b, k));
    HIP_TRY(c, stage_upload_at(c, c->d_wt, c->wt.data(), b, k));
    HIP_TRY(c, stage_upload_at(c, c->d_met, c->met.data(), b, k));
    HIP_TRY(c, stage_upload_at(c, c->d_rev, c->rev.data(), b, k));
    HIP_TRY(c, stage_upload_at(c, c->d_link, c->link.data(), b, k));
    HIP_TRY(c, stage_upload_at(c, c->d_edge_nb, c->edge_nb.data(), b, k));
  }
  for (const auto& r : d.rev_runs) HIP_TRY(c, stage_upload_at(c, c->d_rev, c->rev.data(), r.first, r.second));
  if (d.counts) {  // the lists moved from the first touched node on
    const uint32_t u0 = d.nodes.front();
    const size_t b = c->nb_ptr[u0];
    HIP_TRY(c, stage_upload_at(c, c->d_nb_ptr, c->nb_ptr.data(), u0, c->N + 1 - u0));
    if (c->d_nb_id.n < c->nb_id.size()) {  // (the lists outgrew the buffers)
      HIP_TRY(c, stage_upload(c, c->d_nb_id, c->nb_id.data(), c->nb_id.size()));
      HIP_TRY(c, stage_upload(c, c->d_nb_w, c->nb_w.data(), c->nb_w.size()));
    } else {
      HIP_TRY(c, stage_upload_at(c, c->d_nb_id, c->nb_id.data(), b, c->nb_id.size() - b));
      HIP_TRY(c, stage_upload_at(c, c->d_nb_w, c->nb_w.data(), b, c->nb_w.size() - b));
    }
  } else {
    for (uint32_t u : d.nodes) {
      const size_t b = c->nb_ptr[u], k = c->nb_ptr[u + 1] - b;
      HIP_TRY(c, stage_upload_at(c, c->d_nb_id, c->nb_id.data(), b, k));
      HIP_TRY(c, stage_upload_at(c, c->d_nb_w, c->nb_w.data(), b, k));
    }
  }
  for (uint32_t sl : d.slices) {
    const size_t b = c->sell_ptr[sl], k = c->sell_ptr[sl + 1] - b;
    HIP_TRY(c, stage_upload_at(c, c->d_sell_col, c->sell_col.data(), b, k));
    if (!c->sell4.empty()) {
      const size_t b4 = 2ull * c->sell4_ptr[sl], k4 = 2ull * (c->sell4_ptr[sl + 1] - c->sell4_ptr[sl]);
      HIP_TRY(c, stage_upload_at(c, c->d_sell4, c->sell4.data(), b4, k4));
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  stage_done(c);
  return SPF_OK;
}

}  // namespace

namespace spfi {

// The quotient tables of the loaded graph, rebuilt and uploaded when stale.
spf_status quotient_prepare(spf_ctx* c) {
  if (!graph_host_quotient(c)) return SPF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());  // no launch still reads the old tables
  HIP_TRY(c, c->d_qcls.upload(c->qt.cls.data(), c->qt.cls.size(), c->stream));
  HIP_TRY(c, c->d_qtab.upload(c->qt.tab.data(), c->qt.tab.size(), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SPF_OK;
}

}  // namespace spfi

extern "C" {

spf_status spf_graph_load(spf_ctx* c, const spf_graph* g) {
  if (!c || !g) return fail(c, SPF_E_INVALID, "spf_graph_load: NULL argument");
  GraphDirty d;
  std::string err;
  const spf_status st = graph_host_load(c, g, &d, &err);
  if (st != SPF_OK) return fail(c, st, "%s", err.c_str());
  return uploaded(c, upload_graph(c));
}

// In-place graph patches (openr_spf.h): an overload
// bit or a metric leaves the CSR structure intact, so only the affected
// bytes are rewritten instead of a full spf_graph_load.
spf_status spf_graph_set_overload(spf_ctx* c, const uint32_t* nodes, const uint8_t* overloaded,
                                  uint32_t n) {
  if (!c || (n && (!nodes || !overloaded)))
    return fail(c, SPF_E_INVALID, "spf_graph_set_overload: NULL argument");
  GraphDirty d;
  std::string err;
  const spf_status st = graph_host_set_overload(c, nodes, overloaded, n, &d, &err);
  if (st != SPF_OK) return fail(c, st, "%s", err.c_str());
  return d.changed ? uploaded(c, upload_attributes(c, false)) : SPF_OK;
}

spf_status spf_graph_set_metric(spf_ctx* c, const uint32_t* edges, const int32_t* metric,
                                uint32_t n) {
  if (!c || (n && (!edges || !metric)))
    return fail(c, SPF_E_INVALID, "spf_graph_set_metric: NULL argument");
  GraphDirty d;
  std::string err;
  const spf_status st = graph_host_set_metric(c, edges, metric, n, &d, &err);
  if (st != SPF_OK) return fail(c, st, "%s", err.c_str());
  return d.changed ? uploaded(c, upload_attributes(c, true)) : SPF_OK;
}

// Rows rewritten in place (a link going down or up, or an adjacency withdrawn
// and advertised again, without a reload): the derived tables of the touched
// rows are patched (graph_host_patch_rows) and only the changed ranges
// uploaded.  Plans re-derive at their next execute, as after a metric patch.
// A refused patch changes nothing, on the host or on the device.
spf_status spf_graph_patch_rows(spf_ctx* c, const uint32_t* nodes, uint32_t n, const uint32_t* col,
                                const int32_t* metric, const uint32_t* link) {
  if (!c || (n && (!nodes || !col || !metric || !link)))
    return fail(c, SPF_E_INVALID, "spf_graph_patch_rows: NULL argument");
  GraphDirty d;
  std::string err;
  const spf_status st = graph_host_patch_rows(c, nodes, n, col, metric, link, &d, &err);
  if (st != SPF_OK) return fail(c, st, "%s", err.c_str());
  return d.nodes.empty() ? SPF_OK : uploaded(c, upload_rows(c, d));
}

spf_status spf_twin_classes(uint32_t n_nodes, const uint32_t* nb_ptr, const uint32_t* nb_id,
                            uint32_t* cls, uint32_t* n_classes) {
  if (!nb_ptr || !cls || !n_classes || (n_nodes && nb_ptr[n_nodes] && !nb_id))
    return fail(nullptr, SPF_E_INVALID, "spf_twin_classes: NULL argument");
  for (uint32_t v = 0; v < n_nodes; ++v)
    if (nb_ptr[v] > nb_ptr[v + 1]) return fail(nullptr, SPF_E_INVALID, "nb_ptr not monotone at %u", v);
  *n_classes = twin_classes(n_nodes, nb_ptr, nb_id, cls);
  return SPF_OK;
}

spf_status spf_graph_quotient(spf_ctx* c, uint32_t* n_classes, uint64_t* n_edges, uint32_t* in_use) {
  if (!c) return fail(c, SPF_E_INVALID, "spf_graph_quotient: NULL context");
  if (!c->loaded) return fail(c, SPF_E_STATE, "no graph loaded");
  const spf_status st = quotient_prepare(c);
  if (st != SPF_OK) return st;
  if (n_classes) *n_classes = c->qt.n_cls;
  if (n_edges) *n_edges = c->qt.n_edge;
  if (in_use) *in_use = (c->N <= kMsMaxNodes && !use_planes(c) && use_quotient(c)) ? 1u : 0u;
  return SPF_OK;
}

uint64_t spf_graph_epoch(const spf_ctx* c) { return c ? c->epoch : 0; }
uint64_t spf_graph_loads(const spf_ctx* c) { return c ? c->shape : 0; }

}  // extern "C"
