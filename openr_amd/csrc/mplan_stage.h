// ============================================================================
//  mplan_stage.h -- what the route stages of a multi-device plan share
//  (mplan_routes.cpp, mplan_prefix_routes.cpp): the request mapping (ReqMap),
//  the stage events with the drain of every stream a call queued work on
//  (StageEvents), and the selection tables every stage launches with
//  (route_prepare_rows).  Not part of the C-ABI.
// ============================================================================
#pragma once
#include <algorithm>
#include <initializer_list>

#include "mplan_internal.h"

namespace spfi {

#define M_TRY(expr)                   \
  do {                                \
    const spf_status st_ = (expr);    \
    if (st_ != SPF_OK) return st_;    \
  } while (0)

inline spf_status me_check(const spf_mplan* mp, const uint32_t* me_req, uint32_t n_me) {
  for (uint32_t t = 0; t < n_me; ++t)
    if (me_req[t] >= mp->n_src) return mfail(mp->m, SPF_E_INVALID, "me %u is not a request index", me_req[t]);
  return SPF_OK;
}

// A call's me list (request indices, checked) mapped onto the members.
struct ReqMap {
  std::vector<std::vector<uint32_t>> mine, req;  // per member, slot order: its me's node ids, their indices t
  spf_mplan::Loc loc;                              // request t -> (member, slot)
  std::vector<uint32_t> nodes;                     // node id of request t
  ReqMap(const spf_mplan* mp, const uint32_t* me_req, uint32_t n_me)
      : mine(mp->n_parts), req(mp->n_parts), loc(n_me), nodes(n_me) {
    for (uint32_t t = 0; t < n_me; ++t) {
      const uint32_t r = mp->owner[me_req[t]];
      loc[t] = {r, (uint32_t)mine[r].size()};
      nodes[t] = mp->srcs[me_req[t]];
      mine[r].push_back(nodes[t]);
      req[r].push_back(t);
    }
  }
};

// The events of one call of a stage: `marks` per member with work, created
// only when the call was asked for its kernel time, destroyed on every exit.
// It is the call's IssuedGuard too: open(r) lists member r's stream, and every
// listed stream is drained before the events go -- and, this object being
// declared after the host buffers those streams copy into or upload from,
// before those buffers are freed, on early returns too.
class StageEvents {
 public:
  StageEvents(spf_mctx* m, uint32_t n_parts, uint32_t marks, bool timed)
      : worst(0), m_(m), marks_(marks), ev_(timed ? (size_t)marks * n_parts : 0, nullptr), issued_{m, {}} {}
  ~StageEvents() {
    issued_.drain();
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  // member r has work: its device current, its stream drained on exit
  spf_status open(uint32_t r) {
    M_HIP(m_, hipSetDevice(m_->members[r]->device));
    issued_.members.push_back(r);
    for (uint32_t k = 0; k < marks_ && !ev_.empty(); ++k) M_HIP(m_, hipEventCreate(&ev_[marks_ * r + k]));
    return SPF_OK;
  }
  // mark k on member r's stream (its device current)
  spf_status mark(uint32_t r, uint32_t k) {
    if (!ev_.empty()) M_HIP(m_, hipEventRecord(ev_[marks_ * r + k], m_->exec[r]));
    return SPF_OK;
  }
  // Member r's ms from mark k to mark k + 1, for each k of `from` (r's stream
  // synchronised): stage[i] keeps the slowest member of from[i], `worst` the
  // slowest member in their sum.
  spf_status slowest(uint32_t r, std::initializer_list<uint32_t> from, double* stage = nullptr) {
    if (ev_.empty()) return SPF_OK;
    double sum = 0;
    uint32_t i = 0;
    for (const uint32_t k : from) {
      float t = 0;
      M_HIP(m_, hipEventElapsedTime(&t, ev_[marks_ * r + k], ev_[marks_ * r + k + 1]));
      if (stage) stage[i] = std::max(stage[i], (double)t);
      ++i;
      sum += t;
    }
    worst = std::max(worst, sum);
    return SPF_OK;
  }
  double worst;

 private:
  spf_mctx* m_;
  uint32_t marks_;
  std::vector<hipEvent_t> ev_;
  IssuedGuard issued_;
};

// route_prepare (mplan_routes.cpp) for a call that brings no destination sets:
// every member's tables of the resident rows' and bitmaps' device addresses,
// refreshed when an execute moved them; the plan-flag and LFA residency checks.
spf_status route_prepare_rows(spf_mplan* mp, bool lfa, const uint32_t* me_req, uint32_t n_me);

}  // namespace spfi
