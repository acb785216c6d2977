// ============================================================================
//  engine_ctx.cpp -- the context itself: the error buffer, spf_ctx_create /
//  _destroy and the small accessors, spf_device_check (the fault word of
//  grid_ops.h decoded), the ignore-set upload, the process-wide order of
//  resident launches, spf_debug_stamps.  No kernel lives here.
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "grid_ops.h"

namespace spfi {

thread_local std::string g_err;

spf_status fail(spf_ctx* c, spf_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  g_err = buf;
  return st;
}

// Process-wide order of the launches whose workgroups wait on each other
// (engine_internal.h resident_order): per device, the stream of the last
// such launch and an event recorded after it.  A launch on another stream
// waits for that event first.
namespace {
struct ResidentSlot {
  hipEvent_t ev = nullptr;
  hipStream_t last = nullptr;
  const spf_ctx* owner = nullptr;  // context whose launch recorded ev
};
std::mutex g_resident_mu;
std::map<int, ResidentSlot> g_resident;
}  // namespace

// (a stream being captured into a hipGraph is skipped: a capture may not
// wait on an event recorded outside it, and the graph's replays are ordered
// by the stream they are launched on)
static bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

spf_status resident_order(spf_ctx* c, hipStream_t s) {
  if (capturing(s)) return SPF_OK;
  std::lock_guard<std::mutex> lk(g_resident_mu);
  ResidentSlot& r = g_resident[c->device];
  if (r.ev && r.last != s) HIP_TRY(c, hipStreamWaitEvent(s, r.ev, 0));
  return SPF_OK;
}

spf_status resident_done(spf_ctx* c, hipStream_t s) {
  if (capturing(s)) return SPF_OK;
  std::lock_guard<std::mutex> lk(g_resident_mu);
  ResidentSlot& r = g_resident[c->device];
  if (!r.ev)
    HIP_TRY(c, hipEventCreateWithFlags(&r.ev, hipEventDisableTiming | hipEventDisableSystemFence));
  HIP_TRY(c, hipEventRecord(r.ev, s));
  r.last = s;
  r.owner = c;
  return SPF_OK;
}

// a context going away: its streams may be reused by the runtime, so the
// next launch on any stream waits for the recorded event instead of
// trusting a stale stream handle
void resident_forget(const spf_ctx* c) {
  std::lock_guard<std::mutex> lk(g_resident_mu);
  for (auto& kv : g_resident)
    if (kv.second.owner == c) kv.second.last = nullptr, kv.second.owner = nullptr;
}

// Upload an ignore set (undirected link ids) as a device bitmap; NULL if empty.
spf_status upload_ignore(spf_ctx* c, const uint32_t* ignore, uint32_t n_ignore,
                         const uint32_t** dev) {
  *dev = nullptr;
  if (!ignore || n_ignore == 0) return SPF_OK;
  std::vector<uint32_t> bm(c->max_link / 32 + 1, 0);
  for (uint32_t i = 0; i < n_ignore; ++i)
    if (ignore[i] <= c->max_link) bm[ignore[i] >> 5] |= 1u << (ignore[i] & 31);
  HIP_TRY(c, c->d_ign.upload(bm.data(), bm.size(), c->stream));
  *dev = c->d_ign.p;
  return SPF_OK;
}

}  // namespace spfi

using namespace spfi;

extern "C" {

const char* spf_global_error(void) { return g_err.c_str(); }
const char* spf_last_error(const spf_ctx* c) { return c ? c->err.c_str() : g_err.c_str(); }
uint64_t spf_solves(const spf_ctx* c) { return c ? c->solves : 0; }
uint32_t spf_row_pitch(const spf_ctx* c) { return c ? c->pitch : 0; }
int spf_graph_has_nonpositive_metric(const spf_ctx* c) { return c && c->nonpos; }
int spf_graph_needs_dist64(const spf_ctx* c) { return c && c->needs64; }

spf_status spf_ctx_create(int device, spf_ctx** out) {
  if (!out) return fail(nullptr, SPF_E_INVALID, "spf_ctx_create: out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(nullptr, SPF_E_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n)
    return fail(nullptr, SPF_E_NO_DEVICE, "device %d out of range (%d visible)", device, n);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess)
    return fail(nullptr, SPF_E_NO_DEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, SPF_E_NO_DEVICE, "device %d is %s, engine is built for gfx950",
                device, prop.gcnArchName);
  auto c = std::make_unique<spf_ctx>();
  c->device = device;
  c->n_cu = (uint32_t)std::max(1, prop.multiProcessorCount);
  if (hipSetDevice(device) != hipSuccess)
    return fail(nullptr, SPF_E_HIP, "hipSetDevice(%d) failed", device);
  // a BLOCKING stream: work enqueued with stream = NULL ("the context's
  // stream") is ordered after earlier work on the legacy null stream, so a
  // caller's hipMemset / hipMemcpy on the null stream before an execute is
  // seen by it (round 3 lost a plan's first bitmaps to exactly that race
  // with a non-blocking stream)
  if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess)
    return fail(nullptr, SPF_E_HIP, "hipStreamCreate failed");
  if (c->d_fault.alloc(1) != hipSuccess || hipMemset(c->d_fault.p, 0, 4) != hipSuccess)
    return fail(nullptr, SPF_E_HIP, "fault word allocation failed");
  *out = c.release();
  return SPF_OK;
}

void spf_ctx_destroy(spf_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  spfi::resident_forget(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  spf_plan_destroy(c->rt.plan);  // spf_routes' cached plan, before its context goes
  c->rt.plan = nullptr;
  while (!c->ksp2_snaps.empty()) spf_ksp2_route_snapshot_destroy(c->ksp2_snaps.back());  // (each takes itself off the list)
  if (c->stream) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  if (c->side) {
    (void)hipStreamSynchronize(c->side);
    (void)hipStreamDestroy(c->side);
  }
  if (c->side_fork) (void)hipEventDestroy(c->side_fork);
  if (c->side_join) (void)hipEventDestroy(c->side_join);
  delete c;
}

spf_status spf_device_check(spf_ctx* c) {
  if (!c) return fail(c, SPF_E_INVALID, "spf_device_check: NULL context");
  HIP_TRY(c, hipSetDevice(c->device));
  // every launch of this context may be on a caller's stream: wait for the
  // device, then read and clear THIS context's fault word only (another
  // context's timeout stays for its own check)
  HIP_TRY(c, hipDeviceSynchronize());
  if (!c->d_fault.p) return SPF_OK;
  uint32_t flag = 0;
  HIP_TRY(c, hipMemcpy(&flag, c->d_fault.p, sizeof flag, hipMemcpyDeviceToHost));
  if (!flag) return SPF_OK;
  HIP_TRY(c, hipMemset(c->d_fault.p, 0, sizeof flag));
  if (flag & kFaultListRoom) {
    // a team's fill pass met more entries than its count pass allocated
    // (spf_whatif_changes): the entry was dropped
    return fail(c, SPF_E_HIP,
                "what-if change lists on device %d: an entry past its failure's allocated count "
                "(fault word 0x%08x); the results of this context's launches since the last check are "
                "invalid", c->device, flag);
  }
  if (flag & (kFaultLoopBound | kFaultRange | kFaultProfRow)) {
    // what-if repair diagnostics: a loop bound with its phase, a range check of
    // the profiled instances with its site, or a team past its profile region
    // with its kernel
    return fail(c, SPF_E_HIP,
                "what-if repair on device %d: %s%s%s (fault word 0x%08x: loop phase %u, check site %u, "
                "profile kernel %u); the results of this context's launches since the last check are "
                "invalid",
                c->device, (flag & kFaultLoopBound) ? "a repair loop reached its iteration bound " : "",
                (flag & kFaultRange) ? "a scratch index failed its range check " : "",
                (flag & kFaultProfRow) ? "a team's profile row is outside the profile buffer" : "", flag,
                (flag >> kFaultPhaseShift) & 0xFFu, (flag >> kFaultSiteShift) & 0xFFu,
                flag >> kFaultKernelShift);
  }
  if (flag & kFaultTeamBarrier) {
    // a team BFS gave up waiting for its members (another process's grid
    // held CUs): this context's plans stop using teams -- each re-derives
    // onto msbfs_kernel at its next execute -- instead of polling again
    c->team_off = true;
    return fail(c, SPF_E_HIP,
                "a team BFS barrier timed out on device %d (workgroups not co-resident): the "
                "results of this context's launches since the last check are invalid; its plans "
                "run msbfs_kernel from their next execute", c->device);
  }
  return fail(c, SPF_E_HIP,
              "a grid barrier timed out on device %d (blocks not co-resident?): the "
              "results of this context's launches since the last check are invalid", c->device);
}

spf_status spf_src_neighbors(const spf_ctx* c, uint32_t src, uint32_t* out,
                             uint32_t cap, uint32_t* count) {
  if (!c || !c->loaded) return SPF_E_STATE;
  if (src >= c->N) return SPF_E_INVALID;
  const uint32_t b = c->nb_ptr[src], k = c->nb_ptr[src + 1] - b;
  if (count) *count = k;
  for (uint32_t i = 0; i < k && i < cap && out; ++i) out[i] = c->nb_id[b + i];
  return SPF_OK;
}

spf_status spf_debug_stamps(spf_ctx* c, uint64_t* out, uint32_t cap, uint32_t* n) {
  if (!c || !n) return SPF_E_INVALID;
  *n = 0;
  if (!c->d_stamps.p) return SPF_OK;
  std::vector<uint64_t> buf(kStampWords);
  HIP_TRY(c, hipMemcpy(buf.data(), c->d_stamps.p, buf.size() * 8, hipMemcpyDeviceToHost));
  *n = (uint32_t)std::min<size_t>(cap, buf.size());
  std::copy(buf.begin(), buf.begin() + *n, out);
  return SPF_OK;
}

}  // extern "C"
