// ============================================================================
//  spf_engine.hip -- MI355X (gfx950) all-sources SPF + ECMP engine: the plans.
//
//  Implements the plan calls of include/openr_spf.h.  What the reference
//  computes per source in LinkState::runSpf (openr/decision/LinkState.cpp:
//  808-882) is produced by two data-parallel passes over a CSR graph resident
//  in HBM, each a kernel family in a unit of its own (spf_units.h):
//
//   1. distance rows D[row][0..N): sssp.hip (one workgroup per source row,
//      frontier Bellman-Ford in LDS), msbfs.hip (unit metrics: 64 or 32 sources
//      per workgroup), class_rows.hip (one BFS row per twin class, node rows
//      expanded from those); mssp.hip, msbfs_team.hip, exact.hip and
//      whatif.hip's spf_big_kernel hold the other distance kernels.
//
//   2. next hops: ecmp.hip, a streaming compare of D rows (one bit per
//      distinct up neighbour; proof sketch in DESIGN.md §3).
//
//   3. pathLinks of one source: preds.hip.
//
//  Here: build_plan (which kernels a plan runs, from the graph, the request
//  and the environment's knobs; its host tables come from plan_host.h), plan
//  create / destroy / execute, the traffic model and the timing calls, the
//  result digests and row gathers, spf_solve and spf_solve_exact.  The context
//  itself is engine_ctx.cpp.
//
//  Everything is integer.  Distances are u32; spf_graph_load rejects graphs
//  whose longest possible path does not fit (see openr_spf.h).
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "spf_units.h"

using namespace spfi;

namespace {

// ---------------------------------------------------------------------------
//  copy selected D rows into the caller's dense output (non-direct plans)
// ---------------------------------------------------------------------------
// u8 rows (npitch bytes, a multiple of 16): row rows[i] -> out row i
__global__ void gather_rows_u8_kernel(const uint8_t* __restrict__ Dn, uint32_t npitch,
                                      const uint32_t* __restrict__ rows, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.y;
  const uint4* in = reinterpret_cast<const uint4*>(Dn + (size_t)rows[i] * npitch);
  uint4* o = reinterpret_cast<uint4*>(out + (size_t)i * npitch);
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < npitch / 16;
       t += gridDim.x * blockDim.x)
    o[t] = in[t];
}

// practical HBM ceiling (spf_debug_copy_bandwidth): a grid-stride 16-byte
// copy, the float4-copy shape of MI355X_MICROARCH.md's measured 6.29 TB/s
__global__ __launch_bounds__(256) void copy_bw_kernel(const uint4* __restrict__ src,
                                                      uint4* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    dst[i] = src[i];
}

__global__ void gather_rows_kernel(const uint32_t* __restrict__ D, uint32_t pitch,
                                   const uint32_t* __restrict__ rows,
                                   uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.y;
  const uint4* in = reinterpret_cast<const uint4*>(D + (size_t)rows[i] * pitch);
  uint4* o = reinterpret_cast<uint4*>(out + (size_t)i * pitch);
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < pitch / 4;
       t += gridDim.x * blockDim.x)
    o[t] = in[t];
}

// ---------------------------------------------------------------------------
//  per-source result digests (spf_plan_digest): the checksum a rank ships
//  instead of its rows when results stay resident on its GPU
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t dg_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// Block (chunk of 256 destinations, source i); thread = destination v.  The
// next-hop words of v are assembled 32 neighbours at a time from the planar
// bitmaps (lanes of a wave read the same two words: broadcast loads) and fed
// to FNV-1a in word order; the per-node terms are summed with a wave
// reduction and one 64-bit atomic per wave.
template <bool D64>
__global__ __launch_bounds__(256) void digest_kernel(const void* __restrict__ dist, uint32_t pitch,
                                                     uint32_t N, const uint32_t* __restrict__ nh,
                                                     const uint64_t* __restrict__ nh_off,
                                                     const uint32_t* __restrict__ words,
                                                     unsigned long long* __restrict__ out) {
  const uint32_t i = blockIdx.y;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  uint64_t term = 0;
  if (v < N) {
    const uint64_t d = D64 ? reinterpret_cast<const uint64_t*>(dist)[(size_t)i * pitch + v]
                           : reinterpret_cast<const uint32_t*>(dist)[(size_t)i * pitch + v];
    if (d != (D64 ? ~0ull : (uint64_t)kInf)) {
      const uint32_t k = words[i], wpm = pitch / 32;
      const uint32_t* b = nh + nh_off[i] + v / 32;
      const uint32_t sh = v % 32;
      uint64_t f = 0xcbf29ce484222325ull;
      for (uint32_t j0 = 0; j0 < k; j0 += 32) {
        uint32_t w = 0;
        const uint32_t jn = min(32u, k - j0);
        for (uint32_t j = 0; j < jn; ++j) w |= ((b[(size_t)(j0 + j) * wpm] >> sh) & 1u) << j;
        f ^= w;
        f *= 0x100000001b3ull;
      }
      term = dg_mix64(dg_mix64((uint64_t)v + 1) + d) ^ f;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)term, o, 64), hi = __shfl_xor((uint32_t)(term >> 32), o, 64);
    term += ((uint64_t)hi << 32) | lo;
  }
  if ((threadIdx.x & 63) == 0 && term) atomicAdd(&out[i], (unsigned long long)term);
}

}  // namespace

namespace spfi {

bool plan_has_narrow(const spf_plan* p) {
  return !p->exact && !p->big && p->narrow && !p->sdirect && (p->d_Dn.p || p->cls);
}

// The one entry point (build_plan, spf_sssp): every unit raises the limit of
// its own kernels, once per process.
spf_status set_lds_limits(spf_ctx* c) {
  static bool done = false;
  if (done) return SPF_OK;
  for (auto unit : {sssp_set_lds_limits, msbfs_set_lds_limits, class_rows_set_lds_limits, mssp_set_lds_limits}) {
    const spf_status st = unit(c);
    if (st != SPF_OK) return st;
  }
  done = true;
  return SPF_OK;
}

}  // namespace spfi

namespace {

// The environment's knobs of a plan build (experiments, A/B runs, tests), read
// anew by every build: tests change them between plan creations.
struct PlanKnobs {
  int narrow = -1;  // SPF_NARROW: -1 unset; 0: u32 rows; 1: byte rows, never sliced; 2 (anything else): narrow
  int big = -1;     // SPF_BIG: 0: the exact kernel instead of spf_big_kernel; 1: every plan it can take
  bool pl_order = true;  // SPF_PL_ORDER=0: the register-plane BFS keeps the plan order
  bool wsliced = true;   // SPF_WSLICED=0: weighted plans keep byte rows
  bool expand = false;   // SPF_EXPAND=1: the slicing pass expands the u32 rows
  bool sdirect = true;   // SPF_SDIRECT=0: team plans never slice their rows themselves
  bool class_rows = true;  // SPF_CLASS_ROWS=0: quotient plans keep msbfs_kernel's node rows
  int64_t ecmp_runs = -1;    // SPF_ECMP_RUNS: source runs per XCD (-1: by the plan's size)
  int64_t sliced_unit = -1;  // SPF_SLICED_UNIT: matches per work unit (-1: plan_sliced_unit)
  int sliced_group = 2;      // SPF_SLICED_GROUP: plan_sliced_units' group mode
};

PlanKnobs plan_knobs() {
  auto first = [](const char* name) {  // the value's first character, -1 when unset
    const char* e = std::getenv(name);
    return e ? (int)(unsigned char)e[0] : -1;
  };
  auto number = [](const char* name) {
    const char* e = std::getenv(name);
    return e ? (int64_t)(uint32_t)atoi(e) : -1;
  };
  PlanKnobs k;
  const int nw = first("SPF_NARROW"), big = first("SPF_BIG");
  k.narrow = nw < 0 ? -1 : nw == '0' ? 0 : nw == '1' ? 1 : 2;
  k.big = big == '0' ? 0 : big == '1' ? 1 : -1;
  k.pl_order = first("SPF_PL_ORDER") != '0';
  k.wsliced = first("SPF_WSLICED") != '0';
  k.expand = first("SPF_EXPAND") == '1';
  k.sdirect = first("SPF_SDIRECT") != '0';
  k.class_rows = first("SPF_CLASS_ROWS") != '0';
  k.ecmp_runs = number("SPF_ECMP_RUNS");
  k.sliced_unit = number("SPF_SLICED_UNIT");
  if (const char* e = std::getenv("SPF_SLICED_GROUP")) k.sliced_group = atoi(e);
  return k;
}

// SPF_PLAN_DEBUG: per-phase host time of a plan build on stderr (diagnostics)
bool plan_debug() {
  static const bool on = std::getenv("SPF_PLAN_DEBUG") != nullptr;
  return on;
}

// u8 narrow rows for the next-hop pass: 4x fewer bytes per neighbour row
// read, paid for by a second store per (source, slice, level) in
// msbfs_kernel.  Worth it when next-hop work (sum of neighbour counts)
// outweighs the BFS store work, which grows with the number of levels:
// dense fabrics (degree ~23, 5 levels) yes; always with the register-plane
// BFS (one coalesced store per row).  SPF_NARROW=0/1 overrides (experiments).
bool use_narrow(const spf_ctx* c, const spf_plan* p, const PlanKnobs& kn) {
  if (kn.narrow >= 0) return kn.narrow != 0;
  // the register-plane BFS writes each row once, coalesced: the u8 copy
  // costs one more row store and the next-hop pass reads 4x fewer bytes
  if (use_planes(c)) return true;
  uint64_t nb = 0;
  for (uint32_t i = 0; i < p->n_src; ++i) nb += p->words[i];
  return nb >= 8ull * p->n_src;  // average distinct degree >= 8
}

// Everything a plan derives from the graph's current state (closure over
// non-drained neighbours, narrow/exact mode, next-hop row tables).  Run at
// creation and again by spf_plan_execute after an in-place graph patch
// (spf_graph_set_overload / spf_graph_set_metric); the output layout
// (nh_off, words) depends only on the CSR structure, which patches keep.
// The modes are decided here; the tables come from plan_host.h and go up
// through the pinned stage on c->stream, so each stays alive until the
// synchronize that ends its copy.
spf_status build_plan(spf_ctx* c, spf_plan* p) {
  auto pd_t0 = std::chrono::steady_clock::now();
  auto PD = [&](const char* what) {
    if (!plan_debug()) return;
    (void)hipStreamSynchronize(c->stream);
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "build_plan %s %.1f us\n", what, std::chrono::duration<double, std::micro>(t - pd_t0).count());
    pd_t0 = t;
  };
  const PlanKnobs kn = plan_knobs();
  const uint32_t n_src = p->n_src;
  const uint32_t* srcs = p->srcs.data();
  const bool hop = (p->flags & SPF_FLAG_HOP_COUNT) != 0;
  const bool d64 = (p->flags & SPF_FLAG_DIST64) != 0;
  if (!hop && c->needs64 && !d64)
    return fail(c, SPF_E_UNSUPPORTED,
                "weighted distances of this graph may exceed 32 bits (negative metric or max "
                "metric x hops >= 2^32): create the plan with SPF_FLAG_DIST64");
  const uint32_t N = c->N;
  // the exact kernel replays runSpf step for step: zero-metric plateaus
  // (pop order), u64 labels, and graphs whose distance rows do not fit the
  // LDS-resident kernels
  const bool ms_ok = (hop || c->unit) && N <= kMsMaxNodes;
  const bool lds_ok = sssp_lds_bytes(N, c->pitch, c->big_nodes, N <= 65535) <= kMaxLds;
  p->exact = d64 || (!hop && c->nonpos);
  // graphs beyond the LDS-resident kernels: the whole chip per source
  // (spf_big_kernel); SPF_BIG=0 sends them to the exact kernel, SPF_BIG=1
  // sends every plan it can take there (tests)
  p->big = !p->exact && ((!ms_ok && !lds_ok) ? kn.big != 0 : kn.big == 1);
  if (!ms_ok && !lds_ok && !p->big) p->exact = true;
  {
    NhLayout l = plan_nh_layout(*c, srcs, n_src);
    p->words = std::move(l.words);
    p->nh_off = std::move(l.nh_off);
    p->nh_total = l.nh_total;
    p->wmax = l.wmax;
  }
  if (p->exact || p->big) {  // the request is its own closure; no next-hop pass of ours
    p->closure = p->srcs;
    p->direct = true;
    p->ms = false;
    p->narrow = false;
    p->sliced = false;
    p->expand = false;
    HIP_TRY(c, hipSetDevice(c->device));
    if (p->exact) {
      const spf_status st = exact_reserve(c, &p->xs, n_src, p->wmax);
      if (st != SPF_OK) return st;
    }
    HIP_TRY(c, stage_upload(c, p->d_srcs, p->srcs.data(), n_src));
    HIP_TRY(c, stage_upload(c, p->d_nh_off, p->nh_off.data(), n_src));
    HIP_TRY(c, stage_upload(c, p->d_words, p->words.data(), n_src));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    stage_done(c);
    p->epoch = c->epoch;
    return SPF_OK;
  }
  PD("start");
  PlanRows rows = plan_rows(*c, srcs, n_src);
  p->closure = std::move(rows.closure);
  p->direct = rows.direct;
  const size_t n_rows = p->closure.size();
  // closure[i] == srcs[i] for i < n_src, and no row can saturate the u8
  // copy (whose saturated entries the next-hop pass reads from u32 rows)
  p->prefix = rows.distinct && depth_bound(*c, &c->depth) < kSlSat;
  p->q16 = N <= 65535;
  p->lds_bytes = sssp_lds_bytes(N, c->pitch, c->big_nodes, p->q16);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, stage_upload(c, p->d_srcs, p->srcs.data(), n_src));
  HIP_TRY(c, stage_upload(c, p->d_closure, p->closure.data(), n_rows));
  HIP_TRY(c, stage_upload(c, p->d_row_of, rows.row_of.data(), N));
  HIP_TRY(c, stage_upload(c, p->d_req_rows, rows.req_rows.data(), n_src));
  HIP_TRY(c, stage_upload(c, p->d_nh_off, p->nh_off.data(), n_src));
  HIP_TRY(c, stage_upload(c, p->d_words, p->words.data(), n_src));
  p->ms = ms_ok;
  // register-plane BFS: batches of similar depth, deepest first (more than
  // one round of batches only; SPF_PL_ORDER=0 keeps the plan order, A/B)
  p->pl_order = p->ms && use_planes(c) && n_rows > (size_t)kPlBatch * c->n_cu && kn.pl_order;
  if (p->pl_order) {
    const std::vector<uint32_t> order = plan_depth_order(p->closure, ecc_estimate(*c, &c->depth));
    HIP_TRY(c, stage_upload(c, p->d_pl_order, order.data(), order.size()));
  }
  // few batches (a rank's share of a multi-GPU pass): teams of workgroups
  // per batch (msbfs_team.hip) instead of one workgroup sweeping everything
  // (p->expand: as the plan's previous build left it)
  PD("uploads1");
  p->tm_G = 0;
  if (p->ms && !use_planes(c) && !p->expand && !c->team_off) {
    const uint32_t G = msbfs_team_size(c, (uint32_t)n_rows);
    if (G) {
      const spf_status st = msbfs_team_prepare(c, p, G);
      if (st != SPF_OK) return st;
    }
  }
  // class rows: one BFS row per twin class among the closure rows, the node
  // rows expanded from those (SPF_CLASS_ROWS=0: msbfs_kernel's rows, A/B)
  p->cls = false;
  p->cls_ready = false;
  ClassRows cr;
  if (p->ms && !p->tm_G && !use_planes(c) && kn.class_rows && quotient_allowed(c)) {
    const spf_status st = quotient_prepare(c);
    if (st != SPF_OK) return st;
    p->cls = class_rows_fit(c);
  }
  if (p->cls) {
    cr = plan_class_rows(*c, p->closure);
    p->cls_k = (uint32_t)cr.csrc.size();
    p->cls_pitch = (c->qt.n_cls + 63u) & ~63u;
    HIP_TRY(c, stage_upload(c, p->d_csrc, cr.csrc.data(), cr.csrc.size()));
    HIP_TRY(c, stage_upload(c, p->d_crow_of, cr.crow_of.data(), cr.crow_of.size()));
    HIP_TRY(c, stage_upload(c, p->d_cfwd, cr.fwd.data(), cr.fwd.size()));
  }
  // weighted: S sources per workgroup on mssp_kernel where it applies
  PD("team");
  p->mp = !p->ms && !hop && mssp_words(c) > 0;
  if (p->mp) {
    const spf_status st = mssp_prepare(c);
    if (st != SPF_OK) return st;
    HIP_TRY(c, p->d_redo.alloc(1 + n_rows));
  }
  // The rows the next-hop pass reads.  Weighted plans keep a u8 copy too when
  // the pitches agree (the sssp kernel writes it beside the u32 row; the
  // next-hop pass compares bytes and falls back to u32 rows per wave where
  // the source's row saturates).
  p->narrow = (p->ms || c->pitch == c->npitch) && use_narrow(c, p, kn);
  // bit-sliced rows behind the per-level-store BFS (it reports the deepest
  // level); the register-plane BFS serves deep graphs, where planes would
  // not pay.  SPF_NARROW=1 keeps the byte-row pass (experiments, tests).
  // Weighted plans on mssp_kernel: its u8 rows sliced too, next hops by
  // bit-sliced sums d_x + w (sliced_pass<P, true>); SPF_WSLICED=0: byte rows
  p->sliced = p->narrow && kn.narrow != 1 && ((p->ms && !use_planes(c)) || (p->mp && kn.wsliced));
  // SPF_EXPAND=1 (A/B; measured slower): the BFS stores the u8
  // rows only and the slicing pass expands them into the u32 rows.  By
  // default the BFS stores both: its u32 stores drain behind its
  // latency-bound sweeps (+0.06 ms on fabric_full) where a separate
  // streaming pass costs 0.14 ms and a fused one 0.14 ms of the next-hop
  // kernel's time (r02_v25/r02_v26)
  p->expand = p->sliced && c->pitch <= c->npitch && kn.expand && !p->cls;
  // class plans write u8 rows only for whoever reads them: the byte-row
  // next-hop pass (SPF_NARROW=1), or a caller that asked (plan_ensure_narrow)
  if (p->cls && p->narrow && !p->sliced) p->keep_narrow = true;
  // team plans whose depth stays below the planes' all-ones code write the
  // sliced rows themselves: no u8 rows, no slicing pass (SPF_SDIRECT=0: A/B)
  p->sdirect = p->sliced && p->nh_total && p->tm_G && p->prefix && !p->expand &&
               depth_bound(*c, &c->depth) < (1u << kTeamPlanes) - 1 && kn.sdirect;
  const uint32_t wpm = c->pitch / 32;
  const uint64_t rstride = (uint64_t)kSlSlots * wpm;  // sliced row: words
  // per-source neighbour rows for the next-hop pass
  const NbRows nb = plan_nb_rows(*c, srcs, n_src, rows.row_of,
                                 p->sliced ? rstride : p->narrow ? c->npitch : 0, n_rows);
  p->dead = nb.dead;
  HIP_TRY(c, stage_upload(c, p->d_nb_row, nb.nb_row.data(), nb.nb_row.size()));
  HIP_TRY(c, stage_upload(c, p->d_nb_row_off, nb.nb_row_off.data(), n_src));
  HIP_TRY(c, stage_upload(c, p->d_nb_drained, nb.nb_drained.data(), n_src));
  // next-hop blocks per XCD (a rank's share of a multi-GPU pass -- ~1.3k
  // sources -- does best with two long runs per XCD: 0.097 -> 0.095 ms per
  // world-8 rank, r03_v25)
  const XcdLists xcd = plan_xcd_lists(
      p->words, kn.ecmp_runs >= 0 ? (uint32_t)kn.ecmp_runs : n_src >= 4096 ? kEcmpRunsPerXcd : 2u);
  PD("nb_rows");
  SlicedUnits su;
  if (p->sliced) {
    const uint32_t chunks = (wpm + 63) / 64;
    const uint32_t unit =
        kn.sliced_unit >= 0 ? (uint32_t)kn.sliced_unit : plan_sliced_unit(p->words, chunks, c->n_cu);
    // (weighted plans: no groups -- members share neighbour rows, not metrics)
    su = plan_sliced_units(xcd.list, p->words, nb, chunks, unit, p->mp ? 0 : kn.sliced_group);
    p->max_xcd_units = su.max_xcd_units;
    HIP_TRY(c, stage_upload(c, p->d_units, su.units.data(), su.units.size()));
    HIP_TRY(c, stage_upload(c, p->d_unit_off, su.unit_off.data(), 9));
    HIP_TRY(c, stage_upload(c, p->d_gtab, su.gtab.data(), su.gtab.size()));
  }
  p->slots = xcd.slots;
  HIP_TRY(c, stage_upload(c, p->d_slot_src, xcd.slot.data(), xcd.slot.size()));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host tables' copies end here
  stage_done(c);
  PD("units+slots");
  if (!p->direct) HIP_TRY(c, p->d_D.alloc(n_rows * c->pitch));
  if (p->cls) HIP_TRY(c, p->d_Dc.alloc((size_t)p->cls_k * p->cls_pitch));
  if (p->narrow && !p->sdirect && (!p->cls || p->keep_narrow)) {  // narrow rows + the dead row (all 0xFF) of the next-hop pass
    HIP_TRY(c, p->d_Dn.alloc((n_rows + 1) * c->npitch));
    HIP_TRY(c, hipMemsetAsync(p->d_Dn.p + n_rows * c->npitch, 0xFF, c->npitch, c->stream));
  }
  if (p->sliced) {  // sliced rows + the dead row (all planes all-ones) + padding
    // a wave's last chunk reads up to 64 * kSlSlots words past a row's end
    const size_t pad = 64 * kSlSlots + 64;
    if (((n_rows + 1) * rstride + pad) * 4 >= (1ull << 31))  // buffer byte offsets
      return fail(c, SPF_E_UNSUPPORTED, "sliced rows exceed 32-bit offsets");
    HIP_TRY(c, p->d_S.alloc((n_rows + 1) * rstride + pad));
    HIP_TRY(c, hipMemsetAsync(p->d_S.p + n_rows * rstride, 0xFF, (rstride + pad) * 4, c->stream));
  }
  if (p->sliced || p->cls) HIP_TRY(c, p->d_maxd.alloc(1));
  {
    const spf_status st = set_lds_limits(c);  // kernels need > 64 KiB of dynamic LDS
    if (st != SPF_OK) return st;
  }
  PD("allocs");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  stage_done(c);
  p->epoch = c->epoch;
  return SPF_OK;
}

}  // namespace

extern "C" {

spf_status spf_plan_create(spf_ctx* c, const uint32_t* srcs, uint32_t n_src,
                           uint32_t flags, spf_plan** out) {
  if (!c || !out) return fail(c, SPF_E_INVALID, "spf_plan_create: NULL argument");
  *out = nullptr;
  if (!c->loaded) return fail(c, SPF_E_STATE, "no graph loaded");
  if (n_src == 0 || !srcs) return fail(c, SPF_E_INVALID, "empty source list");
  for (uint32_t i = 0; i < n_src; ++i)
    if (srcs[i] >= c->N) return fail(c, SPF_E_INVALID, "source %u out of range", srcs[i]);
  auto p = std::make_unique<spf_plan>();
  p->ctx = c;
  p->n_src = n_src;
  p->flags = flags;
  p->srcs.assign(srcs, srcs + n_src);
  p->shape = c->shape;
  p->layout = c->layout;
  const spf_status st = build_plan(c, p.get());
  if (st != SPF_OK) return st;
  *out = p.release();
  return SPF_OK;
}


void spf_plan_destroy(spf_plan* p) { delete p; }
uint64_t spf_plan_nh_words(const spf_plan* p) { return p ? p->nh_total : 0; }
uint32_t spf_plan_closure_rows(const spf_plan* p) { return p ? (uint32_t)p->closure.size() : 0; }

spf_status spf_plan_class_rows(const spf_plan* p, uint32_t* n_class_sources, uint32_t* in_use) {
  if (!p) return SPF_E_INVALID;
  if (n_class_sources) *n_class_sources = p->cls ? p->cls_k : 0u;
  if (in_use) *in_use = p->cls ? 1u : 0u;
  return SPF_OK;
}

spf_status spf_plan_kernels(const spf_plan* p, uint32_t* bfs, uint32_t* narrow) {
  if (!p || !bfs || !narrow) return SPF_E_INVALID;
  *bfs = p->big ? 4u : p->exact ? 3u : p->mp ? 5u : !p->ms ? 0u : p->tm_G ? 6u
                                                          : use_planes(p->ctx) ? 2u : 1u;
  *narrow = p->sdirect ? 3u : p->sliced ? 2u : p->narrow ? 1u : 0u;
  return SPF_OK;
}

// Bytes each kernel of one execute must move between HBM and the CUs, given
// the kernel's own structure: what `roofline.achieved` in bench.py divides by
// the kernel's measured time (no credit for on-chip reuse).
//   BFS (msbfs / planes): one read of the sliced-ELL columns and the drain
//     bytes per workgroup (a batch of sources shares one sweep per level;
//     repeated levels hit the L2), plus the distance rows (u32, pitch) and,
//     in narrow mode, the u8 rows (npitch) written once.
//   SSSP (weighted, one workgroup per source): one read of row_ptr, col,
//     metric and drain bytes per source, plus the distance row written.
//   ECMP: every distance row it compares read once (u8 rows in narrow mode,
//     u32 rows otherwise) plus the next-hop bitmaps written once.
spf_status spf_plan_traffic(const spf_plan* p, uint64_t* bfs_bytes, uint64_t* ecmp_bytes) {
  if (!p || !bfs_bytes || !ecmp_bytes) return SPF_E_INVALID;
  uint64_t b[3];
  const spf_status st = spf_plan_traffic_phases(p, b);
  if (st != SPF_OK) return st;
  *bfs_bytes = b[0];
  *ecmp_bytes = b[1] + b[2];
  return SPF_OK;
}

//   Slicing (sliced plans): the u8 rows read, P planes per row written (and,
//     in expand plans, the u32 rows); the sliced next-hop pass then reads P
//     planes per row and writes the bitmaps.
spf_status spf_plan_traffic_phases(const spf_plan* p, uint64_t* bytes) {
  if (!p || !bytes) return SPF_E_INVALID;
  uint64_t* bfs_bytes = &bytes[0];
  uint64_t* ecmp_bytes = &bytes[2];
  bytes[1] = 0;
  const spf_ctx* c = p->ctx;
  const uint64_t N = c->N, E = c->E, rows = p->closure.size();
  uint64_t bfs = 0;
  if (p->big) {  // per source: the CSR a few sweeps (counted once), the row, scratch + bitmaps
    *bfs_bytes = rows * (4ull * (N + 1) + 12ull * E + N + 4ull * c->pitch) + 4ull * p->nh_total;
    *ecmp_bytes = 0;
    return SPF_OK;
  }
  if (p->exact) {  // per source: the CSR once, the labels, the outputs
    const uint64_t lab = (p->flags & SPF_FLAG_DIST64) ? 8ull : 4ull;
    *bfs_bytes = rows * (4ull * (N + 1) + 12ull * E + N + 17ull * N + lab * c->pitch) +
                 4ull * p->nh_total;
    *ecmp_bytes = 0;
    return SPF_OK;
  }
  if (p->tm_G) {  // team BFS: each batch sweeps the column stream once (column + meta
                  // words); rows written: u32 for the prefix when direct, u8 or planes
    const uint64_t batches = (rows + p->tm_bs - 1) / p->tm_bs;
    const bool direct = p->prefix && !p->direct && p->narrow;
    const uint64_t wbytes = 4ull * (c->pitch / 32);
    bfs = batches * (8ull * c->sell_ptr.back() + N) + (direct ? p->n_src : rows) * c->pitch * 4ull +
          (p->sdirect ? rows * kTeamPlanes * wbytes : p->narrow ? rows * c->npitch : 0ull);
  } else if (p->cls) {  // class BFS: the quotient tables and the forwards bytes per workgroup, Dc written
    const uint64_t bs = ms_batch(c, p->cls_k, false);
    const uint64_t groups = (p->cls_k + bs - 1) / bs;
    bfs = groups * (2ull * (c->qt.cls.size() + c->qt.tab.size()) + c->qt.n_cls) +
          2ull * p->cls_k * p->cls_pitch;
  } else if (p->ms) {
    const bool planes = use_planes(c);
    // (the model takes neither SPF_MSBFS_BATCH nor a deepest-first order into account)
    const uint64_t bs = planes ? planes_batch(c, (uint32_t)rows, false) : ms_batch(c, (uint32_t)rows, false);
    const uint64_t groups = (rows + bs - 1) / bs;
    const uint64_t n_slices = c->sell_ptr.size() - 1;
    // (quotient sweep: the class and row/column tables instead of the columns)
    const uint64_t csr = planes ? 8ull * c->sell4_ptr.back() + 4ull * (n_slices + 1)
                         : use_quotient(c) ? 2ull * (c->qt.cls.size() + c->qt.tab.size())
                                           : 4ull * c->sell_ptr.back() + 4ull * (n_slices + 1);
    // expand plans: the u32 rows are written by the slicing pass instead
    bfs = groups * (csr + N) + (p->expand ? 0ull : rows * c->pitch * 4ull) +
          (p->narrow ? rows * c->npitch : 0ull);
  } else if (p->mp) {  // per workgroup: the packed ELL + slice map once; rows written once
    const uint64_t S = mssp_sources(c);
    const uint64_t groups = (rows + S - 1) / S;
    bfs = groups * (4ull * c->sell_ptr.back() + 4ull * c->sell_ptr.size() + 4ull * (N + 1) + N) +
          rows * (4ull * c->pitch + (p->narrow ? c->npitch : 0ull));
  } else {
    bfs = rows * (4ull * (N + 1) + 8ull * E + N + 4ull * c->pitch + (p->narrow ? c->npitch : 0ull));
  }
  *bfs_bytes = bfs;
  // expansion: every closure row's class row read once per width split, the
  // class ids once per row group; the u32 rows (and kept u8 rows) written
  uint64_t cls_expand = 0;
  if (p->cls) {
    const ExpandGrid eg = plan_expand_grid((uint32_t)rows, std::max(c->pitch, p->keep_narrow ? c->npitch : 0u),
                                           expand_resident(c));
    cls_expand = eg.splits * rows * 2ull * p->cls_pitch + (uint64_t)eg.groups * 2ull * N +
                 rows * 4ull * c->pitch + (p->keep_narrow ? rows * c->npitch : 0ull);
  }
  bytes[1] = cls_expand;
  if (p->sliced && p->nh_total) {
    // planes in use: from the last execute's deepest level (one 4-byte read)
    // (sdirect: kTeamPlanes planes written by the BFS itself, no slicing pass)
    const uint64_t wbytes = 4ull * (c->pitch / 32);
    if (p->sdirect) {
      *ecmp_bytes = rows * kTeamPlanes * wbytes + 4ull * p->nh_total;
      return SPF_OK;
    }
    uint32_t md = 0;
    HIP_TRY(p->ctx, hipMemcpy(&md, p->d_maxd.p, 4, hipMemcpyDeviceToHost));
    const uint64_t expand = p->expand ? rows * 4ull * c->pitch : 0ull;  // u32 rows written
    if (md < kSlSat) {
      const uint64_t P = 32u - __builtin_clz(md + 1u);
      bytes[1] = p->cls ? cls_expand + rows * P * wbytes : rows * c->npitch + rows * P * wbytes + expand;
      *ecmp_bytes = rows * P * wbytes + 4ull * p->nh_total;
    } else {
      bytes[1] = p->cls ? cls_expand : expand ? rows * c->npitch + expand : 0ull;
      *ecmp_bytes = rows * 4ull * c->pitch + 4ull * p->nh_total;
    }
    return SPF_OK;
  }
  const uint64_t row_bytes = p->narrow ? c->npitch : 4ull * c->pitch;
  *ecmp_bytes = p->nh_total ? rows * row_bytes + 4ull * p->nh_total : 0ull;
  return SPF_OK;
}

spf_status spf_plan_nh_layout(const spf_plan* p, uint64_t* nh_off, uint32_t* words) {
  if (!p) return SPF_E_INVALID;
  for (uint32_t i = 0; i < p->n_src; ++i) {
    if (nh_off) nh_off[i] = p->nh_off[i];
    if (words) words[i] = p->words[i];
  }
  return SPF_OK;
}

spf_status spf_plan_execute(spf_plan* p, uint32_t* d_dist, uint32_t* d_nh, void* stream) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_plan_execute: NULL plan");
  spf_ctx* c = p->ctx;
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (!d_dist || (p->nh_total && !d_nh))
    return fail(c, SPF_E_INVALID, "spf_plan_execute: NULL output buffer");
  if (p->shape != c->shape)
    return fail(c, SPF_E_STATE, "graph reloaded since the plan was created: recreate it");
  if (p->layout != c->layout) {
    // a row patch changed some node's distinct neighbours: the plan's
    // next-hop layout holds only if none of its sources was one of them
    for (uint32_t i = 0; i < p->n_src; ++i)
      if (c->nb_ptr[p->srcs[i] + 1] - c->nb_ptr[p->srcs[i]] != p->words[i])
        return fail(c, SPF_E_STATE, "source %u's distinct neighbours changed since the plan was "
                                    "created (its next-hop layout): recreate it", p->srcs[i]);
    p->layout = c->layout;
  }
  if (p->epoch != c->epoch || (p->tm_G && c->team_off) || (p->cls && !use_quotient(c))) {
    // patched in place, or teams turned off by a timeout: re-derive, same
    // output layout
    const spf_status st = build_plan(c, p);
    if (st != SPF_OK) return st;
  }
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const uint32_t pitch = c->pitch;
  const bool hop = (p->flags & SPF_FLAG_HOP_COUNT) != 0;
  if (p->exact || p->big) {
    hipEvent_t* ev = nullptr;
    if (p->timing_cap) {
      ev = &p->ev[4 * (p->timing_n % p->timing_cap)];
      ++p->timing_n;
      HIP_TRY(c, hipEventRecord(ev[0], s));
    }
    const spf_status st =
        p->big ? launch_big(c, p, d_dist, d_nh, hop, s)
               : launch_exact(c, &p->xs, p->d_srcs.p, p->n_src, p->d_nh_off.p, p->wmax, hop,
                              (p->flags & SPF_FLAG_DIST64) != 0, nullptr, d_dist, d_nh, nullptr, s);
    if (st != SPF_OK) return st;
    if (ev)
      for (int e = 1; e < 4; ++e) HIP_TRY(c, hipEventRecord(ev[e], s));
    c->solves += p->n_src;
    return SPF_OK;
  }
  // team plans whose closure starts with the request's rows write those
  // rows' u32 distances straight into d_dist (and no others): no scratch
  // rows, no gather
  // (u8 or sliced rows only: the u32-row next-hop pass reads the neighbours'
  // u32 rows, which then exist nowhere)
  const bool team_direct = p->tm_G && p->prefix && !p->direct && p->narrow;
  uint32_t* D = (p->direct || team_direct) ? d_dist : p->d_D.p;
  const uint32_t rows = (uint32_t)p->closure.size();
  const bool sliced = p->sliced && p->nh_total;
  if ((sliced && !p->sdirect) || p->cls)  // the BFS's atomicMax target (sdirect plans: planes fixed)
    HIP_TRY(c, hipMemsetAsync(p->d_maxd.p, 0, 4, s));
  hipEvent_t* ev = nullptr;
  if (p->timing_cap) {
    ev = &p->ev[4 * (p->timing_n % p->timing_cap)];
    ++p->timing_n;
    HIP_TRY(c, hipEventRecord(ev[0], s));
  }
  spf_status st =
      p->cls ? launch_class_bfs(c, p, s)
      : p->tm_G ? launch_msbfs_team(c, p, p->d_closure.p, rows, D,
                                  p->narrow && !p->sdirect ? p->d_Dn.p : nullptr,
                                  sliced && !p->sdirect ? p->d_maxd.p : nullptr, s,
                                  team_direct ? p->n_src : rows,
                                  p->sdirect ? p->d_S.p : nullptr,
                                  kSlSlots * (pitch / 32))
      : p->ms ? launch_msbfs(c, p->d_closure.p, rows, D, p->narrow ? p->d_Dn.p : nullptr,
                                       sliced ? p->d_maxd.p : nullptr, s,
                                       sliced && p->expand ? kSlSat : 0u,
                                       p->pl_order ? p->d_pl_order.p : nullptr)
                  : p->mp ? launch_mssp(c, p->d_closure.p, rows, D, p->narrow ? p->d_Dn.p : nullptr,
                                        p->d_redo.p, s, sliced ? p->d_maxd.p : nullptr)
                        : launch_sssp(c, p->d_closure.p, rows, hop, nullptr, D, s, nullptr,
                                      nullptr, p->narrow ? p->d_Dn.p : nullptr);
  if (st != SPF_OK) return st;
  if (ev) HIP_TRY(c, hipEventRecord(ev[1], s));
  if (p->cls) {  // (the phase timed as slicing)
    st = launch_expand(c, p, D, p->keep_narrow ? p->d_Dn.p : nullptr, sliced ? p->d_S.p : nullptr, s);
    if (st != SPF_OK) return st;
    p->cls_ready = true;
  } else if (sliced && !p->sdirect) {
    st = launch_sliced(c, p, D, s);
    if (st != SPF_OK) return st;
  }
  if (ev) HIP_TRY(c, hipEventRecord(ev[2], s));
  if (p->nh_total) {
    st = sliced ? launch_ecmp_sliced(c, p, D, hop, d_nh, s) : launch_ecmp(c, p, p->narrow, D, hop, d_nh, s);
    if (st != SPF_OK) return st;
  }
  if (ev) HIP_TRY(c, hipEventRecord(ev[3], s));
  if (!p->direct && !team_direct) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(std::min<uint32_t>((pitch / 4 + 255) / 256, 64), p->n_src),
                       dim3(256), 0, s, D, pitch, p->d_req_rows.p, d_dist);
    HIP_TRY(c, hipGetLastError());
  }
  c->solves += p->n_src;
  return SPF_OK;
}

spf_status spf_plan_copy_narrow_rows(spf_plan* p, uint8_t* d_out, void* stream) {
  if (!p || !d_out) return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_plan_copy_narrow_rows: NULL");
  spf_ctx* c = p->ctx;
  if (!plan_has_narrow(p))
    return fail(c, SPF_E_UNSUPPORTED, "spf_plan_copy_narrow_rows: the plan keeps no u8 rows");
  if (c->npitch != c->pitch)
    return fail(c, SPF_E_UNSUPPORTED, "spf_plan_copy_narrow_rows: u8 and u32 row pitches differ");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const spf_status st = plan_ensure_narrow(p, s);
  if (st != SPF_OK) return st;
  hipLaunchKernelGGL(gather_rows_u8_kernel, dim3(std::min<uint32_t>((c->npitch / 16 + 255) / 256, 64), p->n_src),
                     dim3(256), 0, s, p->d_Dn.p, c->npitch, p->d_req_rows.p, d_out);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status spf_plan_digest(spf_plan* p, const void* d_dist, const uint32_t* d_nh, uint64_t* d_out,
                           void* stream) {
  if (!p || !d_dist || !d_out || (p->nh_total && !d_nh))
    return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_plan_digest: NULL argument");
  spf_ctx* c = p->ctx;
  if (p->shape != c->shape)
    return fail(c, SPF_E_STATE, "graph reloaded since the plan was created: recreate it");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(c, hipMemsetAsync(d_out, 0, 8ull * p->n_src, s));
  if (!p->n_src) return SPF_OK;
  const dim3 grid((c->N + 255) / 256, p->n_src);
  const uint32_t* nh = p->nh_total ? d_nh : p->d_words.p;  // never read when every k = 0
  auto* o = reinterpret_cast<unsigned long long*>(d_out);
  if (p->flags & SPF_FLAG_DIST64)
    hipLaunchKernelGGL(digest_kernel<true>, grid, dim3(256), 0, s, d_dist, c->pitch, c->N, nh,
                       p->d_nh_off.p, p->d_words.p, o);
  else
    hipLaunchKernelGGL(digest_kernel<false>, grid, dim3(256), 0, s, d_dist, c->pitch, c->N, nh,
                       p->d_nh_off.p, p->d_words.p, o);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status spf_plan_enable_timing(spf_plan* p, uint32_t max_executes) {
  if (!p) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
  p->ev.assign(4ull * max_executes, nullptr);
  // timing only: no system-scope fence (its L2 writeback + invalidate cost
  // ~5 us per event and left the next kernel a cold L2)
  for (auto& e : p->ev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  p->timing_cap = max_executes;
  p->timing_n = 0;
  return SPF_OK;
}

spf_status spf_plan_timing_phases(spf_plan* p, double* ms, uint32_t* n) {
  if (!p || !p->timing_cap || !ms) return SPF_E_STATE;
  spf_ctx* c = p->ctx;
  const uint32_t cnt = std::min(p->timing_n, p->timing_cap);
  ms[0] = ms[1] = ms[2] = 0;
  for (uint32_t i = 0; i < cnt; ++i) {
    HIP_TRY(c, hipEventSynchronize(p->ev[4 * i + 3]));
    for (int ph = 0; ph < 3; ++ph) {
      float t = 0;
      HIP_TRY(c, hipEventElapsedTime(&t, p->ev[4 * i + ph], p->ev[4 * i + ph + 1]));
      ms[ph] += t;
    }
  }
  if (n) *n = cnt;
  p->timing_n = 0;
  return SPF_OK;
}

spf_status spf_plan_timing(spf_plan* p, double* sssp_ms, double* ecmp_ms, uint32_t* n) {
  double ms[3];
  const spf_status st = spf_plan_timing_phases(p, ms, n);
  if (st != SPF_OK) return st;
  if (sssp_ms) *sssp_ms = ms[0];
  if (ecmp_ms) *ecmp_ms = ms[1] + ms[2];
  return SPF_OK;
}

spf_status spf_plan_execute_host(spf_plan* p, uint32_t* dist_out, uint32_t* nh_out) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_plan_execute_host: NULL plan");
  spf_ctx* c = p->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t lab = (p->flags & SPF_FLAG_DIST64) ? 8 : 4;
  HIP_TRY(c, p->h_dist.alloc((size_t)p->n_src * c->pitch * (lab / 4)));
  HIP_TRY(c, p->h_nh.alloc(std::max<uint64_t>(p->nh_total, 1)));
  const spf_status st = spf_plan_execute(p, p->h_dist.p, p->h_nh.p, nullptr);
  if (st != SPF_OK) return st;
  p->h_epoch = c->epoch;
  if (dist_out) {
    HIP_TRY(c, hipMemcpy2DAsync(dist_out, (size_t)c->N * lab, p->h_dist.p, (size_t)c->pitch * lab,
                                (size_t)c->N * lab, p->n_src, hipMemcpyDeviceToHost, c->stream));
  }
  if (nh_out && p->nh_total) {
    HIP_TRY(c, hipMemcpyAsync(nh_out, p->h_nh.p, p->nh_total * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // grid-resident kernels (spf_big_kernel, the team BFS) report a barrier
  // that gave up (blocks not co-resident) here instead of wrong rows
  return (p->big || p->tm_G) ? spf_device_check(c) : SPF_OK;
}

spf_status spf_solve(spf_ctx* c, const uint32_t* srcs, uint32_t n_src, uint32_t flags,
                     uint32_t* dist_out, uint32_t* nh_out) {
  spf_plan* raw = nullptr;
  spf_status st = spf_plan_create(c, srcs, n_src, flags, &raw);
  if (st != SPF_OK) return st;
  std::unique_ptr<spf_plan> p(raw);
  return spf_plan_execute_host(p.get(), dist_out, nh_out);
}

spf_status spf_debug_copy_bandwidth(spf_ctx* c, uint64_t bytes, uint32_t reps, double* gbs) {
  if (!c || !gbs || bytes < 16 || reps == 0) return fail(c, SPF_E_INVALID, "spf_debug_copy_bandwidth: bad argument");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = bytes / 16;
  DevBuf<uint4> a, b;
  HIP_TRY(c, a.alloc(n));
  HIP_TRY(c, b.alloc(n));
  HIP_TRY(c, hipMemsetAsync(a.p, 1, n * 16, c->stream));
  const dim3 g(c->n_cu * 8), blk(256);
  hipLaunchKernelGGL(copy_bw_kernel, g, blk, 0, c->stream, a.p, b.p, n);  // warm
  HIP_TRY(c, hipGetLastError());
  hipEvent_t e0, e1;
  HIP_TRY(c, hipEventCreate(&e0));
  HIP_TRY(c, hipEventCreate(&e1));
  HIP_TRY(c, hipEventRecord(e0, c->stream));
  for (uint32_t r = 0; r < reps; ++r)
    hipLaunchKernelGGL(copy_bw_kernel, g, blk, 0, c->stream, (r & 1) ? b.p : a.p, (r & 1) ? a.p : b.p, n);
  HIP_TRY(c, hipEventRecord(e1, c->stream));
  HIP_TRY(c, hipEventSynchronize(e1));
  float ms = 0;
  HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *gbs = 2.0 * 16.0 * (double)n * reps / (ms * 1e-3) / 1e9;  // bytes read + written
  return SPF_OK;
}

spf_status spf_solve_exact(spf_ctx* c, uint32_t src, uint32_t flags, const uint32_t* ignore_links,
                           uint32_t n_ignore, uint64_t* dist64_out, uint32_t* dist32_out,
                           uint32_t* nh_out, uint32_t* pop_out) {
  if (!c) return fail(c, SPF_E_INVALID, "spf_solve_exact: NULL context");
  if (!c->loaded) return fail(c, SPF_E_STATE, "no graph loaded");
  if (src >= c->N) return fail(c, SPF_E_INVALID, "source %u out of range", src);
  const bool hop = (flags & SPF_FLAG_HOP_COUNT) != 0;
  if (dist32_out && !hop && c->needs64)
    return fail(c, SPF_E_UNSUPPORTED, "weighted distances may exceed 32 bits: ask for u64 rows");
  const uint32_t* ign = nullptr;
  spf_status st = upload_ignore(c, ignore_links, n_ignore, &ign);
  if (st != SPF_OK) return st;
  const uint32_t k = c->nb_ptr[src + 1] - c->nb_ptr[src];
  const uint64_t wpm = c->pitch / 32, nh_words = (uint64_t)k * wpm;
  const bool d64 = dist32_out == nullptr;
  DevBuf<uint32_t> d_dist, d_nh, d_pop;
  DevBuf<uint64_t> d_off;
  const uint64_t zero = 0;
  HIP_TRY(c, c->d_one_src.upload(&src, 1, c->stream));
  HIP_TRY(c, d_off.upload(&zero, 1, c->stream));
  HIP_TRY(c, d_dist.alloc((size_t)c->pitch * (d64 ? 2 : 1)));
  HIP_TRY(c, d_nh.alloc(std::max<uint64_t>(nh_words, 1)));
  if (pop_out) HIP_TRY(c, d_pop.alloc(c->pitch));
  const uint32_t wk = std::max<uint32_t>(1, (k + 31) / 32);
  st = exact_reserve(c, &c->exact1, 1, wk);
  if (st != SPF_OK) return st;
  st = launch_exact(c, &c->exact1, c->d_one_src.p, 1, d_off.p, wk, hop, d64, ign, d_dist.p, d_nh.p,
                    pop_out ? d_pop.p : nullptr, c->stream);
  if (st != SPF_OK) return st;
  if (d64 && dist64_out)
    HIP_TRY(c, hipMemcpyAsync(dist64_out, d_dist.p, 8ull * c->N, hipMemcpyDeviceToHost, c->stream));
  if (!d64)
    HIP_TRY(c, hipMemcpyAsync(dist32_out, d_dist.p, 4ull * c->N, hipMemcpyDeviceToHost, c->stream));
  if (nh_out && nh_words)
    HIP_TRY(c, hipMemcpyAsync(nh_out, d_nh.p, 4ull * nh_words, hipMemcpyDeviceToHost, c->stream));
  if (pop_out)
    HIP_TRY(c, hipMemcpyAsync(pop_out, d_pop.p, 4ull * c->N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->solves += 1;
  return SPF_OK;
}

}  // extern "C"
