// ============================================================================
//  whatif_repair.h -- what the what-if repair kernels are made of: the failure
//  kinds, the team primitives, the repairs and the three repair kernels, the
//  rank sort of the big failures.  whatif.hip's head describes the method.
//
//  Templates and inline functions only: including this file emits no kernel.
//  Each plan kind's unit (whatif.hip: links; whatif_nodes.hip, whatif_sets.hip,
//  whatif_metrics.hip) instantiates its own kernels into its own code object.
//  Everything sits in an unnamed namespace, so no symbol is shared between
//  those objects.
// ============================================================================
#ifndef OPENR_AMD_WHATIF_REPAIR_H
#define OPENR_AMD_WHATIF_REPAIR_H

#include "engine_internal.h"
#include "grid_ops.h"
#include "wave_ops.h"

using namespace spfi;

namespace {

constexpr uint32_t kBusy = 0xFFFFFFFEu;
constexpr uint32_t kWaveCap = 1024;            // |D| a wave team can hold
constexpr size_t kBigScratch = 8ull << 30;     // HBM budget of the workgroup teams (both sets)
constexpr size_t kWaveScratch = 8ull << 30;    // HBM budget of the wave teams
constexpr uint32_t kDialLevels = 1024;         // distinct distances settled bucket by bucket

// What a plan's failures are, a template parameter of the repairs: one link,
// or a node down / drained (SPF_WHATIF_NODE_DOWN / SPF_WHATIF_NODE_DRAIN).
constexpr int kLink = 0, kDown = 1, kDrain = 2, kSet = 3, kMetric = 4;
static_assert(kDown == SPF_WHATIF_NODE_DOWN && kDrain == SPF_WHATIF_NODE_DRAIN &&
                  kSet == SPF_WHATIF_LINK_SET && kMetric == SPF_WHATIF_LINK_METRIC, "plan kinds");

// Is the edge v -> u (link id `link`) unusable, in both directions, under
// the failure: link l itself, or (node x down) any edge with an end at x.
// `v_is_x`: the caller's row owner v is x (false where it cannot be).
template <int KIND>
__device__ __forceinline__ bool failed(uint32_t x, uint32_t l, bool v_is_x, uint32_t u,
                                       uint32_t link) {
  if constexpr (KIND == kLink) return link == l;
  else if constexpr (KIND == kDown) return v_is_x || u == x;
  else return false;
}
// Is v the node the failure drains (reached, never a transit or a predecessor).
template <int KIND>
__device__ __forceinline__ bool drain_x(uint32_t x, uint32_t v) {
  if constexpr (KIND == kDrain) return v == x;
  else return false;
}


// A set plan's canonical sets on the device (each ascending, no duplicates):
// failure f owns links[ptr[f] .. ptr[f + 1]); link_edge[l] = one directed edge
// of link l, kInf when l is down.  The set kernels' trailing argument.
struct WiSets {
  const uint32_t* ptr;
  const uint32_t* links;
  const uint32_t* link_edge;
};
// The failed set of one repair (KIND == kSet; empty, and so no argument at
// all, for the other kinds): the sorted run in global memory, its length and
// -- team-uniform, in scalar registers -- its first four members, padded with
// kInf (no link id).  Shared-risk groups are mostly two to four links (both
// links of a LAG, a bundle): those never touch memory for the membership test.
constexpr uint32_t kSetRegs = 4;
template <int KIND>
struct SetRef {};
template <>
struct SetRef<kSet> {
  const uint32_t* mem;
  const uint32_t* link_edge;
  uint32_t n, m0, m1, m2, m3;
};
__device__ __forceinline__ SetRef<kSet> set_of(const WiSets& s, uint32_t f) {
  const uint32_t b0 = __builtin_amdgcn_readfirstlane(s.ptr[f]);
  const uint32_t n = __builtin_amdgcn_readfirstlane(s.ptr[f + 1]) - b0;
  const uint32_t* mem = s.links + b0;
  SetRef<kSet> r{mem, s.link_edge, n, kInf, kInf, kInf, kInf};
  if (n > 0) r.m0 = __builtin_amdgcn_readfirstlane(mem[0]);
  if (n > 1) r.m1 = __builtin_amdgcn_readfirstlane(mem[1]);
  if (n > 2) r.m2 = __builtin_amdgcn_readfirstlane(mem[2]);
  if (n > 3) r.m3 = __builtin_amdgcn_readfirstlane(mem[3]);
  return r;
}
// Is `link` a member: up to kSetRegs members by compares against registers,
// longer sets by a binary search of the sorted run (ceil(log2 n) + 1 loads,
// all within the run's few cache lines; a linear scan of a 167-link hub set
// would be 167 per edge).
__device__ __forceinline__ bool set_has(const SetRef<kSet>& r, uint32_t link) {
  if (r.n <= kSetRegs) return link == r.m0 || link == r.m1 || link == r.m2 || link == r.m3;
  uint32_t lo = 0, hi = r.n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (r.mem[mid] < link) lo = mid + 1;
    else hi = mid;
  }
  return lo < r.n && r.mem[lo] == link;
}
// failed() of every kind: a set plan asks the set, the others as above
template <int KIND>
__device__ __forceinline__ bool failed(const SetRef<KIND>& sr, uint32_t x, uint32_t l, bool v_is_x,
                                       uint32_t u, uint32_t link) {
  if constexpr (KIND == kSet) return set_has(sr, link);
  else return failed<KIND>(x, l, v_is_x, u, link);
}

// A metric plan's changes on the device: change f is chg[f] = {e_lo, e_hi,
// w_lo, w_hi} -- the changed link's directed edge out of its endpoint with the
// smaller CSR id, the reverse edge, and what each weighs under the change (a
// kept direction: its current metric); e_lo = kInf for a down link.
// delta[f] is written by classify_metrics_kernel.  The metric kernels'
// trailing argument.
struct WiMet {
  const uint4* chg;
  const uint32_t* delta;
};
// The change of one repair (KIND == kMetric), team-uniform and in scalar
// registers: SetRef's place in the repairs' argument lists.
template <>
struct SetRef<kMetric> {
  uint32_t e_lo, e_hi, w_lo, w_hi, delta;
};
__device__ __forceinline__ SetRef<kMetric> met_of(const WiMet& m, uint32_t f) {
  const uint4 q = m.chg[f];
  const auto uni = [](uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane(x); };
  return SetRef<kMetric>{uni(q.x), uni(q.y), uni(q.z), uni(q.w), uni(m.delta[f])};
}
// What CSR edge e weighs (w_fwd; `w` as read from the graph) and what the edge
// reverse to e weighs (w_rev) under the failure: the graph's weights, except
// for the two directed edges of a metric plan's changed link.
template <int KIND>
__device__ __forceinline__ uint32_t w_fwd(const SetRef<KIND>& sr, uint32_t e, uint32_t w) {
  if constexpr (KIND == kMetric) return e == sr.e_lo ? sr.w_lo : (e == sr.e_hi ? sr.w_hi : w);
  else return w;
}
template <int KIND>
__device__ __forceinline__ uint32_t w_rev(const SetRef<KIND>& sr, uint32_t e, uint32_t w) {
  if constexpr (KIND == kMetric) return e == sr.e_lo ? sr.w_hi : (e == sr.e_hi ? sr.w_lo : w);
  else return w;
}
// Does edge e = x -> c (graph weight w; unfailed distances dx, dc) put c into
// D: a tight edge of the unfailed DAG -- for a metric plan an edge with slack
// <= delta (in 64 bits: dc + delta may pass 2^32), whose head is reachable and
// not src (src never changes, and D's nodes are seeded from outside D).
template <int KIND>
__device__ __forceinline__ bool grows(const SetRef<KIND>& sr, uint32_t src, uint32_t e, uint32_t dx,
                                      uint32_t w, uint32_t c, uint32_t dc) {
  if constexpr (KIND == kMetric)
    return dc != kInf && c != src && (uint64_t)dx + w_fwd<KIND>(sr, e, w) <= (uint64_t)dc + sr.delta;
  else
    return dx + w == dc;
}

struct WiBase {
  const uint32_t* dist;  // [N] unfailed distances
  const uint32_t* nhb;   // [N][W] unfailed next-hop bitsets
  const unsigned long long* H;  // unfailed hash
};

// ---------------------------------------------------------------------------
//  repair of one hot failure by a team (a wave, or a whole workgroup)
// ---------------------------------------------------------------------------
struct TeamCtl {
  uint32_t n, ovf, flag[3], dmin, dmax, nxt[3], lc[3], hub;
  unsigned long long ndist, nnh, dh;
  uint32_t bar;   // group teams: arrivals at the team barrier (monotonic)
  uint32_t next;  // group teams: the failure the team takes next
};

// A team is a wave (64), a workgroup (1024) or a group of TEAM / 1024
// workgroups of one grid-resident launch on one XCD (team_sync = the agent-scope
// release -> arrival counter -> poll -> acquire hand-off of
// MI355X_MICROARCH.md §Workgroup dispatch; the counter only grows, so the
// barrier of the k-th call completes at k * G arrivals)
template <int TEAM, bool GROUP = false>
__device__ __forceinline__ void team_sync(TeamCtl* ctl, uint32_t* fault) {
  if constexpr (GROUP) {
    const uint32_t G = TEAM / blockDim.x;  // workgroups per team
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's stores drained
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const uint32_t ticket =
          __hip_atomic_fetch_add(&ctl->bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t target = (ticket / G + 1) * G;
      uint32_t k = 0;
      for (; k < kBarSpin &&
             __hip_atomic_load(&ctl->bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target;
           ++k) {
        if ((k & 1023u) == 1023u && fault_set(fault)) break;
        __builtin_amdgcn_s_sleep(1);
      }
      if (k == kBarSpin) barrier_timed_out(fault);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
  } else if constexpr (TEAM == 64) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// Returns false (nothing written, scratch clean) when |D| exceeds cap.
// a wave's or workgroup's scratch (mark, dlist, dnew, level lists) is private
// to one workgroup: workgroup-scope accesses may be served by the CU's L1; a
// group team's is shared by several CUs: agent scope (L1 bypassed)
template <bool GROUP>
__device__ __forceinline__ uint32_t ldw(const uint32_t* p) {
  if constexpr (GROUP) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GROUP>
__device__ __forceinline__ void stw(uint32_t* p, uint32_t v) {
  if constexpr (GROUP) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GROUP>
__device__ __forceinline__ unsigned long long ldq(const unsigned long long* p) {
  if constexpr (GROUP) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GROUP>
__device__ __forceinline__ void stq(unsigned long long* p, unsigned long long v) {
  if constexpr (GROUP) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- change lists (spf_whatif_changes): the EMIT instances ----
// The kernels' optional trailing argument (a pack: the production instances
// keep their argument list).
__device__ __forceinline__ const WiEmit* emit_arg() { return nullptr; }
__device__ __forceinline__ const WiEmit* emit_arg(const WiEmit& e) { return &e; }
// (set plans: the pack ends with the WiSets)
__device__ __forceinline__ const WiEmit* emit_arg(const WiSets&) { return nullptr; }
__device__ __forceinline__ const WiEmit* emit_arg(const WiEmit& e, const WiSets&) { return &e; }
__device__ __forceinline__ const WiSets& sets_arg(const WiSets& s) { return s; }
__device__ __forceinline__ const WiSets& sets_arg(const WiEmit&, const WiSets& s) { return s; }
// (metric plans: the pack ends with the WiMet)
__device__ __forceinline__ const WiEmit* emit_arg(const WiMet&) { return nullptr; }
__device__ __forceinline__ const WiEmit* emit_arg(const WiEmit& e, const WiMet&) { return &e; }
__device__ __forceinline__ const WiMet& met_arg(const WiMet& m) { return m; }
__device__ __forceinline__ const WiMet& met_arg(const WiEmit&, const WiMet& m) { return m; }
// failure f's set (set plans) or change (metric plans), nothing for the other kinds
template <int KIND, class... EM>
__device__ __forceinline__ SetRef<KIND> set_arg(uint32_t f, const EM&... em) {
  if constexpr (KIND == kSet) return set_of(sets_arg(em...), f);
  else if constexpr (KIND == kMetric) return met_of(met_arg(em...), f);
  else return SetRef<KIND>{};
}
// do the kernels of this kind end their argument pack with a per-plan table
constexpr bool kind_has_table(int kind) { return kind == kSet || kind == kMetric; }

// The head of link edge e0's tight direction in the unfailed DAG, kInf when
// neither is tight (or e0 = kInf, a down link): classify_kernel's test --
// tail reachable, tail not drained unless it is src, dist[a] + w == dist[b].
// Metrics are positive, so at most one direction is tight.
__device__ __forceinline__ uint32_t tight_head(const WiGraph& g, const uint32_t* dist, uint32_t e0) {
  uint32_t head = kInf;
  if (e0 != kInf) {
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t e = k ? g.rev[e0] : e0;
      const uint32_t a = g.col[g.rev[e]], b = g.col[e];  // a -> b
      if (g.ovl[a] && a != g.src) continue;
      if (dist[a] != kInf && dist[a] + g.wt[e] == dist[b]) head = b;
    }
  }
  return head;
}

// Is D node i (graph node v, new distance d1) an entry of its failure's list:
// its metric or its next-hop row differs from the unfailed result.  (A node
// of D is reachable in the unfailed run, so becoming unreachable is a metric
// change.)
template <bool GROUP>
__device__ __forceinline__ bool entry_changed(const WiBase& B, const uint32_t* nhn, uint32_t W,
                                              uint32_t v, uint32_t i, uint32_t d1) {
  bool changed = d1 != B.dist[v];
  for (uint32_t w = 0; w < W && !changed; ++w)
    changed = B.nhb[(size_t)v * W + w] != ldw<GROUP>(&nhn[(size_t)i * W + w]);
  return changed;
}

// Fill pass, one wave's chunk of D: the lanes in `m` (= __ballot(changed))
// hold an entry each, which goes to at + q0 + (its rank in m) of the pools --
// node, metric (~0 when unreachable) and the W words of its new row (zeros
// when unreachable, not the stale row).  Rows of up to 4 words are copied by
// the entry's own lane, wider ones by the wave, lane = word.  Nothing reads
// the pools again on the device: streaming stores.  An entry past the
// failure's allocated count (`room`) is dropped and sets kFaultListRoom in the fault
// word.  Every lane of the wave must be active.
template <bool GROUP>
__device__ __forceinline__ void emit_entries(const WiEmit& em, uint64_t at, uint32_t room,
                                             uint32_t q0, uint64_t m, bool changed, uint32_t v,
                                             uint32_t i, uint32_t d1, const uint32_t* nhn,
                                             uint32_t lane) {
  const uint32_t W = em.W;
  const uint32_t q = q0 + lanes_below(m);
  const bool put = changed && q < room;
  if (changed && !put && em.fault)
    __hip_atomic_fetch_or(em.fault, kFaultListRoom, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (put) {
    __builtin_nontemporal_store(v, &em.cnode[at + q]);
    __builtin_nontemporal_store(d1 == kInf ? ~0ull : (unsigned long long)d1, &em.cdist[at + q]);
  }
  if (W <= 4) {
    if (put)
      for (uint32_t w = 0; w < W; ++w)
        __builtin_nontemporal_store(d1 == kInf ? 0u : ldw<GROUP>(&nhn[(size_t)i * W + w]),
                                    &em.cnh[(at + q) * W + w]);
  } else {
    for (uint64_t r = m; r; r &= r - 1) {  // wave-uniform
      const uint32_t bl = __ffsll((unsigned long long)r) - 1;
      const uint32_t qb = __builtin_amdgcn_readlane(q, bl);
      if (qb >= room) continue;
      const uint32_t ib = __builtin_amdgcn_readlane(i, bl), db = __builtin_amdgcn_readlane(d1, bl);
      for (uint32_t j = lane; j < W; j += 64)
        __builtin_nontemporal_store(db == kInf ? 0u : ldw<GROUP>(&nhn[(size_t)ib * W + j]),
                                    &em.cnh[(at + qb) * W + j]);
    }
  }
}

// FNV-1a of both next-hop rows of a D node and whether they differ: the
// words in batches of 8, loads of a batch in flight together.  A node's hash
// is mix64(mix64(v + 1) + d) ^ FNV-1a(row), as in the base pass's result hash.
template <bool GROUP>
__device__ __forceinline__ void row_pair_hash(const uint32_t* h0, const uint32_t* h1, uint32_t W,
                                              uint64_t& f0, uint64_t& f1, bool& diff) {
  f0 = f1 = 0xcbf29ce484222325ull;
  for (uint32_t w = 0; w < W; w += 8) {
    uint32_t a[8], c[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      a[q] = w + q < W ? h0[w + q] : 0u;
      c[q] = w + q < W ? ldw<GROUP>(&h1[w + q]) : 0u;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (w + q < W) {
        f0 = (f0 ^ a[q]) * 0x100000001b3ull;
        f1 = (f1 ^ c[q]) * 0x100000001b3ull;
        diff |= a[q] != c[q];
      }
    }
  }
}

// The next-hop row ORs of one flattened edge chunk's tight pairs (lanes in
// pm: a tight predecessor u / its D index mu; lanes in sm: the source itself,
// jk = the node's source-neighbour bit), in lane order.  A pair belongs to D
// node ik.  W <= 64: lane j keeps word j of the current node's row in `acc`
// (`cur` = that node's D index, kInf for none), the loads of 8 pairs in
// flight together, and the row is stored once, when the node changes (a
// node's pairs are contiguous in flattened order, its row is zero before its
// level, and one wave builds it): the caller flushes the last one.  W > 64:
// a read-modify-write of the row per pair.
__device__ __forceinline__ void row_pairs(uint64_t pm, uint64_t sm, uint32_t ik, uint32_t jk,
                                          uint32_t u, uint32_t mu, uint32_t W, uint32_t* nhn,
                                          const uint32_t* nhb, uint32_t lane, uint32_t& cur,
                                          uint32_t& acc) {
  pm |= sm;
  if (W <= 64) {
    while (pm) {  // wave-uniform
      uint32_t pi[8], pj[8], x[8];
      bool pv[8], ps[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        pv[q] = pm != 0;
        ps[q] = false;
        pi[q] = pj[q] = x[q] = 0;
        if (pv[q]) {
          const uint32_t bl = __ffsll((unsigned long long)pm) - 1;
          pm &= pm - 1;
          pi[q] = __builtin_amdgcn_readlane(ik, bl);
          ps[q] = (sm >> bl) & 1;
          if (ps[q]) {
            pj[q] = __builtin_amdgcn_readlane(jk, bl);
          } else {
            const uint32_t pu = __builtin_amdgcn_readlane(u, bl), pmu = __builtin_amdgcn_readlane(mu, bl);
            const uint32_t* from = pmu != kInf ? nhn + (size_t)pmu * W : nhb + (size_t)pu * W;
            if (lane < W) x[q] = from[lane];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (!pv[q]) continue;
        if (pi[q] != cur) {
          if (cur != kInf && lane < W) nhn[(size_t)cur * W + lane] = acc;
          cur = pi[q];
          acc = 0;
        }
        acc |= ps[q] ? (lane == (pj[q] >> 5) ? 1u << (pj[q] & 31) : 0u) : x[q];
      }
    }
  } else {
    for (; pm; pm &= pm - 1) {
      const uint32_t bl = __ffsll((unsigned long long)pm) - 1;
      uint32_t* row = nhn + (size_t)__builtin_amdgcn_readlane(ik, bl) * W;
      if ((sm >> bl) & 1) {
        const uint32_t pj = __builtin_amdgcn_readlane(jk, bl);
        if (lane == ((pj >> 5) & 63) && (pj >> 5) < W) row[pj >> 5] |= 1u << (pj & 31);
      } else {
        const uint32_t pu = __builtin_amdgcn_readlane(u, bl), pmu = __builtin_amdgcn_readlane(mu, bl);
        const uint32_t* from = pmu != kInf ? nhn + (size_t)pmu * W : nhb + (size_t)pu * W;
        for (uint32_t j = lane; j < W; j += 64) row[j] |= from[j];
      }
    }
  }
}

// Nodes per wave chunk of a team's node loops: the count spread over the
// team's waves, 1..64 (team-uniform).
template <int TEAM>
__device__ __forceinline__ uint32_t team_chunk(uint32_t count) {
  constexpr uint32_t kW = TEAM / 64;
  return min(64u, max(1u, (count + kW - 1) / kW));
}

// Phase counters of a profiled repair (SPF_WHATIF_PROF).  Registers (GPH
// false): ph is the caller's array, stored once when the team exits.  Global
// (GPH true, SPF_WHATIF_PROF=global): ph is the team's 16-slot row of the
// prof buffer, updated by the team's first thread with device atomics at
// every event -- the round-5 variant that faulted; its row was
// range-checked by the kernel before it got here.
template <bool GPH>
__device__ __forceinline__ void ph_add(uint64_t* ph, int k, uint64_t v, bool leader) {
  if constexpr (GPH) {
    if (leader) atomicAdd(reinterpret_cast<unsigned long long*>(ph + k), (unsigned long long)v);
  } else {
    ph[k] += v;
  }
}
template <bool GPH>
__device__ __forceinline__ void ph_max(uint64_t* ph, int k, uint64_t v, bool leader) {
  if constexpr (GPH) {
    if (leader) atomicMax(reinterpret_cast<unsigned long long*>(ph + k), (unsigned long long)v);
  } else {
    ph[k] = ph[k] > v ? ph[k] : v;
  }
}

// CHK (the profiled instances, SPF_WHATIF_PROF): every scratch-derived
// index is range-checked before use; an out-of-range one sets bit 4 of the
// fault word with the site in bits 16-23 and is replaced by a safe value
// (results then invalid, reported by spf_device_check).
// EMIT (spf_whatif_changes): the repair also counts (em->cnode NULL) or
// writes (fill pass) failure f's change list, before the digest loop.
// KIND: `y` is the failed link's tight edge (kLink) or the failed node; a set
// plan's failure is `sr` (y is its size estimate, not used here).  kMetric: y
// is the changed link's hot edge u -> v (D's root is its head v), `sr` the
// change; nothing is failed, the edge weights come through w_fwd / w_rev.
template <int TEAM, bool GROUP = false, bool CHK = false, bool GPH = false, bool EMIT = false,
          int KIND = kLink>
__device__ bool repair(const WiGraph& g, const WiBase& B, uint32_t* mark, uint32_t* dlist,
                       uint32_t* dnew, uint32_t* nhn, uint32_t* lvl, uint32_t* ord, uint32_t cap,
                       TeamCtl* ctl, uint32_t tt, uint32_t y, spf_whatif_digest* out,
                       uint64_t* ph = nullptr, const WiEmit* em = nullptr, uint32_t f = 0,
                       SetRef<KIND> sr = SetRef<KIND>{}) {
  // diagnostics (SPF_WHATIF_PROF): 12 counters, accumulated over the team's
  // failures (ph_add) -- [0] repairs, [1..5] 100 MHz ticks in D discovery,
  // seeds, Dial, fallback sweeps, digest; [8] sum |D|, [9] sum Dial levels,
  // [10] max |D|, [11] repairs given up
  uint64_t tprev = ph ? wall_clock64() : 0ull;
#define WI_STAMP(k)                              \
  do {                                           \
    if (ph) {                                    \
      const uint64_t now_ = wall_clock64();      \
      ph_add<GPH>(ph, k, now_ - tprev, tt == 0); \
      tprev = now_;                              \
    }                                            \
  } while (0)
  const uint32_t W = g.W;
  // range check (CHK): x < lim, or x == kInf when `inf_ok`
  auto chk = [&](uint32_t x, uint32_t lim, bool inf_ok, uint32_t site, uint32_t safe) -> uint32_t {
    if constexpr (CHK) {
      if (!(x < lim || (inf_ok && x == kInf))) {
        if (g.fault)
          __hip_atomic_fetch_or(g.fault, kFaultRange | (site << kFaultSiteShift), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return safe;
      }
    }
    return x;
  };
  const uint32_t lane = tt & 63, wv = tt >> 6;
  // D's root b = dlist[0]: the failed link's head, or the failed node x
  const uint32_t x = y;
  const uint32_t l = KIND == kLink ? g.link[y] : 0u;
  const uint32_t b = KIND == kLink || KIND == kMetric ? g.col[y] : y;
  if (tt == 0) {
    stw<GROUP>(&ctl->n, KIND == kSet ? 0u : 1u);
    stw<GROUP>(&ctl->ovf, 0u);
    stw<GROUP>(&ctl->hub, 0u);
    for (int q = 0; q < 3; ++q) stw<GROUP>(&ctl->flag[q], 0u);
    stq<GROUP>(&ctl->ndist, 0ull);
    stq<GROUP>(&ctl->nnh, 0ull);
    stq<GROUP>(&ctl->dh, 0ull);
    if constexpr (KIND != kSet) {
      dlist[0] = b;
      stw<GROUP>(&mark[b], 0);
    }
  }
  team_sync<TEAM, GROUP>(ctl, g.fault);
  if constexpr (KIND == kSet) {
    // D's roots: the heads of the set's tight members.  The team's lanes walk
    // the members, 64 per wave at a time; a head is claimed once (the mark
    // CAS: two members may share it) and the claimed heads of a chunk take
    // the next D indices by ballot compaction, one counter atomic per wave --
    // the level loop's append.  A root below another root is met marked there.
    for (uint32_t c0 = wv * 64; c0 < sr.n; c0 += TEAM) {  // wave-uniform
      const uint32_t i = c0 + lane;
      const uint32_t c = i < sr.n ? tight_head(g, B.dist, sr.link_edge[sr.mem[i]]) : kInf;
      const bool won = c != kInf && atomicCAS(&mark[c], kInf, kBusy) == kInf;
      const uint64_t wm = __ballot(won);
      if (wm) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&ctl->n, (uint32_t)__popcll(wm));
        base = __builtin_amdgcn_readlane(base, 0);
        if (won) {
          const uint32_t idx = base + lanes_below(wm);
          if (idx < cap) {
            dlist[idx] = c;
            stw<GROUP>(&mark[c], idx);
          } else {
            stw<GROUP>(&mark[c], kInf);
            stw<GROUP>(&ctl->ovf, 1u);
          }
        }
      }
    }
    team_sync<TEAM, GROUP>(ctl, g.fault);
  }
  // ---- D = descendants of b in the unfailed DAG (level by level) ----
  // Control words (ctl->n / ovf / hub / flag / nxt / lc) are written by
  // atomics and plain stores of other lanes, waves or CUs: every read of one
  // is an atomic load at the team's scope (ldw), so the compiler can neither
  // keep a stale copy in a register nor move the read across the team
  // barrier.  Every loop is bounded by its worst case + 2 (an iteration adds
  // a node, or settles one more level); a bound hit reports its phase in the
  // fault word and leaves the repair (loop_bound_hit).
  uint32_t lo = 0;
  bool bound_hit = false;
  for (uint32_t iter = 0;; ++iter) {
    const uint32_t n = ldw<GROUP>(&ctl->n);
    team_sync<TEAM, GROUP>(ctl, g.fault);
    if (lo >= n || ldw<GROUP>(&ctl->ovf)) break;
    if (iter > cap + 2) {  // team-uniform
      bound_hit = true;
      if (tt == 0) loop_bound_hit(g.fault, 1);
      break;
    }
    // each wave takes cs frontier nodes at a time (cs = the frontier over
    // the team's waves, at most 64: a small frontier still spreads over every
    // wave), lanes over their flattened edges (wave_edges); new nodes are
    // appended by one counter atomic per wave
    const uint32_t cs = team_chunk<TEAM>(n - lo);
    for (uint32_t c0 = lo + wv * cs; c0 < n; c0 += (TEAM / 64) * cs) {
      const uint32_t i = c0 + lane;
      const bool in = lane < cs && i < n;
      const uint32_t v = in ? chk(dlist[i], g.N, false, 1, b) : 0u;
      const bool x = in && !g.ovl[v];  // drained (v != src): no DAG children
      const uint32_t dv = x ? B.dist[v] : 0u;
      wave_edges(g.row_ptr, v, x, [&](uint32_t k, uint32_t e, bool act) {
        const uint32_t dk = lane_pull(dv, k);
        uint32_t c = 0;
        bool won = false;
        if (act) {
          const uint4 q = g.ed[e];
          c = q.x;
          if (grows<KIND>(sr, g.src, e, dk, q.y, c, B.dist[c]))
            won = atomicCAS(&mark[c], kInf, kBusy) == kInf;
        }
        const uint64_t wm = __ballot(won);
        if (wm) {
          uint32_t base = 0;
          if (lane == 0) base = atomicAdd(&ctl->n, (uint32_t)__popcll(wm));
          base = __builtin_amdgcn_readlane(base, 0);
          if (won) {
            const uint32_t idx = base + lanes_below(wm);
            if (idx < cap) {
              dlist[idx] = c;
              stw<GROUP>(&mark[c], idx);
            } else {
              stw<GROUP>(&mark[c], kInf);
              stw<GROUP>(&ctl->ovf, 1u);
            }
          }
        }
      });
    }
    lo = n;
    team_sync<TEAM, GROUP>(ctl, g.fault);
  }
  const uint32_t n = min(ldw<GROUP>(&ctl->n), cap);
  const bool ovf = ldw<GROUP>(&ctl->ovf) != 0 || bound_hit;
  WI_STAMP(1);
  if (ph) {
    ph_add<GPH>(ph, 0, 1, tt == 0);
    ph_add<GPH>(ph, 8, n, tt == 0);
    ph_max<GPH>(ph, 10, n, tt == 0);
    ph_add<GPH>(ph, 11, ovf, tt == 0);
  }
  team_sync<TEAM, GROUP>(ctl, g.fault);
  if (ovf) {
    for (uint32_t i = tt; i < n; i += TEAM) stw<GROUP>(&mark[dlist[i]], kInf);
    team_sync<TEAM, GROUP>(ctl, g.fault);
    return false;
  }
  // ---- seeds: best in-edge from outside D (unchanged distances) ----
  // waves over 64 D nodes at a time, lanes over their flattened in-edges,
  // the per-node minimum by atomics on dnew
  for (uint32_t i = tt; i < n; i += TEAM) stw<GROUP>(&dnew[i], kInf);
  team_sync<TEAM, GROUP>(ctl, g.fault);
  const uint32_t cs_seed = team_chunk<TEAM>(n);
  for (uint32_t c0 = wv * cs_seed; c0 < n; c0 += (TEAM / 64) * cs_seed) {
    const uint32_t i = c0 + lane;
    const bool in = lane < cs_seed && i < n;
    const uint32_t v = in ? dlist[i] : 0u;
    wave_edges(g.row_ptr, v, in, [&](uint32_t k, uint32_t e, bool act) {
      uint32_t s = kInf;
      const uint4 q = act ? g.ed[e] : make_uint4(0u, 0u, l, 0u);
      // (the row owner is x exactly at D index 0)
      if (act && !failed<KIND>(sr, x, l, c0 + k == 0, q.x, q.z)) {
        const uint32_t u = q.x;
        if (ldw<GROUP>(&mark[u]) == kInf && !(g.ovl[u] && u != g.src)) {
          const uint32_t du = B.dist[u];
          if (du != kInf) s = du + w_rev<KIND>(sr, e, q.w);
        }
      }
      if (s != kInf) {
        if constexpr (GROUP)
          __hip_atomic_fetch_min(&dnew[c0 + k], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
          __hip_atomic_fetch_min(&dnew[c0 + k], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    });
  }
  team_sync<TEAM, GROUP>(ctl, g.fault);
  // nh word j of a D node from its tight expanded predecessors (D or not);
  // used by the fixed-point fallback
  auto nh_of = [&](uint32_t i, uint32_t j) -> uint32_t {
    const uint32_t v = dlist[i];
    const uint32_t dv = ldw<GROUP>(&dnew[i]);
    uint32_t acc = 0;
    for (uint32_t e = g.row_ptr[v]; e < g.row_ptr[v + 1]; ++e) {
      if (failed<KIND>(sr, x, l, false, g.col[e], g.link[e])) continue;  // (dnew[x] is kInf: v != x)
      const uint32_t u = g.col[e];
      if ((g.ovl[u] && u != g.src) || drain_x<KIND>(x, u)) continue;
      const uint32_t mu = chk(ldw<GROUP>(&mark[u]), n, true, 5, kInf);
      const uint32_t du = mu != kInf ? ldw<GROUP>(&dnew[mu]) : B.dist[u];
      if (du == kInf || du + w_rev<KIND>(sr, e, in_w(g, e)) != dv) continue;
      if (u == g.src) {
        const uint32_t jb = g.nbr_bit[v];
        if ((jb >> 5) == j) acc |= 1u << (jb & 31);
      } else {
        acc |= mu != kInf ? nhn[(size_t)mu * W + j] : B.nhb[(size_t)u * W + j];
      }
    }
    return acc;
  };
  const size_t nw = (size_t)n * W;
  for (size_t x = tt; x < nw; x += TEAM) nhn[x] = 0;
  if (tt == 0) {
    stw<GROUP>(&ctl->dmin, kInf);
    stw<GROUP>(&ctl->nxt[0], kInf);
    stw<GROUP>(&ctl->lc[0], 0u);
  }
  team_sync<TEAM, GROUP>(ctl, g.fault);
  {
    uint32_t m = kInf;
    for (uint32_t i = tt; i < n; i += TEAM) m = min(m, ldw<GROUP>(&dnew[i]));
    if (m != kInf) atomicMin(&ctl->dmin, m);
  }
  team_sync<TEAM, GROUP>(ctl, g.fault);
  WI_STAMP(2);
  // ---- Dial: settle D one distance value at a time (metrics are positive:
  // a node holding the smallest pending value is final), next hops inline ----
  bool settled = true;
  uint32_t t = ldw<GROUP>(&ctl->dmin);
  for (uint32_t it = 0; t != kInf; ++it) {
    if (it >= kDialLevels) {  // too many distinct values: sweep instead
      settled = false;
      break;
    }
    uint32_t* next = &ctl->nxt[it % 3];
    uint32_t* cnt = &ctl->lc[it % 3];
    if (tt == 0) {  // the next level's slots, last read two levels ago
      stw<GROUP>(&ctl->nxt[(it + 1) % 3], kInf);
      stw<GROUP>(&ctl->lc[(it + 1) % 3], 0u);
    }
    // (a) the level's nodes (their distance is final) into ord, one counter
    // atomic per wave
    // (4 chunks per pass: their loads in flight together, one atomic)
    uint32_t m = kInf;
    for (uint32_t c0 = wv * 64; c0 < n; c0 += 4 * TEAM) {
      uint32_t d[4];
      uint64_t sm[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t i = c0 + q * TEAM + lane;
        d[q] = i < n ? ldw<GROUP>(&dnew[i]) : kInf;
      }
      uint32_t tot = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (d[q] != kInf && d[q] > t) m = min(m, d[q]);
        sm[q] = __ballot(d[q] == t);
        tot += (uint32_t)__popcll(sm[q]);
      }
      if (tot) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(cnt, tot);
        base = __builtin_amdgcn_readlane(base, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (d[q] == t) stw<GROUP>(&ord[base + lanes_below(sm[q])], c0 + q * TEAM + lane);
          base += (uint32_t)__popcll(sm[q]);
        }
      }
    }
    team_sync<TEAM, GROUP>(ctl, g.fault);
    // (b) level nodes, cs per wave at a time (a level of ~150 nodes in 64-
    // node chunks kept 3 of a group team's 64 waves busy, each walking ~8
    // flattened edge chunks in turn), lanes over their flattened edges:
    // tight predecessors give the next-hop rows (row_pairs), out-edges relax
    // the pending nodes
    const uint32_t K = ldw<GROUP>(cnt);
    const uint32_t cs = team_chunk<TEAM>(K);
    for (uint32_t q0 = wv * cs; q0 < K; q0 += (TEAM / 64) * cs) {
      const uint32_t q = q0 + lane;
      const bool valid = lane < cs && q < K;
      const uint32_t i = valid ? chk(ldw<GROUP>(&ord[q]), n, false, 9, 0) : 0u;
      const uint32_t v = valid ? chk(dlist[i], g.N, false, 10, b) : 0u;
      const uint32_t transit = valid && !g.ovl[v] && !drain_x<KIND>(x, v);  // drained: no transit
      const uint32_t jb = valid ? g.nbr_bit[v] : 0u;
      uint32_t cur = kInf, acc = 0;  // row_pairs' open row
      wave_edges(g.row_ptr, v, valid, [&](uint32_t k, uint32_t e, bool act) {
        const uint32_t ik = lane_pull(i, k), tk = lane_pull(transit, k), jk = lane_pull(jb, k);
        uint32_t u = 0, mu = kInf;
        bool tight = false, from_src = false;
        const uint4 q = act ? g.ed[e] : make_uint4(0u, 0u, l, 0u);
        // (a level's nodes hold a distance: none is a downed x)
        if (act && !failed<KIND>(sr, x, l, false, q.x, q.z)) {
          u = q.x;
          mu = chk(ldw<GROUP>(&mark[u]), n, true, 13, kInf);
          if (!(g.ovl[u] && u != g.src) && !drain_x<KIND>(x, u)) {
            const uint32_t du = mu != kInf ? ldw<GROUP>(&dnew[mu]) : B.dist[u];
            tight = du != kInf && du + w_rev<KIND>(sr, e, g.hop ? 1u : q.w) == t;
          }
          if (tk && mu != kInf) {  // relax v -> u (u pending: its value only drops)
            const uint32_t nd = t + w_fwd<KIND>(sr, e, q.y);
            if (nd < atomicMin(&dnew[mu], nd)) m = min(m, nd);
          }
          if (tight && u == g.src) {
            from_src = true;
            tight = false;
          }
        }
        row_pairs(__ballot(tight), __ballot(from_src), ik, jk, u, mu, W, nhn, B.nhb, lane, cur, acc);
      });
      if (cur != kInf && lane < W) nhn[(size_t)cur * W + lane] = acc;
    }
    if (m != kInf) atomicMin(next, m);
    team_sync<TEAM, GROUP>(ctl, g.fault);
    t = ldw<GROUP>(next);
    if (ph) ph_add<GPH>(ph, 9, 1, tt == 0);
  }
  WI_STAMP(3);
  if (!settled) {
    // ---- label-correcting sweeps inside D (Bellman-Ford: at most n + 1) ----
    for (uint32_t it = 0;; ++it) {
      if (it > n + 2) {  // team-uniform
        if (tt == 0) loop_bound_hit(g.fault, 2);
        break;
      }
      bool any = false;
      for (uint32_t i = tt; i < n; i += TEAM) {
        const uint32_t v = dlist[i];
        const uint32_t dv = ldw<GROUP>(&dnew[i]);
        if (dv == kInf || g.ovl[v] || drain_x<KIND>(x, v)) continue;
        for (uint32_t e = g.row_ptr[v]; e < g.row_ptr[v + 1]; ++e) {
          if (failed<KIND>(sr, x, l, false, g.col[e], g.link[e])) continue;
          const uint32_t ic = chk(ldw<GROUP>(&mark[g.col[e]]), n, true, 14, kInf);
          if (ic == kInf) continue;
          const uint32_t nd = dv + w_fwd<KIND>(sr, e, g.wt[e]);
          if (nd < atomicMin(&dnew[ic], nd)) any = true;
        }
      }
      if (any) stw<GROUP>(&ctl->flag[it % 3], 1u);
      if (tt == 0) stw<GROUP>(&ctl->flag[(it + 1) % 3], 0u);
      team_sync<TEAM, GROUP>(ctl, g.fault);
      if (!ldw<GROUP>(&ctl->flag[it % 3])) break;
    }

    const size_t nw = (size_t)n * W;
    for (size_t x = tt; x < nw; x += TEAM) nhn[x] = 0;
    if (tt == 0) {
      for (int q = 0; q < 3; ++q) stw<GROUP>(&ctl->flag[q], 0u);
      stw<GROUP>(&ctl->dmin, kInf);
      stw<GROUP>(&ctl->dmax, 0u);
    }
    team_sync<TEAM, GROUP>(ctl, g.fault);
    for (uint32_t i = tt; i < n; i += TEAM) {
      const uint32_t d = ldw<GROUP>(&dnew[i]);
      if (d != kInf) {
        atomicMin(&ctl->dmin, d);
        atomicMax(&ctl->dmax, d);
      }
    }
    team_sync<TEAM, GROUP>(ctl, g.fault);
    const uint32_t dmin = ldw<GROUP>(&ctl->dmin);
    const uint32_t nlev = dmin == kInf ? 0u : ldw<GROUP>(&ctl->dmax) - dmin + 1;
    if (nlev <= cap) {
      // counting sort of D by new distance; a predecessor always sits in a
      // lower level (positive metrics), so one pass per level is exact
      for (uint32_t b = tt; b < nlev; b += TEAM) stw<GROUP>(&lvl[b], 0u);
      team_sync<TEAM, GROUP>(ctl, g.fault);
      for (uint32_t i = tt; i < n; i += TEAM) {
        const uint32_t d = ldw<GROUP>(&dnew[i]);
        if (d != kInf) atomicAdd(&lvl[d - dmin], 1u);
      }
      team_sync<TEAM, GROUP>(ctl, g.fault);
      if (tt < 64) {  // exclusive scan by the team's first wave
        uint32_t carry = 0;
        for (uint32_t base = 0; base < nlev; base += 64) {
          const uint32_t b = base + tt;
          const uint32_t x = b < nlev ? ldw<GROUP>(&lvl[b]) : 0u;
          const uint32_t inc = wave_incl_scan32(x);
          if (b < nlev) stw<GROUP>(&lvl[b], carry + inc - x);
          carry += __builtin_amdgcn_readlane(inc, 63);
        }
      }
      team_sync<TEAM, GROUP>(ctl, g.fault);
      for (uint32_t i = tt; i < n; i += TEAM) {
        const uint32_t d = ldw<GROUP>(&dnew[i]);
        if (d != kInf) stw<GROUP>(&ord[atomicAdd(&lvl[d - dmin], 1u)], i);
      }
      team_sync<TEAM, GROUP>(ctl, g.fault);
      uint32_t begin = 0;
      for (uint32_t b = 0; b < nlev; ++b) {
        const uint32_t end = ldw<GROUP>(&lvl[b]);
        if (end == begin) continue;
        const size_t items = (size_t)(end - begin) * W;
        for (size_t x = tt; x < items; x += TEAM) {
          const uint32_t i = chk(ldw<GROUP>(&ord[begin + x / W]), n, false, 15, 0), j = (uint32_t)(x % W);
          nhn[(size_t)i * W + j] = nh_of(i, j);
        }
        begin = end;
        team_sync<TEAM, GROUP>(ctl, g.fault);
      }
    } else {
      // fixed-point sweeps (monotone union over the DAG: at most depth + 1)
      for (uint32_t it = 0;; ++it) {
        if (it > n + 2) {  // team-uniform
          if (tt == 0) loop_bound_hit(g.fault, 3);
          break;
        }
        bool any = false;
        for (uint32_t x = tt; x < nw; x += TEAM) {
          const uint32_t i = x / W, j = x % W;
          if (ldw<GROUP>(&dnew[i]) == kInf) continue;
          const uint32_t acc = nh_of(i, j);
          if (acc != nhn[x]) {
            nhn[x] = acc;
            any = true;
          }
        }
        if (any) stw<GROUP>(&ctl->flag[it % 3], 1u);
        if (tt == 0) stw<GROUP>(&ctl->flag[(it + 1) % 3], 0u);
        team_sync<TEAM, GROUP>(ctl, g.fault);
        if (!ldw<GROUP>(&ctl->flag[it % 3])) break;
      }
    }
  }
  WI_STAMP(4);
  if constexpr (EMIT) {
    // ---- change list: the D nodes whose metric or row changed, a wave per
    // 64 of them; ctl->n is free (|D| was read into n) and counts the team's
    // entries -- summed per wave in the count pass, one returning atomic per
    // wave chunk (ballot + mbcnt ranks) in the fill pass ----
    const bool fill = em->cnode != nullptr;
    const uint64_t at = fill ? em->cptr[f] : 0ull;
    const uint32_t room = fill ? (uint32_t)(em->cptr[f + 1] - at) : 0u;
    if (tt == 0) stw<GROUP>(&ctl->n, 0u);
    team_sync<TEAM, GROUP>(ctl, g.fault);
    uint32_t kw = 0;
    for (uint32_t c0 = wv * 64; c0 < n; c0 += TEAM) {  // wave-uniform
      const uint32_t i = c0 + lane;
      uint32_t v = 0, d1 = kInf;
      bool changed = false;
      if (i < n) {
        v = dlist[i];
        d1 = ldw<GROUP>(&dnew[i]);
        changed = entry_changed<GROUP>(B, nhn, W, v, i, d1);
      }
      const uint64_t m = __ballot(changed);
      if (!m) continue;
      if (fill) {
        uint32_t q0 = 0;
        if (lane == 0) q0 = atomicAdd(&ctl->n, (uint32_t)__popcll(m));
        q0 = __builtin_amdgcn_readlane(q0, 0);
        emit_entries<GROUP>(*em, at, room, q0, m, changed, v, i, d1, nhn, lane);
      } else {
        kw += (uint32_t)__popcll(m);
      }
    }
    if (!fill) {
      if (lane == 0 && kw) atomicAdd(&ctl->n, kw);
      team_sync<TEAM, GROUP>(ctl, g.fault);
      if (tt == 0) em->cnt[f] = ldw<GROUP>(&ctl->n);
    }
  }
  // ---- digest delta over D, scratch reset ----
  uint32_t nd_ = 0, nn_ = 0;
  uint64_t dh = 0;
  for (uint32_t i = tt; i < n; i += TEAM) {
    const uint32_t v = dlist[i];
    const uint32_t d1 = ldw<GROUP>(&dnew[i]), d0 = B.dist[v];
    uint64_t f0, f1;
    bool diff = d1 == kInf;
    row_pair_hash<GROUP>(B.nhb + (size_t)v * W, nhn + (size_t)i * W, W, f0, f1, diff);
    const uint64_t base = mix64((uint64_t)v + 1);
    nd_ += d1 != d0;
    nn_ += diff;
    dh += (d1 == kInf ? 0ull : mix64(base + d1) ^ f1) - (mix64(base + d0) ^ f0);
    stw<GROUP>(&mark[v], kInf);
  }
  if (nd_) atomicAdd(&ctl->ndist, (unsigned long long)nd_);
  if (nn_) atomicAdd(&ctl->nnh, (unsigned long long)nn_);
  if (dh) atomicAdd(&ctl->dh, (unsigned long long)dh);
  team_sync<TEAM, GROUP>(ctl, g.fault);
  if (tt == 0)
    *out = spf_whatif_digest{(uint32_t)ldq<GROUP>(&ctl->ndist), (uint32_t)ldq<GROUP>(&ctl->nnh),
                             (uint64_t)(*B.H + ldq<GROUP>(&ctl->dh))};
  team_sync<TEAM, GROUP>(ctl, g.fault);
  WI_STAMP(5);
#undef WI_STAMP
  return true;
}

// A wave team's node -> D-index map: an open-addressed table of T = 4 * cap
// (a power of two) u64 slots, key (node) in the low word, value (D index, or
// kBusy while being claimed) in the high word, linear probing from a
// multiplicative hash.  It replaces an N-word `mark` array per wave team:
// 4,096 teams x 250k nodes x 4 B = 4 GB of scratch whose random lookups
// missed every cache -- the tables take 32 KB a team.
// Slots start (and are always left) empty (~0): a repair clears the slots it
// used, an aborted one the whole table.
struct WaveSet {
  unsigned long long* tab;
  uint32_t mask, shift;  // T - 1, 32 - log2(T)
};
constexpr unsigned long long kSlotEmpty = ~0ull;
__device__ __forceinline__ unsigned long long ws_ld(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void ws_st(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// insert v (value kBusy): its slot, or ~0u when v is present already; `full`
// when no slot is left (the caller aborts the repair)
__device__ __forceinline__ uint32_t ws_claim(const WaveSet& s, uint32_t v, bool& full) {
  uint32_t h = (v * 0x9E3779B1u) >> s.shift;
  for (uint32_t k = 0; k <= s.mask; ++k, h = (h + 1) & s.mask) {
    const unsigned long long old = atomicCAS(&s.tab[h], kSlotEmpty, ((unsigned long long)kBusy << 32) | v);
    if (old == kSlotEmpty) return h;
    if ((uint32_t)old == v) return ~0u;
  }
  full = true;
  return ~0u;
}
// v's slot, or ~0u when absent
__device__ __forceinline__ uint32_t ws_slot(const WaveSet& s, uint32_t v) {
  uint32_t h = (v * 0x9E3779B1u) >> s.shift;
  for (uint32_t k = 0; k <= s.mask; ++k, h = (h + 1) & s.mask) {
    const unsigned long long x = ws_ld(&s.tab[h]);
    if ((uint32_t)x == v) return h;
    if (x == kSlotEmpty) return ~0u;
  }
  return ~0u;
}
// v's value (its D index), kInf when absent
__device__ __forceinline__ uint32_t ws_find(const WaveSet& s, uint32_t v) {
  uint32_t h = (v * 0x9E3779B1u) >> s.shift;
  for (uint32_t k = 0; k <= s.mask; ++k, h = (h + 1) & s.mask) {
    const unsigned long long x = ws_ld(&s.tab[h]);
    if ((uint32_t)x == v) return (uint32_t)(x >> 32);
    if (x == kSlotEmpty) return kInf;
  }
  return kInf;
}

// A wave team's repair (|D| <= cap): repair()'s three phases -- D discovery,
// seeds, Dial with next hops inline -- and its digest delta, bit for bit, but
// with the wave's lanes over the flattened edges of up to 64 nodes at a time
// (wave_edges) instead of a lane per node walking its edges one by one: a
// node's dependent chain (row_ptr -> col -> mark -> dnew / base row) is paid
// once per 64 edges instead of once per edge.  The team is one wave, so |D|,
// the level list length and the next Dial value live in registers
// (ballot + mbcnt compaction instead of counter atomics); the level list of
// a D of <= 64 nodes never leaves the registers (ds_permute).  |D| <= cap <=
// kDialLevels distinct values, so Dial always settles (no fallback sweeps).
template <bool CHK, bool GPH = false, bool EMIT = false, int KIND = kLink>
__device__ bool repair_wave(const WiGraph& g, const WiBase& B, const WaveSet& hs, uint32_t* dlist,
                            uint32_t* dnew, uint32_t* nhn, uint32_t* ord, uint32_t cap,
                            TeamCtl* ctl, uint32_t lane, uint32_t y, spf_whatif_digest* out,
                            uint64_t* ph, const WiEmit* em = nullptr, uint32_t f = 0,
                            SetRef<KIND> sr = SetRef<KIND>{}) {
  uint64_t tprev = ph ? wall_clock64() : 0ull;
#define WI_STAMP(k)                                \
  do {                                             \
    if (ph) {                                      \
      const uint64_t now_ = wall_clock64();        \
      ph_add<GPH>(ph, k, now_ - tprev, lane == 0); \
      tprev = now_;                                \
    }                                              \
  } while (0)
  auto chk = [&](uint32_t x, uint32_t lim, bool inf_ok, uint32_t site, uint32_t safe) -> uint32_t {
    if constexpr (CHK) {
      if (!(x < lim || (inf_ok && x == kInf))) {
        if (g.fault)
          __hip_atomic_fetch_or(g.fault, kFaultRange | (site << kFaultSiteShift), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return safe;
      }
    }
    return x;
  };
  auto sync = [&]() { team_sync<64>(ctl, g.fault); };
  const uint32_t W = g.W;
  const uint32_t x = y;  // (repair(): l, b)
  const uint32_t l = KIND == kLink ? g.link[y] : 0u;
  const uint32_t b = KIND == kLink || KIND == kMetric ? g.col[y] : y;
  if (lane == 0) {
    if constexpr (KIND != kSet) {
      dlist[0] = b;
      bool full = false;
      const uint32_t s0 = ws_claim(hs, b, full);  // (the table is empty)
      ws_st(&hs.tab[s0], b);                      // value 0: D index 0
    }
    stq<false>(&ctl->ndist, 0ull);
    stq<false>(&ctl->nnh, 0ull);
    stq<false>(&ctl->dh, 0ull);
  }
  sync();
  // ---- D = descendants of b in the unfailed DAG, frontier by frontier ----
  uint32_t n = KIND == kSet ? 0u : 1u, lo = 0;
  bool bad = false;
  if constexpr (KIND == kSet) {
    // D's roots: the heads of the set's tight members, the lanes over the
    // members 64 at a time; a head is claimed once (ws_claim: two members may
    // share it), the claimed heads of a chunk take D indices n, n + 1, ... by
    // ballot compaction -- the frontier loop's append.  More roots than cap,
    // or a full table, is the overflow below.
    bool full = false;
    for (uint32_t c0 = 0; c0 < sr.n && n <= cap; c0 += 64) {
      const uint32_t i = c0 + lane;
      const uint32_t c = i < sr.n ? tight_head(g, B.dist, sr.link_edge[sr.mem[i]]) : kInf;
      uint32_t slot = ~0u;
      if (c != kInf) slot = ws_claim(hs, c, full);
      const bool won = slot != ~0u;
      const uint64_t wm = __ballot(won);
      if (won) {
        const uint32_t idx = n + lanes_below(wm);
        ws_st(&hs.tab[slot], ((unsigned long long)(idx < cap ? idx : kInf) << 32) | c);
        if (idx < cap) dlist[idx] = c;
      }
      n += (uint32_t)__popcll(wm);
    }
    if (__ballot(full)) {
      bad = true;
      lo = n;  // (no frontier pass)
    }
    sync();
  }
  for (uint32_t iter = 0; lo < n && n <= cap; ++iter) {
    if (iter > cap + 2) {  // wave-uniform
      bad = true;
      if (lane == 0) loop_bound_hit(g.fault, 1);
      break;
    }
    const uint32_t hi = n;
    for (uint32_t c0 = lo; c0 < hi && n <= cap; c0 += 64) {
      const uint32_t i = c0 + lane;
      const uint32_t v = i < hi ? chk(ldw<false>(&dlist[i]), g.N, false, 1, b) : 0u;
      const bool x = i < hi && !g.ovl[v];  // drained (v != src): no DAG children
      const uint32_t dv = x ? B.dist[v] : 0u;
      bool full = false;
      wave_edges(g.row_ptr, v, x, [&](uint32_t k, uint32_t e, bool act) {
        const uint32_t dk = lane_pull(dv, k);
        uint32_t c = 0, slot = ~0u;
        if (act) {
          const uint4 q = g.ed[e];
          c = q.x;
          if (grows<KIND>(sr, g.src, e, dk, q.y, c, B.dist[c])) slot = ws_claim(hs, c, full);
        }
        const bool won = slot != ~0u;
        const uint64_t wm = __ballot(won);
        if (won) {
          const uint32_t idx = n + lanes_below(wm);
          ws_st(&hs.tab[slot], ((unsigned long long)(idx < cap ? idx : kInf) << 32) | c);
          if (idx < cap) dlist[idx] = c;
        }
        n += (uint32_t)__popcll(wm);
      });
      if (__ballot(full)) {  // no slot left: abort as an overflow
        bad = true;
        break;
      }
    }
    lo = hi;
    sync();
    if (bad) break;
  }
  const bool ovf = n > cap || bad;
  n = min(n, cap);
  WI_STAMP(1);
  if (ph) {
    ph_add<GPH>(ph, 0, 1, lane == 0);
    ph_add<GPH>(ph, 8, n, lane == 0);
    ph_max<GPH>(ph, 10, n, lane == 0);
    ph_add<GPH>(ph, 11, ovf, lane == 0);
  }
  if (ovf) {  // slots past the cap hold kInf values: clear the whole table
    for (uint32_t q = lane; q <= hs.mask; q += 64) ws_st(&hs.tab[q], kSlotEmpty);
    sync();
    return false;
  }
  // ---- seeds: best in-edge from outside D (unchanged distances) ----
  for (uint32_t i = lane; i < n; i += 64) stw<false>(&dnew[i], kInf);
  for (size_t x = lane; x < (size_t)n * W; x += 64) nhn[x] = 0;
  sync();
  for (uint32_t c0 = 0; c0 < n; c0 += 64) {
    const uint32_t i = c0 + lane;
    const uint32_t v = i < n ? ldw<false>(&dlist[i]) : 0u;
    wave_edges(g.row_ptr, v, i < n, [&](uint32_t k, uint32_t e, bool act) {
      uint32_t s = kInf;
      const uint4 q = act ? g.ed[e] : make_uint4(0u, 0u, l, 0u);
      if (act && !failed<KIND>(sr, x, l, c0 + k == 0, q.x, q.z)) {
        const uint32_t u = q.x;
        if (ws_find(hs, u) == kInf && !(g.ovl[u] && u != g.src)) {
          const uint32_t du = B.dist[u];
          if (du != kInf) s = du + w_rev<KIND>(sr, e, q.w);
        }
      }
      if (s != kInf)
        __hip_atomic_fetch_min(&dnew[c0 + k], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    });
  }
  sync();
  // the D of <= 64 nodes stays in registers through Dial: lane i holds D
  // node i (index, node, the source-neighbour bit)
  const bool small = n <= 64;
  const uint32_t sv = small && lane < n ? ldw<false>(&dlist[lane]) : 0u;
  uint32_t t = kInf;
  for (uint32_t c0 = 0; c0 < n; c0 += 64) {
    const uint32_t i = c0 + lane;
    t = min(t, i < n ? ldw<false>(&dnew[i]) : kInf);
  }
  t = wave_min32(t);
  WI_STAMP(2);
  // ---- Dial: settle D one distance value at a time (metrics are positive:
  // a node holding the smallest pending value is final), next hops inline ----
  for (uint32_t it = 0; t != kInf; ++it) {
    if (it > n + 2) {  // every level settles a node: cannot happen
      if (lane == 0) loop_bound_hit(g.fault, 4);
      break;
    }
    // (a) the level's nodes (their distance is final) and the next value
    uint32_t m = kInf, K = 0, li = 0, lv = 0;
    if (small) {
      const uint32_t d = lane < n ? ldw<false>(&dnew[lane]) : kInf;
      const bool sel = d == t;
      if (d != kInf && d > t) m = d;
      const uint64_t sm = __ballot(sel);
      K = (uint32_t)__popcll(sm);
      // compact: the r-th level node to lane r, the rest after them
      const uint32_t r = lanes_below(sm);
      const uint32_t dst = sel ? r : K + lane - r;
      li = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)lane);
      lv = (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)sv);
    } else {
      for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        const uint32_t i = c0 + lane;
        const uint32_t d = i < n ? ldw<false>(&dnew[i]) : kInf;
        const bool sel = d == t;
        if (d != kInf && d > t) m = min(m, d);
        const uint64_t sm = __ballot(sel);
        if (sel) stw<false>(&ord[K + lanes_below(sm)], i);
        K += (uint32_t)__popcll(sm);
      }
      sync();
    }
    // (b) level nodes, 64 at a time: tight predecessors give the next-hop
    // rows, out-edges relax the pending nodes
    for (uint32_t q0 = 0; q0 < K; q0 += 64) {
      const uint32_t q = q0 + lane;
      const bool valid = q < K;
      uint32_t i = li, v = lv;
      if (!small) {
        i = valid ? chk(ldw<false>(&ord[q]), n, false, 9, 0) : 0u;
        v = valid ? chk(ldw<false>(&dlist[i]), g.N, false, 10, b) : 0u;
      }
      const uint32_t transit = valid && !g.ovl[v] && !drain_x<KIND>(x, v);  // drained: no transit
      const uint32_t jb = valid ? g.nbr_bit[v] : 0u;
      uint32_t cur = kInf, acc = 0;  // row_pairs' open row
      wave_edges(g.row_ptr, v, valid, [&](uint32_t k, uint32_t e, bool act) {
        const uint32_t ik = lane_pull(i, k), tk = lane_pull(transit, k), jk = lane_pull(jb, k);
        uint32_t u = 0, mu = kInf;
        bool tight = false, from_src = false;
        const uint4 q = act ? g.ed[e] : make_uint4(0u, 0u, l, 0u);
        if (act && !failed<KIND>(sr, x, l, false, q.x, q.z)) {
          u = q.x;
          mu = chk(ws_find(hs, u), n, true, 13, kInf);
          if (!(g.ovl[u] && u != g.src) && !drain_x<KIND>(x, u)) {
            const uint32_t du = mu != kInf ? ldw<false>(&dnew[mu]) : B.dist[u];
            tight = du != kInf && du + w_rev<KIND>(sr, e, g.hop ? 1u : q.w) == t;
          }
          if (tk && mu != kInf) {  // relax v -> u (u pending: its value only drops)
            const uint32_t nd = t + w_fwd<KIND>(sr, e, q.y);
            if (nd < atomicMin(&dnew[mu], nd)) m = min(m, nd);
          }
          if (tight && u == g.src) {
            from_src = true;
            tight = false;
          }
        }
        // the row ORs, one tight pair at a time in lane order
        row_pairs(__ballot(tight), __ballot(from_src), ik, jk, u, mu, W, nhn, B.nhb, lane, cur, acc);
      });
      if (cur != kInf && lane < W) nhn[(size_t)cur * W + lane] = acc;
    }
    sync();
    t = wave_min32(m);
    if (ph) ph_add<GPH>(ph, 9, 1, lane == 0);
  }
  WI_STAMP(3);
  if constexpr (EMIT) {
    // ---- change list: the D nodes whose metric or row changed (read here:
    // the digest loop overwrites dnew with slot indices); the team is one
    // wave, so the entry counter is a register ----
    const bool fill = em->cnode != nullptr;
    const uint64_t at = fill ? em->cptr[f] : 0ull;
    const uint32_t room = fill ? (uint32_t)(em->cptr[f + 1] - at) : 0u;
    uint32_t k = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
      const uint32_t i = c0 + lane;
      uint32_t v = 0, d1 = kInf;
      bool changed = false;
      if (i < n) {
        v = ldw<false>(&dlist[i]);
        d1 = ldw<false>(&dnew[i]);
        changed = entry_changed<false>(B, nhn, W, v, i, d1);
      }
      const uint64_t m = __ballot(changed);
      if (fill && m) emit_entries<false>(*em, at, room, k, m, changed, v, i, d1, nhn, lane);
      k += (uint32_t)__popcll(m);
    }
    if (!fill && lane == 0) em->cnt[f] = k;
  }
  // ---- digest delta over D, scratch reset ----
  uint32_t nd_ = 0, nn_ = 0;
  uint64_t dh = 0;
  for (uint32_t i = lane; i < n; i += 64) {
    const uint32_t v = ldw<false>(&dlist[i]);
    const uint32_t d1 = ldw<false>(&dnew[i]), d0 = B.dist[v];
    uint64_t f0, f1;
    bool diff = d1 == kInf;
    row_pair_hash<false>(B.nhb + (size_t)v * W, nhn + (size_t)i * W, W, f0, f1, diff);
    const uint64_t base = mix64((uint64_t)v + 1);
    nd_ += d1 != d0;
    nn_ += diff;
    dh += (d1 == kInf ? 0ull : mix64(base + d1) ^ f1) - (mix64(base + d0) ^ f0);
    stw<false>(&dnew[i], ws_slot(hs, v));  // (every lookup is done: find the slots, then clear)
  }
  sync();
  for (uint32_t i = lane; i < n; i += 64) {
    const uint32_t q = ldw<false>(&dnew[i]);
    if (q <= hs.mask) ws_st(&hs.tab[q], kSlotEmpty);
  }
  if (nd_) atomicAdd(&ctl->ndist, (unsigned long long)nd_);
  if (nn_) atomicAdd(&ctl->nnh, (unsigned long long)nn_);
  if (dh) atomicAdd(&ctl->dh, (unsigned long long)dh);
  sync();
  if (lane == 0)
    *out = spf_whatif_digest{(uint32_t)ldq<false>(&ctl->ndist), (uint32_t)ldq<false>(&ctl->nnh),
                             (uint64_t)(*B.H + ldq<false>(&ctl->dh))};
  sync();
  WI_STAMP(5);
#undef WI_STAMP
  return true;
}

// The profiled instances' phase-counter row of `team` (16 slots) in a
// region of `rows` rows: a team past the region sets kFaultProfRow in the fault word
// (kernel in bits 24-31) and counts nothing -- the layout of the prof buffer
// ([block / group teams][base][wave teams] x 16, spf_whatif_plan_create) is
// checked, not assumed.
__device__ __forceinline__ uint64_t* prof_row(unsigned long long* prof, size_t team, uint32_t rows,
                                              uint32_t kernel, uint32_t* fault) {
  if (team < rows) return reinterpret_cast<uint64_t*>(prof + 16 * team);
  if (fault) __hip_atomic_fetch_or(fault, kFaultProfRow | (kernel << kFaultKernelShift), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return nullptr;
}

// wave teams over the hot list; failures whose D overflows kWaveCap are
// queued for the workgroup teams.  PROF (SPF_WHATIF_PROF): separate
// instances with the per-team phase counters (prof row `team`, prof_rows
// rows) -- 1: in registers, stored at team exit; 2: global read-modify-writes
// per event -- so the production instance's registers, which set its
// co-residency with the group teams (spf_whatif_plan_create), do not change
// with diagnostics.  EMIT (spf_whatif_changes; PROF 0 only): likewise separate
// instances of the three repair kernels, with one more argument, the WiEmit,
// as a trailing pack -- the production instances keep their argument list and
// compile to what they did without it.  A set plan's instances (KIND kSet)
// end the pack with the WiSets; the work item's failure index h.x selects the
// set (set_arg).
template <int PROF, bool EMIT = false, int KIND = kLink, class... EM>
__global__ __launch_bounds__(256) void repair_wave_kernel(
    WiGraph g, WiBase B, const uint2* __restrict__ hot, const uint32_t* __restrict__ n_hot,
    uint32_t* cursor, uint2* big, uint32_t* n_big, unsigned long long* tab, uint32_t* dlist,
    uint32_t* dnew, uint32_t* nhn, uint32_t* lvl, uint32_t* ord, spf_whatif_digest* out, uint32_t cap,
    uint32_t tab_log2, unsigned long long* prof, uint32_t prof_rows, EM... em) {
  static_assert(sizeof...(EM) == (EMIT ? 1 : 0) + (kind_has_table(KIND) ? 1 : 0) && (!EMIT || PROF == 0),
                "EMIT: a WiEmit, PROF 0; set plans: a WiSets last, metric plans: a WiMet");
  __shared__ TeamCtl ctl[4];
  const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t team = (size_t)blockIdx.x * 4 + w;
  const WaveSet hs{tab + (team << tab_log2), (1u << tab_log2) - 1u, 32u - tab_log2};
  dlist += team * cap;
  dnew += team * cap;
  nhn += team * cap * g.W;
  lvl += team * (cap + 1);
  ord += team * 2 * cap;  // level list + its hubs
  const uint32_t total = *n_hot;
  uint64_t ph[12] = {};
  uint64_t* gph = PROF == 2 ? prof_row(prof, team, prof_rows, 1, lane == 0 ? g.fault : nullptr) : nullptr;
  for (;;) {
    uint32_t k = 0;
    if (lane == 0) k = atomicAdd(cursor, 1u);
    k = __builtin_amdgcn_readlane(k, 0);
    if (k >= total) break;
    const uint2 h = hot[k];
    if (!repair_wave<PROF != 0, PROF == 2, EMIT, KIND>(g, B, hs, dlist, dnew, nhn, ord, cap, &ctl[w],
                                                      lane, h.y, out + h.x, PROF == 1 ? ph : gph,
                                                      emit_arg(em...), h.x, set_arg<KIND>(h.x, em...))) {
      if (lane == 0) big[atomicAdd(n_big, 1u)] = h;
    }
  }
  if (PROF == 1 && lane == 0)
    if (uint64_t* r = prof_row(prof, team, prof_rows, 1, g.fault))
      for (int q = 0; q < 12; ++q) r[q] = ph[q];
}

template <int PROF, bool EMIT = false, int KIND = kLink, class... EM>
__global__ __launch_bounds__(1024) void repair_block_kernel(
    WiGraph g, WiBase B, const uint2* __restrict__ big, const uint32_t* __restrict__ n_big,
    uint32_t* mark, uint32_t* dlist, uint32_t* dnew, uint32_t* nhn, uint32_t* lvl, uint32_t* ord,
    spf_whatif_digest* out, unsigned long long* prof, uint32_t prof_rows, EM... em) {
  static_assert(sizeof...(EM) == (EMIT ? 1 : 0) + (kind_has_table(KIND) ? 1 : 0) && (!EMIT || PROF == 0),
                "EMIT: a WiEmit, PROF 0; set plans: a WiSets last, metric plans: a WiMet");
  __shared__ TeamCtl ctl;
  // the largest repairs are the critical path of a batch and share their CU
  // with wave teams running concurrently: win the issue arbitration
  __builtin_amdgcn_s_setprio(3);
  const size_t team = blockIdx.x;
  mark += team * g.N;
  dlist += team * g.N;
  dnew += team * g.N;
  nhn += team * (size_t)g.N * g.W;
  lvl += team * ((size_t)g.N + 1);
  ord += team * 2 * (size_t)g.N;  // level list + its hubs
  const uint32_t total = *n_big;
  uint64_t ph[12] = {};
  uint64_t* gph =
      PROF == 2 ? prof_row(prof, team, prof_rows, 2, threadIdx.x == 0 ? g.fault : nullptr) : nullptr;
  for (uint32_t k = blockIdx.x; k < total; k += gridDim.x) {
    const uint2 h = big[k];
    repair<1024, false, false, PROF == 2, EMIT, KIND>(g, B, mark, dlist, dnew, nhn, lvl, ord, g.N,
                                                      &ctl, threadIdx.x, h.y, out + h.x,
                                                      PROF == 1 ? ph : gph, emit_arg(em...), h.x,
                                                      set_arg<KIND>(h.x, em...));
  }
  if (PROF == 1 && threadIdx.x == 0)
    if (uint64_t* r = prof_row(prof, team, prof_rows, 2, g.fault))
      for (int q = 0; q < 12; ++q) r[q] = ph[q];
}

// The classified big failures, largest first (the order the group teams pull
// them in): a rank sort by one workgroup; lists longer than kSortCap keep
// their order.  KEY maps a work item's y to its size: the parent subtree of
// the hot edge's head (link and metric plans), of the failed node itself (node
// plans), or y itself, a set plan's size estimate.
struct KeySubOfHead {
  const uint32_t *sub, *col;
  __device__ uint32_t operator()(uint32_t y) const { return sub[col[y]]; }
};
struct KeySubOfNode {
  const uint32_t* sub;
  __device__ uint32_t operator()(uint32_t y) const { return sub[y]; }
};
struct KeyItself {
  __device__ uint32_t operator()(uint32_t y) const { return y; }
};
constexpr uint32_t kSortCap = 8192;
template <class KEY>
__global__ __launch_bounds__(1024) void sort_big_kernel(const uint2* __restrict__ in,
                                                        const uint32_t* __restrict__ n_in, KEY key,
                                                        uint2* __restrict__ out) {
  const uint32_t n = *n_in;
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
    if (n > kSortCap) {
      out[i] = in[i];
      continue;
    }
    const uint32_t ki = key(in[i].y);
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t kj = key(in[j].y);
      r += kj > ki || (kj == ki && j < i);
    }
    out[r] = in[i];
  }
}

// Group teams of G workgroups of kGroupWg threads (one grid-resident launch, a
// workgroup per CU): the largest repairs get G CUs each.  Half-size
// workgroups (8 waves, 2 per SIMD) co-reside with the wave teams' blocks, so
// both progress from the start.  Members of a team sit on one XCD (blocks x
// and x + 8 share one); teams pull failures, largest first.
constexpr int kGroupWg = 512;
template <int G, int PROF, bool EMIT = false, int KIND = kLink, class... EM>
__global__ __launch_bounds__(kGroupWg) void repair_group_kernel(
    WiGraph g, WiBase B, const uint2* __restrict__ big, const uint32_t* __restrict__ n_big,
    uint32_t* cursor, TeamCtl* ctls, uint32_t* mark, uint32_t* dlist, uint32_t* dnew,
    uint32_t* nhn, uint32_t* lvl, uint32_t* ord, spf_whatif_digest* out,
    unsigned long long* prof, uint32_t prof_rows, EM... em) {
  static_assert(sizeof...(EM) == (EMIT ? 1 : 0) + (kind_has_table(KIND) ? 1 : 0) && (!EMIT || PROF == 0),
                "EMIT: a WiEmit, PROF 0; set plans: a WiSets last, metric plans: a WiMet");
  constexpr int TEAM = kGroupWg * G;
  __builtin_amdgcn_s_setprio(3);
  const uint32_t idx = blockIdx.x >> 3;
  const uint32_t member = idx % G;
  const size_t team = (size_t)(idx / G) * 8 + (blockIdx.x & 7);
  TeamCtl* ctl = ctls + team;
  const uint32_t tt = member * kGroupWg + threadIdx.x;
  mark += team * g.N;
  dlist += team * g.N;
  dnew += team * g.N;
  nhn += team * (size_t)g.N * g.W;
  lvl += team * ((size_t)g.N + 1);
  ord += team * 2 * (size_t)g.N;
  const uint32_t total = *n_big;
  uint64_t ph[12] = {};
  uint64_t* gph = PROF == 2 ? prof_row(prof, team, prof_rows, 3, tt == 0 ? g.fault : nullptr) : nullptr;
  for (;;) {
    if (tt == 0) stw<true>(&ctl->next, atomicAdd(cursor, 1u));
    team_sync<TEAM, true>(ctl, g.fault);
    const uint32_t k = ldw<true>(&ctl->next);
    if (k >= total) break;  // team-uniform
    const uint2 h = big[k];
    repair<TEAM, true, false, PROF == 2, EMIT, KIND>(g, B, mark, dlist, dnew, nhn, lvl, ord, g.N, ctl,
                                                     tt, h.y, out + h.x, PROF == 1 ? ph : gph,
                                                     emit_arg(em...), h.x, set_arg<KIND>(h.x, em...));
  }
  if (PROF == 1 && tt == 0)
    if (uint64_t* r = prof_row(prof, team, prof_rows, 3, g.fault))
      for (int q = 0; q < 12; ++q) r[q] = ph[q];
}

}  // namespace

#endif  // OPENR_AMD_WHATIF_REPAIR_H
