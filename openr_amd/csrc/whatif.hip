// ============================================================================
//  whatif.hip -- what-if batches: the SPF of one source re-run for every
//  single-link failure of a list, reduced to a
//  per-failure digest.
//
//  Reference semantics per failure l: runSpf(src, true, {l})
//  (openr/decision/LinkState.cpp:808-882 with linksToIgnore = {l}, the
//  primitive getKthPaths uses at :776-779), compared with runSpf(src).
//
//  Exact incremental evaluation instead of one full Dijkstra per failure:
//    * l is "cold" when neither direction is a tight edge of the unfailed
//      shortest-path DAG (tail expanded, d(tail) + w = d(head)).  Removing a
//      link that no shortest path uses changes no distance, no pathLinks and
//      so no next hop: the digest is the unfailed one.
//    * l is "hot" when a -> b is tight (one direction at most: metrics are
//      positive).  Only D = the DAG descendants of b (b included) can change:
//      a node outside D has no tight path through a -> b, keeps its distance
//      and its tight predecessors, none of which is in D.  On D:
//        - distances: seeds from in-edges leaving nodes outside D (exact,
//          unchanged) and a label-correcting sweep inside D;
//        - next hops: nh(v) = union over tight expanded predecessors u of
//          ({v} if u = src else nh(u)) -- the reference's addNextHops rule
//          (:867-872) -- iterated to its fixed point (monotone union over a
//          DAG, so the least fixed point is the Dijkstra result);
//        - the digest delta is summed over D.
//  Teams: a wave per hot failure while |D| fits its scratch (4096 nodes),
//  the rest re-done by whole 1024-thread workgroups with room for all nodes.
//
//  Node failures (spf_whatif_plan_create_nodes) run the same repairs with the
//  failure kind as a compile-time parameter (failed / drain_x below):
//    * DOWN x = runSpf(src, true, linksFromNode(x)): D = the DAG descendants
//      of x, x included (dlist[0] = x); every edge with an end at x is failed,
//      so x gets no seed and no relaxation, stays at kInf and is counted and
//      listed as unreachable.  Cold when x is unreachable in the unfailed run.
//    * DRAIN x = runSpf(src) with x overloaded: D is the same set, and x sits
//      in it (dlist[0] = x) as a node that is reached but never a transit: its
//      tight predecessors are all outside D, so its seed is its unfailed
//      distance and its row its unfailed row -- it contributes nothing to the
//      digest and is never an entry -- while nothing is relaxed out of it and
//      it is nobody's predecessor.  Cold when x is unreachable, drained
//      already, or has no tight out-edge.
//
//  Link sets (spf_whatif_plan_create_sets, shared-risk groups) are the fourth
//  kind: failure i = runSpf(src, true, S_i) for a set S_i of links.  An edge is
//  failed when its link id is a member of S_i, and D = the DAG descendants of
//  several roots, the heads of every tight member (two members with one head
//  claim it once; a root below another root is found marked by the level
//  loop).  The argument above carries over: a node outside D has no tight path
//  through any failed link.  Cold when no member is tight (an empty set, down
//  or non-tight members only).  A single link is a set of one, DOWN x the set
//  linksFromNode(x).
//
//  Link metric changes (spf_whatif_plan_create_metrics: cost-out, undrain) are
//  the fifth kind: change i = (link l, m_lo, m_hi) is runSpf(src) on the graph
//  in which l's two directions weigh m_lo (smaller CSR id -> larger) and m_hi
//  (0 keeps a direction).  Nothing is failed: what changes is what an edge
//  WEIGHS (w_fwd / w_rev below substitute the two new weights wherever a weight
//  of l's two directed edges is read).  One direction at most can matter,
//  because metrics are positive: if u -> v is tight, or becomes useful
//  (d(u) + w' <= d(v)), then d(u) < d(v), and v -> u cannot reach u at or below
//  d(u) whatever it weighs.
//    * cold: l is down; both directions kept or equal to the current metric; a
//      raised direction that is not tight; a lowered u -> v with
//      d(u) + w' > d(v), or u unreachable, or u not expanded (drained, not src).
//    * raise of a tight u -> v: D = the DAG descendants of v, the link plan's D,
//      but the edge stays: it seeds v from u at w'.
//    * lower with d(u) + w' <= d(v): delta = d(v) - d(u) - w' >= 0 (0: a new
//      ECMP tie, distances stay, next hops grow).  No node improves by more
//      than delta.  D grows from v over edges x -> c with
//      d(x) + w(x, c) <= d(c) + delta (unfailed distances on both sides; c
//      reachable and not src, which never changes): a shortest new path from v
//      to a changed node runs through changed nodes only, and each of its edges
//      has slack <= delta.  The set is closed -- a node outside it keeps its
//      distance and its tight predecessors -- and the repair is exact for any
//      D whose complement is unchanged; unchanged nodes of D add nothing to
//      the digest and are no entries.  With delta = 0 the test is the tight
//      test: raises and lowers share one loop, delta a team-uniform scalar.
//  No change alters src's neighbour set or anyone's reachability.
//
//  Digest of a result (same definition in oracle/spf_oracle.cpp):
//    n_dist_changed, n_nh_changed (a node becoming unreachable counts in both)
//    hash = sum over reachable v of mix(mix(v + 1) + d(v)) ^ fnv(nh(v) words)
//  with nh(v) a bitset over the distinct up neighbours of src in the unfailed
//  graph (ascending id).
//
//  This unit holds the unfailed pass, what every plan kind shares on the host
//  (plan_build, execute, changes) and the link kind.  The repairs are
//  whatif_repair.h, their one launch path whatif_plan.h; node, set and metric
//  plans instantiate theirs in whatif_nodes.hip, whatif_sets.hip and
//  whatif_metrics.hip, a code object each.
// ============================================================================
#include "whatif_plan.h"

namespace {

// ---------------------------------------------------------------------------
//  grid-synchronised (XGrid) single-source SSSP and unfailed result
// ---------------------------------------------------------------------------
constexpr int kCoopThreads = 512;  // one block per CU: always co-resident
constexpr uint32_t kCoopHubDeg = 32;  // nodes above this degree get a whole wave

// Grid barrier of the grid-resident kernels, XCD-hierarchical (MI355X_MICROARCH
// barrier-xcd: 4.1 us at 256 workgroups against 26.3 us for the software
// cooperative_groups grid sync, which the what-if base pass crossed ~70
// times).  Blocks are grouped by blockIdx % 8 (the XCD round-robin of the
// dispatcher); each arrival bumps its group's counter, the group's last
// arrival bumps the top counter, waits for every group and publishes the
// generation its group polls.  Counters only grow within a launch (the k-th
// barrier completes at k arrivals per block) and are zeroed before each
// launch (kGridBarWords words, one 128-byte line per counter).
constexpr uint32_t kBarPad = 32;
constexpr uint32_t kGridBarWords = 17 * kBarPad;  // cnt[8], top, gen[8]

struct XGrid {
  uint32_t* bar;
  uint32_t* fault;
  __device__ void sync() const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's stores drained
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t nb = gridDim.x, x = blockIdx.x & 7u;
      const uint32_t nx = (nb - x + 7u) / 8u;  // blocks of this group (>= 1)
      const uint32_t ngroups = nb < 8u ? nb : 8u;
      uint32_t* top = bar + 8 * kBarPad;
      uint32_t* gen = bar + (9 + x) * kBarPad;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const uint32_t t =
          __hip_atomic_fetch_add(bar + x * kBarPad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t g = t / nx + 1;  // the generation this arrival completes
      uint32_t k = 0;
      if (t % nx == nx - 1) {         // last of its group: the group's leader
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (; k < kBarSpin &&
               __hip_atomic_load(top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < g * ngroups;
             ++k) {
          if ((k & 1023u) == 1023u && fault_set(fault)) break;
          __builtin_amdgcn_s_sleep(1);
        }
        __hip_atomic_store(gen, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        for (; k < kBarSpin &&
               __hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < g;
             ++k) {
          if ((k & 1023u) == 1023u && fault_set(fault)) break;
          __builtin_amdgcn_s_sleep(1);
        }
      }
      if (k == kBarSpin) barrier_timed_out(fault);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
  }
};

struct CoopSssp {
  const uint32_t* row_ptr;
  const uint32_t* col;
  const uint32_t* wt;
  const uint8_t* ovl;
  const uint32_t* link;
  const uint32_t* ign;  // optional link bitmap
  uint32_t N, src, hop;
  uint32_t* dist;
  uint32_t* qa;
  uint32_t* qb;
  uint32_t* bm;   // [ceil(N/32)] next-frontier bitmap
  uint32_t* ctr;  // [4] rotating queue lengths + spare
  uint32_t* bar = nullptr;  // [kGridBarWords] XGrid counters, zero at launch
  uint32_t* fault = nullptr;  // the context's barrier-timeout word
};

// Frontier Bellman-Ford over the whole grid: expansion, grid barrier,
// bitmap compaction into the other queue, grid barrier.  Data written by
// other workgroups is read with agent-scope atomics (ld) or atomicExch.
__device__ void coop_sssp(const XGrid& grid, const CoopSssp& a) {
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t gsz = gridDim.x * blockDim.x;  // a multiple of 64
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t bm_words = (a.N + 31) / 32;
  for (uint32_t v = gtid; v < a.N; v += gsz) st(&a.dist[v], v == a.src ? 0u : kInf);
  for (uint32_t i = gtid; i < bm_words; i += gsz) st(&a.bm[i], 0u);
  if (gtid == 0) {
    st(&a.qa[0], a.src);
    st(&a.ctr[0], 1u);
    st(&a.ctr[1], 0u);
    st(&a.ctr[2], 0u);
  }
  grid.sync();
  for (uint32_t it = 0;; ++it) {
    const uint32_t len = ld(&a.ctr[it % 3]);
    if (len == 0) break;
    const uint32_t* cur = (it & 1) ? a.qb : a.qa;
    uint32_t* nxt = (it & 1) ? a.qa : a.qb;
    uint32_t* nctr = &a.ctr[(it + 1) % 3];
    if (gtid == 0) st(&a.ctr[(it + 2) % 3], 0u);  // read last at iteration it - 1
    // wave-uniform sweep over the frontier: a lane expands its own node
    // unless the node is a hub (degree > kCoopHubDeg), whose edges the whole
    // wave then relaxes together -- one thread walking a scale-free hub's
    // thousands of returning atomics serially was the critical path
    auto relax = [&](uint32_t e, uint32_t du) {
      if (a.ign && ((a.ign[a.link[e] >> 5] >> (a.link[e] & 31)) & 1u)) return;
      const uint32_t v = a.col[e];
      const uint32_t nd = du + (a.hop ? 1u : a.wt[e]);
      if (nd < atomicMin(&a.dist[v], nd)) atomicOr(&a.bm[v >> 5], 1u << (v & 31));
    };
    // a wave takes 64 frontier nodes at a time, lanes over their flattened
    // out-edges (wave_edges): a node's relaxations go out 64 at a time
    // instead of one returning atomic after another per lane (a degree-30
    // node was 30 dependent round trips of the iteration's critical path)
    for (uint32_t b = gtid - lane; b < len; b += gsz) {
      const uint32_t i = b + lane;
      uint32_t u = 0, du = 0;
      bool x = false;
      if (i < len) {
        u = ld(&cur[i]);
        x = !a.ovl[u] || u == a.src;  // drained: recorded, not expanded
        if (x) du = ld(&a.dist[u]);
      }
      wave_edges(a.row_ptr, u, x, [&](uint32_t k, uint32_t e, bool act) {
        const uint32_t dk = lane_pull(du, k);
        if (act) relax(e, dk);
      });
    }
    grid.sync();
    for (uint32_t wb = gtid - lane; wb < bm_words; wb += gsz) {  // wave-uniform
      const uint32_t w = wb + lane;
      uint32_t word = w < bm_words ? atomicExch(&a.bm[w], 0u) : 0u;
      // one queue-counter atomic per wave (a returning atomic per word on one
      // counter serialises at ~88 per us)
      const uint32_t cnt = (uint32_t)__popc(word);
      const uint32_t incl = wave_incl_scan32(cnt);
      const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
      if (!total) continue;
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(nctr, total);
      base = __builtin_amdgcn_readlane(base, 0);
      uint32_t at = base + incl - cnt;
      while (word) {
        const uint32_t b = __ffs(word) - 1;
        word &= word - 1;
        st(&nxt[at++], w * 32 + b);
      }
    }
    grid.sync();
  }
}

__global__ __launch_bounds__(kCoopThreads) void gsssp_coop_kernel(CoopSssp a) {
  const XGrid grid{a.bar, a.fault};
  coop_sssp(grid, a);
}

// The unfailed result of a what-if batch in one grid-resident launch:
// SPF, next-hop bitsets in distance order (bucketed by distance value when
// at most kMaxLevels distinct values occur, fixed-point sweeps otherwise),
// result hash.
constexpr uint32_t kLevelCap = 1u << 16;  // distance values bucketed directly
constexpr uint32_t kMaxLevels = 1024;     // non-empty levels worth a barrier each
constexpr uint32_t kLdsHist = 4096;       // distance values a block histograms in LDS

struct BaseArgs {
  CoopSssp sp;
  WiGraph g;
  uint32_t* nhb;        // [N][W]
  uint32_t* lvl;        // [kLevelCap + 1] bucket counts / offsets
  uint32_t* order;      // [N] nodes by distance
  uint32_t* misc;       // [8]: 0 max dist, 1 nonempty levels, 2..4 flags
  unsigned long long* H;
  unsigned long long* prof;  // SPF_WHATIF_PROF: [16] phase clocks of block 0
  uint32_t* parent;     // [N] one tight expanded predecessor (levels path)
  uint32_t* sub;        // [N] subtree sizes of the parent tree, 0 without levels
  unsigned long long* lprof = nullptr;  // SPF_WHATIF_PROF: [2 x 64] per-level clock, size
};

// word j of nh(v) from v's in-edges first, first + stride, ... (a wave
// splits a hub's edges over its lanes and ORs the parts)
__device__ __forceinline__ uint32_t nh_word(const WiGraph& g, const uint32_t* dist,
                                            const uint32_t* nhb, uint32_t v, uint32_t j,
                                            uint32_t first = 0, uint32_t stride = 1) {
  // edges in groups of 4, each stage's loads issued together: the column and
  // reverse-edge ids, then the tails' distances / drain bytes / metrics, then
  // the tight tails' words -- three memory round trips per group where an
  // edge-at-a-time loop made three per edge
  const uint32_t dv = dist[v];
  uint32_t acc = 0;
  const uint32_t e1 = g.row_ptr[v + 1];
  for (uint32_t e = g.row_ptr[v] + first; e < e1; e += 4 * stride) {
    uint32_t u[4], r[4], du[4], w[4], x[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t ek = e + k * stride;
      ok[k] = ek < e1;
      u[k] = ok[k] ? g.col[ek] : 0u;
      r[k] = ok[k] && !g.hop ? g.rev[ek] : 0u;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      du[k] = ok[k] ? ld(&dist[u[k]]) : kInf;
      w[k] = ok[k] ? (g.hop ? 1u : g.wt[r[k]]) : 0u;
      if (ok[k] && g.ovl[u[k]] && u[k] != g.src) du[k] = kInf;  // drained: not expanded
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = 0;
      if (du[k] != kInf && du[k] + w[k] == dv) {
        if (u[k] == g.src) {
          const uint32_t jb = g.nbr_bit[v];
          if ((jb >> 5) == j) x[k] = 1u << (jb & 31);
        } else {
          x[k] = ld(&nhb[(size_t)u[k] * g.W + j]);
        }
      }
    }
    acc |= x[0] | x[1] | x[2] | x[3];
  }
  return acc;
}

// nh(v) of a hub by one wave: lanes test v's in-edges 64 at a time, then
// every tight predecessor's W words are ORed in with lane = word (a (v, j)
// item per thread would rescan the hub's edges W times)
__device__ void hub_nh(const WiGraph& g, const uint32_t* dist, uint32_t* nhb, uint32_t* parent,
                       uint32_t v, uint32_t lane) {
  const uint32_t dv = dist[v], W = g.W;
  const uint32_t e0 = g.row_ptr[v], e1 = g.row_ptr[v + 1];
  bool have_parent = false;
  for (uint32_t j0 = 0; j0 < W; j0 += 64) {
    const uint32_t j = j0 + lane;
    uint32_t acc = 0;
    // 4 chunks of 64 in-edges per pass, each stage's loads issued together
    // (ids, then the tails' distances / drains / metrics): a hub's scan was
    // one dependent round trip chain per 64 edges and set its level's time
    for (uint32_t eb4 = e0; eb4 < e1; eb4 += 256) {
    uint32_t cu4[4], r4[4], u4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t e = eb4 + q * 64 + lane;
      cu4[q] = e < e1 ? g.col[e] : kInf;
      r4[q] = e < e1 && !g.hop ? g.rev[e] : 0u;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u4[q] = kInf;
      if (cu4[q] != kInf) {
        const uint32_t cu = cu4[q];
        const uint32_t du = ld(&dist[cu]);
        const uint32_t w = g.hop ? 1u : g.wt[r4[q]];
        if ((!g.ovl[cu] || cu == g.src) && du != kInf && du + w == dv) u4[q] = cu;
      }
    }
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {  // chunks in CSR order: the first tight tail is the parent
      const uint32_t u = u4[c4];
      const uint64_t tight = __ballot(u != kInf);
      if (tight && !have_parent) {  // wave-uniform
        have_parent = true;
        const uint32_t first = __builtin_amdgcn_readlane(u, __builtin_ctzll(tight));
        if (lane == 0) st(&parent[v], first);
      }
      // the tight tails' words 8 at a time, their loads issued together
      for (uint64_t t = tight; t;) {
        uint32_t tu[8], x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          tu[q] = kInf;
          if (t) {  // wave-uniform
            tu[q] = __builtin_amdgcn_readlane(u, __builtin_ctzll(t));
            t &= t - 1;
          }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
          x[q] = tu[q] != kInf && tu[q] != g.src && j < W ? ld(&nhb[(size_t)tu[q] * W + j]) : 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          acc |= x[q];
          if (tu[q] == g.src) {
            const uint32_t jb = g.nbr_bit[v];
            if (j == (jb >> 5)) acc |= 1u << (jb & 31);
          }
        }
      }
    }
    }
    if (j < W) st(&nhb[(size_t)v * W + j], acc);
  }
}

// nh(v) and parent[v] of a non-hub node (degree <= kCoopHubDeg) by a
// segment of S lanes (S = a power of two >= min(W, 64), 64 / S nodes per
// wave, segment-uniform call): lane l of the segment tests in-edges l, l + S,
// ... once, then every tight tail's words are ORed in with lane = word.  An
// item per (v, word) instead rescans v's in-edges W times (what-if base:
// W = 31, next hops 4.3 ms of the 5.7 ms pass, r02_v61).
__device__ void seg_nh(const WiGraph& g, const uint32_t* dist, uint32_t* nhb, uint32_t* parent,
                       uint32_t v, uint32_t S, uint32_t lane) {
  const uint32_t sl = lane & (S - 1), base = lane - sl;
  const uint64_t segmask = (S == 64 ? ~0ull : ((1ull << S) - 1ull)) << base;
  const uint32_t dv = ld(&dist[v]), W = g.W;
  const uint32_t e0 = g.row_ptr[v], e1 = g.row_ptr[v + 1];
  bool have_parent = false;
  for (uint32_t j0 = 0; j0 < W; j0 += S) {
    const uint32_t j = j0 + sl;
    uint32_t acc = 0;
    for (uint32_t eb = e0; eb < e1; eb += S) {  // segment-uniform
      const uint32_t e = eb + sl;
      uint32_t u = kInf;
      if (e < e1) {
        const uint32_t cu = g.col[e];
        const uint32_t du = ld(&dist[cu]);
        const uint32_t w = g.hop ? 1u : g.wt[g.rev[e]];
        if ((!g.ovl[cu] || cu == g.src) && du != kInf && du + w == dv) u = cu;
      }
      uint64_t tight = __ballot(u != kInf) & segmask;
      if (tight && !have_parent) {  // segment-uniform: CSR order, first tight tail
        have_parent = true;
        const uint32_t first = __shfl(u, __builtin_ctzll(tight), 64);
        if (sl == 0) st(&parent[v], first);
      }
      while (tight) {  // the tight tails' words, 4 loads in flight
        uint32_t tu[4], x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          tu[q] = kInf;
          if (tight) {
            tu[q] = __shfl(u, __builtin_ctzll(tight), 64);
            tight &= tight - 1;
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          x[q] = tu[q] != kInf && tu[q] != g.src && j < W ? ld(&nhb[(size_t)tu[q] * W + j]) : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc |= x[q];
          if (tu[q] == g.src) {
            const uint32_t jb = g.nbr_bit[v];
            if (j == (jb >> 5)) acc |= 1u << (jb & 31);
          }
        }
      }
    }
    if (j < W) st(&nhb[(size_t)v * W + j], acc);
  }
  if (!have_parent && sl == 0) st(&parent[v], kInf);
}

// Next-hop bitsets nhb[v][W] of the SPF in `dist` (every distance final,
// after coop_sssp): nodes bucketed by distance value and settled level by
// level (every tight predecessor of a level-d node sits at a lower level)
// when at most kMaxLevels distinct values occur, fixed-point sweeps of the
// monotone union otherwise.  nhb must be zero and lvl[0..kLevelCap],
// misc[0..7] zero on entry.  Returns whether the level path ran (then
// lvl[d] = end of bucket d in `order`).  Starts and ends with a grid barrier.
__device__ bool level_nh(const XGrid& grid, const WiGraph& g, const uint32_t* dist,
                         uint32_t* nhb, uint32_t* lvl, uint32_t* order, uint32_t* misc,
                         uint32_t* parent, unsigned long long* lstamp = nullptr) {
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t gsz = gridDim.x * blockDim.x;  // a multiple of 64
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t N = g.N, W = g.W;
  const uint64_t NW = (uint64_t)N * W;
  // per-block histogram of the distance values and the block's write
  // cursors into `order` (LDS, when maxd < kLdsHist): one global atomic per
  // (block, value) instead of one per node -- 250k node atomics on ~30
  // counters (and on one for the maximum) were 1.6 ms of the what-if base
  // pass's 2.4 ms next-hop phase (per-level clocks, r05_wb)
  __shared__ uint32_t bh[kLdsHist], bc[kLdsHist];
  grid.sync();
  // ---- distance range (one atomic per wave) and per-value counts ----
  {
    uint32_t m = 0;
    for (uint32_t v = gtid; v < N; v += gsz) {
      const uint32_t d = ld(&dist[v]);
      if (d != kInf) m = max(m, d);
    }
    m = wave_max32(m);
    if (lane == 0 && m) atomicMax(&misc[0], m);
  }
  grid.sync();
  const uint32_t maxd = ld(&misc[0]);
  bool levels = maxd < kLevelCap;
  const bool hist = maxd < kLdsHist;  // block-uniform
  if (levels) {
    if (hist) {
      for (uint32_t i = threadIdx.x; i <= maxd; i += blockDim.x) bh[i] = 0u;
      __syncthreads();
      for (uint32_t v = gtid; v < N; v += gsz) {
        const uint32_t d = ld(&dist[v]);
        if (d != kInf) atomicAdd(&bh[d], 1u);
      }
      __syncthreads();
      for (uint32_t i = threadIdx.x; i <= maxd; i += blockDim.x)
        if (bh[i] && atomicAdd(&lvl[i], bh[i]) == 0) atomicAdd(&misc[1], 1u);
    } else {
      for (uint32_t v = gtid; v < N; v += gsz) {
        const uint32_t d = ld(&dist[v]);
        if (d != kInf && atomicAdd(&lvl[d], 1u) == 0) atomicAdd(&misc[1], 1u);
      }
    }
    grid.sync();
    levels = ld(&misc[1]) <= kMaxLevels;
  }
  if (levels) {
    // exclusive scan of the counts by block 0 (maxd + 1 <= kLevelCap entries)
    if (blockIdx.x == 0) {
      __shared__ uint32_t carry;
      if (threadIdx.x == 0) carry = 0;
      __syncthreads();
      for (uint32_t base = 0; base <= maxd; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i <= maxd ? ld(&lvl[i]) : 0u;
        // block scan through LDS
        __shared__ uint32_t buf[kCoopThreads];
        buf[threadIdx.x] = x;
        __syncthreads();
        for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
          const uint32_t y = threadIdx.x >= d ? buf[threadIdx.x - d] : 0u;
          __syncthreads();
          buf[threadIdx.x] += y;
          __syncthreads();
        }
        const uint32_t incl = buf[threadIdx.x] + carry;
        if (i <= maxd) st(&lvl[i], incl - x);
        __syncthreads();
        if (threadIdx.x == blockDim.x - 1) carry = incl;
        __syncthreads();
      }
      if (threadIdx.x == 0) st(&lvl[maxd + 1], carry);
    }
    grid.sync();
    // scatter nodes into distance order (lvl[d] advances to the bucket end):
    // with the block histogram, one global atomic per (block, value)
    // reserves the block's range, LDS cursors place its nodes
    if (hist) {
      for (uint32_t i = threadIdx.x; i <= maxd; i += blockDim.x)
        if (bh[i]) bc[i] = atomicAdd(&lvl[i], bh[i]);
      __syncthreads();
      for (uint32_t v = gtid; v < N; v += gsz) {
        const uint32_t d = ld(&dist[v]);
        if (d != kInf) st(&order[atomicAdd(&bc[d], 1u)], v);
      }
    } else {
      for (uint32_t v = gtid; v < N; v += gsz) {
        const uint32_t d = ld(&dist[v]);
        if (d != kInf) st(&order[atomicAdd(&lvl[d], 1u)], v);
      }
    }
    grid.sync();
    // level by level: every predecessor of a level-d node sits at a lower level
    uint32_t begin = ld(&lvl[0]);  // bucket 0 (the source) ends here
    for (uint32_t d = 1; d <= maxd; ++d) {
      const uint32_t end = ld(&lvl[d]);
      if (end == begin) continue;  // empty level: uniform skip
      const uint32_t n_lvl = end - begin;
      // 64 / S nodes per wave, a segment of S lanes each (seg_nh)
      const uint32_t S = W <= 16 ? 16u : (W <= 32 ? 32u : 64u);
      const uint32_t per_wave = 64 / S, seg = lane / S;
      const uint32_t waves = gsz / 64, wave = gtid / 64;
      for (uint32_t wb = wave * per_wave; wb < n_lvl; wb += waves * per_wave) {  // wave-uniform
        const uint32_t i = wb + seg;
        uint32_t v = 0;
        bool hub = false;
        if (i < n_lvl) {
          v = ld(&order[begin + i]);
          hub = g.row_ptr[v + 1] - g.row_ptr[v] > kCoopHubDeg;
          if (!hub) seg_nh(g, dist, nhb, parent, v, S, lane);  // segment-uniform
        }
        // a hub's W words are made once, by the whole wave
        for (uint64_t hubs = __ballot(hub && (lane & (S - 1)) == 0); hubs; hubs &= hubs - 1)
          hub_nh(g, dist, nhb, parent, __builtin_amdgcn_readlane(v, __builtin_ctzll(hubs)), lane);
      }
      begin = end;
      grid.sync();
      // diagnostics (SPF_WHATIF_PROF): the clock after level d, its size
      if (lstamp && gtid == 0 && d < 64) {
        lstamp[2 * d] = wall_clock64();
        lstamp[2 * d + 1] = n_lvl;
      }
    }
  } else {
    // fixed-point sweeps (monotone union over the DAG), flags rotate by 3
    for (uint32_t it = 0;; ++it) {
      bool any = false;
      for (uint64_t x = gtid; x < NW; x += gsz) {
        const uint32_t v = (uint32_t)(x / W), j = (uint32_t)(x % W);
        if (v == g.src || ld(&dist[v]) == kInf) continue;
        const uint32_t acc = nh_word(g, dist, nhb, v, j);
        if (acc != ld(&nhb[x])) {
          st(&nhb[x], acc);
          any = true;
        }
      }
      if (any) st(&misc[2 + it % 3], 1u);
      if (gtid == 0) st(&misc[2 + (it + 1) % 3], 0u);
      grid.sync();
      if (!ld(&misc[2 + it % 3])) break;
    }
  }
  grid.sync();
  return levels;
}

__global__ __launch_bounds__(kCoopThreads) void whatif_base_kernel(BaseArgs a) {
  const XGrid grid{a.sp.bar, a.sp.fault};
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t gsz = gridDim.x * blockDim.x;  // a multiple of 64
  const WiGraph& g = a.g;
  const uint32_t N = g.N, W = g.W;
  const uint64_t NW = (uint64_t)N * W;
  for (uint64_t x = gtid; x < NW; x += gsz) st(&a.nhb[x], 0u);
  for (uint32_t i = gtid; i <= kLevelCap; i += gsz) st(&a.lvl[i], 0u);
  for (uint32_t v = gtid; v < N; v += gsz) st(&a.sub[v], 0u);
  if (gtid == 0) {
    for (int i = 0; i < 8; ++i) st(&a.misc[i], 0u);
    *a.H = 0;
  }
  const bool stamp = a.prof && gtid == 0;
  if (stamp) a.prof[0] = wall_clock64();
  coop_sssp(grid, a.sp);  // starts and ends with a grid barrier
  if (stamp) a.prof[1] = wall_clock64();
  const uint32_t* dist = a.sp.dist;
  const bool levels = level_nh(grid, g, dist, a.nhb, a.lvl, a.order, a.misc, a.parent, a.lprof);
  if (stamp) a.prof[6] = wall_clock64();
  if (levels) {
    const uint32_t maxd = ld(&a.misc[0]);
    // subtree sizes of the parent tree, deepest level first: a lower bound
    // on the DAG descendants a failure of the tree edge into v can change,
    // used to hand big repairs to workgroup teams up front
    for (uint32_t v = gtid; v < N; v += gsz)
      if (ld(&dist[v]) != kInf) atomicAdd(&a.sub[v], 1u);
    grid.sync();
    for (uint32_t d = maxd; d >= 1; --d) {
      const uint32_t lo = ld(&a.lvl[d - 1]), hi = ld(&a.lvl[d]);
      if (lo == hi) continue;  // empty level: uniform skip
      for (uint32_t x = lo + gtid; x < hi; x += gsz) {
        const uint32_t v = ld(&a.order[x]);
        const uint32_t pu = ld(&a.parent[v]);
        if (pu != kInf) atomicAdd(&a.sub[pu], ld(&a.sub[v]));
      }
      grid.sync();
    }
  }
  if (stamp) {
    a.prof[2] = wall_clock64();
    a.prof[4] = ld(&a.misc[0]);
    a.prof[5] = ld(&a.misc[1]);
  }
  // ---- result hash ----
  uint64_t h = 0;
  for (uint32_t v = gtid; v < N; v += gsz) {
    const uint32_t d = ld(&dist[v]);
    if (d == kInf) continue;
    uint64_t f = 0xcbf29ce484222325ull;
    for (uint32_t w = 0; w < W; ++w) {
      f ^= ld(&a.nhb[(size_t)v * W + w]);
      f *= 0x100000001b3ull;
    }
    h += mix64(mix64((uint64_t)v + 1) + d) ^ f;
  }
  uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
  for (int d = 32; d >= 1; d >>= 1) {  // wave sum, one atomic per wave
    const uint32_t l2 = __shfl_down(lo, d, 64), h2 = __shfl_down(hi, d, 64);
    const uint64_t t = ((uint64_t)hi << 32 | lo) + ((uint64_t)h2 << 32 | l2);
    lo = (uint32_t)t;
    hi = (uint32_t)(t >> 32);
  }
  if ((threadIdx.x & 63) == 0 && (lo | hi)) atomicAdd(a.H, ((unsigned long long)hi << 32) | lo);
  if (stamp) a.prof[3] = wall_clock64();
}

// ---------------------------------------------------------------------------
//  batched SPF + next hops beyond the LDS-resident kernels (plans on graphs
//  too large for them, positive metrics or hop counts)
// ---------------------------------------------------------------------------
// One grid-resident launch walks the plan's sources one after another, the
// whole chip on each: frontier SSSP straight into the source's output row
// (coop_sssp), next hops per node in distance order (level_nh, node-major
// scratch nhb[v][W]), then a transpose into the plan's bitmap layout (bit v
// of word v/32 of neighbour j's bitmap): a wave holds the scratch word w of
// 64 consecutive nodes, one ballot per bit j of it is the 64-node slice of
// bitmap 32w + j, and lanes 0..31 store the 32 slices as 8-byte words.
struct BigArgs {
  CoopSssp sp;  // src and dist set per source
  WiGraph g;    // src, W set per source; g.nbr_bit = nbr_bit below
  const uint32_t* srcs;
  uint32_t n_src;
  const uint32_t* nb_ptr;  // distinct up neighbours (ascending id)
  const uint32_t* nb_id;
  uint32_t* D;  // [n_src][pitch] output rows
  uint32_t pitch;
  uint32_t* nh;  // output bitmaps
  const uint64_t* nh_off;
  uint32_t* nbr_bit;  // [N] scratch, kInf between sources
  uint32_t* nhb;      // [N][W] scratch
  uint32_t* lvl;      // [kLevelCap + 1]
  uint32_t* order;    // [N]
  uint32_t* misc;     // [8]
  uint32_t* parent;   // [N]
};

__global__ __launch_bounds__(kCoopThreads) void spf_big_kernel(BigArgs a) {
  const XGrid grid{a.sp.bar, a.sp.fault};
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t gsz = gridDim.x * blockDim.x;  // a multiple of 64
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t N = a.g.N, wpm = a.pitch / 32;
  for (uint32_t i = 0; i < a.n_src; ++i) {
    const uint32_t s = a.srcs[i];
    const uint32_t nb0 = a.nb_ptr[s], k = a.nb_ptr[s + 1] - nb0;
    const uint32_t W = k ? (k + 31) / 32 : 1u;
    WiGraph g = a.g;
    g.src = s;
    g.W = W;
    CoopSssp sp = a.sp;
    sp.src = s;
    sp.dist = a.D + (size_t)i * a.pitch;
    // per-source state (the previous source's readers finished at its last barrier)
    for (uint32_t j = gtid; j < k; j += gsz) st(&a.nbr_bit[a.nb_id[nb0 + j]], j);
    const uint64_t NW = (uint64_t)N * W;
    for (uint64_t x = gtid; x < NW; x += gsz) st(&a.nhb[x], 0u);
    for (uint32_t d = gtid; d <= kLevelCap; d += gsz) st(&a.lvl[d], 0u);
    if (gtid < 8) st(&a.misc[gtid], 0u);
    for (uint32_t v = N + gtid; v < a.pitch; v += gsz) st(&sp.dist[v], kInf);  // row padding
    coop_sssp(grid, sp);  // starts and ends with a grid barrier
    level_nh(grid, g, sp.dist, a.nhb, a.lvl, a.order, a.misc, a.parent);
    // transpose into the plan's bitmaps: items (64-node group, scratch word)
    if (k) {
      uint32_t* out = a.nh + a.nh_off[i];
      const uint32_t groups = a.pitch / 64;
      const uint64_t items = (uint64_t)groups * W;
      for (uint64_t t = (gtid >> 6); t < items; t += gsz / 64) {  // a wave per item
        const uint32_t grp = (uint32_t)(t / W), w = (uint32_t)(t % W);
        const uint32_t v = grp * 64 + lane;
        const uint32_t x = v < N ? ld(&a.nhb[(size_t)v * W + w]) : 0u;
        uint64_t mine = 0;
#pragma unroll 4
        for (uint32_t jj = 0; jj < 32; ++jj) {
          const uint64_t m = __ballot((x >> jj) & 1u);
          if (lane == jj) mine = m;
        }
        const uint32_t j = w * 32 + lane;
        if (lane < 32 && j < k) {
          uint2* o = reinterpret_cast<uint2*>(out + (size_t)j * wpm + grp * 2);
          *o = make_uint2((uint32_t)mine, (uint32_t)(mine >> 32));
        }
      }
    }
    for (uint32_t j = gtid; j < k; j += gsz) st(&a.nbr_bit[a.nb_id[nb0 + j]], kInf);
    grid.sync();
  }
}

// ---------------------------------------------------------------------------
//  classify failures: cold -> digest now, hot -> work list (failure, edge)
// ---------------------------------------------------------------------------
__global__ void classify_kernel(WiGraph g, const uint32_t* __restrict__ dist,
                                const unsigned long long* __restrict__ H,
                                const uint32_t* __restrict__ fails, uint32_t n_fail,
                                const uint32_t* __restrict__ link_edge,
                                const uint32_t* __restrict__ sub, uint32_t wave_cap,
                                spf_whatif_digest* out, uint2* hot, uint32_t* n_hot,
                                uint2* big, uint32_t* n_big) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_fail) return;
  const uint32_t e0 = link_edge[fails[f]];
  uint32_t tight = kInf;
  if (e0 != kInf) {
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t e = k ? g.rev[e0] : e0;
      const uint32_t a = g.col[g.rev[e]], b = g.col[e];  // a -> b
      if (g.ovl[a] && a != g.src) continue;
      if (dist[a] != kInf && dist[a] + g.wt[e] == dist[b]) tight = e;
    }
  }
  if (tight == kInf) {
    out[f] = spf_whatif_digest{0u, 0u, (uint64_t)*H};
  } else if (sub[g.col[tight]] > wave_cap) {  // |D| >= subtree: a workgroup's repair
    big[atomicAdd(n_big, 1u)] = make_uint2(f, tight);
  } else {
    hot[atomicAdd(n_hot, 1u)] = make_uint2(f, tight);
  }
}

// cptr[0 .. n] = exclusive scan of the failures' entry counts, cptr[n] the
// total: one workgroup, 8 counts per thread and tile, the per-thread sums
// scanned with the DPP wave scans (a sum < 2^35 as two words of 24 and 11
// bits: 64 of either stay below 2^32), u64 offsets.  Count t is cnt[t *
// STRIDE]: 1 for the lists' own arrays, 8 for the counts inside the impact
// summaries (spfi::whatif_scan).
constexpr uint32_t kListScanPer = 8;
static_assert(1024 * kListScanPer == spfi::kWhatifScanTile, "the tile the tests cross");
template <uint32_t STRIDE>
__global__ __launch_bounds__(1024) void whatif_scan_kernel(const uint32_t* __restrict__ cnt,
                                                           uint32_t n,
                                                           unsigned long long* __restrict__ cptr) {
  __shared__ unsigned long long s_wave[16];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (uint64_t t0 = 0; t0 < n; t0 += 1024ull * kListScanPer) {  // block-uniform
    const uint64_t b = t0 + (uint64_t)threadIdx.x * kListScanPer;
    uint32_t x[kListScanPer];
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kListScanPer; ++j) {
      x[j] = b + j < n ? cnt[(b + j) * STRIDE] : 0u;
      sum += x[j];
    }
    uint32_t tl = 0, th = 0;
    const uint32_t el = wave_excl_scan((uint32_t)sum & 0xFFFFFFu, &tl);
    const uint32_t eh = wave_excl_scan((uint32_t)(sum >> 24), &th);
    if (lane == 0) s_wave[wv] = tl + ((unsigned long long)th << 24);
    __syncthreads();
    unsigned long long run = carry + el + ((unsigned long long)eh << 24);
    for (uint32_t w = 0; w < 16; ++w) {
      const unsigned long long t = s_wave[w];
      if (w < wv) run += t;
      carry += t;
    }
#pragma unroll
    for (uint32_t j = 0; j < kListScanPer; ++j) {
      if (b + j < n) cptr[b + j] = run;
      run += x[j];
    }
    __syncthreads();  // s_wave is rewritten by the next tile
  }
  if (threadIdx.x == 0) cptr[n] = carry;
}

__global__ void base_digest_kernel(spf_whatif_digest* o, const unsigned long long* H) {
  *o = spf_whatif_digest{0u, 0u, (uint64_t)*H};
}

}  // namespace

namespace spfi {

// A launch whose blocks meet at barriers (XGrid, the group teams'
// team_sync): a regular launch of at most `per_cu` blocks per CU, checked
// against the occupancy calculator so that every block of the grid fits on
// the chip at once -- the barriers' precondition, which the cooperative
// launch used to assert.  Blocks of other kernels running beside it (the
// wave teams) never wait on it, so its blocks all become resident.  (The
// cooperative launch is not used: under rocprofv3 a process that made one
// faulted in exit-time runtime teardown)
hipError_t launch_resident(const void* kernel, uint32_t blocks, uint32_t threads, void** args,
                           uint32_t n_cu, hipStream_t s) {
  int fit = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kernel, threads, 0);
  if (e != hipSuccess) return e;
  if (fit < 1 || (uint64_t)fit * n_cu < blocks) return hipErrorCooperativeLaunchTooLarge;
  return hipLaunchKernel(kernel, dim3(blocks), dim3(threads), args, 0, s);
}

hipError_t whatif_scan(const uint32_t* cnt, uint32_t stride, uint32_t n, unsigned long long* ptr,
                       hipStream_t s) {
  if (stride == 1) hipLaunchKernelGGL(whatif_scan_kernel<1>, dim3(1), dim3(1024), 0, s, cnt, n, ptr);
  else if (stride == 8) hipLaunchKernelGGL(whatif_scan_kernel<8>, dim3(1), dim3(1024), 0, s, cnt, n, ptr);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

void whatif_lists_view(spf_whatif_plan* p, WiListsView* v) {
  const spf_ctx* c = p->ctx;
  v->ctx = p->ctx;
  v->rt = &p->rt;
  v->imp[SPF_WHATIF_BY_NODE] = &p->imp_node;
  v->imp[SPF_WHATIF_BY_SET] = &p->imp_set;
  v->up = &p->up;
  v->kind = p->kind;
  v->exact = p->exact != nullptr;
  v->fails = p->d_fails.p;
  v->set_links = p->d_set_links.p;
  v->met = p->d_met.p;
  v->nbr_bit = p->d_nbr_bit.p;
  v->changes = &p->lists;
  v->no_nbr = p->src + 1 < c->nb_ptr.size() && c->nb_ptr[p->src + 1] == c->nb_ptr[p->src];
  v->epoch = p->epoch;
  v->src = p->src;
  v->n_fail = p->n_fail;
  v->W = p->W;
  v->base_d32 = p->exact ? nullptr : p->d_dist.p;
  v->base_d64 = p->exact ? p->exact->base_d.p : nullptr;
  v->base_nh = p->exact ? p->exact->base_nh.p : p->d_nhb.p;
}

// Blocks of a grid-barrier launch: `per_cu` 512-thread blocks per CU, clamped
// to what the occupancy calculator says stays co-resident (XGrid needs every
// block resident).  SPF_COOP_PER_CU overrides (A/B).
uint32_t coop_blocks(spf_ctx* c, const void* kernel, uint32_t per_cu) {
  if (const char* e = std::getenv("SPF_COOP_PER_CU")) per_cu = std::max(1, atoi(e));
  int fit = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kernel, kCoopThreads, 0) != hipSuccess ||
      fit < 1) {
    (void)hipGetLastError();
    fit = 1;
  }
  return c->n_cu * std::min<uint32_t>(per_cu, (uint32_t)fit);
}

spf_status launch_gsssp(spf_ctx* c, uint32_t src, bool hop, const uint32_t* ign, uint32_t* dist,
                        hipStream_t s) {
  const uint32_t N = c->N;
  HIP_TRY(c, c->d_gq.alloc(N));
  HIP_TRY(c, c->d_gq2.alloc(N));
  HIP_TRY(c, c->d_gbm.alloc((N + 31) / 32));
  HIP_TRY(c, c->d_gctr.alloc(4));
  HIP_TRY(c, c->d_gbar.alloc(kGridBarWords));
  HIP_TRY(c, hipMemsetAsync(c->d_gbar.p, 0, 4 * kGridBarWords, s));
  CoopSssp a{c->d_row_ptr.p, c->d_col.p, c->d_wt.p, c->d_ovl.p, c->d_link.p, ign, N, src,
             hop ? 1u : 0u, dist, c->d_gq.p, c->d_gq2.p, c->d_gbm.p, c->d_gctr.p};
  a.bar = c->d_gbar.p;
  a.fault = c->d_fault.p;
  void* args[] = {&a};
  if (const spf_status st = resident_order(c, s); st != SPF_OK) return st;
  HIP_TRY(c, launch_resident((const void*)gsssp_coop_kernel,
                             coop_blocks(c, (const void*)gsssp_coop_kernel, 1), kCoopThreads, args,
                             c->n_cu, s));
  return resident_done(c, s);
}

spf_status launch_big(spf_ctx* c, spf_plan* p, uint32_t* d_dist, uint32_t* d_nh, bool hop,
                      hipStream_t s) {
  const uint32_t N = c->N;
  HIP_TRY(c, p->b_q.alloc(N));
  HIP_TRY(c, p->b_q2.alloc(N));
  HIP_TRY(c, p->b_bm.alloc((N + 31) / 32));
  HIP_TRY(c, p->b_ctr.alloc(4));
  HIP_TRY(c, p->b_bar.alloc(kGridBarWords));
  HIP_TRY(c, hipMemsetAsync(p->b_bar.p, 0, 4 * kGridBarWords, s));
  if (!p->b_nbr_bit.p) {
    HIP_TRY(c, p->b_nbr_bit.alloc(N));
    HIP_TRY(c, hipMemsetAsync(p->b_nbr_bit.p, 0xFF, 4ull * N, s));
  }
  HIP_TRY(c, p->b_nhb.alloc((size_t)N * p->wmax));
  HIP_TRY(c, p->b_lvl.alloc(kLevelCap + 1));
  HIP_TRY(c, p->b_order.alloc(N));
  HIP_TRY(c, p->b_misc.alloc(8));
  HIP_TRY(c, p->b_parent.alloc(N));
  WiGraph g{c->d_row_ptr.p, c->d_col.p, c->d_wt.p, c->d_rev.p, c->d_link.p, c->d_ovl.p,
            p->b_nbr_bit.p, N, 0u, 1u, hop ? 1u : 0u, c->d_fault.p};
  BigArgs a{CoopSssp{c->d_row_ptr.p, c->d_col.p, c->d_wt.p, c->d_ovl.p, c->d_link.p, nullptr, N,
                     0u, hop ? 1u : 0u, d_dist, p->b_q.p, p->b_q2.p, p->b_bm.p, p->b_ctr.p},
            g, p->d_srcs.p, p->n_src, c->d_nb_ptr.p, c->d_nb_id.p, d_dist, c->pitch, d_nh,
            p->d_nh_off.p, p->b_nbr_bit.p, p->b_nhb.p, p->b_lvl.p, p->b_order.p, p->b_misc.p,
            p->b_parent.p};
  a.sp.bar = p->b_bar.p;
  a.sp.fault = c->d_fault.p;
  void* args[] = {&a};
  if (const spf_status st = resident_order(c, s); st != SPF_OK) return st;
  HIP_TRY(c, launch_resident((const void*)spf_big_kernel,
                             coop_blocks(c, (const void*)spf_big_kernel, 1), kCoopThreads, args,
                             c->n_cu, s));
  return resident_done(c, s);
}

}  // namespace spfi

namespace {

// SPF_WHATIF_PROF: unset 0 (production instances), "global" 2 (per-event
// global read-modify-writes), anything else 1 (register counters)
int whatif_prof_mode() {
  const char* e = std::getenv("SPF_WHATIF_PROF");
  return !e ? 0 : (std::strcmp(e, "global") == 0 ? 2 : 1);
}

spf_status run_base(spf_whatif_plan* p, const WiGraph& g, hipStream_t s) {
  spf_ctx* c = p->ctx;
  const uint32_t N = c->N;
  // 1. unfailed SPF, next hops, hash: one grid-resident launch
  {
    BaseArgs a{CoopSssp{c->d_row_ptr.p, c->d_col.p, c->d_wt.p, c->d_ovl.p, c->d_link.p, nullptr,
                        N, p->src, 0u, p->d_dist.p, p->d_q.p, p->d_q2.p, p->d_bm.p, p->d_ctr.p},
               g, p->d_nhb.p, p->d_lvl.p, p->d_order.p, p->d_misc.p, p->d_H.p,
               p->d_prof.p ? p->d_prof.p + 16ull * p->big_teams : nullptr, p->d_parent.p,
               p->d_sub.p};
    a.sp.bar = p->d_bar.p;
    a.sp.fault = c->d_fault.p;
    if (p->d_prof.p) a.lprof = p->d_prof.p + 16ull * (p->big_teams + 1 + p->wave_teams);
    HIP_TRY(c, hipMemsetAsync(p->d_bar.p, 0, 4 * kGridBarWords, s));
    void* args[] = {&a};
    if (const spf_status st = resident_order(c, s); st != SPF_OK) return st;
    HIP_TRY(c, launch_resident((const void*)whatif_base_kernel,
                               coop_blocks(c, (const void*)whatif_base_kernel, 1), kCoopThreads,
                               args, c->n_cu, s));
    if (const spf_status st = resident_done(c, s); st != SPF_OK) return st;
  }
  return SPF_OK;
}

// Link plans: work items (failure, tight edge), sorted by the parent subtree
// of the edge's head; the only kind with profiled instances.
struct LinkKind {
  static constexpr int kKind = kLink;
  static constexpr bool kProfiled = true;
  static constexpr const char* kDebugName = "";
  static constexpr const char* kPlanName = "a link plan (spf_whatif_plan_links)";
  static std::tuple<> table(const spf_whatif_plan*) { return {}; }
  static void classify(spf_whatif_plan* p, const WiGraph& g, spf_whatif_digest* d_out, hipStream_t s) {
    hipLaunchKernelGGL(classify_kernel, dim3((p->n_fail + 255) / 256), dim3(256), 0, s, g,
                       p->d_dist.p, p->d_H.p, p->d_fails.p, p->n_fail, p->d_link_edge.p,
                       p->d_sub.p, p->classify_cap, d_out, p->d_hot.p, p->d_cnt.p, p->d_big0.p,
                       p->d_cnt.p + 3);
  }
  using SortKey = KeySubOfHead;
  static SortKey sort_key(const spf_whatif_plan* p) { return {p->d_sub.p, p->ctx->d_col.p}; }
};

}  // namespace

namespace spfi {

const WiKindOps kLinkOps = kind_ops_of<LinkKind>();

const WiKindOps& kind_ops(uint32_t kind) {
  static const WiKindOps* const ops[] = {&kLinkOps, &kDownOps, &kDrainOps, &kSetOps, &kMetricOps};
  static_assert(kLink == 0 && sizeof ops / sizeof *ops == kMetric + 1, "indexed by the plan's kind");
  assert(kind <= (uint32_t)kMetric);  // (a plan's kind is set by its create call)
  return *ops[kind];
}

spf_status create_prologue(spf_ctx* c, spf_whatif_plan** out, uint32_t src, const char* who) {
  if (!c || !out) return fail(c, SPF_E_INVALID, "%s: NULL argument", who);
  *out = nullptr;
  if (!c->loaded) return fail(c, SPF_E_STATE, "no graph loaded");
  if (src >= c->N) return fail(c, SPF_E_INVALID, "source %u out of range", src);
  return SPF_OK;
}

std::unique_ptr<spf_whatif_plan> new_plan(spf_ctx* c, uint32_t src, uint32_t kind, uint32_t n_fail) {
  auto p = std::make_unique<spf_whatif_plan>();
  p->ctx = c;
  p->src = src;
  p->kind = kind;
  p->n_fail = n_fail;
  return p;
}

// Up links only (a dead slot is a self-loop).  The edge is the first met in
// row order, so the one out of the endpoint with the smaller CSR id: a metric
// plan names a link's two directions by it (m_lo, m_hi).
std::vector<uint32_t> link_edges(const spf_ctx* c) {
  std::vector<uint32_t> link_edge((size_t)c->max_link + 1, kInf);
  for (uint32_t u = 0; u < c->N; ++u)
    for (uint32_t e = c->row_ptr[u]; e < c->row_ptr[u + 1]; ++e)
      if (c->col[e] != u && link_edge[c->link[e]] == kInf) link_edge[c->link[e]] = e;
  return link_edge;
}

// The part of plan creation that every kind shares, from the
// source's neighbour bits to the teams' scratch: p holds ctx, src, kind and
// n_fail, `fails` its list (link ids with `link_edge`, node ids without; a set
// plan's set_ptr with `link_edge`, its members uploaded by the caller).
spf_status plan_build(spf_ctx* c, std::unique_ptr<spf_whatif_plan>& p,
                      const std::vector<uint32_t>& fails, const std::vector<uint32_t>* link_edge,
                      spf_whatif_plan** out) {
  const uint32_t N = c->N, src = p->src;
  const WiKindOps& ops = kind_ops(p->kind);
  p->prof_mode = p->kind ? 0 : whatif_prof_mode();  // only link plans have profiled instances
  // bit of each distinct up neighbour of src
  std::vector<uint32_t> nbr_bit(N, kInf);
  const uint32_t k = c->nb_ptr[src + 1] - c->nb_ptr[src];
  for (uint32_t j = 0; j < k; ++j) nbr_bit[c->nb_id[c->nb_ptr[src] + j]] = j;
  p->W = std::max<uint32_t>(1, (k + 31) / 32);
  {  // wave teams: 16 per CU within the scratch budget (failures on the
     // 1M-link graph, r02_v75 with 8 GB: 12: 17.9 ms, 16: 16.4, 20: 20.2,
     // 24: 19.6; r02_v30 before the lane-read / DPP repairs: 12 best)
     // (SPF_WHATIF_WAVES=<per CU>, a multiple of 4: A/B)
    const char* e = std::getenv("SPF_WHATIF_WAVES");
    const size_t per_cu = e ? std::max(4, atoi(e) & ~3) : 16;
    if (const char* ec = std::getenv("SPF_WHATIF_WAVECAP")) p->wave_cap = std::max(64, atoi(ec));
    p->classify_cap = p->wave_cap;
    if (const char* ec = std::getenv("SPF_WHATIF_CLASSIFY")) p->classify_cap = std::max(1, atoi(ec));
    const size_t cap = p->wave_cap;
    const size_t per_team = 4ull * (N + cap * (4ull + p->W) + cap + 1);
    const size_t fit = std::max<size_t>(4, kWaveScratch / per_team) & ~size_t(3);
    p->wave_teams = (uint32_t)std::min<size_t>(per_cu * c->n_cu, fit);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, p->d_fails.upload(fails.data(), fails.size(), c->stream));
  if (link_edge) HIP_TRY(c, p->d_link_edge.upload(link_edge->data(), link_edge->size(), c->stream));
  HIP_TRY(c, p->d_nbr_bit.upload(nbr_bit.data(), N, c->stream));
  HIP_TRY(c, p->d_dist.alloc(N));
  HIP_TRY(c, p->d_q.alloc(N));
  HIP_TRY(c, p->d_q2.alloc(N));
  HIP_TRY(c, p->d_bm.alloc((N + 31) / 32));
  HIP_TRY(c, p->d_nhb.alloc((size_t)N * p->W));
  HIP_TRY(c, p->d_ctr.alloc(4));
  HIP_TRY(c, p->d_bar.alloc(kGridBarWords));
  HIP_TRY(c, p->d_lvl.alloc(kLevelCap + 1));
  HIP_TRY(c, p->d_order.alloc(N));
  HIP_TRY(c, p->d_misc.alloc(8));
  HIP_TRY(c, p->d_H.alloc(1));
  HIP_TRY(c, p->d_hot.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_big.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_big0.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_big1.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, p->d_parent.alloc(N));
  HIP_TRY(c, p->d_sub.alloc(N));
  if (!c->side) {  // the classified big failures' workgroup teams run here
    HIP_TRY(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->side_fork, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->side_join, hipEventDisableTiming));
  }
  HIP_TRY(c, p->d_cnt.alloc(8));
  {  // workgroup teams: one per CU, two sets (b_*, c_*) within the scratch budget
    const size_t per_team = 4ull * ((size_t)N * (6 + p->W) + 1);
    p->big_teams = (uint32_t)std::max<size_t>(4, std::min<size_t>(c->n_cu, kBigScratch / 2 / per_team));
  }
  const size_t bt = p->big_teams;
  {  // group teams over the concurrent (c_*) scratch sets: G workgroups each,
     // n_cu / G teams (a multiple of 8: members share an XCD), no more teams
     // than scratch sets (SPF_WHATIF_GROUP=1: one-workgroup teams, A/B).
     // G = 8 by default: ba_whatif's failures took 9.3 ms at G = 8 against
     // 10.2 at 4 and 14.8 at 16 (profiles/r05_whatif/flat)
    const char* e = std::getenv("SPF_WHATIF_GROUP");
    uint32_t G = e ? (uint32_t)atoi(e) : 8u;
    if (G > 1) {
      while (G <= 16 && (c->n_cu / G > bt || (c->n_cu / G) % 8)) G *= 2;
      if (G <= 16 && c->n_cu % (8 * G) == 0 && c->n_cu / G >= 8) {
        p->group = G;
        p->group_teams = c->n_cu / G;
        HIP_TRY(c, p->d_ctl.alloc(sizeof(TeamCtl) * p->group_teams));
      }
    }
  }
  if (p->group) {
    // The group teams' members must all be resident while the wave teams'
    // blocks hold their CUs (launched beside them on the side stream; a
    // member that cannot be placed stalls its team at every barrier).  Per
    // SIMD: the wave teams' waves (one per 256-thread block) and the group
    // workgroup's 2 waves share 512 VGPRs (granule 8).  Fewer wave teams per
    // CU until both fit.  (Round 4's stamp pointer in the wave kernel --
    // 75 -> 80+ VGPRs at 4 waves per SIMD beside 2 x 88 -- broke this sum.)
    // Every kind launches its own instances: the sum is made with their
    // registers (kind_regs).
    int rw = 0, rg = 0;
    HIP_TRY(c, ops.regs(p.get(), rw, rg));
    const auto gran = [](int r) { return (uint32_t)((std::max(r, 1) + 7) & ~7); };
    const uint32_t per_simd_group = kGroupWg / 64 / 4;
    const uint32_t vw = gran(rw), vg = gran(rg);
    uint32_t per_simd_wave = (p->wave_teams + 4 * c->n_cu - 1) / (4 * c->n_cu);
    while (per_simd_wave > 1 && per_simd_wave * vw + per_simd_group * vg > 512) --per_simd_wave;
    p->wave_teams = std::min(p->wave_teams, per_simd_wave * 4 * c->n_cu);
    if (std::getenv("SPF_WHATIF_DEBUG"))
      std::fprintf(stderr, "whatif%s: wave kernel %d VGPRs, group<%u> %d VGPRs: %u wave teams (%u per SIMD)\n",
                   ops.debug_name, rw, p->group, rg, p->wave_teams, per_simd_wave);
  }
  const size_t wt = p->wave_teams;
  while ((1u << p->tab_log2) < 4 * p->wave_cap) ++p->tab_log2;
  {  // WiGraph::ed from the context's host CSR (the plan lives within one graph epoch)
    std::vector<uint4> ed(std::max<uint32_t>(c->E, 1));
    for (uint32_t e = 0; e < c->E; ++e) ed[e] = make_uint4(c->col[e], c->wt[e], c->link[e], c->wt[c->rev[e]]);
    HIP_TRY(c, p->d_ed.upload(ed.data(), ed.size(), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (ed is freed on return)
  }
  HIP_TRY(c, p->w_tab.alloc(wt << p->tab_log2));
  HIP_TRY(c, p->w_dlist.alloc(wt * p->wave_cap));
  HIP_TRY(c, p->w_dnew.alloc(wt * p->wave_cap));
  HIP_TRY(c, p->w_nhn.alloc(wt * p->wave_cap * p->W));
  HIP_TRY(c, p->w_lvl.alloc(wt * (p->wave_cap + 1)));
  HIP_TRY(c, p->w_ord.alloc(wt * 2 * p->wave_cap));
  HIP_TRY(c, p->b_mark.alloc(bt * N));
  HIP_TRY(c, p->b_dlist.alloc(bt * N));
  HIP_TRY(c, p->b_dnew.alloc(bt * N));
  HIP_TRY(c, p->b_nhn.alloc(bt * N * p->W));
  HIP_TRY(c, p->b_lvl.alloc(bt * (N + 1)));
  HIP_TRY(c, p->b_ord.alloc(bt * 2 * N));
  HIP_TRY(c, p->c_mark.alloc(bt * N));
  HIP_TRY(c, p->c_dlist.alloc(bt * N));
  HIP_TRY(c, p->c_dnew.alloc(bt * N));
  HIP_TRY(c, p->c_nhn.alloc(bt * N * p->W));
  HIP_TRY(c, p->c_lvl.alloc(bt * (N + 1)));
  HIP_TRY(c, p->c_ord.alloc(bt * 2 * N));
  HIP_TRY(c, hipMemsetAsync(p->c_mark.p, 0xFF, bt * N * 4, c->stream));
  // marks start (and are always left) at kInf
  HIP_TRY(c, hipMemsetAsync(p->w_tab.p, 0xFF, (wt << p->tab_log2) * 8, c->stream));
  HIP_TRY(c, hipMemsetAsync(p->b_mark.p, 0xFF, bt * N * 4, c->stream));
  if (p->prof_mode) {  // [bt teams][base][wave teams] x 16 (row bounds checked in the kernels)
    const size_t slots = 16 * (bt + 1 + p->wave_teams) + 128;  // + the base's per-level clocks
    HIP_TRY(c, p->d_prof.alloc(slots));
    HIP_TRY(c, hipMemsetAsync(p->d_prof.p, 0, slots * 8, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  p->epoch = c->epoch;
  *out = p.release();
  return SPF_OK;
}

}  // namespace spfi

extern "C" {

spf_status spf_whatif_plan_create(spf_ctx* c, uint32_t src, const uint32_t* fail_links,
                                  uint32_t n_fail, spf_whatif_plan** out) {
  if (const spf_status st = create_prologue(c, out, src, "spf_whatif_plan_create"); st != SPF_OK)
    return st;
  const std::vector<uint32_t> link_edge = link_edges(c);
  std::vector<uint32_t> fails;
  if (fail_links) {
    fails.assign(fail_links, fail_links + n_fail);
    for (uint32_t l : fails)
      if (l > c->max_link || link_edge[l] == kInf)
        return fail(c, SPF_E_INVALID, "link %u is not an up link of the graph", l);
  } else {  // every up link, ascending id
    for (uint32_t l = 0; l <= c->max_link && c->E; ++l)
      if (link_edge[l] != kInf) fails.push_back(l);
  }
  auto p = new_plan(c, src, (uint32_t)kLink, (uint32_t)fails.size());
  if (c->nonpos || c->needs64) {
    // zero / negative metrics, u64 labels: the exact kernel replays
    // runSpf(src, true, {l}) for every failure touching a pathLink
    HIP_TRY(c, hipSetDevice(c->device));
    p->exact = std::make_unique<spfi::ExactWhatIf>();
    const spf_status st = exact_whatif_prepare(c, p->exact.get(), src, fails, link_edge);
    if (st != SPF_OK) return st;
    if (!fails.empty()) HIP_TRY(c, p->d_fails.upload(fails.data(), fails.size(), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    p->W = p->exact->W;
    p->epoch = c->epoch;
    *out = p.release();
    return SPF_OK;
  }
  return plan_build(c, p, fails, &link_edge, out);
}

void spf_whatif_plan_destroy(spf_whatif_plan* p) { delete p; }
uint32_t spf_whatif_plan_failures(const spf_whatif_plan* p) { return p ? p->n_fail : 0; }

spf_status spf_whatif_plan_links(const spf_whatif_plan* p, uint32_t* links) {
  if (!p || !links) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  if (p->kind) return fail(c, SPF_E_STATE, "spf_whatif_plan_links: %s", kind_ops(p->kind).plan_name);
  HIP_TRY(c, hipMemcpy(links, p->d_fails.p, 4ull * p->n_fail, hipMemcpyDeviceToHost));
  return SPF_OK;
}

spf_status spf_whatif_plan_kind(const spf_whatif_plan* p, uint32_t* kind) {
  if (!p || !kind) return SPF_E_INVALID;
  *kind = p->kind;
  return SPF_OK;
}

spf_status spf_whatif_execute(spf_whatif_plan* p, spf_whatif_digest* d_out,
                              spf_whatif_digest* d_base, void* stream) {
  if (!p || !d_out) return fail(p ? p->ctx : nullptr, SPF_E_INVALID, "spf_whatif_execute: NULL");
  spf_ctx* c = p->ctx;
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (p->epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  p->last = s;
  hipEvent_t* ev = nullptr;
  if (p->timing_cap) {
    ev = &p->ev[3 * (p->timing_n % p->timing_cap)];
    ++p->timing_n;
    HIP_TRY(c, hipEventRecord(ev[0], s));
  }
  if (p->exact) {
    const spf_status st = exact_whatif_launch(c, p->exact.get(), d_out, d_base, s, ev ? ev[1] : nullptr);
    if (st != SPF_OK) return st;
    if (ev) HIP_TRY(c, hipEventRecord(ev[2], s));
    c->solves += 1ull + p->n_fail;
    return SPF_OK;
  }
  const WiGraph g = wi_graph(p);
  if (const spf_status st = run_base(p, g, s); st != SPF_OK) return st;
  if (ev) HIP_TRY(c, hipEventRecord(ev[1], s));
  if (const spf_status st = kind_ops(p->kind).run(p, d_out, s, nullptr); st != SPF_OK) return st;
  if (p->d_prof.p) {  // diagnostics: phase ticks (100 MHz) per team, accumulated over repairs
    const size_t bt = p->big_teams, wt = p->wave_teams;
    std::vector<unsigned long long> h(16ull * (bt + 1 + wt) + 128);
    HIP_TRY(c, hipMemcpyAsync(h.data(), p->d_prof.p, h.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    auto line = [&](const char* who, const unsigned long long* r) {
      std::fprintf(stderr, "whatif %s repairs=%llu sum|D|=%llu max|D|=%llu dial_levels=%llu gave_up=%llu "
                   "bfs=%llu seeds=%llu dial=%llu fallback=%llu digest=%llu (x10ns)\n", who, r[0], r[8],
                   r[10], r[9], r[11], r[1], r[2], r[3], r[4], r[5]);
    };
    for (size_t t = 0; t < bt; ++t) {
      const unsigned long long* r = &h[16 * t];
      if (!r[0]) continue;
      char who[32];
      std::snprintf(who, sizeof who, "team %zu", t);
      line(who, r);
    }
    std::vector<unsigned long long> sum(16, 0);  // the wave teams, summed
    unsigned long long busiest = 0;
    for (size_t t = 0; t < wt; ++t) {
      const unsigned long long* r = &h[16 * (bt + 1 + t)];
      for (int k = 0; k < 16; ++k) sum[k] = k == 10 ? std::max(sum[k], r[k]) : sum[k] + r[k];
      busiest = std::max(busiest, r[1] + r[2] + r[3] + r[4] + r[5]);
    }
    line("wave-teams(sum)", sum.data());
    std::fprintf(stderr, "whatif wave teams %zu, busiest team %llu ticks (x10ns)\n", wt, busiest);
    const unsigned long long* r = &h[16 * bt];
    std::fprintf(stderr, "whatif base sssp=%llu nh=%llu (of which subtree sizes %llu) hash=%llu (x10ns) maxd=%llu levels=%llu W=%u\n",
                 r[1] - r[0], r[2] - r[1], r[6] ? r[2] - r[6] : 0ull, r[3] - r[2], r[4], r[5], p->W);
    const unsigned long long* lv = &h[16 * (bt + 1 + wt)];
    unsigned long long prev = 0;
    std::string line2 = "whatif base levels (distance:nodes:ticks)";
    for (int d = 1; d < 64; ++d) {
      if (!lv[2 * d]) continue;
      const unsigned long long t0 = prev ? prev : lv[2 * d];
      line2 += " " + std::to_string(d) + ":" + std::to_string(lv[2 * d + 1]) + ":" +
               std::to_string(prev ? lv[2 * d] - t0 : 0ull);
      prev = lv[2 * d];
    }
    std::fprintf(stderr, "%s\n", line2.c_str());
  }
  if (d_base) {
    // the unfailed digest: nothing changed, hash = H
    hipLaunchKernelGGL(base_digest_kernel, dim3(1), dim3(1), 0, s, d_base, p->d_H.p);
    HIP_TRY(c, hipGetLastError());
  }
  if (ev) HIP_TRY(c, hipEventRecord(ev[2], s));
  c->solves += 1ull + p->n_fail;
  return SPF_OK;
}

spf_status spf_whatif_changes(spf_whatif_plan* p, spf_whatif_digest* d_out, spf_whatif_digest* d_base,
                              uint64_t* n_entries, uint64_t* pool_bytes, double* kernel_ms,
                              void* stream) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_whatif_changes: NULL plan");
  spf_ctx* c = p->ctx;
  WiPool& L = p->lists;
  L.valid = false;             // after a failed call the plan holds no lists
  p->rt.pool.valid = false;    // ... and the route lists were built from the old ones
  p->imp_node.pool.valid = p->imp_set.pool.valid = false;  // ... as were the transpositions
  p->up.ent.valid = p->up.rec.valid = false;                // ... and the route updates
  if (!c->loaded) return fail(c, SPF_E_STATE, "graph no longer loaded");
  if (p->epoch != c->epoch)
    return fail(c, SPF_E_STATE, "graph changed since the plan was created: recreate it");
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const uint32_t nf = p->n_fail;
  HIP_TRY(c, p->l_cnt.alloc(std::max<uint32_t>(1, nf)));
  HIP_TRY(c, L.ptr.alloc((size_t)nf + 1));
  if (!d_out) {
    HIP_TRY(c, p->l_dig.alloc(std::max<uint32_t>(1, nf)));
    d_out = p->l_dig.p;
  }
  for (hipEvent_t& e : p->l_ev)
    if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  p->last = s;
  WiEmit em;
  em.cnt = p->l_cnt.p;
  em.W = p->W;
  em.fault = c->d_fault.p;
  // one pass over the failures with the EMIT instances (count, then fill)
  const WiGraph g = p->exact ? WiGraph{} : wi_graph(p);
  auto pass = [&](bool first) -> spf_status {
    if (p->exact)
      return exact_whatif_launch(c, p->exact.get(), d_out, first ? d_base : nullptr, s, nullptr, &em,
                                 first);
    return kind_ops(p->kind).run(p, d_out, s, &em);
  };
  if (!p->exact)
    if (const spf_status st = run_base(p, g, s); st != SPF_OK) return st;
  // count: cnt[f] = failure f's entries (0 for cold ones: the memset)
  HIP_TRY(c, hipMemsetAsync(p->l_cnt.p, 0, 4ull * std::max<uint32_t>(1, nf), s));
  HIP_TRY(c, hipEventRecord(p->l_ev[0], s));
  if (const spf_status st = pass(true); st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(p->l_ev[1], s));
  HIP_TRY(c, whatif_scan(p->l_cnt.p, 1, nf, L.ptr.p, s));
  HIP_TRY(c, hipEventRecord(p->l_ev[2], s));
  // the pool is sized from the scan's total
  unsigned long long total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, L.ptr.p + nf, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  if (const spf_status st = pool_size(c, &L, total, p->W, "spf_whatif_changes"); st != SPF_OK) return st;
  // fill: the repairs again, entries to cptr[f] + k
  em.cptr = L.ptr.p;
  em.cnode = L.key.p;
  em.cdist = L.val.p;
  em.cnh = L.rows.p;
  if (const spf_status st = pass(false); st != SPF_OK) return st;
  HIP_TRY(c, hipEventRecord(p->l_ev[3], s));
  if (d_base && !p->exact) {
    hipLaunchKernelGGL(base_digest_kernel, dim3(1), dim3(1), 0, s, d_base, p->d_H.p);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  for (int k = 0; k < 3; ++k) HIP_TRY(c, hipEventElapsedTime(&p->l_ms[k], p->l_ev[k], p->l_ev[k + 1]));
  L.n_owners = nf;
  L.total = total;
  L.valid = true;
  c->solves += 1ull + nf;
  if (n_entries) *n_entries = total;
  if (pool_bytes) *pool_bytes = spfi::pool_bytes(L);
  if (kernel_ms) *kernel_ms = (double)p->l_ms[0] + p->l_ms[1] + p->l_ms[2];
  return SPF_OK;
}

spf_status spf_whatif_changes_timing(const spf_whatif_plan* p, double* ms) {
  if (!p || !ms) return SPF_E_INVALID;
  WiListsView v;
  if (const spf_status st = pool_held(const_cast<spf_whatif_plan*>(p), kPoolChanges,
                                      "spf_whatif_changes_timing", &v); st != SPF_OK)
    return st;
  for (int k = 0; k < 3; ++k) ms[k] = p->l_ms[k];
  return SPF_OK;
}

spf_status spf_whatif_changes_buffers(spf_whatif_plan* p, const uint64_t** d_ptr, const uint32_t** d_node,
                                      const uint64_t** d_dist, const uint32_t** d_nh, uint32_t* W,
                                      uint64_t* n_entries) {
  return pool_buffers(p, kPoolChanges, "spf_whatif_changes_buffers", d_ptr, d_node, d_dist, d_nh, nullptr,
                      W, n_entries);
}

spf_status spf_whatif_changes_read(spf_whatif_plan* p, uint64_t* ptr, uint32_t* node, uint64_t* dist,
                                   uint32_t* nh) {
  return pool_read(p, kPoolChanges, "spf_whatif_changes_read", ptr, node, dist, nh);
}

spf_status spf_whatif_changes_db(spf_whatif_plan* p, uint32_t i, uint32_t* node, uint64_t* dist,
                                 uint32_t* nh, uint64_t cap, uint64_t* n) {
  return pool_db(p, kPoolChanges, "spf_whatif_changes_db", i, node, dist, nh, cap, n);
}

spf_status spf_whatif_base(spf_whatif_plan* p, uint64_t* dist, uint32_t* nh, uint32_t* W) {
  if (!p) return fail(nullptr, SPF_E_INVALID, "spf_whatif_base: NULL plan");
  spf_ctx* c = p->ctx;
  if (!p->last) return fail(c, SPF_E_STATE, "spf_whatif_base: no execute yet");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(p->last));
  const size_t N = c->N, Wp = p->W;
  if (W) *W = p->W;
  std::vector<uint64_t> d(N);
  if (p->exact) {
    HIP_TRY(c, hipMemcpy(d.data(), p->exact->base_d.p, 8 * N, hipMemcpyDeviceToHost));
  } else {
    std::vector<uint32_t> d32(N);
    HIP_TRY(c, hipMemcpy(d32.data(), p->d_dist.p, 4 * N, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < N; ++v) d[v] = d32[v] == kInf ? ~0ull : d32[v];
  }
  if (dist) std::memcpy(dist, d.data(), 8 * N);
  if (nh) {
    // rows of W words in both plans (the exact plan's Wmax is its W); an
    // unreachable node's row, and a source's without neighbours, is zero
    const uint32_t* rows = p->exact ? p->exact->base_nh.p : p->d_nhb.p;
    HIP_TRY(c, hipMemcpy(nh, rows, 4 * N * Wp, hipMemcpyDeviceToHost));
    const bool no_nbr = c->nb_ptr[p->src + 1] == c->nb_ptr[p->src];
    for (size_t v = 0; v < N; ++v)
      if (d[v] == ~0ull || no_nbr) std::memset(nh + v * Wp, 0, 4 * Wp);
  }
  return SPF_OK;
}

spf_status spf_whatif_stats(spf_whatif_plan* p, uint32_t* n_hot, uint32_t* n_big) {
  if (!p) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  uint32_t cnt[4] = {0, 0, 0, 0};
  if (!p->last) return fail(c, SPF_E_STATE, "spf_whatif_stats: no execute yet");
  if (p->exact) {  // every failure is a re-run on the exact kernel (cold ones skipped inside)
    HIP_TRY(c, hipStreamSynchronize(p->last));
    if (n_hot) *n_hot = p->n_fail;
    if (n_big) *n_big = 0;
    return SPF_OK;
  }
  // the counters are written on the execute stream (non-blocking, so the
  // null stream does not order after it): copy on that stream and wait
  HIP_TRY(c, hipMemcpyAsync(cnt, p->d_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, p->last));
  HIP_TRY(c, hipStreamSynchronize(p->last));
  if (const spf_status st = spf_device_check(c); st != SPF_OK) return st;
  if (n_hot) *n_hot = cnt[0] + cnt[3];  // wave list + classified big
  if (n_big) *n_big = cnt[2] + cnt[3];  // wave overflow + classified big
  return SPF_OK;
}

spf_status spf_whatif_enable_timing(spf_whatif_plan* p, uint32_t max_executes) {
  if (!p) return SPF_E_INVALID;
  spf_ctx* c = p->ctx;
  for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
  p->ev.assign(3ull * max_executes, nullptr);
  // timing only: no system-scope fence (its L2 writeback + invalidate cost
  // ~5 us per event and left the next kernel a cold L2)
  for (auto& e : p->ev) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableSystemFence));
  p->timing_cap = max_executes;
  p->timing_n = 0;
  return SPF_OK;
}

spf_status spf_whatif_timing(spf_whatif_plan* p, double* base_ms, double* fail_ms, uint32_t* n) {
  if (!p || !p->timing_cap) return SPF_E_STATE;
  spf_ctx* c = p->ctx;
  const uint32_t cnt = std::min(p->timing_n, p->timing_cap);
  double a = 0, b = 0;
  for (uint32_t i = 0; i < cnt; ++i) {
    float t0 = 0, t1 = 0;
    HIP_TRY(c, hipEventSynchronize(p->ev[3 * i + 2]));
    HIP_TRY(c, hipEventElapsedTime(&t0, p->ev[3 * i], p->ev[3 * i + 1]));
    HIP_TRY(c, hipEventElapsedTime(&t1, p->ev[3 * i + 1], p->ev[3 * i + 2]));
    a += t0;
    b += t1;
  }
  if (base_ms) *base_ms = a;
  if (fail_ms) *fail_ms = b;
  if (n) *n = cnt;
  p->timing_n = 0;
  return SPF_OK;
}

spf_status spf_whatif_solve(spf_ctx* c, uint32_t src, const uint32_t* fail_links,
                            uint32_t n_fail, spf_whatif_digest* out, spf_whatif_digest* base) {
  if (!c || !out) return fail(c, SPF_E_INVALID, "spf_whatif_solve: NULL argument");
  spf_whatif_plan* raw = nullptr;
  spf_status st = spf_whatif_plan_create(c, src, fail_links, n_fail, &raw);
  if (st != SPF_OK) return st;
  std::unique_ptr<spf_whatif_plan> p(raw);
  DevBuf<spf_whatif_digest> d_out, d_base;
  HIP_TRY(c, d_out.alloc(std::max<uint32_t>(1, p->n_fail)));
  HIP_TRY(c, d_base.alloc(1));
  st = spf_whatif_execute(p.get(), d_out.p, d_base.p, c->stream);
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipMemcpyAsync(out, d_out.p, sizeof(spf_whatif_digest) * p->n_fail,
                            hipMemcpyDeviceToHost, c->stream));
  if (base)
    HIP_TRY(c, hipMemcpyAsync(base, d_base.p, sizeof(spf_whatif_digest), hipMemcpyDeviceToHost,
                              c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return spf_device_check(c);
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
  if (flag & 64u) {
    // a team's fill pass met more entries than its count pass allocated
    // (spf_whatif_changes): the entry was dropped
    return fail(c, SPF_E_HIP,
                "what-if change lists on device %d: an entry past its failure's allocated count "
                "(fault word 0x%08x); the results of this context's launches since the last check are "
                "invalid", c->device, flag);
  }
  if (flag & 56u) {
    // what-if repair diagnostics: a loop bound (bit 3, phase in bits 8-15), a
    // range check of the profiled instances (bit 4, site in bits 16-23) or a
    // team past its profile region (bit 5, kernel in bits 24-31)
    return fail(c, SPF_E_HIP,
                "what-if repair on device %d: %s%s%s (fault word 0x%08x: loop phase %u, check site %u, "
                "profile kernel %u); the results of this context's launches since the last check are "
                "invalid",
                c->device, (flag & 8u) ? "a repair loop reached its iteration bound " : "",
                (flag & 16u) ? "a scratch index failed its range check " : "",
                (flag & 32u) ? "a team's profile row is outside the profile buffer" : "", flag,
                (flag >> 8) & 0xFFu, (flag >> 16) & 0xFFu, flag >> 24);
  }
  if (flag & 2u) {
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

}  // extern "C"
