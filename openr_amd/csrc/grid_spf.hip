// ============================================================================
//  grid_spf.hip -- SPF in global memory by the whole chip, one grid-resident
//  launch: the engine's path for graphs beyond the LDS-resident kernels
//  (spf_big_kernel, a plan's sources one after another), the single-source
//  SSSP of any graph size (gsssp_coop_kernel) and the unfailed pass of a
//  what-if batch (whatif_base_kernel).  The three share coop_sssp and level_nh
//  as device functions, so they are one translation unit.  Also the launch
//  rule of every grid-barrier kernel of the library (launch_resident,
//  coop_blocks).  Built from grid_ops.h; nothing of the what-if plans is seen
//  here -- whatif.hip hands the base pass its buffers in a BaseBufs.
// ============================================================================
#include <cstdlib>

#include "engine_internal.h"
#include "grid_ops.h"
#include "wave_ops.h"

using namespace spfi;

namespace {

// ---------------------------------------------------------------------------
//  grid-synchronised (XGrid) single-source SSSP and unfailed result
// ---------------------------------------------------------------------------
constexpr int kCoopThreads = 512;  // one block per CU: always co-resident
constexpr uint32_t kCoopHubDeg = 32;  // nodes above this degree get a whole wave

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

spf_status launch_base(spf_ctx* c, const BaseBufs& b, hipStream_t s) {
  WiGraph g{c->d_row_ptr.p, c->d_col.p, c->d_wt.p, c->d_rev.p, c->d_link.p, c->d_ovl.p,
            b.nbr_bit, c->N, b.src, b.W};
  g.fault = c->d_fault.p;
  BaseArgs a{CoopSssp{c->d_row_ptr.p, c->d_col.p, c->d_wt.p, c->d_ovl.p, c->d_link.p, nullptr,
                      c->N, b.src, 0u, b.dist, b.q, b.q2, b.bm, b.ctr},
             g, b.nhb, b.lvl, b.order, b.misc, b.H, b.prof, b.parent, b.sub};
  a.sp.bar = b.bar;
  a.sp.fault = c->d_fault.p;
  a.lprof = b.lprof;
  HIP_TRY(c, hipMemsetAsync(b.bar, 0, 4 * kGridBarWords, s));
  void* args[] = {&a};
  if (const spf_status st = resident_order(c, s); st != SPF_OK) return st;
  HIP_TRY(c, launch_resident((const void*)whatif_base_kernel,
                             coop_blocks(c, (const void*)whatif_base_kernel, 1), kCoopThreads,
                             args, c->n_cu, s));
  return resident_done(c, s);
}

}  // namespace spfi
