// ============================================================================
//  msbfs.hip -- multi-source BFS for unit metrics and hop counts:
//  msbfs_kernel (64 sources per workgroup, a level's distances stored as they
//  are found; plain, LDS-column, double-buffered and twin-class quotient
//  sweeps) and msbfs_planes_kernel (32 sources, distances kept in register bit
//  planes, each row written once).  The kernels, their LDS and batch sizes,
//  which of them a graph gets (use_planes, use_quotient), one instance table
//  per kernel, and launch_msbfs.
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "spf_units.h"
#include "wave_ops.h"

using namespace spfi;

namespace {

// ---------------------------------------------------------------------------
//  1b. multi-source BFS for unit metrics: 64 sources per workgroup
// ---------------------------------------------------------------------------
// Every node carries a 64-bit mask, bit s = "source s of this batch".  A level
// is one pull sweep: new(v) = OR_{u in N(v)} F(u) & ~visited(v), where F holds
// the previous level's new masks.  A drained node is recorded but expands only
// as the source (LinkState.cpp:831-838): its producer writes F(v) masked to its
// own source bit, so the consumer loop is branch-free.  One edge sweep serves
// 64 sources, against 64 sweeps for the per-source kernel.
//   * F lives in LDS (8 B/node, F[N] = 0 is the padding target).
//   * visited / new masks of the nodes a thread owns (v = tid + i*1024) live in
//     registers; the 64 lanes of a wave own 64 consecutive nodes = one slice
//     of the sliced-ELL column array, so neighbour j of all 64 nodes is one
//     coalesced 256-byte load (kMsUnroll of them in flight).
//   * distances are written per level as predicated stores over the sources
//     that have new nodes in the wave; one store covers 64 consecutive nodes
//     of one source row.  The u8 narrow copy for the next-hop pass saturates at
//     254.
constexpr uint32_t kMsBatch = 64;
constexpr int kMsUnroll = 8;
constexpr uint32_t kMsLaneStoreRatio = 4;  // per-lane stores when 4 * max per-node count < #sources
// Narrow (u8) distance rows: npitch bytes (a multiple of 1024), node v at
// byte v -- a level's stores are 64 consecutive bytes per (source, slice),
// lane-ordered like the u32 ones (any permutation of the lanes' addresses
// costs the store path measurably).


//   LCOL: the sliced-ELL columns are staged once in LDS as u16 (when they fit
//   beside F -- low-degree graphs such as grids), so the pull sweep issues no
//   global loads: no vmcnt wait, and a level's stores drain in the background
//   instead of stalling the next sweep's first column load.
//   Level 0 is pushed, not pulled: its frontier is the batch's own sources,
//   so each wave ORs its sources' bits into their neighbours' F entries
//   (LDS 64-bit atomics over the sources' CSR rows) where a pull would sweep
//   every column of the graph (~1/5 of a fabric batch's time, r02 stamps).
//   Links are up in both directions or neither, so CSR out-neighbours are
//   the in-neighbours the pull reads.  (Pushing later levels, whose
//   frontiers live in the owners' registers, spilled msbfs_kernel<10>.)
//   Q: the sweep runs on the quotient graph of false-twin classes (nodes with
//   the same neighbour set; a fabric pod's rack switches, a plane's spines).
//   Twins receive the same OR at every level, and a node adjacent to one
//   member of a class is adjacent to all of them (links are up in both
//   directions or neither), so the frontier is kept per class, CF[class] =
//   OR of its members' new masks (a drained member's masked to its own
//   source bit first), and a level is
//     1. per quotient row, QA[class] = OR of CF over its neighbour classes
//        (rows cut into chunks of kQChunk columns, one chunk per thread, the
//        chunks of a wide row joined by an LDS atomic OR);
//     2. per owned node, new = QA[class of node] & ~visited, the row stores
//        as in the plain sweep, and new ORed into the next CF[class].
//   Classes, rows and columns are u16 tables staged in LDS once; a level
//   issues no global load.  Level 1 is the same sweep from the sources' bits
//   in their class slots.  CF and QA are double-buffered: two barriers a level.
constexpr int kQMaxOwn = 12;  // (the 16-slot instance spills its owned nodes' state: N <= 12288)
template <int OWN, bool LCOL, bool DB = false, bool Q = false>
__global__ __launch_bounds__(kMsThreads) void msbfs_kernel(
    const uint32_t* __restrict__ sell_ptr, const uint32_t* __restrict__ sell_col,
    uint32_t n_col, const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ ovl, const uint32_t* __restrict__ rows_src,
    uint32_t n_rows, uint32_t bs, uint32_t N, uint32_t pitch, uint32_t npitch,
    uint32_t* __restrict__ D, uint8_t* __restrict__ Dn, uint32_t* __restrict__ maxd,
    uint32_t d_from, const uint32_t* __restrict__ smap,
    unsigned long long* __restrict__ stamps /* diagnostics, usually null */,
    const uint16_t* __restrict__ q_cls, const uint16_t* __restrict__ q_tab, uint32_t q_nc,
    uint32_t q_nv /* Q: class of node, row/column tables, classes, row chunks */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* F = reinterpret_cast<uint64_t*>(smem);             // [N + 1]
  uint64_t* F2 = F + (DB ? N + 1 : 0);                         // [N + 1] (DB) second frontier
  // Q: class frontiers CF[2][q_nc + 1] and row results QA[2][q_nc + 1] (slot
  // q_nc of each stays 0: the padding column, the class of nodes past N),
  // the chunk -> row table and the chunk-major columns, the small arrays, and
  // self[N]: 1 + batch index of the nodes that are sources
  const uint32_t q_nvp = (q_nv + 7u) & ~7u;
  uint64_t* const CF = reinterpret_cast<uint64_t*>(smem);
  uint64_t* const QA = CF + 2 * (q_nc + 1);
  uint16_t* const vrow = reinterpret_cast<uint16_t*>(QA + 2 * (q_nc + 1));  // [q_nvp]
  uint16_t* const vcol = vrow + q_nvp;                                       // [kQChunk][q_nvp]
  uint32_t* o_node = Q ? reinterpret_cast<uint32_t*>(vcol + kQChunk * q_nvp)
                       : reinterpret_cast<uint32_t*>(F2 + N + 1);  // [64] drained batch sources
  uint32_t* o_cnt = o_node + kMsBatch;                         // [1]
  uint32_t* flag = o_cnt + 1;                                  // [3] progress flags
  uint32_t* src_l = flag + 3;                                  // [64] the batch's sources
  uint32_t* e_base = src_l + kMsBatch;                         // [64] their first CSR edge
  uint32_t* e_pre = e_base + kMsBatch;                         // [65] degree prefix sums
  uint16_t* lcol = reinterpret_cast<uint16_t*>(e_pre + kMsBatch + 1);  // [n_col] (LCOL)
  uint8_t* const self = reinterpret_cast<uint8_t*>(e_pre + kMsBatch + 1);  // [N] (Q)

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t row0 = blockIdx.x * bs;  // bs <= 64 sources per workgroup
  // sell_col with its padding columns (spf_graph_load: 32 past the last slice)
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(sell_col), 0, (int)((n_col + 32u * kSliceW) * 4u), 0x00020000);
  const uint32_t nb = min(bs, n_rows - row0);
  const uint64_t all = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
  // diagnostics: lane 0 of every wave of workgroup 0 logs phase clocks into
  // stamps[wave * 64 + 1 ..], the count into stamps[wave * 64]
  // (the workgroup logged: stamps[1024], SPF_STAMPS=<workgroup>)
  const bool stamp = stamps && blockIdx.x == (uint32_t)stamps[64 * 16] && lane == 0;
  unsigned long long* my_stamps = stamps + (tid >> 6) * 64;
  uint32_t n_stamp = 0;
#define MS_STAMP()                                                   \
  do {                                                               \
    if (stamp && n_stamp < 63) my_stamps[++n_stamp] = __builtin_amdgcn_s_memtime(); \
  } while (0)
  MS_STAMP();

  if constexpr (Q) {
    for (uint32_t t = tid; t < 4 * (q_nc + 1); t += kMsThreads) CF[t] = 0;  // CF and QA
    const uint4* tab4 = reinterpret_cast<const uint4*>(q_tab);
    for (uint32_t t = tid; t < (1 + kQChunk) * q_nvp / 8; t += kMsThreads)
      reinterpret_cast<uint4*>(vrow)[t] = tab4[t];
    for (uint32_t t = tid; t < (N + 3) / 4; t += kMsThreads) reinterpret_cast<uint32_t*>(self)[t] = 0;
  } else {
  for (uint32_t v = tid; v <= N; v += kMsThreads) F[v] = 0;
  }
  if (LCOL)
    for (uint32_t t = tid; t < n_col; t += kMsThreads) lcol[t] = (uint16_t)sell_col[t];
  if (DB)
    for (uint32_t v = N + tid; v <= N; v += kMsThreads) F2[v] = 0;  // the padding target
  if (tid == 0) {
    *o_cnt = 0;
    flag[0] = flag[1] = flag[2] = 0;
  }
  __syncthreads();
  // ---- the batch's sources (wave 0): level 0, drained sources, their CSR
  // rows as one flat edge list (exclusive scan of the degrees), and their own
  // bits marked in F for the owners to pick up ----
  if constexpr (Q) {
    if (tid < nb) {
      const uint32_t src = rows_src[row0 + tid];  // sources of a batch are distinct
      if (ovl[src]) o_node[atomicAdd(o_cnt, 1u)] = src | (tid << 24);
      if (D && d_from == 0) D[(size_t)(row0 + tid) * pitch + src] = 0;  // level 0
      if (Dn) Dn[(size_t)(row0 + tid) * npitch + src] = 0;
      self[src] = (uint8_t)(tid + 1);
      // level 0's frontier: a source expands even when drained
      atomicOr(reinterpret_cast<unsigned long long*>(&CF[q_cls[src]]), 1ull << tid);
    }
  } else if (tid < 64) {
    uint32_t deg = 0;
    if (tid < nb) {
      const uint32_t src = rows_src[row0 + tid];  // sources of a batch are distinct
      src_l[tid] = src;
      if (ovl[src]) o_node[atomicAdd(o_cnt, 1u)] = src | (tid << 24);
      if (D && d_from == 0) D[(size_t)(row0 + tid) * pitch + src] = 0;  // level 0
      if (Dn) Dn[(size_t)(row0 + tid) * npitch + src] = 0;
      e_base[tid] = row_ptr[src];
      deg = row_ptr[src + 1] - e_base[tid];
      F[src] = 1ull << tid;
    }
    uint32_t total;
    const uint32_t ex = wave_excl_scan(deg, &total);
    e_pre[tid] = ex;
    if (tid == 0) e_pre[64] = total;
  }
  __syncthreads();
  const uint32_t n_osrc = *o_cnt;
  // the part of mask x a drained node v may expand: its own source bit
  auto own_bits = [&](uint32_t v, uint64_t x) {
    uint64_t own = 0;
    for (uint32_t k = 0; k < n_osrc; ++k)
      if ((o_node[k] & 0xFFFFFFu) == v) own = 1ull << (o_node[k] >> 24);
    return x & own;
  };

  // owned slices: slot i of this wave holds slice smap[wave * OWN + i] (the
  // host deals slices to waves balanced by column width; an unused slot's
  // nodes lie past N)
  const uint32_t wv = tid >> 6;
  uint32_t sv[OWN];  // first node of owned slice i (wave-uniform)
  uint64_t vis[OWN], nv[OWN];
  uint32_t drained = 0;  // bit i: owned node i is drained
  uint32_t cl[Q ? OWN : 1];  // (Q) class of owned node i
#pragma unroll
  for (int i = 0; i < OWN; ++i) {
    sv[i] = __builtin_amdgcn_readfirstlane(smap[wv * OWN + i]) * kSliceW;
    const uint32_t v = sv[i] + lane;
    if constexpr (Q) {
      const uint32_t me = v < N ? self[v] : 0u;
      vis[i] = me ? 1ull << (me - 1) : 0ull;
      cl[i] = v < N ? q_cls[v] : q_nc;
    } else {
    vis[i] = v < N ? F[v] : 0ull;  // the node's own source bit, if it is a source
    }
    if (v < N && ovl[v]) drained |= 1u << i;
  }
  bool level1 = false;
  if constexpr (!Q) {
  __syncthreads();  // the self marks are read
  if (tid < nb) F[src_l[tid]] = 0;
  __syncthreads();
  // ---- level 1 by push: each source's bit ORed into its neighbours' F (a
  // source expands even when drained); the batch's edges dealt over the
  // whole workgroup, their loads all independent ----
  {
    const uint32_t n_e = e_pre[64];
    for (uint32_t t = tid; t < n_e; t += kMsThreads) {
      uint32_t lo = 0, hi = nb;  // the source b with e_pre[b] <= t < e_pre[b + 1]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (e_pre[mid] <= t) lo = mid;
        else hi = mid;
      }
      atomicOr(reinterpret_cast<unsigned long long*>(&F[col[e_base[lo] + t - e_pre[lo]]]),
               1ull << lo);
    }
  }
  __syncthreads();
  uint64_t any1 = 0;
#pragma unroll
  for (int i = 0; i < OWN; ++i) {
    const uint32_t v = sv[i] + lane;
    nv[i] = v < N ? F[v] & ~vis[i] : 0ull;  // level 1
    vis[i] |= nv[i];
    any1 |= nv[i];
  }
  __syncthreads();  // every read of the pushed F is done
#pragma unroll
  for (int i = 0; i < OWN; ++i) {
    const uint32_t v = sv[i] + lane;
    if (v < N) F[v] = ((drained >> i) & 1u) ? own_bits(v, nv[i]) : nv[i];
  }
  if (any1) flag[0] = 1;  // level 1 is not empty (flag[1] stays 0 for level 1's sweep)
  __syncthreads();
  level1 = flag[0] != 0;  // read before level 1 resets flag[0]
  }

  MS_STAMP();
  // ---- record a level: D[s][v] = L for every new (s, v) of owned slice i
  // (mask x); only the sources with a new node in the slice (wave OR) ----
  auto record = [&](int i, uint64_t x, uint32_t L) {
    // most slices have no new node at a given level: one ballot skips them
    if (__ballot(x != 0ull) == 0ull) return;
    const uint32_t nl = min(L, 254u);
    uint32_t* const DL = L >= d_from ? D : nullptr;  // u32 rows this level (uniform)
    // the wave-uniform mask lives in SGPRs: row addressing is scalar work
    const uint64_t wm = wave_or64(x);
    uint32_t mlo = __builtin_amdgcn_readfirstlane((uint32_t)wm);
    uint32_t mhi = __builtin_amdgcn_readfirstlane((uint32_t)(wm >> 32));
    uint32_t v = sv[i] + lane;
    // (Q: formed per call -- ten slots' row addresses hoisted out of the level
    // loop spilled VGPRs)
    if constexpr (Q) asm volatile("" : "+v"(v));
    // Two ways to cover the (source, node) pairs of the slice: one
    // coalesced store per source (row-major; best when a source discovers
    // many nodes of the slice at once -- dense fabrics), or each lane
    // walking its own new sources (scattered stores; best when every source
    // discovers a node or two per level -- grids, rings).  Trip counts:
    // #sources vs the largest per-node count.
    const uint32_t nsrc = (uint32_t)__popcll(((uint64_t)mhi << 32) | mlo);
    const uint32_t maxpop = wave_max32((uint32_t)__popcll(x));
    if (maxpop * kMsLaneStoreRatio < nsrc) {
      uint64_t m = x;
      for (uint32_t it = 0; it < maxpop; ++it) {
        if (m) {
          const uint32_t s = __ffsll((unsigned long long)m) - 1;
          if (DL) __builtin_nontemporal_store(L, &DL[(size_t)(row0 + s) * pitch + v]);
          if (Dn) Dn[(size_t)(row0 + s) * npitch + v] = (uint8_t)nl;
          m &= m - 1;
        }
      }
      return;
    }
    for (uint64_t m = ((uint64_t)mhi << 32) | mlo; m; m &= m - 1) {
      const uint32_t s = __ffsll((unsigned long long)m) - 1;
      if ((x >> s) & 1ull) {
        if (DL) __builtin_nontemporal_store(L, &DL[(size_t)(row0 + s) * pitch + v]);
        if (Dn) Dn[(size_t)(row0 + s) * npitch + v] = (uint8_t)nl;
      }
    }
  };
  // ---- pull of owned slice i from frontier Fc: the slice's unfinished
  // nodes OR their neighbours' frontier masks; returns the new bits ----
  auto pull = [&](int i, const uint64_t* Fc) -> uint64_t {
    const uint32_t v = sv[i] + lane;
    const bool need = v < N && vis[i] != all;
    uint64_t nx = 0;
    if (__ballot(need)) {  // wave-uniform: the slice has unfinished nodes
      // the slice's column base and width: scalar loads per call (ten
      // slices' pairs held across the level loop spilled SGPRs to VGPR
      // lanes: 110 spills -> 5, fabric_full BFS 0.161 -> 0.157 ms)
      uint32_t sl = sv[i] / kSliceW;
      asm volatile("" : "+s"(sl));
      const uint32_t sbi = sell_ptr[sl];
      const uint32_t w = (sell_ptr[sl + 1] - sbi) / kSliceW;
      const uint32_t* cp = sell_col + sbi + lane;
      const uint16_t* lp = lcol + sbi + lane;
      uint64_t acc = 0;
      uint32_t j = 0;
      if constexpr (!LCOL) {
        // columns from L2: two groups of kMsUnroll loads in flight, issued
        // unconditionally (sell_col is padded past its last slice; columns
        // past w read the next slice's valid ids and are not ORed) -- a load
        // under a branch makes the join's wait count drain the group in
        // flight, one L2 round trip per group
        // buffer loads: the slice's column base in an SGPR, the lane's
        // offset in a VGPR (a 64-bit address pair per owned slice spilled)
        uint32_t ca[kMsUnroll], cb[kMsUnroll];
        auto load = [&](uint32_t j0, uint32_t (&c)[kMsUnroll]) {
#pragma unroll
          for (int u = 0; u < kMsUnroll; ++u)
            c[u] = __builtin_amdgcn_raw_buffer_load_b32(crs, (int)(lane * 4u),
                                                        (int)((sbi + (j0 + u) * kSliceW) * 4u), 0);
        };
        auto fold = [&](const uint32_t (&c)[kMsUnroll], uint32_t n) {
          uint64_t f[kMsUnroll];
#pragma unroll
          for (int u = 0; u < kMsUnroll; ++u) f[u] = Fc[c[u]];
#pragma unroll
          for (int u = 0; u < kMsUnroll; ++u)
            if ((uint32_t)u < n) acc |= f[u];
        };
        load(0, ca);
        for (; j < w; j += 2 * kMsUnroll) {
          load(j + kMsUnroll, cb);
          fold(ca, w - j);
          load(j + 2 * kMsUnroll, ca);
          if (j + kMsUnroll < w) fold(cb, w - j - kMsUnroll);
        }
        if (need) {
          nx = acc & ~vis[i];
          vis[i] |= nx;
        }
        return nx;
      }
      // LDS columns: kMsUnroll loads at a time, then the remainder in groups
      // of 4, 2, 1 (w is wave-uniform: scalar branches, no F reads wasted on
      // padding -- the LDS port is what bounds the sweep)
      for (; j + kMsUnroll <= w; j += kMsUnroll) {
        uint32_t c[kMsUnroll];
#pragma unroll
        for (int u = 0; u < kMsUnroll; ++u)
          c[u] = LCOL ? (uint32_t)lp[(j + u) * kSliceW] : cp[(j + u) * kSliceW];
#pragma unroll
        for (int u = 0; u < kMsUnroll; ++u) acc |= Fc[c[u]];
      }
#pragma unroll
      for (int g = kMsUnroll / 2; g >= 1; g >>= 1) {
        if (j + g <= w) {
          uint32_t c[kMsUnroll / 2];
#pragma unroll
          for (int u = 0; u < g; ++u)
            c[u] = LCOL ? (uint32_t)lp[(j + u) * kSliceW] : cp[(j + u) * kSliceW];
#pragma unroll
          for (int u = 0; u < g; ++u) acc |= Fc[c[u]];
          j += g;
        }
      }
      if (need) {
        nx = acc & ~vis[i];
        vis[i] |= nx;
      }
    }
    return nx;
  };
  uint32_t last = 0;  // deepest level of the batch
  if constexpr (Q) {
    // flag[L mod 3] as in the double-buffered loop below.  Buffer L & 1 of CF
    // holds level L's frontier and of QA its rows' results; the other two are
    // cleared during the row phase (their last readers passed a barrier).
    for (uint32_t L = 0;; ++L) {
      const uint64_t* CFc = CF + (L & 1u) * (q_nc + 1);
      uint64_t* CFn = CF + ((L + 1) & 1u) * (q_nc + 1);
      uint64_t* QAc = QA + (L & 1u) * (q_nc + 1);
      uint64_t* QAn = QA + ((L + 1) & 1u) * (q_nc + 1);
      for (uint32_t r = tid; r < q_nv; r += kMsThreads) {
        uint32_t k[kQChunk];
#pragma unroll
        for (uint32_t j = 0; j < kQChunk; ++j) k[j] = vcol[j * q_nvp + r];
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t j = 0; j < kQChunk; ++j) acc |= CFc[k[j]];
        if (acc) atomicOr(reinterpret_cast<unsigned long long*>(&QAc[vrow[r]]), acc);
      }
      for (uint32_t t = tid; t <= q_nc; t += kMsThreads) {
        CFn[t] = 0;
        QAn[t] = 0;
      }
      MS_STAMP();
      __syncthreads();
      MS_STAMP();
      uint64_t any = 0;
#pragma unroll
      for (int i = 0; i < OWN; ++i) {
        const uint64_t nx = QAc[cl[i]] & ~vis[i];  // (nodes past N: slot q_nc, 0)
        vis[i] |= nx;
        const uint64_t f = ((drained >> i) & 1u) ? own_bits(sv[i] + lane, nx) : nx;
        if (f) atomicOr(reinterpret_cast<unsigned long long*>(&CFn[cl[i]]), f);
        any |= nx;
        record(i, nx, L + 1);
      }
      if (any) flag[L % 3] = 1;
      if (tid == 0) flag[(L + 1) % 3] = 0;
      MS_STAMP();
      __syncthreads();
      MS_STAMP();
      if (!flag[L % 3]) {
        last = L;
        break;
      }
    }
  } else if constexpr (DB) {
    // Double-buffered frontier (graphs whose two F arrays fit in LDS): a
    // slice is pulled from level L's frontier, its level L + 1 bits go
    // straight into the other buffer and its stores are issued at once --
    // one barrier per level, no per-slice state kept across it.
    // flag[L mod 3]: set during level L, read after its barrier, cleared
    // during level L + 2's predecessor (its last readers passed a barrier).
#pragma unroll
    for (int i = 0; i < OWN; ++i) record(i, nv[i], 1);
    uint64_t* Fc = F;
    uint64_t* Fn = F2;
    for (uint32_t L = 1; level1; ++L) {
      uint64_t any = 0;
#pragma unroll
      for (int i = 0; i < OWN; ++i) {
        const uint64_t nx = pull(i, Fc);
        const uint32_t v = sv[i] + lane;
        if (v < N) Fn[v] = ((drained >> i) & 1u) ? own_bits(v, nx) : nx;
        any |= nx;
        record(i, nx, L + 1);
      }
      if (any) flag[L % 3] = 1;
      if (tid == 0) flag[(L + 1) % 3] = 0;
      MS_STAMP();
      __syncthreads();
      MS_STAMP();
      if (!flag[L % 3]) {
        last = L;
        break;
      }
      uint64_t* t = Fc;
      Fc = Fn;
      Fn = t;
    }
  } else {
    for (uint32_t L = 1; level1; ++L) {
#pragma unroll
      for (int i = 0; i < OWN; ++i) record(i, nv[i], L);
      MS_STAMP();
      uint64_t any = 0;
      // ---- pull sweep for level L+1 ----
#pragma unroll
      for (int i = 0; i < OWN; ++i) {
        nv[i] = pull(i, F);
        any |= nv[i];
      }
      MS_STAMP();
      __syncthreads();  // every read of F for this level is done
      MS_STAMP();
#pragma unroll
      for (int i = 0; i < OWN; ++i) {
        const uint32_t v = sv[i] + lane;
        if (v < N) F[v] = ((drained >> i) & 1u) ? own_bits(v, nv[i]) : nv[i];  // drained: own source only
      }
      if (any) flag[L & 1] = 1;
      if (tid == 0) flag[(L + 1) & 1] = 0;
      __syncthreads();
      if (!flag[L & 1]) {
        last = L;
        break;
      }
    }
  }
  // the plan's deepest level: how many bit planes the sliced rows need
  if (maxd && tid == 0) atomicMax(maxd, last);
  MS_STAMP();
  // ---- unreachable (s, v) pairs and row padding ----
  uint64_t miss = 0;
#pragma unroll
  for (int i = 0; i < OWN; ++i)
    if (sv[i] + lane < N) miss |= ~vis[i] & all;
  for (uint64_t m = wave_or64(miss); m; m &= m - 1) {
    const uint32_t s = __ffsll((unsigned long long)m) - 1;
    uint32_t* drow = D + (size_t)(row0 + s) * pitch;
    uint8_t* nrow = Dn + (size_t)(row0 + s) * npitch;
#pragma unroll
    for (int i = 0; i < OWN; ++i) {
      const uint32_t v = sv[i] + lane;
      if (v < N && !((vis[i] >> s) & 1ull)) {
        if (D && d_from == 0) __builtin_nontemporal_store(kInf, &drow[v]);
        if (Dn) nrow[v] = 0xFF;
      }
    }
  }
  {  // row padding past N: one flat (row, entry) index over the workgroup
    const uint32_t pw = npitch - N, tot = nb * pw;
    for (uint32_t t = tid; t < tot; t += kMsThreads) {
      const uint32_t s = t / pw, v = N + t % pw;
      if (D && d_from == 0 && v < pitch) __builtin_nontemporal_store(kInf, &D[(size_t)(row0 + s) * pitch + v]);
      if (Dn) Dn[(size_t)(row0 + s) * npitch + v] = 0xFF;
    }
  }
  MS_STAMP();
  if (stamp) my_stamps[0] = n_stamp;
#undef MS_STAMP
}

// ---------------------------------------------------------------------------
//  1c. multi-source BFS with register-resident distances (bit planes)
// ---------------------------------------------------------------------------
// msbfs_kernel writes every (source, node) distance at the level it is found:
// on a large-diameter graph (grid100: 198 levels) a 64-node slice of a source
// row is found over dozens of levels, so its lines leave L2 partially written
// again and again (PMC: 3.1 GB written for a 0.4 GB result).  This variant
// keeps the distances on chip and writes each row once, coalesced:
//   * <= 32 sources per workgroup, u32 masks (F in LDS is 4 B/node);
//   * for every owned node, 8 bit planes: bit s of plane b = bit b of
//     d(source s, node) -- a level L ORs the new mask into the planes of L's
//     set bits (uniform branches, popcount(L) ORs per node);
//   * at the end, per source, lane v assembles its distance from the planes
//     and the wave stores 64 consecutive entries of the row (and of the u8
//     copy when the next-hop pass reads narrow rows).
// Planes hold 255 levels (a window); a search deeper than that flushes the
// window, marks the entries found so far and starts the next window.
// Register budget: 8 planes + visited + new per owned node = 10 VGPRs, so
// OWN <= 10 (N <= 10240); the host picks msbfs_kernel otherwise.
// (kPlBatch: spf_units.h)
constexpr int kPlanes = 8;
constexpr uint32_t kPlWindow = (1u << kPlanes) - 1;  // relative levels 0..254, 255 = marker
//   Columns: SELL-64 packed four u16 byte offsets (4 * id) per lane (uint2), every live slice
//   at least one group wide (padding id N, F[N] == 0), staged in LDS when
//   they fit.  Group 0 of all owned slices is straight-line code (a grid's
//   whole sweep: one 8-byte column load and four F loads per node); lanes
//   whose node is finished read F[N] (a broadcast).
//   F is double-buffered: one barrier per level.

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <int OWN, bool LCOL>
__global__ __launch_bounds__(kMsThreads) void msbfs_planes_kernel(
    const uint32_t* __restrict__ sell4_ptr, const uint2* __restrict__ sell4, uint32_t n4,
    const uint8_t* __restrict__ ovl, const uint32_t* __restrict__ rows_src, uint32_t n_rows,
    uint32_t bs, uint32_t N, uint32_t pitch, uint32_t npitch, uint32_t* __restrict__ D,
    uint8_t* __restrict__ Dn, const uint32_t* __restrict__ order /* slot -> row, or null */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint2* lcol = reinterpret_cast<uint2*>(smem);                   // [n4] (LCOL)
  // F0/F1: one word per owned node slot (OWN * 1024 >= N + 1); slots past
  // N keep F = 0 (their vis is `all`), so every slot is written unconditionally
  constexpr uint32_t kF = OWN * kMsThreads;
  uint32_t* F0 = reinterpret_cast<uint32_t*>(smem + (LCOL ? 8ull * n4 : 0));  // [kF]
  uint32_t* F1 = F0 + kF;                                         // [kF]
  uint32_t* o_node = F1 + kF;                                     // [32] drained batch sources
  uint32_t* o_cnt = o_node + kPlBatch;                            // [1]
  uint32_t* flag = o_cnt + 1;                                     // [3] progress, L mod 3

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t row0 = blockIdx.x * bs;  // bs <= 32
  const uint32_t nb = min(bs, n_rows - row0);
  const uint32_t all = nb == 32 ? ~0u : ((1u << nb) - 1u);
  // column entries from L2 by buffer loads: the slice's entry base in an
  // SGPR, the lane's offset in a VGPR (per-slice 64-bit addresses spilled)
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint2*>(sell4), 0, (int)(n4 * 8u), 0x00020000);
  auto col4 = [&](uint32_t entry, uint32_t ln) -> uint2 {
    const u32x2 x = __builtin_amdgcn_raw_buffer_load_b64(crs, (int)(ln * 8u), (int)(entry * 8u), 0);
    return make_uint2(x.x, x.y);
  };

  for (uint32_t v = tid; v < kF; v += kMsThreads) F0[v] = F1[v] = 0;
  if (LCOL)
    for (uint32_t t = tid; t < n4; t += kMsThreads) lcol[t] = sell4[t];
  if (tid == 0) {
    *o_cnt = 0;
    flag[0] = flag[1] = flag[2] = 0;
  }
  __syncthreads();
  if (tid < nb) {
    const uint32_t src = rows_src[order ? order[row0 + tid] : row0 + tid];
    F0[src] = 1u << tid;  // sources of a batch are distinct
    if (ovl[src]) o_node[atomicAdd(o_cnt, 1u)] = src | (tid << 24);
  }
  __syncthreads();
  const uint32_t n_osrc = *o_cnt;

  uint32_t vis[OWN], P[OWN][kPlanes];
  uint32_t dslices = 0;  // bit i: owned slice i holds a drained node (wave-uniform)
  uint32_t dlane = 0;    // bit i: this lane's node of slot i is drained (no ovl loads per level)
  uint32_t sb[OWN], sg[OWN];  // owned slice i: first packed entry, groups (wave-uniform)
#pragma unroll
  for (int i = 0; i < OWN; ++i) {
    const uint32_t v = tid + i * kMsThreads;
    vis[i] = v < N ? F0[v] : all;
#pragma unroll
    for (int b = 0; b < kPlanes; ++b) P[i][b] = 0u;
    const bool dr = v < N && ovl[v];
    dlane |= (uint32_t)dr << i;
    if (__ballot(dr)) dslices |= 1u << i;
    const uint32_t slice = (tid - lane + i * kMsThreads) / kSliceW;
    const bool live = slice * kSliceW < N;
    const uint32_t b = live ? sell4_ptr[slice] : 0u;
    const uint32_t e = live ? sell4_ptr[slice + 1] : kSliceW;
    sb[i] = __builtin_amdgcn_readfirstlane(b);
    sg[i] = __builtin_amdgcn_readfirstlane((e - b) / kSliceW);
  }

  uint32_t base = 0;  // level of relative value 0 in the current window
  for (uint32_t L = 1;; ++L) {
    const uint32_t* Fc = (L & 1) ? F0 : F1;  // frontier of level L - 1
    uint32_t* Fn = (L & 1) ? F1 : F0;        // frontier of level L
    // opaque lane id, recomputed per level: hoisting the owned slices'
    // addresses out of the level loop would spill
    uint32_t ln = tid;
    asm volatile("" : "+v"(ln));
    ln &= 63u;
    const uint32_t rel = L - base;  // relative level recorded in the planes
    uint32_t any = 0;
    const unsigned char* Fb = reinterpret_cast<const unsigned char*>(Fc);
#define PL_F(off) (*reinterpret_cast<const uint32_t*>(Fb + (off)))
    uint2 qn = LCOL ? lcol[sb[0] + ln] : col4(sb[0], ln);
#pragma unroll
    for (int i = 0; i < OWN; ++i) {
      const uint32_t v = tid + i * kMsThreads;
      uint32_t nx = 0;
      const uint2 q = qn;
      // group 0 of slice i + 1 is loaded while slice i waits for its F reads
      if (i + 1 < OWN) qn = LCOL ? lcol[sb[i + 1] + ln] : col4(sb[i + 1], ln);
      // a uniform branch per slice: skips finished slices and keeps the
      // scheduler from hoisting ten slices' loads (register pressure).
      // No per-lane masking: a finished node gets nx = 0 from ~vis, a slot
      // past N has only padding columns (F[N] == 0).
      if (__ballot(vis[i] != all)) {
        // all four reads in flight before the first use (one LDS round trip)
        uint32_t f0 = PL_F(q.x & 0xFFFFu), f1 = PL_F(q.x >> 16), f2 = PL_F(q.y & 0xFFFFu),
                 f3 = PL_F(q.y >> 16);
        asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3));
        uint32_t acc = f0 | f1 | f2 | f3;
#pragma unroll 1
        for (uint32_t g = 1; g < sg[i]; ++g) {  // wider slices: the remaining groups
          const uint2 r = LCOL ? lcol[sb[i] + g * kSliceW + ln] : col4(sb[i] + g * kSliceW, ln);
          acc |= PL_F(r.x & 0xFFFFu) | PL_F(r.x >> 16) | PL_F(r.y & 0xFFFFu) | PL_F(r.y >> 16);
        }
        nx = acc & ~vis[i];
        vis[i] |= nx;
        any |= nx;
#pragma unroll
        for (int b = 0; b < kPlanes; ++b)
          if ((rel >> b) & 1u) P[i][b] |= nx;
      }
      uint32_t f = nx;
      if ((dslices >> i) & 1u) {  // the slice holds a drained node (uniform test)
        if ((dlane >> i) & 1u) {  // drained: expands only as its own source
          uint32_t own = 0;
          for (uint32_t k = 0; k < n_osrc; ++k)
            if ((o_node[k] & 0xFFFFFFu) == v) own = 1u << (o_node[k] >> 24);
          f &= own;
        }
      }
      Fn[v] = f;
    }
#undef PL_F
    // flag[L mod 3]: set during level L, read after its barrier; cleared
    // during level L - 2 (its last reader finished before barrier L - 1)
    if (any) flag[L % 3] = 1;
    if (tid == 0) flag[(L + 1) % 3] = 0;
    __syncthreads();
    const bool done = !flag[L % 3];
    if (done || rel == kPlWindow - 1) {
      // Flush the window.  The first one writes every entry of the batch's
      // rows (unreached = kInf, row padding); a later one (searches deeper
      // than 254 levels) only the entries found in it -- entries of earlier
      // windows carry the marker value kPlWindow in their planes.
      const bool first = base == 0;
      for (uint32_t s = 0; s < nb; ++s) {
        const uint32_t row = order ? order[row0 + s] : row0 + s;
        uint32_t* drow = D + (size_t)row * pitch;
        uint8_t* nrow = Dn ? Dn + (size_t)row * npitch : nullptr;
#pragma unroll
        for (int i = 0; i < OWN; ++i) {
          const uint32_t v = tid + i * kMsThreads;
          uint32_t r = 0;
#pragma unroll
          for (int b = 0; b < kPlanes; ++b) r |= ((P[i][b] >> s) & 1u) << b;
          const bool seen = v < N && ((vis[i] >> s) & 1u);
          const uint32_t d = seen ? base + r : kInf;
          if (first || (seen && r != kPlWindow)) {
            if (v < pitch) __builtin_nontemporal_store(d, &drow[v]);
            if (nrow && v < npitch) nrow[v] = d == kInf ? 0xFFu : (uint8_t)min(d, 254u);
          }
        }
      }
      if (done) break;
#pragma unroll
      for (int i = 0; i < OWN; ++i)
#pragma unroll
        for (int b = 0; b < kPlanes; ++b) P[i][b] |= vis[i];
      base += kPlWindow;
    }
  }
}

// ---------------------------------------------------------------------------
//  instance tables: one row per entry of SPF_MS_OWNS (graph_host.h), which
//  ms_own's bands come from too.  The launches look a row up by ms_own(N);
//  msbfs_set_lds_limits registers every kernel of every row -- an instance
//  cannot be launched without having been registered.
// ---------------------------------------------------------------------------
using MsbfsFn = decltype(&msbfs_kernel<1, false>);
struct MsbfsInst {
  uint32_t own;
  MsbfsFn plain, lcol, db, q;  // q: null past kQMaxOwn
};
template <int OWN>
constexpr MsbfsInst msbfs_inst() {
  MsbfsInst r{OWN, msbfs_kernel<OWN, false>, msbfs_kernel<OWN, true>, msbfs_kernel<OWN, false, true>, nullptr};
  if constexpr (OWN <= kQMaxOwn) r.q = msbfs_kernel<OWN, false, false, true>;
  return r;
}

constexpr int kPlMaxOwn = 10;  // msbfs_planes_kernel's register budget (N <= 10240)
using PlanesFn = decltype(&msbfs_planes_kernel<1, false>);
struct PlanesInst {
  uint32_t own;
  PlanesFn plain, lcol;  // null past kPlMaxOwn
};
template <int OWN>
constexpr PlanesInst planes_inst() {
  PlanesInst r{OWN, nullptr, nullptr};
  if constexpr (OWN <= kPlMaxOwn) {
    r.plain = msbfs_planes_kernel<OWN, false>;
    r.lcol = msbfs_planes_kernel<OWN, true>;
  }
  return r;
}

#define MS_INST(o) msbfs_inst<o>(),
#define PL_INST(o) planes_inst<o>(),
constexpr MsbfsInst kMsbfsTab[] = {SPF_MS_OWNS(MS_INST)};
constexpr PlanesInst kPlanesTab[] = {SPF_MS_OWNS(PL_INST)};
#undef PL_INST
#undef MS_INST

// the row of ms_own(N) (ms_own returns entries of the list the tables are made
// of); null when the row holds no kernel
template <typename Inst, size_t K>
const Inst* inst_of(const Inst (&tab)[K], uint32_t own) {
  for (const Inst& r : tab)
    if (r.own == own && r.plain) return &r;
  return nullptr;
}

// ---------------------------------------------------------------------------
//  LDS sizes and sources per workgroup
// ---------------------------------------------------------------------------
size_t msbfs_lds_bytes(uint32_t N, bool db = false) {
  return 8ull * (N + 1) * (db ? 2 : 1) + 4ull * (4 * kMsBatch + 5);
}

// msbfs_kernel with a double-buffered frontier: when the columns do not fit
// in LDS beside one F array but two F arrays do (SPF_MSBFS_DB=0: single, A/B)
bool ms_double_buffer(const spf_ctx* c) {
  const char* e = std::getenv("SPF_MSBFS_DB");
  if (e && e[0] == '0') return false;
  const size_t n_col = c->sell_ptr.back();
  return msbfs_lds_bytes(c->N) + 2ull * n_col > kMaxLds && msbfs_lds_bytes(c->N, true) <= kMaxLds;
}

// LDS of msbfs_kernel's quotient variant: CF and QA (two buffers each), the
// row/column tables, the small arrays, the source marks
size_t msbfs_q_lds_bytes(uint32_t N, uint32_t n_cls, uint32_t n_vrow) {
  const size_t nvp = (n_vrow + 7u) & ~7u;
  return 32ull * (n_cls + 1) + 2ull * (1 + kQChunk) * nvp + 4ull * (4 * kMsBatch + 5) + ((N + 3u) & ~3u);
}

size_t planes_lds_bytes(uint32_t own) { return 8ull * own * kMsThreads + 4ull * (kPlBatch + 4); }

// Sources per workgroup that spread `rows` over every CU: the fewest rounds
// of `full`-source workgroups the chip needs, then those rounds filled evenly
// (a batch costs one edge sweep per level whatever its size, but its stores
// scale with it).
uint32_t spread_batch(const spf_ctx* c, uint32_t rows, uint32_t full) {
  const uint32_t rounds = (rows + full * c->n_cu - 1) / (full * c->n_cu);
  return std::min<uint32_t>(full, (rows + rounds * c->n_cu - 1) / (rounds * c->n_cu));
}

// ---------------------------------------------------------------------------
//  launches: one typed helper per kernel, the argument list written once
// ---------------------------------------------------------------------------
// msbfs_kernel: the quotient sweep when the graph has one, else the columns in
// LDS when they fit beside F, else the double-buffered frontier when two F
// arrays fit, else the plain sweep.
// One workgroup per CU per round: a batch costs one edge sweep per level
// whatever its size, but its stores scale with it, so the sources are spread
// over every CU rather than filling 64-source batches on fewer CUs.
void msbfs_launch(spf_ctx* c, const MsbfsInst& k, const uint32_t* rows_src, uint32_t rows, uint32_t* D,
                  uint8_t* Dn, uint32_t* maxd, uint32_t d_from, hipStream_t s) {
  const uint32_t n_col = c->sell_ptr.back();
  const size_t lds_col = msbfs_lds_bytes(c->N) + 2ull * n_col;
  const bool q = k.q && use_quotient(c);
  MsbfsFn fn = k.plain;
  size_t lds = msbfs_lds_bytes(c->N);
  if (q) fn = k.q, lds = msbfs_q_lds_bytes(c->N, c->qt.n_cls, c->qt.n_vrow);
  else if (lds_col <= kMaxLds) fn = k.lcol, lds = lds_col;
  else if (ms_double_buffer(c)) fn = k.db, lds = msbfs_lds_bytes(c->N, true);
  const uint32_t bs = ms_batch(c, rows);
  hipLaunchKernelGGL(fn, dim3((rows + bs - 1) / bs), dim3(kMsThreads), lds, s, c->d_sell_ptr.p,
                     c->d_sell_col.p, n_col, c->d_row_ptr.p, c->d_col.p, c->d_ovl.p, rows_src, rows, bs,
                     c->N, c->pitch, c->npitch, D, Dn, maxd, d_from, c->d_ms_smap.p, c->d_stamps.p,
                     q ? c->d_qcls.p : nullptr, q ? c->d_qtab.p : nullptr, q ? c->qt.n_cls : 0u,
                     q ? c->qt.n_vrow : 0u);
}

//   order (optional): rows sorted by estimated eccentricity, deepest first.
//   A batch runs until its deepest source's search ends, so batches of
//   similar depth waste no levels, and the deep ones start first while the
//   shallow ones fill the CUs that free up (grid 100x100: eccentricities
//   100..198; 313 full batches are 1.22 rounds of the chip); without it the
//   batches are spread evenly over rounds.
void planes_launch(spf_ctx* c, const PlanesInst& k, const uint32_t* rows_src, uint32_t rows, uint32_t* D,
                   uint8_t* Dn, const uint32_t* order, hipStream_t s) {
  const uint32_t n4 = c->sell4_ptr.back();
  const size_t lds = planes_lds_bytes(k.own), lds_col = lds + 8ull * n4;
  const bool lcol = lds_col <= kMaxLds;
  const uint32_t bs = planes_batch(c, rows, order != nullptr);
  hipLaunchKernelGGL(lcol ? k.lcol : k.plain, dim3((rows + bs - 1) / bs), dim3(kMsThreads),
                     lcol ? lds_col : lds, s, c->d_sell4_ptr.p, reinterpret_cast<const uint2*>(c->d_sell4.p),
                     n4, c->d_ovl.p, rows_src, rows, bs, c->N, c->pitch, c->npitch, D, Dn, order);
}

}  // namespace

namespace spfi {

// The quotient sweep is taken when it reads at most half the columns of the
// plain one (a grid or a ring has no twins: every node its own class) and its
// tables fit in LDS.  SPF_QUOTIENT=0 keeps the plain sweep (A/B, parity tests).
bool quotient_allowed(const spf_ctx* c) {
  if (c->N > kMsMaxNodes || ms_own(c->N) > (uint32_t)kQMaxOwn) return false;
  const char* e = std::getenv("SPF_QUOTIENT");
  return !(e && e[0] == '0');
}

bool use_quotient(const spf_ctx* c) {
  const spf_ctx::Quotient& q = c->qt;
  if (!quotient_allowed(c) || q.stale || q.n_cls == 0 || 2 * q.n_edge > c->nb_id.size()) return false;
  return msbfs_q_lds_bytes(c->N, q.n_cls, q.n_vrow) <= kMaxLds;
}

// Which BFS variant: the register-plane kernel needs N <= 10240; it wins
// when levels are many (partial-line rewrites dominate msbfs_kernel) and
// loses when the edge sweep dominates (it runs 32 sources per sweep, not
// 64).  SPF_MSBFS=planes|masks overrides (experiments).
bool use_planes(const spf_ctx* c) {
  if (c->N > (uint32_t)kPlMaxOwn * kMsThreads || c->sell4.empty()) return false;
  if (const char* e = std::getenv("SPF_MSBFS")) return e[0] == 'p';
  return c->sell_ptr.back() <= 8ull * c->N;  // sliced-ELL width <= 8 on average
}

uint32_t ms_batch(const spf_ctx* c, uint32_t rows, bool knob) {
  if (const char* e = knob ? std::getenv("SPF_MSBFS_BATCH") : nullptr) {
    const int b = atoi(e);
    if (b >= 1 && b <= (int)kMsBatch) return (uint32_t)b;
  }
  return spread_batch(c, rows, kMsBatch);
}

uint32_t planes_batch(const spf_ctx* c, uint32_t rows, bool ordered) {
  return ordered ? kPlBatch : spread_batch(c, rows, kPlBatch);
}

spf_status msbfs_set_lds_limits(spf_ctx* c) {
  for (const MsbfsInst& k : kMsbfsTab)
    for (MsbfsFn fn : {k.plain, k.lcol, k.db, k.q}) {
      const spf_status st = fn ? raise_lds_limit(c, (const void*)fn) : SPF_OK;
      if (st != SPF_OK) return st;
    }
  for (const PlanesInst& k : kPlanesTab)
    for (PlanesFn fn : {k.plain, k.lcol}) {
      const spf_status st = fn ? raise_lds_limit(c, (const void*)fn) : SPF_OK;
      if (st != SPF_OK) return st;
    }
  return SPF_OK;
}

spf_status launch_msbfs(spf_ctx* c, const uint32_t* rows_src, uint32_t rows, uint32_t* D, uint8_t* Dn,
                        uint32_t* maxd, hipStream_t s, uint32_t d_from, const uint32_t* order) {
  if (!c->d_stamps.p && std::getenv("SPF_STAMPS")) {
    HIP_TRY(c, c->d_stamps.alloc(kStampWords));
    HIP_TRY(c, hipMemsetAsync(c->d_stamps.p, 0, 64 * 16 * 8, s));
    const unsigned long long wg = std::strtoull(std::getenv("SPF_STAMPS"), nullptr, 10);
    HIP_TRY(c, hipMemcpyAsync(c->d_stamps.p + 64 * 16, &wg, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  const uint32_t own = ms_own(c->N);
  if (use_planes(c)) {
    const PlanesInst* k = inst_of(kPlanesTab, own);
    if (!k) return fail(c, SPF_E_UNSUPPORTED, "no msbfs_planes_kernel instance owns %u slots", own);
    planes_launch(c, *k, rows_src, rows, D, Dn, order, s);
    HIP_TRY(c, hipGetLastError());
    return SPF_OK;
  }
  if (quotient_allowed(c)) {  // (else the tables stay stale: nothing is built for a path not taken)
    const spf_status st = quotient_prepare(c);
    if (st != SPF_OK) return st;
  }
  const MsbfsInst* k = inst_of(kMsbfsTab, own);
  if (!k) return fail(c, SPF_E_UNSUPPORTED, "no msbfs_kernel instance owns %u slots", own);
  msbfs_launch(c, *k, rows_src, rows, D, Dn, maxd, d_from, s);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

}  // namespace spfi
