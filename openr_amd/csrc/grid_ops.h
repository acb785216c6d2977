// ============================================================================
//  grid_ops.h -- what the grid-resident and team kernels are made of below any
//  method: the context's fault word, agent-scope loads and stores, the graph as
//  a kernel argument, bounded barrier spins and the XCD-hierarchical grid
//  barrier, lanes over flattened edges.  grid_spf.hip (the engine's large-graph
//  kernels) and whatif_repair.h (the what-if repairs) are built from it; every
//  unit that raises a fault bit includes it for the bit's name.
//
//  Constants and inline functions only: including this file emits no kernel.
//  The device part sits in an unnamed namespace, so no symbol is shared between
//  the code objects that include it; a host-only unit (engine_ctx.cpp, which
//  decodes the fault word) sees the constants alone.
// ============================================================================
#ifndef OPENR_AMD_GRID_OPS_H
#define OPENR_AMD_GRID_OPS_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spfi {

// The context's fault word (spf_ctx::d_fault): kernels OR bits into it, the
// host reads and clears it (spf_device_check, engine_ctx.cpp) and reports
// SPF_E_HIP instead of the launches' output.  One word per context, so a check
// on one context neither reports nor clears another's.
constexpr uint32_t kFaultGridBarrier = 1u << 0;  // a grid barrier timed out (XGrid, team_sync)
constexpr uint32_t kFaultTeamBarrier = 1u << 1;  // a team BFS barrier timed out (msbfs_team.hip)
constexpr uint32_t kFaultLoopBound = 1u << 3;    // a repair loop hit its bound: the phase field
constexpr uint32_t kFaultRange = 1u << 4;        // a range check of the profiled instances failed: the site field
constexpr uint32_t kFaultProfRow = 1u << 5;      // a profile row is outside its buffer: the kernel field
constexpr uint32_t kFaultListRoom = 1u << 6;     // a list entry past its allocated count (dropped)
constexpr uint32_t kFaultPhaseShift = 8, kFaultSiteShift = 16, kFaultKernelShift = 24;  // 8-bit fields

// Counters of one grid barrier (XGrid below), zeroed before each launch: one
// 128-byte line per counter.
constexpr uint32_t kBarPad = 32;
constexpr uint32_t kGridBarWords = 17 * kBarPad;  // cnt[8], top, gen[8]

}  // namespace spfi

#ifdef __HIPCC__

namespace {

__device__ __forceinline__ uint32_t ld(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Wave-wide minimum with DPP moves (row shifts, then row broadcasts; lanes
// with no source keep ~0u) -- __shfl compiles to ds_bpermute, an LDS round
// trip per step.  Every lane of the wave must be active.
__device__ __forceinline__ uint32_t wave_min32(uint32_t x) {
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(~0u, x, 0x111, 0xf, 0xf, false));  // row_shr:1
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(~0u, x, 0x112, 0xf, 0xf, false));  // row_shr:2
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(~0u, x, 0x114, 0xf, 0xf, false));  // row_shr:4
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(~0u, x, 0x118, 0xf, 0xf, false));  // row_shr:8
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(~0u, x, 0x142, 0xa, 0xf, false));  // row_bcast:15
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp(~0u, x, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return __builtin_amdgcn_readlane(x, 63);
}

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

struct WiGraph {
  const uint32_t* row_ptr;
  const uint32_t* col;
  const uint32_t* wt;
  const uint32_t* rev;
  const uint32_t* link;
  const uint8_t* ovl;
  const uint32_t* nbr_bit;  // [N] j if v is the src's j-th distinct neighbour, else kInf
  uint32_t N, src, W;
  uint32_t hop = 0;  // hop counts: every up link weighs 1 (useLinkMetric = false)
  uint32_t* fault = nullptr;  // the context's barrier-timeout word (spf_device_check)
  // per CSR edge, interleaved: {col, wt, link, wt of the reverse edge} -- one
  // 16-byte load where the wave teams' repairs read four arrays (and the
  // rev -> wt chain) at random nodes (what-if plans)
  const uint4* ed = nullptr;
};

// directed weight of the edge reverse to e (tail -> head of the in-edge)
__device__ __forceinline__ uint32_t in_w(const WiGraph& g, uint32_t e) {
  return g.hop ? 1u : g.wt[g.rev[e]];
}

constexpr uint32_t kBarSpin = 1u << 26;            // ~seconds: never a silent hang

// A barrier spin that ran out (a member never arrived: not co-resident, or
// a fault) sets the launching context's fault word and falls through; the
// host reads and clears it (spf_device_check) and reports SPF_E_HIP instead
// of the launch's output.
__device__ __forceinline__ void barrier_timed_out(uint32_t* fault) {
  if (fault) __hip_atomic_fetch_or(fault, spfi::kFaultGridBarrier, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// A repair loop that reached its iteration bound (it cannot, for a correct
// kernel: every bound is the loop's worst case + 2) reports where instead of
// spinning on: kFaultLoopBound, the phase in its field (spf_device_check names
// it).  1 D discovery, 2 label-correcting sweeps, 3 next-hop fixed point.
__device__ __forceinline__ void loop_bound_hit(uint32_t* fault, uint32_t phase) {
  if (fault)
    __hip_atomic_fetch_or(fault, spfi::kFaultLoopBound | (phase << spfi::kFaultPhaseShift), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_SYSTEM);
}

// After one barrier timed out the launch's results are void; later barriers
// must not each wait out their own spin (a desynchronised team would cross
// thousands of them): a spin polls the fault word every 1024 polls and gives
// up once it is set.
__device__ __forceinline__ bool fault_set(const uint32_t* fault) {
  return fault && __hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

// inclusive prefix sum over the wave (DPP row shifts + row broadcasts)
__device__ __forceinline__ uint32_t wave_incl_scan32(uint32_t x) {
  x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, true);   // row_shr:1
  x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, true);   // row_shr:2
  x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, true);   // row_shr:4
  x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, true);   // row_shr:8
  x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return x;
}

// ---------------------------------------------------------------------------
//  wave helpers: lanes over flattened edges
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_pull(uint32_t x, uint32_t k) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(k << 2), (int)x);
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The edges of up to 64 nodes (lane k holds node v, `valid`), flattened:
// chunks of 64 (node slot, edge) pairs.  f(k, e, act) runs on every lane of
// the wave (so it may ballot / pull); `act` marks the lanes holding an edge,
// k is the node slot (lane) that edge belongs to.  All 64 lanes must be
// active.
template <class F>
__device__ __forceinline__ void wave_edges(const uint32_t* __restrict__ row_ptr, uint32_t v,
                                           bool valid, F&& f) {
  const uint32_t lane = threadIdx.x & 63;
  uint32_t b0 = 0, deg = 0;
  if (valid) {
    b0 = row_ptr[v];
    deg = row_ptr[v + 1] - b0;
  }
  const uint32_t incl = wave_incl_scan32(deg);
  const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
  const uint32_t excl = incl - deg;
  for (uint32_t base = 0; base < total; base += 64) {
    const uint32_t s = base + lane;
    // owner: the last slot whose first edge is <= s (slots with no edges
    // share their successor's offset and lose to it)
    uint32_t k = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1)
      if (lane_pull(excl, k + step) <= s) k += step;
    const uint32_t e = lane_pull(b0, k) + s - lane_pull(excl, k);
    f(k, e, s < total);
  }
}

// Grid barrier of the grid-resident kernels, XCD-hierarchical (MI355X_MICROARCH
// barrier-xcd: 4.1 us at 256 workgroups against 26.3 us for the software
// cooperative_groups grid sync, which the what-if base pass crossed ~70
// times).  Blocks are grouped by blockIdx % 8 (the XCD round-robin of the
// dispatcher); each arrival bumps its group's counter, the group's last
// arrival bumps the top counter, waits for every group and publishes the
// generation its group polls.  Counters only grow within a launch (the k-th
// barrier completes at k arrivals per block) and are zeroed before each
// launch (kGridBarWords words, one 128-byte line per counter).
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
      uint32_t* top = bar + 8 * spfi::kBarPad;
      uint32_t* gen = bar + (9 + x) * spfi::kBarPad;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const uint32_t t =
          __hip_atomic_fetch_add(bar + x * spfi::kBarPad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

}  // namespace

#endif  // __HIPCC__

#endif  // OPENR_AMD_GRID_OPS_H
