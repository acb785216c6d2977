// ============================================================================
//  class_rows.hip -- class-row plans (unit metrics on a graph with a twin-class
//  quotient): class_bfs_kernel solves one BFS row per twin
//  class among the closure rows, expand_rows_kernel writes the node rows (u32,
//  bit planes, u8) from them.  The kernels, their LDS sizes, whether a graph's
//  tables fit, the two launches and plan_ensure_narrow.
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spf_units.h"
#include "wave_ops.h"

using namespace spfi;

namespace {

// ---------------------------------------------------------------------------
//  1d. class rows: the BFS over class sources, and the rows expanded from it
// ---------------------------------------------------------------------------
// On a quotient graph d(s, v), v != s, depends only on the classes of s and
// v: msbfs_kernel's Q sweep with classes for nodes.  A class
// source's bit starts in its class's frontier slot and expands whatever its
// drain bit; its own class is not marked visited, so it is reached again
// through a forwarding neighbour (level 2, usually) and Dc[k][own class]
// comes out as the distance of the source's twins.  A class reached later
// forwards when one of its members is not drained (fwd).  Visited masks live
// in LDS (VIS): a thread owns classes tid, tid + 1024, ...
// Dc[k][c] (u16, 0xFFFF unreachable, also the padding up to cpitch) is stored
// per level, 64 consecutive classes of one class source per wave store.
__global__ __launch_bounds__(kMsThreads) void class_bfs_kernel(
    const uint16_t* __restrict__ q_cls, const uint16_t* __restrict__ q_tab, uint32_t q_nc,
    uint32_t q_nv, const uint32_t* __restrict__ csrc, uint32_t K, uint32_t bs,
    const uint8_t* __restrict__ fwd, uint16_t* __restrict__ Dc, uint32_t cpitch,
    uint32_t* __restrict__ maxd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t q_nvp = (q_nv + 7u) & ~7u;
  const uint32_t nc1 = (q_nc + 2u) & ~1u;  // slots per array: q_nc + 1, even (16-byte tables behind)
  uint64_t* const CF = reinterpret_cast<uint64_t*>(smem);  // [2][nc1]
  uint64_t* const QA = CF + 2 * nc1;                       // [2][nc1]
  uint64_t* const VIS = QA + 2 * nc1;                      // [nc1]
  uint16_t* const vrow = reinterpret_cast<uint16_t*>(VIS + nc1);  // [q_nvp]
  uint16_t* const vcol = vrow + q_nvp;                                    // [kQChunk][q_nvp]
  uint32_t* const flag = reinterpret_cast<uint32_t*>(vcol + kQChunk * q_nvp);  // [4]
  uint8_t* const fw = reinterpret_cast<uint8_t*>(flag + 4);                    // [q_nc]

  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t row0 = blockIdx.x * bs;
  const uint32_t nb = min(bs, K - row0);
  const uint64_t all = nb == 64 ? ~0ull : ((1ull << nb) - 1ull);
  for (uint32_t t = tid; t < 5 * nc1; t += kMsThreads) CF[t] = 0;  // CF, QA, VIS
  const uint4* tab4 = reinterpret_cast<const uint4*>(q_tab);
  for (uint32_t t = tid; t < (1 + kQChunk) * q_nvp / 8; t += kMsThreads)
    reinterpret_cast<uint4*>(vrow)[t] = tab4[t];
  for (uint32_t t = tid; t < q_nc; t += kMsThreads) fw[t] = fwd[t];
  if (tid < 3) flag[tid] = 0;
  __syncthreads();
  if (tid < nb)
    atomicOr(reinterpret_cast<unsigned long long*>(&CF[q_cls[csrc[row0 + tid]]]), 1ull << tid);
  __syncthreads();
  uint32_t last = 0;
  for (uint32_t L = 0;; ++L) {
    const uint64_t* CFc = CF + (L & 1u) * nc1;
    uint64_t* CFn = CF + ((L + 1) & 1u) * nc1;
    uint64_t* QAc = QA + (L & 1u) * nc1;
    uint64_t* QAn = QA + ((L + 1) & 1u) * nc1;
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
    __syncthreads();
    uint64_t any = 0;
    for (uint32_t t0 = tid - lane; t0 < q_nc; t0 += kMsThreads) {  // wave-uniform trips
      const uint32_t t = t0 + lane;
      uint64_t nx = 0;
      if (t < q_nc) {
        const uint64_t v = VIS[t];
        nx = QAc[t] & ~v;
        if (nx) {
          VIS[t] = v | nx;
          if (fw[t]) CFn[t] = nx;
        }
      }
      any |= nx;
      for (uint64_t m = wave_or64(nx); m; m &= m - 1) {
        const uint32_t s = __ffsll((unsigned long long)m) - 1;
        if ((nx >> s) & 1ull) Dc[(size_t)(row0 + s) * cpitch + t] = (uint16_t)(L + 1);
      }
    }
    if (any) flag[L % 3] = 1;
    if (tid == 0) flag[(L + 1) % 3] = 0;
    __syncthreads();
    if (!flag[L % 3]) {
      last = L;
      break;
    }
  }
  if (tid == 0) atomicMax(maxd, last);
  // unreachable classes and the padding of the batch's rows
  for (uint32_t t0 = tid - lane; t0 < q_nc; t0 += kMsThreads) {
    const uint32_t t = t0 + lane;
    const uint64_t miss = t < q_nc ? ~VIS[t] & all : 0ull;
    for (uint64_t m = wave_or64(miss); m; m &= m - 1) {
      const uint32_t s = __ffsll((unsigned long long)m) - 1;
      if ((miss >> s) & 1ull) Dc[(size_t)(row0 + s) * cpitch + t] = 0xFFFFu;
    }
  }
  const uint32_t pw = cpitch - q_nc;
  for (uint32_t t = tid; t < nb * pw; t += kMsThreads)
    Dc[(size_t)(row0 + t / pw) * cpitch + q_nc + t % pw] = 0xFFFFu;
}

// Node rows from class rows.  A workgroup owns whole groups of kExRows
// closure rows over the row width (small plans: a range of the width,
// plan_expand_grid).  Per group it stages the rows' class rows once -- thread
// o reads classes 8o .. 8o + 7 of each row's Dc row with one 16-byte load and
// writes them transposed, T[class] = its kExRows distances (u16), over all
// q_nc classes (T[q_nc]: the padding past N, always unreachable) -- and then
// its waves sweep the width in pieces of kExPiece nodes, four per lane: the
// lane's class ids from q_cls (L2), four 16-byte LDS loads, one 16-byte store
// per row.  T is double-buffered: the next group's Dc loads are issued before
// the sweep and written to the other half behind it, one barrier per group.
//   d(closure[r], v) = Dc[crow_of[r]][class of v]; the node closure[r] itself
//   gets 0.
//   D:  the u32 rows (pitch; unreachable and padding kInf), streaming stores.
//   S:  with maxd < kSlSat, the rows' bit planes in ecmp_sliced_kernel's
//       layout (S + r * kSlSlots * wpm + w * P): a thread's four nodes give a
//       nibble per plane, eight lanes' nibbles one word (three xor shuffles),
//       and lane 8q + b of a wave stores plane b of the wave's word q.
//   Dn: the u8 rows (npitch; min(d, 254), 255 unreachable and padding).
// Any of the three may be null.
#ifndef SPF_EX_THREADS
#define SPF_EX_THREADS 1024
#endif
constexpr uint32_t kExThreads = SPF_EX_THREADS;  // (build-time A/B)
constexpr uint32_t kExWaves = kExThreads / 64;
constexpr uint32_t kExMaxCls = 8 * kExThreads - 8;  // one class octet per thread, the padding's entry behind
// entries of one half of T: q_nc classes and the padding's, whole octets
__host__ __device__ constexpr uint32_t ex_entries(uint32_t q_nc) { return (q_nc + 8u) & ~7u; }

// classes 8o .. 8o + 7 of the group's rows (a row past the plan's last, or an
// octet past the class pitch: unreachable)
__device__ __forceinline__ void ex_stage_load(uint4 (&x)[kExRows], const uint16_t* __restrict__ Dc,
                                              uint32_t cpitch, const uint32_t* __restrict__ crow_of,
                                              uint32_t r0, uint32_t rows, uint32_t o) {
#pragma unroll
  for (uint32_t j = 0; j < kExRows; ++j) {
    x[j] = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (r0 + j < rows && 8u * o < cpitch)
      x[j] = *reinterpret_cast<const uint4*>(Dc + (size_t)crow_of[r0 + j] * cpitch + 8u * o);
  }
}

// ... transposed into T[8o .. 8o + 7]
__device__ __forceinline__ void ex_stage_write(uint4* __restrict__ T, const uint4 (&x)[kExRows], uint32_t o) {
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    uint32_t h[kExRows];
#pragma unroll
    for (uint32_t j = 0; j < kExRows; ++j) {
      const uint32_t w = i / 2 == 0 ? x[j].x : i / 2 == 1 ? x[j].y : i / 2 == 2 ? x[j].z : x[j].w;
      h[j] = (i & 1u) ? w >> 16 : w & 0xFFFFu;
    }
    T[8u * o + i] = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
  }
}

__global__ __launch_bounds__(kExThreads) void expand_rows_kernel(
    const uint16_t* __restrict__ Dc, uint32_t cpitch, const uint32_t* __restrict__ crow_of,
    const uint32_t* __restrict__ closure, uint32_t rows, uint32_t gper, uint32_t pieces, uint32_t pps,
    const uint16_t* __restrict__ q_cls, uint32_t q_nc, uint32_t N, uint32_t pitch, uint32_t npitch,
    uint32_t* __restrict__ D, uint8_t* __restrict__ Dn, uint32_t* __restrict__ S,
    const uint32_t* __restrict__ maxd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t nT = ex_entries(q_nc);
  uint4* const T = reinterpret_cast<uint4*>(smem);  // [2][nT]

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t groups = (rows + kExRows - 1) / kExRows;
  const uint32_t g_begin = blockIdx.x * gper, g_end = min(groups, g_begin + gper);
  const uint32_t p_begin = blockIdx.y * pps, p_end = min(pieces, p_begin + pps);
  const uint32_t md = *maxd;
  const uint32_t P = (S && md < kSlSat) ? 32u - __clz(md + 1u) : 0u;
  const uint32_t wpm = pitch / 32;
  const bool stager = tid < nT / 8;
  // the plane the lane stores of its eight lanes' word (32 nodes)
  const uint32_t pb = lane & 7u, nsh = 4u * pb;

  uint4 x[kExRows];
  if (stager && g_begin < g_end) {
    ex_stage_load(x, Dc, cpitch, crow_of, g_begin * kExRows, rows, tid);
    ex_stage_write(T, x, tid);
  }
  for (uint32_t g = g_begin; g < g_end; ++g) {
    const uint4* const cur = T + ((g - g_begin) & 1u) * nT;
    __syncthreads();  // this group's half is written, the other half's readers are through
    const bool more = stager && g + 1 < g_end;
    if (more) ex_stage_load(x, Dc, cpitch, crow_of, (g + 1) * kExRows, rows, tid);
    const uint32_t r0 = g * kExRows, nr = min(kExRows, rows - r0);
    for (uint32_t pc = p_begin + wave; pc < p_end; pc += kExWaves) {
      const uint32_t pbase = pc * kExPiece, v0 = pbase + lane * 4;
      uint32_t cl[4];
      if (v0 + 4 <= N) {
        const uint2 c2 = *reinterpret_cast<const uint2*>(q_cls + v0);
        cl[0] = c2.x & 0xFFFFu, cl[1] = c2.x >> 16, cl[2] = c2.y & 0xFFFFu, cl[3] = c2.y >> 16;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) cl[k] = v0 + k < N ? q_cls[v0 + k] : q_nc;
      }
      uint4 t[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = cur[cl[k]];
      const uint32_t w = v0 / 32;
      const bool d_live = D && v0 < pitch, n_live = Dn && v0 < npitch, s_live = pb < P && w < wpm;
#pragma unroll
      for (uint32_t j = 0; j < kExRows; ++j) {
        if (j >= nr) break;  // uniform
        const uint32_t r = r0 + j;
        uint32_t d[4];  // 0xFFFF sign-extends to kInf; finite distances stay below 2^15
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t pair = j / 2 == 0 ? t[k].x : j / 2 == 1 ? t[k].y : j / 2 == 2 ? t[k].z : t[k].w;
          d[k] = (uint32_t)(int32_t)(int16_t)(pair >> (16 * (j & 1)));
        }
        const uint32_t own = closure[r];  // the row's own node: distance 0
        if (own - pbase < kExPiece) {     // uniform
          const uint32_t self = own - v0;
#pragma unroll
          for (int k = 0; k < 4; ++k) d[k] = self == (uint32_t)k ? 0u : d[k];
        }
        if (d_live) {
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 o = {d[0], d[1], d[2], d[3]};
          __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(D + (size_t)r * pitch + v0));
        }
        if (n_live) {
          uint32_t b = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) b |= (d[k] == kInf ? 0xFFu : min(d[k], 254u)) << (8 * k);
          __builtin_nontemporal_store(b, reinterpret_cast<uint32_t*>(Dn + (size_t)r * npitch + v0));
        }
        if (P) {  // uniform
          uint32_t mine = 0;
          for (uint32_t b = 0; b < P; ++b) {
            uint32_t nib = ((d[0] >> b) & 1u) | ((d[1] >> b) & 1u) << 1 | ((d[2] >> b) & 1u) << 2 |
                           ((d[3] >> b) & 1u) << 3;
            nib <<= nsh;
            // lanes ^ 1, ^ 2 (quad permutes), then the other quad of the eight
            // lanes: row_shl 4 into quads 0 and 2, row_shr 4 into quads 1 and 3
            nib |= (uint32_t)__builtin_amdgcn_update_dpp(0u, nib, 0xB1, 0xf, 0xf, true);
            nib |= (uint32_t)__builtin_amdgcn_update_dpp(0u, nib, 0x4E, 0xf, 0xf, true);
            nib |= (uint32_t)__builtin_amdgcn_update_dpp(0u, nib, 0x104, 0xf, 0x5, true) |
                   (uint32_t)__builtin_amdgcn_update_dpp(0u, nib, 0x114, 0xf, 0xa, true);
            mine = pb == b ? nib : mine;
          }
          // (plain stores: the next-hop pass reads the planes next, from L2;
          // streaming ones cost it 12 us on fabric_full)
          if (s_live) S[(size_t)r * kSlSlots * wpm + (size_t)w * P + pb] = mine;
        }
      }
    }
    if (more) ex_stage_write(T + ((g + 1 - g_begin) & 1u) * nT, x, tid);
  }
}

// LDS of class_bfs_kernel (frontiers, row results and visited masks per class,
// the quotient tables, the flags, the forwards bytes) and of expand_rows_kernel
// (both halves of the staged class rows)
size_t class_bfs_lds_bytes(uint32_t n_cls, uint32_t n_vrow) {
  const size_t nvp = (n_vrow + 7u) & ~7u, nc1 = (n_cls + 2u) & ~1u;
  return 40ull * nc1 + 2ull * (1 + kQChunk) * nvp + 16 + ((n_cls + 15u) & ~15u);
}
size_t expand_lds_bytes(uint32_t n_cls) { return 2ull * 16 * ex_entries(n_cls); }

}  // namespace

namespace spfi {

spf_status class_rows_set_lds_limits(spf_ctx* c) {
  for (const void* k : {(const void*)class_bfs_kernel, (const void*)expand_rows_kernel}) {
    const spf_status st = raise_lds_limit(c, k);
    if (st != SPF_OK) return st;
  }
  return SPF_OK;
}

// Class rows need the quotient sweep and both kernels' tables in LDS, and a
// class octet per thread of the expansion's staging.
bool class_rows_fit(const spf_ctx* c) {
  return use_quotient(c) && class_bfs_lds_bytes(c->qt.n_cls, c->qt.n_vrow) <= kMaxLds &&
         c->qt.n_cls <= kExMaxCls && expand_lds_bytes(c->qt.n_cls) <= kMaxLds;
}

// The plan's class sources, spread over the CUs as ms_batch spreads rows.
spf_status launch_class_bfs(spf_ctx* c, spf_plan* p, hipStream_t s) {
  const uint32_t bs = ms_batch(c, p->cls_k);
  hipLaunchKernelGGL(class_bfs_kernel, dim3((p->cls_k + bs - 1) / bs), dim3(kMsThreads),
                     class_bfs_lds_bytes(c->qt.n_cls, c->qt.n_vrow), s, c->d_qcls.p, c->d_qtab.p,
                     c->qt.n_cls, c->qt.n_vrow, p->d_csrc.p, p->cls_k, bs, p->d_cfwd.p, p->d_Dc.p,
                     p->cls_pitch, p->d_maxd.p);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

// Workgroups of the expansion the chip holds at once: what its LDS and its
// registers let a CU hold, by the runtime's own count, times CUs.
uint32_t expand_resident(const spf_ctx* c) {
  static size_t for_lds = 0;
  static int per_cu = 0;
  const size_t lds = expand_lds_bytes(c->qt.n_cls);
  if (lds != for_lds) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, expand_rows_kernel, (int)kExThreads, lds) != hipSuccess)
      n = 0;
    per_cu = std::max(1, n);
    for_lds = lds;
  }
  return c->n_cu * (uint32_t)per_cu;
}

// The closure rows from the class rows: u32 rows into D, bit planes into S,
// u8 rows into Dn (each optional); the grid by plan_expand_grid.
spf_status launch_expand(spf_ctx* c, spf_plan* p, uint32_t* D, uint8_t* Dn, uint32_t* S,
                         hipStream_t s) {
  const uint32_t rows = (uint32_t)p->closure.size();
  const uint32_t span = std::max((D || S) ? c->pitch : 0u, Dn ? c->npitch : 0u);
  const ExpandGrid eg = plan_expand_grid(rows, span, expand_resident(c));
  hipLaunchKernelGGL(expand_rows_kernel, dim3(eg.wgs, eg.splits), dim3(kExThreads),
                     expand_lds_bytes(c->qt.n_cls), s, p->d_Dc.p, p->cls_pitch, p->d_crow_of.p,
                     p->d_closure.p, rows, eg.gper, eg.pieces, eg.pps, c->d_qcls.p, c->qt.n_cls, c->N,
                     c->pitch, c->npitch, D, Dn, S, p->d_maxd.p);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status plan_ensure_narrow(spf_plan* p, hipStream_t s) {
  spf_ctx* c = p->ctx;
  if (!plan_has_narrow(p)) return fail(c, SPF_E_UNSUPPORTED, "the plan keeps no u8 rows");
  if (!p->cls || p->keep_narrow) return SPF_OK;
  // a class plan asked for the first time: the rows of its last execute from
  // that execute's class rows, and every later expansion writes them too
  const size_t n_rows = p->closure.size();
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, p->d_Dn.alloc((n_rows + 1) * c->npitch));
  HIP_TRY(c, hipMemsetAsync(p->d_Dn.p + n_rows * c->npitch, 0xFF, c->npitch, s));
  p->keep_narrow = true;
  return p->cls_ready ? launch_expand(c, p, nullptr, p->d_Dn.p, nullptr, s) : SPF_OK;
}

}  // namespace spfi
