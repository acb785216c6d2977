// ============================================================================
//  sssp.hip -- single-source shortest paths, one workgroup per source row
//  (sssp_kernel): weighted plans that mssp_kernel does not take, spf_sssp, and
//  every caller of launch_sssp (KSP2, routes, mssp's overflow rows).  The
//  kernel, its LDS size, its instance table, its launch and spf_sssp.
// ============================================================================
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "spf_units.h"
#include "wave_ops.h"

using namespace spfi;

namespace {

// LDS control words of the SSSP kernel
enum { C_QLEN = 0, C_NBIG = 1, C_NWORDS = 4 };

// ---------------------------------------------------------------------------
//  1. single-source shortest paths, one workgroup per source row
// ---------------------------------------------------------------------------
//   THREADS: a workgroup's distance row sits in LDS, so a large graph fits
//   only one or two workgroups per CU; those then get 1024 threads, so the
//   CU still holds 32 waves of relaxations in flight (PMC r02_v9, fabric_rtt
//   with 256 threads: 75 % of wave cycles waiting, ~8 waves per CU).
template <typename QT, bool UNIT, int THREADS>
__global__ __launch_bounds__(THREADS) void sssp_kernel(
    const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
    const uint32_t* __restrict__ wt, const uint8_t* __restrict__ ovl,
    const uint32_t* __restrict__ link, const uint32_t* __restrict__ ign,
    const uint32_t* __restrict__ rows_src, uint32_t N, uint32_t pitch,
    uint32_t bm_words, uint32_t big_cap, uint32_t* __restrict__ D,
    uint8_t* __restrict__ Dn /* optional u8 copy (npitch == pitch) */,
    const uint32_t* __restrict__ redo /* optional [count, rows...]: redo only those rows */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* dist = reinterpret_cast<uint32_t*>(smem);  // [pitch]
  uint32_t* bm = dist + pitch;                         // [bm_words] next frontier
  uint32_t* ctl = bm + bm_words;                       // [C_NWORDS]
  uint32_t* big = ctl + C_NWORDS;                      // [big_cap]
  QT* q = reinterpret_cast<QT*>(big + big_cap);        // [N] frontier list

  const uint32_t tid = threadIdx.x;
  const uint32_t lane = lane_id();
  const uint32_t wave = tid >> 6;
  constexpr uint32_t kWaves = THREADS / 64;
  uint32_t row = blockIdx.x;
  if (redo) {  // mssp_kernel's overflow rows (launched over all rows, mostly empty)
    if (row >= redo[0]) return;
    row = redo[1 + row];
  }
  const uint32_t src = rows_src[row];

  for (uint32_t v = tid; v < pitch; v += THREADS) dist[v] = kInf;
  for (uint32_t i = tid; i < bm_words; i += THREADS) bm[i] = 0;
  if (tid == 0) {
    ctl[C_QLEN] = 0;
    ctl[C_NBIG] = 0;
  }
  __syncthreads();
  if (tid == 0) {
    dist[src] = 0;
    q[0] = (QT)src;
  }
  __syncthreads();

  uint32_t qlen = 1;
  while (qlen != 0) {
    // ---- expand: small-degree nodes one per thread, big ones per wave ----
    for (uint32_t i = tid; i < qlen; i += THREADS) {
      const uint32_t u = q[i];
      if (ovl[u] && u != src) continue;  // drained node: recorded, not expanded
      const uint32_t b = row_ptr[u], e = row_ptr[u + 1];
      if (e - b > kBigDeg) {
        big[atomicAdd(&ctl[C_NBIG], 1u)] = u;
        continue;
      }
      const uint32_t du = dist[u];
      for (uint32_t k = b; k < e; ++k) {
        if (ign && link_ignored(ign, link[k])) continue;  // KSP linksToIgnore
        const uint32_t v = col[k];
        const uint32_t nd = du + (UNIT ? 1u : wt[k]);
        if (UNIT) {
          // level-synchronous BFS: every writer of v writes the same value
          if (dist[v] > nd) {
            dist[v] = nd;
            atomicOr(&bm[v >> 5], 1u << (v & 31));
          }
        } else {
          if (nd < atomicMin(&dist[v], nd)) atomicOr(&bm[v >> 5], 1u << (v & 31));
        }
      }
    }
    __syncthreads();
    const uint32_t nbig = ctl[C_NBIG];
    for (uint32_t i = wave; i < nbig; i += kWaves) {
      const uint32_t u = big[i];
      const uint32_t du = dist[u];
      const uint32_t e = row_ptr[u + 1];
      for (uint32_t k = row_ptr[u] + lane; k < e; k += 64) {
        if (ign && link_ignored(ign, link[k])) continue;
        const uint32_t v = col[k];
        const uint32_t nd = du + (UNIT ? 1u : wt[k]);
        if (UNIT) {
          if (dist[v] > nd) {
            dist[v] = nd;
            atomicOr(&bm[v >> 5], 1u << (v & 31));
          }
        } else {
          if (nd < atomicMin(&dist[v], nd)) atomicOr(&bm[v >> 5], 1u << (v & 31));
        }
      }
    }
    __syncthreads();
    if (tid == 0) ctl[C_NBIG] = 0;  // every thread has read nbig by now

    // ---- compact the next-frontier bitmap into q (wave ballot/scan) ----
    for (uint32_t base = 0; base < bm_words; base += THREADS) {
      const uint32_t i = base + tid;
      uint32_t word = 0;
      if (i < bm_words) {
        word = bm[i];
        bm[i] = 0;
      }
      uint32_t tot;
      const uint32_t pre = wave_excl_scan(__popc(word), &tot);
      uint32_t at = 0;
      if (lane == 0 && tot) at = atomicAdd(&ctl[C_QLEN], tot);
      at = __builtin_amdgcn_readlane(at, 0) + pre;
      while (word) {
        const uint32_t b = __ffs(word) - 1;
        word &= word - 1;
        q[at++] = (QT)(i * 32 + b);
      }
    }
    __syncthreads();
    qlen = ctl[C_QLEN];
    __syncthreads();
    if (tid == 0) ctl[C_QLEN] = 0;
  }
  __syncthreads();

  // ---- write the distance row (16-byte stores) and, for narrow plans, its
  // u8 copy (min(d, 254), 255 = unreachable) for the next-hop pass ----
  uint4* out = reinterpret_cast<uint4*>(D + (size_t)row * pitch);
  const uint4* in = reinterpret_cast<const uint4*>(dist);
  for (uint32_t i = tid; i < pitch / 4; i += THREADS) {
    const uint4 d = in[i];
    out[i] = d;
    if (Dn) {
      const uint32_t x[4] = {d.x, d.y, d.z, d.w};
      uint32_t b = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) b |= (x[k] == kInf ? 0xFFu : min(x[k], 254u)) << (8 * k);
      reinterpret_cast<uint32_t*>(Dn + (size_t)row * pitch)[i] = b;
    }
  }
}

// Every instance, written once: launch_sssp picks a row, sssp_set_lds_limits
// walks them all.
using SsspFn = decltype(&sssp_kernel<uint16_t, true, 256>);
struct SsspInst {
  bool q16, unit;
  uint32_t threads;
  SsspFn fn;
};
#define SSSP_ROWS(QT, U)                                                                     \
  {sizeof(QT) == 2, U, 256, sssp_kernel<QT, U, 256>}, {sizeof(QT) == 2, U, 512, sssp_kernel<QT, U, 512>}, \
      {sizeof(QT) == 2, U, 1024, sssp_kernel<QT, U, 1024>}
constexpr SsspInst kSssp[] = {SSSP_ROWS(uint16_t, true), SSSP_ROWS(uint16_t, false), SSSP_ROWS(uint32_t, true),
                              SSSP_ROWS(uint32_t, false)};
#undef SSSP_ROWS

}  // namespace

namespace spfi {

size_t sssp_lds_bytes(uint32_t N, uint32_t pitch, uint32_t big, bool q16) {
  const uint32_t bm_words = (N + 31) / 32;
  size_t b = 4ull * pitch + 4ull * bm_words + 4ull * C_NWORDS + 4ull * big;
  b += (q16 ? 2ull : 4ull) * N;
  return (b + 15) & ~size_t(15);
}

spf_status sssp_set_lds_limits(spf_ctx* c) {
  for (const SsspInst& k : kSssp) {
    const spf_status st = raise_lds_limit(c, (const void*)k.fn);
    if (st != SPF_OK) return st;
  }
  return SPF_OK;
}

// Launch the SSSP kernel over `rows` closure rows (device list rows_src).
spf_status launch_sssp(spf_ctx* c, const uint32_t* rows_src, uint32_t rows, bool hop,
                       const uint32_t* ign, uint32_t* D, hipStream_t s, const uint32_t* wt,
                       const uint8_t* ovl, uint8_t* Dn, const uint32_t* redo) {
  if (!wt) wt = c->d_wt.p;
  if (!ovl) ovl = c->d_ovl.p;
  const uint32_t N = c->N, pitch = c->pitch, bm_words = (N + 31) / 32;
  const bool q16 = N <= 65535;
  const size_t lds = sssp_lds_bytes(N, pitch, c->big_nodes, q16);
  const bool unit = hop || c->max_metric == 1;
  // threads per workgroup from how many workgroups the LDS row lets a CU hold
  // (SPF_SSSP_THREADS overrides, experiments)
  uint32_t threads = lds > kMaxLds / 3 ? 1024u : lds > kMaxLds / 6 ? 512u : 256u;
  if (const char* e = std::getenv("SPF_SSSP_THREADS")) threads = (uint32_t)atoi(e);
  threads = threads >= 1024 ? 1024u : threads >= 512 ? 512u : 256u;
  for (const SsspInst& k : kSssp) {
    if (k.q16 != q16 || k.unit != unit || k.threads != threads) continue;
    hipLaunchKernelGGL(k.fn, dim3(rows), dim3(threads), lds, s, c->d_row_ptr.p, c->d_col.p, wt, ovl,
                       c->d_link.p, ign, rows_src, N, pitch, bm_words, c->big_nodes, D, Dn, redo);
    HIP_TRY(c, hipGetLastError());
    return SPF_OK;
  }
  return fail(c, SPF_E_INVALID, "launch_sssp: no sssp_kernel instance");  // (the table holds all twelve)
}

}  // namespace spfi

extern "C" {

spf_status spf_sssp(spf_ctx* c, uint32_t src, uint32_t flags, const uint32_t* ignore_links,
                    uint32_t n_ignore, uint32_t* dist_out) {
  if (!c || !dist_out) return fail(c, SPF_E_INVALID, "spf_sssp: NULL argument");
  if (!c->loaded) return fail(c, SPF_E_STATE, "no graph loaded");
  if (src >= c->N) return fail(c, SPF_E_INVALID, "source %u out of range", src);
  const bool hop = (flags & SPF_FLAG_HOP_COUNT) != 0;
  if (!hop && (c->nonpos || c->needs64)) {  // the exact kernel (u32 rows when they fit)
    if (c->needs64)
      return fail(c, SPF_E_UNSUPPORTED, "weighted distances may exceed 32 bits: use spf_solve_exact");
    return spf_solve_exact(c, src, flags, ignore_links, n_ignore, nullptr, dist_out, nullptr,
                           nullptr);
  }
  spf_status st = set_lds_limits(c);
  if (st != SPF_OK) return st;
  const uint32_t* ign = nullptr;
  st = upload_ignore(c, ignore_links, n_ignore, &ign);
  if (st != SPF_OK) return st;
  HIP_TRY(c, c->d_one_src.upload(&src, 1, c->stream));
  HIP_TRY(c, c->d_row.alloc(c->pitch));
  const bool grid_resident = sssp_lds_bytes(c->N, c->pitch, c->big_nodes, c->N <= 65535) > kMaxLds;
  if (grid_resident) {
    st = launch_gsssp(c, src, hop, ign, c->d_row.p, c->stream);
  } else {
    st = launch_sssp(c, c->d_one_src.p, 1, hop, ign, c->d_row.p, c->stream);
  }
  if (st != SPF_OK) return st;
  HIP_TRY(c, hipMemcpyAsync(dist_out, c->d_row.p, 4ull * c->N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->solves += 1;
  return grid_resident ? spf_device_check(c) : SPF_OK;
}

}  // extern "C"
