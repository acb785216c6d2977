// ============================================================================
//  ecmp.hip -- the next-hop (ECMP) passes over a plan's distance rows:
//  ecmp_kernel (u8 narrow rows or exact u32 rows), slice_rows_kernel (u8 rows
//  -> bit-sliced rows) and ecmp_sliced_kernel (bit-sliced rows, unit and
//  weighted matches, grouped sources), with their three launches.  For
//  positive metrics x in nh_s(v) <=> (x == v or x not drained) and
//  w(s, x) + d_x(v) == d_s(v) over the distinct up neighbours x of s
//  (DESIGN.md §3): a streaming compare of rows, one bit per neighbour.
// ============================================================================
#include <hip/hip_runtime.h>

#include <algorithm>

#include "spf_units.h"

using namespace spfi;

namespace {

constexpr int kEcmpThreads = 256;

// ---------------------------------------------------------------------------
//  2. next-hop (ECMP) pass
// ---------------------------------------------------------------------------
// Output: per source, one destination bitmap per distinct up neighbour x
// (ascending id): bit v of bitmap j <=> neighbour j is in nh_s(v).  Each wave
// owns a 1024-destination chunk and stores, per neighbour, 32 consecutive u32
// words.
//   NARROW: distances from the u8 copy: lane l loads destinations
//           cbase + 16l .. +15 of the neighbour's row (16 bytes), compares
//           them with the precomputed targets d_s(v) - 1 into a 16-bit mask,
//           and even lanes merge their odd neighbour's half into one word; a
//           wave whose source row holds a saturated entry (>= 254) decides on
//           the exact u32 rows instead.
//   exact:  u32 rows, one coalesced dword load per 64 destinations.

constexpr int kEcmpUnroll = 4;         // neighbour rows per group (two groups in flight)
constexpr uint32_t kEcmpChunk = 1024;  // destinations per wave
constexpr uint32_t kEcmpWaves = kEcmpThreads / 64;

// Zero-byte flags of x at bit 7 of each byte (exact: no carries cross bytes).
__device__ __forceinline__ uint32_t zero_bytes(uint32_t x) {
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// Byte-equality mask of a lane's 16-byte narrow slice against its packed
// targets: bit n = destination cbase + 16*lane + n.  Dword k byte b is
// destination 4k + b; shifting dword k's zero-byte flags right by 3 - k puts
// it at bit 8b + 4 + k (high nibbles), a shift-or and a byte permute pack the
// nibbles to bit 4b + k, and two delta swaps transpose that 4x4 bit matrix
// to bit 4k + b.
__device__ __forceinline__ uint32_t eq_mask16(const uint4& a, const uint4& t) {
  const uint32_t z = (zero_bytes(a.x ^ t.x) >> 3) | (zero_bytes(a.y ^ t.y) >> 2) |
                     (zero_bytes(a.z ^ t.z) >> 1) | zero_bytes(a.w ^ t.w);
  uint32_t x = __builtin_amdgcn_perm(0u, z | (z << 4), 0x0c0c0301u);
  uint32_t d = (x ^ (x >> 3)) & 0x0A0Au;
  x ^= d ^ (d << 3);
  d = (x ^ (x >> 6)) & 0x00CCu;
  return x ^ d ^ (d << 6);
}

// Weighted narrow match without per-neighbour targets: bit n (eq_mask16's
// order) set iff a_n + w == s_n for the neighbour's byte a_n and the
// source's byte s_n, bytes split into 16-bit halves so the add cannot carry
// (SWAR: ~12 ops per 4 destinations where deriving targets d_s - w per
// neighbour cost ~100 per 16).  No false matches: a = 255 (unreachable,
// drained neighbour's dead row) or 254 (saturated) sums past every
// unsaturated source byte; s = 255 needs a finite a only through a drained
// x, whose row is the dead row; s = 0 (the source) needs w = 0.  w >= 254
// matches nothing in the fast path (the source bytes stay below 254).
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t weighted_mask16(const uint4& a4, const uint32_t (&sl)[4],
                                                    const uint32_t (&sh)[4], uint32_t w) {
  if (w >= 0xFEu) return 0u;
  const u16x2 W2 = {(unsigned short)w, (unsigned short)w};
  const u16x2 one = {1, 1};
  const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w};
  // per word q: bytes 0, 2 and bytes 1, 3 as 16-bit halves (v_perm), a + w
  // and the xor with the source's halves packed (v_pk_add_u16), zero halves
  // -> 1 by a saturating 1 - x (v_pk_sub_u16 clamp); the four result bits
  // land at 4q, 4q + 1 (bytes 0, 1) and 16 + 4q, 17 + 4q (bytes 2, 3)
  uint32_t T = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const u16x2 lo = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(0u, a[q], 0x0c020c00u));
    const u16x2 hi = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm(0u, a[q], 0x0c030c01u));
    const uint32_t xl = __builtin_bit_cast(uint32_t, (u16x2)(lo + W2)) ^ sl[q];
    const uint32_t xh = __builtin_bit_cast(uint32_t, (u16x2)(hi + W2)) ^ sh[q];
    const uint32_t zl = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(one, __builtin_bit_cast(u16x2, xl)));
    const uint32_t zh = __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(one, __builtin_bit_cast(u16x2, xh)));
    T |= (zl | (zh << 1)) << (4 * q);
  }
  return (T | (T >> 14)) & 0xFFFFu;
}

// nb_row[nb_row_off[i] + j]: byte offset in Dn (row * npitch) of the narrow
// row of the request's source i's neighbour j (ascending id) -- the D row
// itself for plans without narrow rows -- or `dead` if it is drained: the
// offset of an all-0xFF row after the plan's narrow rows (kInf without them).
// Each source's list starts 16-byte aligned and is padded with `dead` to
// roundup(k, 8) + 8 entries (the pipelined loads run one group ahead).  nb_drained[i] counts the drained neighbours.
// Every per-neighbour quantity is wave-uniform and read with scalar loads:
// no LDS staging, no workgroup barriers -- a wave is independent.
template <bool NARROW>
__global__ __launch_bounds__(kEcmpThreads) void ecmp_kernel(
    const uint8_t* __restrict__ Dn, uint32_t npitch, const uint32_t* __restrict__ D,
    uint32_t pitch, uint32_t N, const uint32_t* __restrict__ req_src,
    const uint32_t* __restrict__ row_of, const uint32_t* __restrict__ nb_ptr,
    const uint32_t* __restrict__ nb_id, const uint32_t* __restrict__ nb_w,
    const uint32_t* __restrict__ nb_row, const uint32_t* __restrict__ nb_row_off,
    const uint32_t* __restrict__ nb_drained, uint32_t dead, uint32_t hop, uint32_t weighted,
    const uint64_t* __restrict__ nh_off, uint32_t* __restrict__ nh, uint32_t chunks,
    const uint32_t* __restrict__ slot_src) {
  // Block b runs on XCD b % 8.  slot_src (spf_plan_create) lists each XCD's
  // sources: runs of consecutive request sources (the racks of one pod, the
  // spines of one plane -- the same neighbour rows, shared in that XCD's L2)
  // dealt to the XCDs by work; a source's chunks are consecutive blocks.
  // (Long-lived blocks walking the list were slower at every size tried,
  // profiles/r02_v10_ab_ecmp_blocks.txt.)
  const uint32_t grp = blockIdx.x & 7, pos = blockIdx.x >> 3;
  const uint32_t i = slot_src[(pos / chunks) * 8 + grp];
  const uint32_t c = pos % chunks;
  if (i == kInf) return;
  const uint32_t s = req_src[i];
  const uint32_t nb0 = nb_ptr[s], k = nb_ptr[s + 1] - nb0;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t cbase = (c * kEcmpWaves + (threadIdx.x >> 6)) * kEcmpChunk;
  if (k == 0 || cbase >= N) return;  // whole wave: no barriers below
  const uint32_t srow = row_of[s];
  const uint32_t wpm = pitch / 32;  // u32 words per bitmap
  const uint32_t* offs = nb_row + nb_row_off[i];
  uint32_t* out_w = nh + nh_off[i] + cbase / 32;  // word base of bitmap 0

  // NARROW: the u8 value a neighbour must hold at this lane's 16 slice
  // bytes, packed like the row; 0xFE = none (never held by a non-drained
  // neighbour where the source row is not saturated: d_x(s) = w(x, s) < 0xFE,
  // and a node s cannot reach no neighbour reaches either)
  uint4 tg = make_uint4(0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu, 0xFEFEFEFEu);
  uint4 raw = tg;  // the source's 16 bytes (weighted matches derive targets per neighbour)
  bool exact = !NARROW;
  if (NARROW) {
    raw = *reinterpret_cast<const uint4*>(Dn + (size_t)srow * npitch + cbase + lane * 16);
    const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t t[4];
    bool sat = false;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      uint32_t o = 0;
#pragma unroll
      for (int bq = 0; bq < 4; ++bq) {
        const uint32_t x = (rw[w] >> (8 * bq)) & 0xFFu;
        sat |= x == 0xFEu;
        o |= ((x == 0u || x >= 0xFEu) ? 0xFEu : x - 1u) << (8 * bq);  // d_x = d_s - 1
      }
      t[w] = o;
    }
    tg = make_uint4(t[0], t[1], t[2], t[3]);
    exact = __ballot(sat) != 0;
  }

  if (!exact) {
    // fast path: lane l stores the 16-bit slice of destinations
    // cbase + 16l .. +15; two groups of kEcmpUnroll neighbour rows in flight
    // (ping-pong); a drained neighbour's row reads as "unreachable" (0xFF
    // never equals a target) and its single possible bit is patched below
    const bool st = cbase / 16 + lane < pitch / 16;
    const uint32_t loff = lane * 16;
    const uint8_t* dn_c = Dn + cbase;
    // weighted: the source's bytes as 16-bit halves (weighted_mask16)
    uint32_t ssl[4], ssh[4];
    {
      const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ssl[q] = rw[q] & 0x00FF00FFu;
        ssh[q] = (rw[q] >> 8) & 0x00FF00FFu;
      }
    }
    // unconditional loads (drained neighbours and list padding point at the
    // all-0xFF dead row), so the waits count exactly: group B's loads stay in
    // flight while group A is matched
    auto load_group = [&](uint32_t j0, uint4* r) {
      const uint4 o4 = *reinterpret_cast<const uint4*>(offs + j0);  // one scalar load
      const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
      for (int u = 0; u < kEcmpUnroll; ++u) r[u] = *reinterpret_cast<const uint4*>(dn_c + o[u] + loff);
    };
    auto match_group = [&](uint32_t j0, const uint4* r) {
#pragma unroll
      for (int u = 0; u < kEcmpUnroll; ++u) {
        if (j0 + u >= k) break;
        uint32_t m;
        if (weighted) {  // wave-uniform: d_x + w(s, x) == d_s, byte-wise
          m = weighted_mask16(r[u], ssl, ssh, nb_w[nb0 + j0 + u]);
        } else {
          m = eq_mask16(r[u], tg);
        }
        uint16_t* o = reinterpret_cast<uint16_t*>(out_w + (size_t)(j0 + u) * wpm);
        if (st) __builtin_nontemporal_store((uint16_t)m, &o[lane]);
      }
    };
    uint4 ra[kEcmpUnroll], rb[kEcmpUnroll];
    load_group(0, ra);
    for (uint32_t j0 = 0; j0 < k; j0 += 2 * kEcmpUnroll) {
      load_group(j0 + kEcmpUnroll, rb);
      match_group(j0, ra);
      load_group(j0 + 2 * kEcmpUnroll, ra);
      match_group(j0 + kEcmpUnroll, rb);
    }
  } else {
    // exact u32 rows ("wide"): lane l holds the source's distances of
    // destinations cbase + 16l .. +15 in registers and, per neighbour, compares
    // four 16-byte loads of the neighbour's row: bit k set iff
    // d_x(v) + w(s, x) == d_s(v) (d_x finite; then the sum stays below kInf).
    // Same 16-bit lane stores as the narrow path.
    const bool st = cbase / 16 + lane < pitch / 16;
    uint32_t b[16];
    {
      const uint4* Ds = reinterpret_cast<const uint4*>(D + (size_t)srow * pitch + cbase) + lane * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 t = st ? Ds[q] : make_uint4(kInf, kInf, kInf, kInf);
        b[4 * q] = t.x;
        b[4 * q + 1] = t.y;
        b[4 * q + 2] = t.z;
        b[4 * q + 3] = t.w;
      }
    }
    for (uint32_t j = 0; j < k; ++j) {
      const uint32_t oj = offs[j], wj = hop ? 1u : nb_w[nb0 + j];
      uint32_t m = 0;
      if (oj != dead && st) {
        const uint32_t rj = NARROW ? oj / npitch : oj;
        const uint4* Dx = reinterpret_cast<const uint4*>(D + (size_t)rj * pitch + cbase) + lane * 4;
        uint4 t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = Dx[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t a[4] = {t[q].x, t[q].y, t[q].z, t[q].w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            m |= (uint32_t)(a[e] != kInf && a[e] + wj == b[4 * q + e]) << (4 * q + e);
        }
      }
      if (st) __builtin_nontemporal_store((uint16_t)m, &reinterpret_cast<uint16_t*>(out_w + (size_t)j * wpm)[lane]);
    }
  }
  // drained neighbour x: its bitmap is empty except, possibly, x itself --
  // reached directly over the link when d_s(x) == w(s, x)
  if (nb_drained[i]) {
    for (uint32_t j = 0; j < k; ++j) {
      if (offs[j] != dead) continue;
      const uint32_t x = nb_id[nb0 + j];
      if (x < cbase || x >= cbase + kEcmpChunk) continue;
      const uint32_t wj = hop ? 1u : nb_w[nb0 + j];
      if (lane == (x - cbase) / 32 && D[(size_t)srow * pitch + x] == wj)
        out_w[(size_t)j * wpm + lane] = 1u << (x & 31);
    }
  }
}

// ---------------------------------------------------------------------------
//  2b. next-hop pass over bit-sliced rows (msbfs_kernel plans)
// ---------------------------------------------------------------------------
// A row's distances as P bit planes: word w of plane b holds bit b of the
// distances of nodes 32w .. 32w + 31 (bit t = node 32w + t); all-ones =
// unreachable.  P = the bits of maxd + 1 (maxd = the plan's deepest BFS
// level, from msbfs_kernel), so every finite distance stays below the
// all-ones code: a fabric (4-5 levels) needs 3 planes, 3/8 of the u8 row.
// With unit metrics (w(s, x) = 1) the test of 32 destinations against one
// neighbour row is OR_b (x_b ^ t_b) == 0 with t = d_s - 1, decremented
// bit-sliced once per source word: ~2 bit operations per plane and
// neighbour word where the byte compare of narrow rows spends ~30 per 16
// destinations, and the result is already the output word (bit v of word
// v / 32 of bitmap j).  When maxd reaches the u8 copy's saturation (254)
// the planes stay unwritten and the pass decides on the u32 rows.
constexpr uint32_t kSlChunk = 2048;  // destinations per pass of a wave: one word per lane
// (kSlSlots plane slots per word of a sliced row, kSlSat: plan_host.h)

// Sliced row r starts at S + r * kSlSlots * wpm; word w's P planes sit at
// w * P .. w * P + P - 1, so a lane's planes are one P-dword load and a
// wave's 64 loads cover 64 * P consecutive dwords.

// u8 narrow rows -> bit-sliced rows; one thread per (row, word): two 16-byte
// loads, P words stored.  With D (expand plans, SPF_EXPAND=1, whose BFS
// stores only the u8 rows) the same thread also writes the row's u32
// distances of its 32 nodes:
// byte b < 254 is the distance, 255 unreachable (kInf, also the row padding),
// and 254 -- saturated, level >= 254 -- keeps the exact value the BFS wrote
// into D for those levels only.
__global__ __launch_bounds__(256) void slice_rows_kernel(const uint8_t* __restrict__ Dn,
                                                         uint32_t npitch, uint32_t rows, uint32_t wpm,
                                                         const uint32_t* __restrict__ maxd,
                                                         uint32_t* __restrict__ S,
                                                         uint32_t* __restrict__ D, uint32_t pitch) {
  const uint32_t md = *maxd;
  const bool planes = md < kSlSat;
  if (!planes && !D) return;
  const uint32_t P = 32u - __clz(md + 1u);
  const uint64_t total = (uint64_t)rows * wpm;
  for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < total;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = (uint32_t)(t / wpm), w = (uint32_t)(t % wpm);
    const uint4* in = reinterpret_cast<const uint4*>(Dn + (size_t)r * npitch + 32ull * w);
    const uint4 a = in[0], b = in[1];
    const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (planes) {
      uint32_t* out = S + (size_t)r * kSlSlots * wpm + (size_t)w * P;
      for (uint32_t pl = 0; pl < P; ++pl) {
        uint32_t word = 0;
        // bit pl of bytes 4q .. 4q + 3 -> bits 4q .. 4q + 3 (the multiply moves
        // byte i's bit to bit 24 + i; no cross term lands in bits 24..31)
#pragma unroll
        for (int q = 0; q < 8; ++q)
          word |= ((((d[q] >> pl) & 0x01010101u) * 0x01020408u) >> 24) << (4 * q);
        out[pl] = word;
      }
    }
    if (D) {
      uint4* o = reinterpret_cast<uint4*>(D + (size_t)r * pitch + 32ull * w);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        uint32_t x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t y = (d[q] >> (8 * k)) & 0xFFu;
          x[k] = y == 0xFFu ? kInf : y;
        }
        // saturated bytes (254) keep the BFS's exact u32 (rare: deep graphs)
        const uint32_t z = d[q] ^ 0xFEFEFEFEu;  // a zero byte where d[q] holds 254
        if (__builtin_expect(((z - 0x01010101u) & ~z & 0x80808080u) != 0, 0)) {
          const uint4 old = o[q];
          const uint32_t ov[4] = {old.x, old.y, old.z, old.w};
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (((d[q] >> (8 * k)) & 0xFFu) == 0xFEu) x[k] = ov[k];
        }
        o[q] = make_uint4(x[0], x[1], x[2], x[3]);
      }
    }
  }
}

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template <int P>
struct Planes {
  uint32_t v[P];
};

typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// N consecutive dwords by buffer loads: wave-uniform byte offset in soff (an
// SGPR), the lane's in voff -- no 64-bit vector addresses
template <int N>
__device__ __forceinline__ void bload(uint32_t* d, __amdgpu_buffer_rsrc_t r, uint32_t voff,
                                      uint32_t soff) {
  if constexpr (N >= 4) {
    const u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
    if constexpr (N > 4) bload<N - 4>(d + 4, r, voff + 16, soff);
  } else if constexpr (N == 3) {
    const u32x3 a = __builtin_amdgcn_raw_buffer_load_b96(r, (int)voff, (int)soff, 0);
    d[0] = a.x, d[1] = a.y, d[2] = a.z;
  } else if constexpr (N == 2) {
    const u32x2 a = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0);
    d[0] = a.x, d[1] = a.y;
  } else {
    d[0] = __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0);
  }
}

// The sliced match of one 64-word chunk: lane = output word w.  Loads are
// unconditional (rows are padded past the last lane's word), stores
// predicated on `live`.  Two groups of U neighbour rows in flight, one
// P-dword load per row (U * P <= 16 keeps the registers low).
//   rs: the sliced rows (S); ro: the source's bitmaps (nh + nh_off[i]).
//   offs/k: the unit's neighbour range (its row offsets, its length); jb:
//   the range's first neighbour index (the bitmap the first result goes to).
#ifndef SPF_SL_STORE_AUX
#define SPF_SL_STORE_AUX 2
#endif
// bitmap store cache policy: 2 = nt (streaming: the bitmaps are outputs,
// never re-read by the pass; fabric_full next hops 0.102 -> 0.079 ms,
// gpurun_out/r03_nt); 0 = default (build-time A/B)
constexpr int kSlStoreAux = SPF_SL_STORE_AUX;
//   WEIGHTED (weighted plans, wts = the unit's neighbour metrics): the
//   test is d_x + w(s, x) == d_s, the sum formed bit-sliced with w a
//   wave-uniform constant (sum_b = a_b ^ c ^ w_b, carry = a_b c | (a_b ^ c)
//   w_b) -- ~6 bit operations per plane and 32 destinations where the byte
//   rows spend ~65 per 16.  A carry out of the top plane (the sum passes the
//   all-ones code: a drained neighbour's dead row, an unreachable node, or a
//   metric past the planes) matches nothing; an unreachable d_s (all ones)
//   cannot equal a finite d_x + w (d_x finite makes d_s finite).
template <int P, bool WEIGHTED = false, int U = (P <= 4 ? 4 : 2)>
__device__ __forceinline__ void sliced_pass(__amdgpu_buffer_rsrc_t rs, __amdgpu_buffer_rsrc_t ro,
                                            uint32_t wpm, uint32_t srow,
                                            const uint32_t* __restrict__ offs, uint32_t k,
                                            uint32_t jb, uint32_t w, bool live,
                                            const uint32_t* __restrict__ wts = nullptr) {
  const uint32_t wpb = w * P * 4;  // the lane's plane bytes inside any row
  Planes<P> sv;
  bload<P>(sv.v, rs, wpb, srow * kSlSlots * wpm * 4);
  uint32_t t[P];
  uint32_t ones = ~0u, zeros = ~0u, borrow = ~0u;
#pragma unroll
  for (int b = 0; b < P; ++b) {
    const uint32_t x = sv.v[b];
    ones &= x;
    zeros &= ~x;
    t[b] = WEIGHTED ? x : x ^ borrow;  // unit metrics: t = d_s - 1
    borrow &= ~x;
  }
  // the source itself (d = 0) and unreachable destinations take no next hop;
  // elsewhere t is finite and never the all-ones code of a drained (dead) row
  const uint32_t valid = ~(ones | zeros);
  auto load_group = [&](uint32_t j0, Planes<P> (&r)[U]) {
    uint32_t o[U];  // one scalar load of U row offsets
    if constexpr (U == 4) {
      const uint4 o4 = *reinterpret_cast<const uint4*>(offs + j0);
      o[0] = o4.x, o[1] = o4.y, o[2] = o4.z, o[3] = o4.w;
    } else {
      const uint2 o2 = *reinterpret_cast<const uint2*>(offs + j0);
      o[0] = o2.x, o[1] = o2.y;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) bload<P>(r[u].v, rs, wpb, o[u] * 4);
  };
  auto match_group = [&](uint32_t j0, const Planes<P> (&r)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u >= k) break;
      uint32_t diff = 0;
      if constexpr (WEIGHTED) {
        const uint32_t wj = wts[j0 + u];  // wave-uniform: a scalar load
        if (wj >> P) {
          diff = ~0u;  // d_x + w past the planes: no finite d_s there
        } else {
          uint32_t c = 0;
#pragma unroll
          for (int b = 0; b < P; ++b) {
            const uint32_t a = r[u].v[b], wb = 0u - ((wj >> b) & 1u), ac = a ^ c;
            diff |= ac ^ wb ^ t[b];
            c = (a & c) | (ac & wb);
          }
          diff |= c;
        }
      } else {
#pragma unroll
        for (int b = 0; b < P; ++b) diff |= r[u].v[b] ^ t[b];
      }
      if (live)
        __builtin_amdgcn_raw_buffer_store_b32(~diff & valid, ro, (int)(w * 4),
                                              (int)((jb + j0 + u) * wpm * 4), kSlStoreAux);
    }
  };
  Planes<P> ra[U], rb[U];
  load_group(0, ra);
  for (uint32_t j0 = 0; j0 < k; j0 += 2 * U) {
    load_group(j0 + U, rb);
    match_group(j0, ra);
    load_group(j0 + 2 * U, ra);
    match_group(j0 + U, rb);
  }
}

// Grouped match (sources with identical neighbour lists: a pod's rack
// switches, a plane's spines): the group's source planes of one 64-word chunk
// stay in registers and every neighbour row is loaded once for all of them
// (the per-source pass loads it once per source -- the next-hop pass is
// bound by those L2 reads).  gs <= kSlGroup sources; lane = output word w.
// (kSlGroup, kSlSeg: plan_host.h, with plan_sliced_units, which forms the groups)
template <int P>
__device__ __forceinline__ void grouped_pass(__amdgpu_buffer_rsrc_t rs, uint32_t* __restrict__ nh,
                                             const uint64_t* __restrict__ nh_off,
                                             const uint32_t* __restrict__ row_of,
                                             const uint32_t* __restrict__ req_src,
                                             const uint32_t* __restrict__ gm, uint32_t gs,
                                             uint32_t wpm, const uint32_t* __restrict__ offs,
                                             uint32_t j0, uint32_t j1, uint32_t w, bool live) {
  const uint32_t wpb = w * P * 4;
  uint32_t t[kSlGroup][P], valid[kSlGroup];
  uint32_t* out[kSlGroup];
#pragma unroll
  for (uint32_t q = 0; q < kSlGroup; ++q) {
    valid[q] = 0;
    out[q] = nh;
#pragma unroll
    for (int b = 0; b < P; ++b) t[q][b] = 0;
    if (q < gs) {
      const uint32_t i = gm[q];
      out[q] = nh + nh_off[i];
      Planes<P> sv;
      bload<P>(sv.v, rs, wpb, row_of[req_src[i]] * kSlSlots * wpm * 4);
      uint32_t ones = ~0u, zeros = ~0u, borrow = ~0u;
#pragma unroll
      for (int b = 0; b < P; ++b) {
        const uint32_t x = sv.v[b];
        ones &= x;
        zeros &= ~x;
        t[q][b] = x ^ borrow;  // t = d_s - 1
        borrow &= ~x;
      }
      valid[q] = ~(ones | zeros);
    }
  }
  // two groups of 4 neighbour rows in flight (row offset lists are padded:
  // loads past j1 read the dead row)
  constexpr int U = 4;
  offs += j0;
  const uint32_t k = j1 - j0;
  auto load_group = [&](uint32_t jj, Planes<P> (&r)[U]) {
    const uint4 o4 = *reinterpret_cast<const uint4*>(offs + jj);
    const uint32_t o[U] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
    for (int v = 0; v < U; ++v) bload<P>(r[v].v, rs, wpb, o[v] * 4);
  };
  auto match_group = [&](uint32_t jj, const Planes<P> (&r)[U]) {
#pragma unroll
    for (int v = 0; v < U; ++v) {
      if (jj + v >= k) break;
      const size_t at = (size_t)(j0 + jj + v) * wpm + w;
#pragma unroll
      for (uint32_t q = 0; q < kSlGroup; ++q) {
        if (q >= gs) break;  // wave-uniform
        uint32_t diff = 0;
#pragma unroll
        for (int b = 0; b < P; ++b) diff |= r[v].v[b] ^ t[q][b];
        if (live) {
          if constexpr (kSlStoreAux) __builtin_nontemporal_store(~diff & valid[q], &out[q][at]);
          else out[q][at] = ~diff & valid[q];
        }
      }
    }
  };
  Planes<P> ra[U], rb[U];
  load_group(0, ra);
  for (uint32_t jj = 0; jj < k; jj += 2 * U) {
    load_group(jj + U, rb);
    match_group(jj, ra);
    load_group(jj + 2 * U, ra);
    match_group(jj + U, rb);
  }
}

// Work units: (source i, chunks [c0, c1) of 64 words, neighbours [j0, j1)),
// at most about kSlUnit neighbour-chunk matches each (spf_plan_create keeps
// light sources whole and cuts heavy ones per chunk and neighbour range),
// one wave per unit, units of an XCD's source runs on that XCD.  A wave's
// matches are latency-bound (two groups of row loads in flight), so one wave
// per source left the spine switches (173 neighbours x 5 chunks) running
// long after the rest; one wave per (source, chunk) was bound by wave launch;
// persistent waves pulling units through per-XCD atomic counters serialised
// on the counters (r02_v20: 2.4x slower); sc1 bitmap stores (lines leave L2)
// changed nothing (r02_v22).
// neighbour-chunk matches per unit (at most, about): fabric_full's pass 68.5
// us at 128, 66 at 512, 72 at 1024, 92 at 2048 (gpurun_out/r04_s1, r04_s2)
// (the figure is kSlUnit, plan_host.h)

__global__ __launch_bounds__(kEcmpThreads) void ecmp_sliced_kernel(
    const uint32_t* __restrict__ S, const uint32_t* __restrict__ maxd,
    const uint32_t* __restrict__ D, uint32_t pitch,
    const uint32_t* __restrict__ req_src, const uint32_t* __restrict__ row_of,
    const uint32_t* __restrict__ nb_ptr, const uint32_t* __restrict__ nb_id,
    const uint32_t* __restrict__ nb_w, const uint32_t* __restrict__ nb_row,
    const uint32_t* __restrict__ nb_row_off, const uint32_t* __restrict__ nb_drained,
    uint32_t dead, uint32_t hop, const uint64_t* __restrict__ nh_off, uint32_t* __restrict__ nh,
    const uint4* __restrict__ units, const uint32_t* __restrict__ unit_off,
    const uint32_t* __restrict__ gtab /* group units: [n, sources...] */, uint32_t s_bytes,
    uint32_t fixed_p /* rows sliced by the BFS itself (sdirect): P planes, maxd unused */,
    uint32_t weighted /* d_x + w(s, x) == d_s (weighted plans) instead of d_x == d_s - 1 */) {
  const uint32_t md = fixed_p ? 0u : *maxd;
  const uint32_t g = blockIdx.x & 7;  // this block's XCD (round-robin placement)
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wpm = pitch / 32;
  const uint32_t P = fixed_p ? fixed_p : md < kSlSat ? 32u - __clz(md + 1u) : 0u;  // 0: saturated
  const uint32_t rstride = kSlSlots * wpm;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint32_t*>(S), 0, (int)s_bytes, 0x00020000);
  // wave-uniform to the compiler too (readfirstlane): the unit's values then
  // live in SGPRs and its row offsets arrive by scalar loads
  const uint32_t t = (blockIdx.x >> 3) * kEcmpWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t u_begin = unit_off[g];
  if (t >= unit_off[g + 1] - u_begin) return;  // whole wave: no barriers below
  // one source's units: chunks [c0, c1), neighbours [j0, j1)
  auto single = [&](const uint32_t i, const uint32_t c0, const uint32_t c1, const uint32_t j0,
                    const uint32_t j1) {
    const uint32_t s = req_src[i];
    const uint32_t nb0 = nb_ptr[s], k = j1 - j0;
    const uint32_t srow = row_of[s];
    const uint32_t* offs = nb_row + nb_row_off[i];
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        nh + nh_off[i], 0, (int)((nb_ptr[s + 1] - nb0) * wpm * 4), 0x00020000);
    for (uint32_t c = c0; c < c1; ++c) {
      const uint32_t w0 = c * 64, w = w0 + lane;
      const bool live = w < wpm;
#define SL_CASE(PV)                                                                          \
  case PV:                                                                                   \
    if (weighted)                                                                            \
      sliced_pass<PV, true>(rs, ro, wpm, srow, offs + j0, k, j0, w, live, nb_w + nb0 + j0);  \
    else                                                                                     \
      sliced_pass<PV>(rs, ro, wpm, srow, offs + j0, k, j0, w, live);                         \
    break;
      switch (P) {
        SL_CASE(1)
        SL_CASE(2)
        SL_CASE(3)
        SL_CASE(4)
        SL_CASE(5)
        SL_CASE(6)
        SL_CASE(7)
        SL_CASE(8)
#undef SL_CASE
        default: {
          uint32_t* out = nh + nh_off[i] + w;
          // saturated: exact u32 rows, 32 destinations per lane (offsets are
          // sliced-row offsets, row = offset / rstride)
          for (uint32_t j = j0; j < j1; ++j) {
            const uint32_t oj = offs[j], wj = hop ? 1u : nb_w[nb0 + j];
            uint32_t m = 0;
            if (oj != dead && live) {
              const uint4* Dx = reinterpret_cast<const uint4*>(D + (size_t)(oj / rstride) * pitch + 32ull * w);
              const uint4* Ds = reinterpret_cast<const uint4*>(D + (size_t)srow * pitch + 32ull * w);
#pragma unroll 1
              for (int q = 0; q < 8; ++q) {
                const uint4 a4 = Dx[q], b4 = Ds[q];
                const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) m |= (uint32_t)(a[e] != kInf && a[e] + wj == b[e]) << (4 * q + e);
              }
            }
            if (live) out[(size_t)j * wpm] = m;
          }
        }
      }
      // drained neighbour x: only x itself, reached directly when d_s(x) == w(s, x)
      if (nb_drained[i]) {
        uint32_t* out = nh + nh_off[i] + w;
        const uint32_t cbase = w0 * 32;
        for (uint32_t j = j0; j < j1; ++j) {
          if (offs[j] != dead) continue;
          const uint32_t x = nb_id[nb0 + j];
          if (x < cbase || x >= cbase + kSlChunk) continue;
          const uint32_t wj = hop ? 1u : nb_w[nb0 + j];
          if (lane == (x - cbase) / 32 && D[(size_t)srow * pitch + x] == wj)
            out[(size_t)j * wpm] = 1u << (x & 31);
        }
      }
    }
  };
  const uint4 u = units[u_begin + t];
  if (u.y >> 31) {  // a group unit: sources with identical neighbour lists, one chunk
    const uint32_t* gm = gtab + u.x + 1;
    const uint32_t gs = __builtin_amdgcn_readfirstlane(gtab[u.x]), c = u.y & 0xFFFFu;
    const uint32_t* offs = nb_row + nb_row_off[gm[0]];  // the same list for every member
    const uint32_t w = c * 64 + lane;
    const bool live = w < wpm;
    switch (P) {
      case 1: grouped_pass<1>(rs, nh, nh_off, row_of, req_src, gm, gs, wpm, offs, u.z, u.w, w, live); break;
      case 2: grouped_pass<2>(rs, nh, nh_off, row_of, req_src, gm, gs, wpm, offs, u.z, u.w, w, live); break;
      case 3: grouped_pass<3>(rs, nh, nh_off, row_of, req_src, gm, gs, wpm, offs, u.z, u.w, w, live); break;
      case 4: grouped_pass<4>(rs, nh, nh_off, row_of, req_src, gm, gs, wpm, offs, u.z, u.w, w, live); break;
      default:  // deeper planes or saturated rows: member by member
        for (uint32_t q = 0; q < gs; ++q) single(gm[q], c, c + 1, u.z, u.w);
    }
    return;
  }
  single(u.x, u.y & 0xFFFFu, u.y >> 16, u.z, u.w);
}

}  // namespace

namespace spfi {

spf_status launch_ecmp(spf_ctx* c, spf_plan* p, bool narrow, const uint32_t* D, bool hop, uint32_t* d_nh,
                       hipStream_t s) {
  const uint32_t per_block = kEcmpChunk * kEcmpWaves;
  const uint32_t chunks = (c->N + per_block - 1) / per_block;
  const uint32_t nb = chunks * (uint32_t)p->slots;
  const uint32_t weighted = narrow && !hop && !c->unit ? 1u : 0u;
  hipLaunchKernelGGL(narrow ? ecmp_kernel<true> : ecmp_kernel<false>, dim3(nb), dim3(kEcmpThreads), 0, s,
                     narrow ? p->d_Dn.p : nullptr, c->npitch, D, c->pitch, c->N, p->d_srcs.p, p->d_row_of.p,
                     c->d_nb_ptr.p, c->d_nb_id.p, c->d_nb_w.p, p->d_nb_row.p, p->d_nb_row_off.p,
                     p->d_nb_drained.p, p->dead, hop ? 1u : 0u, weighted, p->d_nh_off.p, d_nh, chunks,
                     p->d_slot_src.p);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_sliced(spf_ctx* c, spf_plan* p, uint32_t* D, hipStream_t s) {
  const uint32_t wpm = c->pitch / 32;
  const uint32_t rows = (uint32_t)p->closure.size();
  const uint64_t words = (uint64_t)rows * wpm;
  const uint32_t sb = (uint32_t)std::min<uint64_t>((words + 255) / 256, 16ull * c->n_cu);
  hipLaunchKernelGGL(slice_rows_kernel, dim3(std::max(sb, 1u)), dim3(256), 0, s, p->d_Dn.p, c->npitch,
                     rows, wpm, p->d_maxd.p, p->d_S.p, p->expand ? D : nullptr, c->pitch);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

spf_status launch_ecmp_sliced(spf_ctx* c, spf_plan* p, const uint32_t* D, bool hop, uint32_t* d_nh,
                              hipStream_t s) {
  // one wave per unit; block b serves XCD b % 8 (round-robin placement)
  const uint32_t blocks = 8 * std::max(1u, (p->max_xcd_units + kEcmpWaves - 1) / kEcmpWaves);
  hipLaunchKernelGGL(ecmp_sliced_kernel, dim3(blocks), dim3(kEcmpThreads), 0, s, p->d_S.p,
                     p->d_maxd.p, D, c->pitch, p->d_srcs.p, p->d_row_of.p,
                     c->d_nb_ptr.p, c->d_nb_id.p, c->d_nb_w.p, p->d_nb_row.p, p->d_nb_row_off.p,
                     p->d_nb_drained.p, p->dead, hop ? 1u : 0u, p->d_nh_off.p, d_nh,
                     reinterpret_cast<const uint4*>(p->d_units.p), p->d_unit_off.p, p->d_gtab.p,
                     (uint32_t)(p->d_S.n * 4), p->sdirect ? kTeamPlanes : 0u, p->mp ? 1u : 0u);
  HIP_TRY(c, hipGetLastError());
  return SPF_OK;
}

}  // namespace spfi
