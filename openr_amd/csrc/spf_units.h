// ============================================================================
//  spf_units.h -- what the units of the SPF / ECMP engine offer each other:
//  sssp.hip, msbfs.hip, class_rows.hip, ecmp.hip (a kernel family each, with
//  its LDS and batch arithmetic, its launches and its dynamic-LDS
//  registration) and spf_engine.hip (build_plan, execute, the traffic model),
//  which decides among them.  engine_internal.h holds the context, the plans
//  and what the rest of the library calls (launch_sssp, use_quotient,
//  use_planes, plan_ensure_narrow, preds_from_row, set_lds_limits, ...).
// ============================================================================
#pragma once
#include "engine_internal.h"

// (between the engine's units only: none of this is exported from the library)
#pragma GCC visibility push(hidden)
namespace spfi {

// dynamic LDS a workgroup of the LDS-resident kernels may ask for
constexpr size_t kMaxLds = 160 * 1024;

// Raise one kernel's dynamic-LDS limit to kMaxLds (the default stops at
// 64 KiB).  Each unit registers its own kernels, walking the same instance
// table its launches dispatch through: <unit>_set_lds_limits, called once per
// process by set_lds_limits.
inline spf_status raise_lds_limit(spf_ctx* c, const void* kernel) {
  HIP_TRY(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
  return SPF_OK;
}
spf_status sssp_set_lds_limits(spf_ctx* c);
spf_status msbfs_set_lds_limits(spf_ctx* c);
spf_status class_rows_set_lds_limits(spf_ctx* c);

// ---- sssp.hip (launch_sssp: engine_internal.h) ----
size_t sssp_lds_bytes(uint32_t N, uint32_t pitch, uint32_t big, bool q16);

// ---- msbfs.hip: msbfs_kernel and msbfs_planes_kernel ----
constexpr uint32_t kPlBatch = 32;  // msbfs_planes_kernel's sources per workgroup, at most
// may the BFS sweep the twin-class quotient at all (size, SPF_QUOTIENT)
bool quotient_allowed(const spf_ctx* c);
// msbfs_kernel's sources per workgroup.  knob: SPF_MSBFS_BATCH=1..64 fixes it
// (tests: full batches on graphs too small to fill the chip with them).
uint32_t ms_batch(const spf_ctx* c, uint32_t rows, bool knob = true);
// msbfs_planes_kernel's: full batches when the rows come deepest first
uint32_t planes_batch(const spf_ctx* c, uint32_t rows, bool ordered);
// Whichever of the two use_planes picks, over `rows` closure rows.  maxd: the
// deepest level (atomicMax, msbfs_kernel only); u32 rows from level d_from on;
// order: the register-plane kernel's rows, deepest first.
spf_status launch_msbfs(spf_ctx* c, const uint32_t* rows_src, uint32_t rows, uint32_t* D, uint8_t* Dn,
                        uint32_t* maxd, hipStream_t s, uint32_t d_from, const uint32_t* order);

// ---- class_rows.hip: class_bfs_kernel and expand_rows_kernel ----
bool class_rows_fit(const spf_ctx* c);
uint32_t expand_resident(const spf_ctx* c);
spf_status launch_class_bfs(spf_ctx* c, spf_plan* p, hipStream_t s);
spf_status launch_expand(spf_ctx* c, spf_plan* p, uint32_t* D, uint8_t* Dn, uint32_t* S, hipStream_t s);

// ---- ecmp.hip: the next-hop passes ----
// ecmp_kernel over the plan's u8 rows (narrow: p->d_Dn) or the u32 rows D
spf_status launch_ecmp(spf_ctx* c, spf_plan* p, bool narrow, const uint32_t* D, bool hop, uint32_t* d_nh,
                       hipStream_t s);
// slice_rows_kernel: p->d_Dn -> p->d_S (expand plans: and the u32 rows D)
spf_status launch_sliced(spf_ctx* c, spf_plan* p, uint32_t* D, hipStream_t s);
spf_status launch_ecmp_sliced(spf_ctx* c, spf_plan* p, const uint32_t* D, bool hop, uint32_t* d_nh,
                              hipStream_t s);

}  // namespace spfi
#pragma GCC visibility pop
