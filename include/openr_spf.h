/*
 * openr_spf.h -- C-ABI of the MI355X SPF engine (libopenr_spf.so).
 *
 * Graph-level interface: the caller (the LinkState facade of
 * openr_linkstate.h, or a host program that already has a CSR) hands over a
 * flattened link-state graph once, then asks for batches of single-source
 * shortest-path-first solves.  Each solve reproduces, bit for bit, what the
 * reference computes in LinkState::runSpf (openr/decision/LinkState.cpp:808-882):
 *   - dist[v]  = NodeSpfResult::metric() of v, or SPF_UNREACHABLE
 *   - nh bits  = NodeSpfResult::nextHops() of v as a bitset over the source's
 *                distinct up neighbours (ascending node id = ascending name)
 * The reference entry points this replaces are LinkState::getSpfResult
 * (LinkState.h:271-272, LinkState.cpp:793-803) for a batch of sources at once.
 *
 * Conventions
 *   - Node ids 0..n_nodes-1 MUST be assigned in ascending std::string order of
 *     the node names: the reference's Dijkstra queue breaks metric ties by
 *     node name (LinkState.h:488-498) and the engine breaks them by node id.
 *   - A directed edge u->v exists for every *up* link (Link::isUp,
 *     LinkState.cpp:233-236); its metric is the metric advertised by u
 *     (Link::getMetricFromNode(u), LinkState.cpp:195-204).  Edges of one node
 *     appear in linksFromNode(u) iteration order.
 *   - overloaded[u] != 0: u is recorded but never expanded unless it is the
 *     source (LinkState.cpp:831-838).
 *   - Distances are u32 unless the plan asks for SPF_FLAG_DIST64 (u64, the
 *     reference's LinkStateMetric).  Weighted solves of graphs whose longest
 *     possible path plus one more link (max metric x n_nodes) does not fit 32
 *     bits, or with a negative metric (the reference's i32 -> u64 conversion wraps), need
 *     SPF_FLAG_DIST64.
 *   - Zero or negative metrics, u64 distances and graphs too large for the
 *     LDS-resident kernels run the exact kernel (exact.hip): runSpf replayed
 *     step for step, one wavefront per source, heap pop order (metric, id)
 *     reproduced -- the next-hop sets under zero-cost plateaus depend on it.
 *   - Row pitch: dist and next-hop rows are stored with pitch
 *     spf_row_pitch() = n_nodes rounded up to a multiple of 1024 (every
 *     next-hop bitmap then starts on a 128-byte line).
 *
 * Errors: every call returns spf_status; spf_last_error() describes the last
 * failure.  No exceptions cross the ABI.  All calls on one context must come
 * from one host thread (the reference is single-threaded too,
 * openr/decision/Decision.cpp:1484).
 */
#ifndef OPENR_SPF_H_
#define OPENR_SPF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum spf_status {
  SPF_OK = 0,
  SPF_E_INVALID = 1,     /* bad argument / malformed graph            */
  SPF_E_UNSUPPORTED = 2, /* input outside the exact-parity envelope   */
  SPF_E_HIP = 3,         /* HIP runtime failure                       */
  SPF_E_NO_DEVICE = 4,   /* no usable gfx950 device                   */
  SPF_E_NOMEM = 5,
  SPF_E_STATE = 6        /* call out of order (e.g. no graph loaded)  */
} spf_status;

#define SPF_UNREACHABLE 0xFFFFFFFFu

/* solve flags */
#define SPF_FLAG_HOP_COUNT 0x1u /* useLinkMetric == false: every edge costs 1 */
/* Distance rows are u64 (LinkStateMetric, LinkState.h:22): pitch entries of
 * 8 bytes, UINT64_MAX = unreachable.  Required for weighted solves of graphs
 * with a negative metric or max metric x n_nodes >= 2^32 - 1 (the longest
 * possible path plus one more link: the u32 kernels add before they compare). */
#define SPF_FLAG_DIST64 0x2u
#define SPF_UNREACHABLE64 0xFFFFFFFFFFFFFFFFull

typedef struct spf_ctx spf_ctx;
typedef struct spf_plan spf_plan;

/* Dead slots: an edge u -> u (a self-loop) with metric 1 stands for no edge
 * -- a link of u that is down, or withdrawn, kept in place so that a later
 * change of that link patches the row instead of reloading the graph
 * (spf_graph_patch_rows).  Both slots of such a link are self-loops sharing
 * its link id.  No kernel relaxes, pushes or pulls over one; they are not
 * distinct neighbours and never next hops or pathLinks. */
typedef struct spf_graph {
  uint32_t n_nodes;
  uint32_t n_edges;             /* directed up edges (and dead slots)           */
  const uint32_t* row_ptr;      /* [n_nodes+1]                                  */
  const uint32_t* col;          /* [n_edges] head node of edge                  */
  const int32_t* metric;        /* [n_edges] metric advertised by the tail      */
  const uint32_t* link_id;      /* [n_edges] undirected link id (shared by both directions) */
  const uint8_t* overloaded;    /* [n_nodes]                                    */
} spf_graph;

/* ---- context ------------------------------------------------------------ */
spf_status spf_ctx_create(int device, spf_ctx** out);
void spf_ctx_destroy(spf_ctx* ctx);
const char* spf_last_error(const spf_ctx* ctx);
/* Thread-local message for failures before a context exists. */
const char* spf_global_error(void);

/* Copies the graph to the device (replaces any previous graph). */
spf_status spf_graph_load(spf_ctx* ctx, const spf_graph* g);

/* In-place patches of the loaded graph: the CSR
 * structure (nodes, up edges, their order) stays, so no spf_graph_load is
 * needed when an adjacency-database update only toggles node overload bits or
 * changes metrics of up links -- the reference re-runs updateAdjacencyDatabase
 * (openr/decision/LinkState.cpp:564-719) and clears its SPF memo
 * (:509-512, :714-717) on every such publication.
 *   spf_graph_set_overload: overloaded[i] != 0 drains node nodes[i]
 *     (LinkState::updateNodeOverloaded, LinkState.cpp:480-493).
 *   spf_graph_set_metric: new metric of directed edge edges[i] (CSR edge id),
 *     i.e. Link::getMetricFromNode of its tail (LinkState.cpp:195-204).
 * Every change bumps spf_graph_epoch(); SPF plans (spf_plan_*) re-derive
 * their internal state on their next execute (same output layout); KSP2 and
 * what-if plans return SPF_E_STATE and must be recreated; any plan returns
 * SPF_E_STATE after a spf_graph_load. */
spf_status spf_graph_set_overload(spf_ctx* ctx, const uint32_t* nodes, const uint8_t* overloaded,
                                  uint32_t n);
spf_status spf_graph_set_metric(spf_ctx* ctx, const uint32_t* edges, const int32_t* metric,
                                uint32_t n);
/* Rows of nodes[0..n) rewritten in place, each with its current length:
 * col / metric / link hold the new rows back to back (a dead slot: col = the
 * node, metric 1).  What a link going down or up, or an adjacency withdrawn
 * and advertised again, does to the CSR (LinkState::updateAdjacencyDatabase,
 * LinkState.cpp:564-719; Link::isUp, :233-236) when every link id keeps its
 * two slots.  Reverse edges, distinct-neighbour lists and the kernels' tables
 * are patched; plans re-derive on their next execute, except a plan one of
 * whose sources gained or lost a distinct neighbour (its next-hop layout):
 * that one returns SPF_E_STATE and must be recreated. */
spf_status spf_graph_patch_rows(spf_ctx* ctx, const uint32_t* nodes, uint32_t n, const uint32_t* col,
                                const int32_t* metric, const uint32_t* link);
uint64_t spf_graph_epoch(const spf_ctx* ctx);
/* Number of spf_graph_load calls so far (patches do not count). */
uint64_t spf_graph_loads(const spf_ctx* ctx);
uint32_t spf_row_pitch(const spf_ctx* ctx);
/* 1 when the loaded graph has an up edge with metric <= 0 (weighted solves
 * of such graphs run the exact kernel, which reproduces the heap pop order the
 * reference's next-hop sets depend on under zero-cost plateaus). */
int spf_graph_has_nonpositive_metric(const spf_ctx* ctx);
/* 1 when weighted solves need u64 distances (SPF_FLAG_DIST64). */
int spf_graph_needs_dist64(const spf_ctx* ctx);

/* Distinct up neighbours of `src` in ascending id: the bit order of its
 * next-hop sets.  Writes min(count, cap) ids; *count = total. */
spf_status spf_src_neighbors(const spf_ctx* ctx, uint32_t src, uint32_t* out,
                             uint32_t cap, uint32_t* count);

/* False-twin classes (host only): nodes whose distinct-neighbour lists
 * (nb_id[nb_ptr[v] .. nb_ptr[v+1]), ascending ids, as spf_src_neighbors gives
 * them) are equal share a class; classes are numbered by their first member.
 * cls = [n_nodes]; *n_classes = their number.  The unit-metric BFS sweeps the
 * quotient graph of these classes when that removes at least half of its
 * columns (a fabric pod's rack switches and a plane's spines are one class
 * each).  No reference counterpart. */
spf_status spf_twin_classes(uint32_t n_nodes, const uint32_t* nb_ptr, const uint32_t* nb_id,
                            uint32_t* cls, uint32_t* n_classes);
/* The loaded graph's quotient: its classes, its directed quotient edges, and
 * *in_use = 1 when msbfs_kernel plans sweep it (0: the plain sweep -- too few
 * twins, tables too large for LDS, another BFS kernel, or SPF_QUOTIENT=0 in
 * the environment).  Any output may be NULL.  Engine introspection. */
spf_status spf_graph_quotient(spf_ctx* ctx, uint32_t* n_classes, uint64_t* n_edges, uint32_t* in_use);

/* ---- plans: a fixed batch of sources, executable many times ------------- */
/* Next-hop layout of source i of the plan: one destination bitmap per
 * distinct up neighbour (k_i bitmaps, neighbours in ascending id), each of
 * pitch/32 32-bit words:
 *   neighbour j in nextHops(v)  <=>  nh[nh_off[i] + j*(pitch/32) + v/32] bit (v%32).
 * spf_plan_nh_layout reports nh_off[i] and k_i ("words" = bitmaps). */
spf_status spf_plan_create(spf_ctx* ctx, const uint32_t* srcs, uint32_t n_src,
                           uint32_t flags, spf_plan** out);
void spf_plan_destroy(spf_plan* plan);
uint64_t spf_plan_nh_words(const spf_plan* plan);     /* total u32 words   */
spf_status spf_plan_nh_layout(const spf_plan* plan, uint64_t* nh_off,
                              uint32_t* words);       /* n_src entries each */
uint32_t spf_plan_closure_rows(const spf_plan* plan); /* sources actually solved */
/* Which kernels the next execute runs (diagnostics, benchmarks):
 * *bfs = 0 sssp_kernel (weighted, per source), 1 msbfs_kernel (64 sources per
 * sweep, per-level stores), 2 msbfs_planes_kernel (32 sources, register bit
 * planes, rows written once), 3 exact_spf_kernel, 4 spf_big_kernel (graphs
 * beyond the LDS-resident kernels: one source at a time on the whole chip,
 * next hops inside), 5 mssp_kernel (weighted, positive metrics: 2-16 sources
 * per workgroup, u16 labels in LDS, min-plus sweeps), 6 msbfs_team_kernel (unit
 * metrics, plans with few sources: each batch's sweep split over a team of
 * workgroups on one XCD); *narrow = 0 when the
 * next-hop pass (ecmp_kernel) reads the u32 rows, 1 when it reads u8 rows,
 * 2 when slice_rows_kernel turns the u8 rows into bit planes and
 * ecmp_sliced_kernel matches those, 3 when msbfs_team_kernel writes the bit
 * planes itself (4 per word; no u8 rows, no slicing pass).
 * No reference counterpart (engine introspection). */
spf_status spf_plan_kernels(const spf_plan* plan, uint32_t* bfs, uint32_t* narrow);
/* Class rows: *in_use = 1 when the plan's unit-metric BFS solves one row per
 * false-twin class among its closure rows (class_bfs_kernel) and
 * expand_rows_kernel writes the node rows, their bit planes and, once asked
 * for, their u8 copies from those -- msbfs_kernel plans (spf_plan_kernels
 * keeps reporting *bfs = 1 and *narrow = 2 for them) on a graph whose
 * quotient is in use; SPF_CLASS_ROWS=0 in the environment at the plan's build
 * keeps msbfs_kernel's rows.  *n_class_sources = the rows the BFS solves (0 when
 * not in use).  Either output may be NULL.  Engine introspection. */
spf_status spf_plan_class_rows(const spf_plan* plan, uint32_t* n_class_sources, uint32_t* in_use);
/* Bytes the distance kernel and the next-hop kernel of one execute must move
 * to or from HBM (compulsory traffic given each kernel's structure: one
 * column sweep per BFS workgroup or per SSSP source, every output written
 * once, every compared distance row read once).  Denominator-free roofline
 * input for benchmarks; no reference counterpart. */
spf_status spf_plan_traffic(const spf_plan* plan, uint64_t* bfs_bytes, uint64_t* ecmp_bytes);
/* The same per phase: bytes[0] distance kernel, bytes[1] row slicing (0
 * unless *narrow == 2), bytes[2] next-hop kernel.  For sliced plans the
 * plane count comes from the last execute's deepest level (a 4-byte read). */
spf_status spf_plan_traffic_phases(const spf_plan* plan, uint64_t* bytes);

/* Execute on device buffers: d_dist = [n_src][pitch] u32, d_nh = nh words.
 * Enqueued on `stream` (a hipStream_t); NULL = the context's stream, a
 * BLOCKING stream, so work the caller put on the legacy null stream before
 * (a hipMemset / hipMemcpy of the outputs) is ordered before the execute.  A
 * caller's own non-blocking stream gets no such ordering: order it yourself.
 * Steady state (same graph epoch as the previous execute of the plan): no
 * host synchronisation, no allocation -- capturable into a hipGraph
 * (spf_mplan_set_graphs does).  The FIRST execute after an in-place patch
 * (spf_graph_set_overload / _metric) re-derives the plan on the host and
 * uploads its tables with a stream synchronisation, and a big plan's first
 * execute allocates its scratch: run one execute on a new epoch before
 * capturing.  Launches whose workgroups wait on each other (team BFS, grid
 * barriers) are ordered after any other such launch of the process on the
 * same device (see spf_device_check). */
spf_status spf_plan_execute(spf_plan* plan, uint32_t* d_dist, uint32_t* d_nh,
                            void* stream);
/* Per-source digests of an execute's output (d_dist / d_nh as passed to
 * spf_plan_execute), enqueued on `stream`: d_out[i] (u64) = sum mod 2^64 over
 * reachable v of mix(mix(v + 1) + dist(v)) ^ fnv1a64(nh(v) as u32 words),
 * mix = splitmix64's finaliser, nh(v) = v's next-hop set as a bitset over the
 * source's distinct up neighbours (the what-if digest's node term).  What a
 * rank ships when its rows stay resident on its GPU (multi-GPU all-sources),
 * and what the parity tests compare with the oracle's digests.  No
 * reference counterpart. */
spf_status spf_plan_digest(spf_plan* plan, const void* d_dist, const uint32_t* d_nh,
                           uint64_t* d_out, void* stream);
/* The narrow (u8) distance rows of the plan's last execute, for plans whose
 * distance kernel keeps them (spf_plan_kernels: *narrow != 0): row i (source
 * srcs[i]) byte v = d(srcs[i], v) when below 254, 254 when d >= 254, 255
 * when unreachable or v >= n_nodes -- lossless when every finite distance of
 * the execute is below 254 (unit-metric fabrics: 4 levels; grid 100x100:
 * 198).  n_src rows of spf_row_pitch bytes are copied to d_out on `stream`
 * (after the execute on that stream).  SPF_E_UNSUPPORTED for plans without
 * them.  Used to ship rows compactly (multi-GPU gather); no reference
 * counterpart (the reference's metric is u64, LinkState.h:22). */
spf_status spf_plan_copy_narrow_rows(spf_plan* plan, uint8_t* d_out, void* stream);
/* spf_plan_execute into host buffers: dist [n_src][n_nodes] (dense, no row
 * padding) and the next-hop words (spf_plan_nh_words of them); either may be
 * NULL.  Device staging is owned by the plan. */
spf_status spf_plan_execute_host(spf_plan* plan, uint32_t* dist, uint32_t* nh);
/* (with SPF_FLAG_DIST64, `dist` is read as uint64_t[n_src][n_nodes]) */
/* pathLinks of every source of the plan's last spf_plan_execute_host, one
 * batched launch (the batch form of spf_preds): pred_ptr = [n_src][n_nodes+1]
 * absolute offsets into pred_edge (source i's list for v is
 * pred_edge[pred_ptr[i*(n+1)+v] .. pred_ptr[i*(n+1)+v+1]), directed CSR edge
 * ids in the reference's order, LinkState.cpp:857-873); *n_preds = total.
 * With pred_edge == NULL only the offsets are written; SPF_E_NOMEM when cap <
 * *n_preds.  SPF_E_UNSUPPORTED for exact / big plans (spf_solve_exact's pop
 * ranks order those). */
spf_status spf_plan_preds(spf_plan* plan, uint32_t* pred_ptr, uint32_t* pred_edge, uint64_t cap,
                          uint64_t* n_preds);

/* Kernel timing with HIP events recorded on the execute stream: after
 * spf_plan_enable_timing(plan, K), each of the next K executes records events
 * around its SSSP and ECMP kernels; spf_plan_timing() waits for them and
 * returns the summed milliseconds of each kernel and the number of executes
 * (then resets the count). */
spf_status spf_plan_enable_timing(spf_plan* plan, uint32_t max_executes);
spf_status spf_plan_timing(spf_plan* plan, double* sssp_ms, double* ecmp_ms, uint32_t* n);
/* The same per phase: ms[0] distance kernel, ms[1] row slicing, ms[2]
 * next-hop kernel (spf_plan_timing's ecmp_ms = ms[1] + ms[2]). */
spf_status spf_plan_timing_phases(spf_plan* plan, double* ms, uint32_t* n);

/* Convenience: plan + execute + copy back to host buffers.
 * dist_out = [n_src][n_nodes] (dense, no pitch); nh_out sized by
 * spf_plan_nh_words with the planar layout above (pitch = spf_row_pitch). */
spf_status spf_solve(spf_ctx* ctx, const uint32_t* srcs, uint32_t n_src,
                     uint32_t flags, uint32_t* dist_out, uint32_t* nh_out);

/* ---- single-source primitives (LinkState facade, KSP) -------------------- */
/* Distances of one source with an optional set of undirected link ids to
 * ignore -- the reference's runSpf(src, true, linksToIgnore) used by
 * getKthPaths (LinkState.cpp:776-779).  dist_out = [n_nodes]. */
spf_status spf_sssp(spf_ctx* ctx, uint32_t src, uint32_t flags,
                    const uint32_t* ignore_links, uint32_t n_ignore,
                    uint32_t* dist_out);

/* runSpf(src, useLinkMetric, linksToIgnore) on the exact kernel, into host
 * buffers: distances as u64 (dist64_out, UINT64_MAX unreachable) when
 * dist32_out is NULL, else as u32; next-hop bitmaps in the plan layout
 * (spf_src_neighbors(src) bitmaps of pitch/32 words); pop_out[v] = the
 * position of v in the reference's Dijkstra pop order (UINT32_MAX
 * unreachable), from which pathLinks follow: the tight up in-edges (u -> v)
 * of expanded u with pop(u) < pop(v), ordered by (pop(u), linksFromNode
 * order).  Any pointer but one distance buffer may be NULL. */
spf_status spf_solve_exact(spf_ctx* ctx, uint32_t src, uint32_t flags,
                           const uint32_t* ignore_links, uint32_t n_ignore,
                           uint64_t* dist64_out, uint32_t* dist32_out, uint32_t* nh_out,
                           uint32_t* pop_out);

/* Predecessor ("pathLinks") lists of one source given its distance row `dist`
 * (from spf_solve / spf_sssp with the same flags and ignore set), in the
 * reference's order (LinkState.cpp:857-873: predecessors u in Dijkstra pop
 * order, then u's links in linksFromNode(u) order).  Entries are directed
 * edge ids u->v.  pred_ptr = [n_nodes+1]; call with pred_edge == NULL first
 * to size (*n_preds). */
spf_status spf_preds(spf_ctx* ctx, uint32_t src, uint32_t flags,
                     const uint32_t* ignore_links, uint32_t n_ignore,
                     const uint32_t* dist, uint32_t* pred_ptr,
                     uint32_t* pred_edge, uint32_t cap, uint32_t* n_preds);

/* ---- batched KSP2: getKthPaths(src, dst, 1) and (src, dst, 2) ------------ */
/* For every pair (srcs[i], d), d = 0..n_nodes-1, the k = 1 and k = 2 paths the
 * reference returns from LinkState::getKthPaths (LinkState.cpp:762-791): k = 1
 * traces edge-disjoint paths in the SPF of src (traceOnePath, :398-419, with
 * the shared visited-link set); k = 2 re-runs SPF from src ignoring every link
 * of the k = 1 paths and traces again.  Paths are lists of undirected link
 * ids (spf_graph.link_id) in src -> dst order, in the reference's discovery
 * order.  src == dst and unreachable pairs have no paths.
 *
 * Output: pairs[i * n_nodes + d] (below) and a pool of u32 words holding path
 * records [n_links, next record offset (SPF_KSP2_NONE = last), link ids...];
 * the k = 1 and k = 2 lists of a pair start at first[0] / first[1].
 * Graphs with a metric <= 0, u64 labels, more than 65535 nodes or a
 * working set past the LDS run on the exact kernel (runSpf replayed in pop
 * order per pair, HBM scratch): same output, far slower. */
#define SPF_KSP2_NONE 0xFFFFFFFFu
typedef struct spf_ksp2_pair {
  uint32_t first[2];   /* pool offset of the first k = 1 / k = 2 record */
  uint32_t n_paths[2]; /* number of k = 1 / k = 2 paths                  */
} spf_ksp2_pair;

typedef struct spf_ksp2_plan spf_ksp2_plan;
spf_status spf_ksp2_plan_create(spf_ctx* ctx, const uint32_t* srcs, uint32_t n_src,
                                spf_ksp2_plan** out);
void spf_ksp2_plan_destroy(spf_ksp2_plan* plan);
/* Sources per KSP2 workgroup (a block is one destination x this many
 * sources; the graph is staged once per block): for traffic accounting. */
uint32_t spf_ksp2_plan_chunk(const spf_ksp2_plan* plan);
/* What spf_ksp2_plan_create decided for the plan (read-only; no device work):
 * the kernel its executes launch and that kernel's launch parameters.
 *   EXACT    exact_ksp2_kernel: metrics <= 0 or u64 labels, more than 65535
 *            nodes, or per-wave rows past the LDS (SPF_KSP2_EXACT forces it)
 *   HBM      ksp2_kernel: the graph read from HBM (>= 65536 directed edges, a
 *            metric >= 65536, a degree >= 32768, a link that is not exactly
 *            one {e, rev(e)} pair, or a staged graph that leaves no room for
 *            two waves; SPF_KSP2_HBM forces it)
 *   LDS_U32  ksp2_lds_kernel<u32>: the graph staged in LDS, u32 labels
 *   LDS_U16  ksp2_lds_kernel<u16>, then ksp2_redo_kernel for the pairs whose
 *            labels or paths outgrow the compact waves
 * On EXACT plans every other field is 0. */
typedef enum spf_ksp2_kind {
  SPF_KSP2_KIND_EXACT = 0,
  SPF_KSP2_KIND_HBM = 1,
  SPF_KSP2_KIND_LDS_U32 = 2,
  SPF_KSP2_KIND_LDS_U16 = 3
} spf_ksp2_kind;
struct spf_ksp2_plan_info { /* (a tag, no typedef: the call below bears the name) */
  uint32_t kind;       /* spf_ksp2_kind */
  uint32_t waves;      /* waves per workgroup of the pair kernel */
  uint32_t redo_waves; /* waves per workgroup of the redo pass (LDS_U16), else 0 */
  uint32_t chunk;      /* sources per workgroup (SPF_KSP2_CHUNK) */
  uint32_t delta;      /* bucket width of the k = 2 SPF (SPF_KSP2_DELTA) */
  uint32_t grab;       /* pool words a wave reserves at a time (SPF_KSP2_GRAB) */
  uint64_t lds_bytes;  /* dynamic LDS of the pair kernel */
};
/* SPF_E_INVALID when either argument is NULL (*out untouched). */
spf_status spf_ksp2_plan_info(const spf_ksp2_plan* plan, struct spf_ksp2_plan_info* out);
/* Enqueue on `stream` (NULL = context stream).  d_pairs = [n_src * n_nodes],
 * d_pool = pool_words u32, d_counters = 4 u64 zeroed by the call:
 *   [0] pool words claimed, reservations' unused tails included (may
 *       exceed pool_words without an overflow: bit 0 of [2] is the only
 *       overflow signal; the written words are at most min([0], pool_words)),
 *   [1] k = 2 SPF runs (the reference's un-memoised runSpf calls, :778-779),
 *   [2] bit 0 = overflow (bit 1: redo list full, never on plans made by
 *       spf_ksp2_plan_create, which size it for every pair),
 *   [3] pairs the u16-label waves of a compact plan handed to the u32 redo
 *       pass (labels past 65534 or paths deeper than 512 links; 0 otherwise).
 * No host synchronisation, no allocation. */
spf_status spf_ksp2_execute(spf_ksp2_plan* plan, spf_ksp2_pair* d_pairs, uint32_t* d_pool,
                            uint64_t pool_words, uint64_t* d_counters, void* stream);
/* Per-source digests of an execute's output, on the GPU (enqueued on
 * `stream`): d_out[i] = sum mod 2^64 over destinations d of
 * mix(h(i, d) + mix(d + 1)), h = FNV-1a over (0x1000 + n_paths[k], then per path
 * 0x2000 + length and link_hash[link] of each link) for k = 1, 2 and mix =
 * splitmix64's finaliser.  link_hash[id] identifies link `id` by value (the
 * caller hashes its ordered (node, ifname) key), so digests compare across
 * engines and the oracle.  What the parity checks of all-pairs KSP2 compare;
 * no reference counterpart. */
spf_status spf_ksp2_digest(spf_ksp2_plan* plan, const spf_ksp2_pair* d_pairs, const uint32_t* d_pool,
                           const uint64_t* d_link_hash, uint64_t* d_out, void* stream);
/* HIP-event kernel timing of the next `max_executes` executes: summed ms of
 * the k = 1 SPF kernel and of the KSP2 kernel. */
spf_status spf_ksp2_enable_timing(spf_ksp2_plan* plan, uint32_t max_executes);
spf_status spf_ksp2_timing(spf_ksp2_plan* plan, double* spf_ms, double* ksp_ms, uint32_t* n);
/* Convenience: plan + execute (growing the device pool on overflow) + copy
 * back.  pairs_out = [n_src * n_nodes]; the records are repacked densely in
 * pair order (k = 1 then k = 2, list order), so *pool_used -- the packed
 * size -- is the same on every call.  With pool_out == NULL or pool_cap <
 * *pool_used only the pairs are copied (the latter returns SPF_E_NOMEM): call
 * again with a pool of *pool_used words. */
spf_status spf_ksp2_solve(spf_ctx* ctx, const uint32_t* srcs, uint32_t n_src,
                          spf_ksp2_pair* pairs_out, uint32_t* pool_out, uint64_t pool_cap,
                          uint64_t* pool_used);

/* ---- every source's KSP2_ED_ECMP routes (SR-MPLS label stacks) ------------ */
/* SpfSolver::selectBestPathsKsp2 (Decision.cpp:895-1018) for one area, for
 * every me = srcs[i] of the plan and every destination set p = set_nodes[
 * set_ptr[p] .. set_ptr[p + 1]) (a prefix's best advertisers), read from the
 * device-resident pairs and pool of an spf_ksp2_execute of the same plan that
 * did not overflow.  No path data crosses to the host.
 *   candidates  the k = 1 paths of every member in the set's order (list order
 *               within a member; a member equal to me contributes nothing,
 *               :923-925), then in the same member order every k = 2 path that
 *               contains none of the route's k = 1 paths as a contiguous run
 *               of link ids (LinkState::pathAInPathB, :934-957);
 *   per path    me -> v1 -> ... -> vk: cost = the sum of the metric each link
 *               advertises from the node the walk leaves it by (:973); first
 *               hop = the CSR edge of me's row with the path's first link id;
 *               label stack in labelVec order = [prepend(vk)?, L(vk), L(vk-1),
 *               ..., L(v2)] -- the first hop's own label dropped (PHP, :979),
 *               L(v) = node_label[v] as given (0 = advertises none: the
 *               reference pushes the thrift default unchecked), prepend = the
 *               member's set_prepend entry unless it is -1.  An empty stack
 *               means no MPLS action (:990);
 *   dedup       the reference collects std::unordered_set<NextHopThrift>: two
 *               candidates with the same first CSR edge, cost and label
 *               sequence are one next hop, the first in candidate order kept.
 *               A 64-bit key pre-filters; equality is decided by walking both
 *               paths again.
 * addBestPaths (:1020-1080: the min-nexthop threshold, the static next hops of
 * a self-advertised prefix), thrift formatting and the union over several
 * areas stay with the host.
 * Layout (CSR throughout, exactly sized: count, exclusive scan, fill as
 * ordinary launches on the plan's context stream, no atomics):
 *   rptr[n_src * n_sets + 1] u64  route (i, p)'s next hops are
 *                                 rec[rptr[i * n_sets + p] .. rptr[.. + 1])
 *   rec[n_hops]              u64  CSR edge | cost << 32 (with negative metrics
 *                                 the cost's low 32 bits, two's complement)
 *   lptr[n_hops + 1]         u64  next hop h's stack is lab[lptr[h] .. lptr[h + 1])
 *   lab[n_label_words]       i32
 * *pool_bytes = 8 n_hops + 8 (n_src n_sets + 1) + 8 (n_hops + 1) + 4 n_label_words;
 * *kernel_ms = the three passes together (spf_ksp2_routes_timing: apart); the
 * outputs are optional.  The pools are kept by the plan while they are large
 * enough; the same inputs give byte-identical arrays.  Waits.
 * SPF_E_INVALID: a NULL plan / d_pairs / d_pool / set_ptr / node_label, a set
 * node >= n_nodes, a non-monotone set_ptr.  SPF_E_UNSUPPORTED: max |metric| x
 * (n_nodes - 1) >= 2^32 (a cost might not fit the record).  SPF_E_STATE: the
 * graph changed since the plan was created.  All checked before anything is
 * launched; after a failed call the plan holds no routes. */
spf_status spf_ksp2_routes(spf_ksp2_plan* plan, const spf_ksp2_pair* d_pairs, const uint32_t* d_pool,
                           const uint32_t* set_ptr, const uint32_t* set_nodes, uint32_t n_sets,
                           const int32_t* set_prepend /* parallel to set_nodes, -1 = none; may be NULL */,
                           const int32_t* node_label /* [n_nodes] */, uint64_t* n_hops,
                           uint64_t* n_label_words, uint64_t* pool_bytes, double* kernel_ms);
/* ms[3] = count, scan, fill of the last spf_ksp2_routes (SPF_E_STATE: none). */
spf_status spf_ksp2_routes_timing(const spf_ksp2_plan* plan, double* ms);
/* srcs[i]'s share of the last spf_ksp2_routes, rebased to 0: rptr = [n_sets +
 * 1], rec = its *n_rec next hops (rec_cap entries; SPF_E_NOMEM when fewer),
 * lptr = [*n_rec + 1] (needs rec_cap >= *n_rec as well), lab = its *n_lab
 * label words (lab_cap entries; SPF_E_NOMEM when fewer).  Any output may be
 * NULL.  SPF_E_STATE when the plan holds no routes.  Waits. */
spf_status spf_ksp2_route_db(spf_ksp2_plan* plan, uint32_t i, uint64_t* rptr, uint64_t* rec,
                             uint64_t rec_cap, uint64_t* n_rec, uint64_t* lptr, int32_t* lab,
                             uint64_t lab_cap, uint64_t* n_lab);
/* The device arrays of the last spf_ksp2_routes, for device-side consumers
 * (valid until the next call on the plan); every output may be NULL.
 * SPF_E_STATE when the plan holds no routes. */
spf_status spf_ksp2_route_buffers(spf_ksp2_plan* plan, const uint64_t** d_rptr, const uint64_t** d_rec,
                                  const uint64_t** d_lptr, const int32_t** d_lab, uint64_t* n_hops,
                                  uint64_t* n_label_words);

/* ---- KSP2 route databases: snapshot, delta and update payload -------------- */
/* DecisionRouteDb::calculateUpdate (Decision.cpp:111-146) over the routes of
 * spf_ksp2_routes, for every source of a plan at once: the old generation held
 * by an spf_ksp2_snapshot, the new one by a plan; the three calls mirror
 * spf_mplan_route_snapshot / _delta / _update.
 *
 * spf_ksp2_route_snapshot: the device pools of the last successful
 * spf_ksp2_routes on `plan` (rptr, rec, lptr, lab) move into *out -- nothing is
 * copied -- and the plan holds no routes, exactly as after a failed call
 * (spf_ksp2_route_db / _buffers: SPF_E_STATE; the next spf_ksp2_routes
 * allocates afresh).  Kept by value: the plan's srcs, n_nodes, n_sets, the
 * totals, and on the device key_old[e] = link_hash[link_id[e]] for every CSR
 * edge of the graph as it is now.  link_hash[id] (n_links entries) names link
 * `id` by value (LinkState.linkValueHashes()): records name CSR edges, row
 * patches reorder slots and a reload may re-issue link ids, so only this key
 * compares across generations.  The snapshot belongs to the plan's spf_ctx and
 * outlives the plan, row patches and reloads; it is destroyed by
 * spf_ksp2_route_snapshot_destroy or, at the latest, with the context.
 * spf_ksp2_route_snapshot_bytes: the device memory it holds.  Waits.
 * SPF_E_INVALID: a NULL argument, or n_links not covering every link id
 * loaded.  SPF_E_STATE: the plan holds no routes, or the graph changed since
 * the plan was created.  A refused call moves nothing. */
typedef struct spf_ksp2_snapshot spf_ksp2_snapshot;
spf_status spf_ksp2_route_snapshot(spf_ksp2_plan* plan, const uint64_t* link_hash, uint32_t n_links,
                                   spf_ksp2_snapshot** out);
void spf_ksp2_route_snapshot_destroy(spf_ksp2_snapshot* snap);
uint64_t spf_ksp2_route_snapshot_bytes(const spf_ksp2_snapshot* snap);
/* spf_ksp2_route_delta: the plan's current routes (new; the last
 * spf_ksp2_routes) against the snapshot's (old).  A route's value is its set
 * of next hops, a next hop the triple (key of its first-hop CSR edge in its
 * own generation -- key_new is built by this call from link_hash and the
 * current link ids --, cost, label stack as a sequence): what a NextHopThrift
 * of the route is a function of.  spf_ksp2_routes de-duplicates within a
 * generation, so each side is a set.  Route (i, p) is
 *   unchanged  both sides have no next hop, or the sets are equal whatever
 *              their order in the pools;
 *   DELETE     only the old side has next hops;
 *   UPDATE     the new side has next hops and the route is new or its set
 *              differs.
 * Node labels, prepend labels and set membership may differ between the
 * generations: they show only through the stacks and next hops.
 * Output on the device, resident until the next call (count, exclusive scan,
 * fill as ordinary launches on the context's stream; no atomic per route):
 *   dptr[n_src + 1] u64   source slot i's entries are dset[dptr[i] .. dptr[i + 1])
 *   dset[total]     u32   the set index, | SPF_DELTA_DELETE on a delete,
 *                         ascending within a source
 * totals[3] = updates, deletes, routes decided by matching the next hops as
 * sets (equal counts, but not equal position by position) -- optional, as is
 * *kernel_ms = the three passes together.  The snapshot is only read: a second
 * call gives byte-identical lists.  Waits.
 * SPF_E_INVALID: a NULL plan / snap / link_hash, n_links not covering every
 * link id loaded, the snapshot is another context's, the plan's srcs (same
 * ids, same order), n_nodes or n_sets differ from the snapshot's (a changed
 * node set shifts ids: out of scope, as for spf_mplan_route_delta), or n_sets
 * >= 2^31.  SPF_E_STATE: the plan holds no routes, or the graph changed since
 * they were built.  All checked before anything is launched; after a failed
 * call the plan holds no delta (the _db / _buffers / update calls below:
 * SPF_E_STATE). */
spf_status spf_ksp2_route_delta(spf_ksp2_plan* plan, const spf_ksp2_snapshot* snap,
                                const uint64_t* link_hash, uint32_t n_links, uint64_t* totals /* [3] */,
                                double* kernel_ms);
/* Source slot i's entries of the last spf_ksp2_route_delta: *n their number,
 * set[cap] the entries (SPF_E_NOMEM with *n set when cap < *n; set may be NULL
 * to ask for *n).  SPF_E_STATE without a delta.  Waits. */
spf_status spf_ksp2_route_delta_db(spf_ksp2_plan* plan, uint32_t i, uint32_t* set, uint64_t cap,
                                   uint64_t* n);
/* The device lists of the last spf_ksp2_route_delta (valid until the next
 * call on the plan); every output may be NULL.  SPF_E_STATE without a delta. */
spf_status spf_ksp2_route_delta_buffers(spf_ksp2_plan* plan, const uint64_t** d_dptr,
                                        const uint32_t** d_dset, uint64_t* n_entries);
/* spf_ksp2_route_update: the payload of the last spf_ksp2_route_delta gathered
 * out of the plan's current pools into contiguous, exactly sized pools
 * parallel to dset (count, scan, fill; ordinary launches, no atomics):
 *   uptr[total + 1]    u64  entry j's records are urec[uptr[j] .. uptr[j + 1])
 *                           (a DELETE owns none)
 *   urec[n_urec]       u64  the records as the database holds them (CSR edge |
 *                           cost << 32), in pool order
 *   ulptr[n_urec + 1]  u64  record k's stack is ulab[ulptr[k] .. ulptr[k + 1])
 *   ulab[n_words]      i32
 * totals[3] = update entries, records, label words; *pool_bytes = 8 (total +
 * 1) + 8 n_urec + 8 (n_urec + 1) + 4 n_words; *kernel_ms = the passes
 * together; all optional.  Waits.  SPF_E_STATE without a delta, or when the
 * plan's routes are no longer the ones the delta compared (a later
 * spf_ksp2_routes, or a snapshot that moved them away). */
spf_status spf_ksp2_route_update(spf_ksp2_plan* plan, uint64_t* totals /* [3] */, uint64_t* pool_bytes,
                                 double* kernel_ms);
/* ms[6] = count, scan, fill of the last spf_ksp2_route_delta, then of the
 * spf_ksp2_route_update of that delta (zeros while there is none).
 * SPF_E_STATE without a delta. */
spf_status spf_ksp2_route_delta_timing(const spf_ksp2_plan* plan, double* ms /* [6] */);
/* Source slot i's payload of the last spf_ksp2_route_update, rebased to 0 and
 * parallel to spf_ksp2_route_delta_db's entries (m of them): uptr = [m + 1],
 * urec = its *n_rec records (rec_cap entries; SPF_E_NOMEM when fewer), ulptr =
 * [*n_rec + 1] (needs rec_cap >= *n_rec as well), ulab = its *n_lab label
 * words (lab_cap entries; SPF_E_NOMEM when fewer).  Any output may be NULL.
 * SPF_E_STATE without an update.  Waits. */
spf_status spf_ksp2_route_update_db(spf_ksp2_plan* plan, uint32_t i, uint64_t* uptr, uint64_t* urec,
                                    uint64_t rec_cap, uint64_t* n_rec, uint64_t* ulptr, int32_t* ulab,
                                    uint64_t lab_cap, uint64_t* n_lab);
/* The whole payload in one copy per array: n[4] = source slots, entries,
 * records, label words (ask with the arrays NULL first), then dptr[n[0] + 1],
 * dset[n[1]], uptr[n[1] + 1], urec[n[2]], ulptr[n[2] + 1], ulab[n[3]].  Every
 * output may be NULL.  SPF_E_STATE without an update.  Waits. */
spf_status spf_ksp2_route_update_read(spf_ksp2_plan* plan, uint64_t* n /* [4] */, uint64_t* dptr,
                                      uint32_t* dset, uint64_t* uptr, uint64_t* urec, uint64_t* ulptr,
                                      int32_t* ulab);
/* The device pools of the last spf_ksp2_route_update (valid until the next
 * call on the plan); every output may be NULL.  SPF_E_STATE without an
 * update. */
spf_status spf_ksp2_route_update_buffers(spf_ksp2_plan* plan, const uint64_t** d_uptr,
                                         const uint64_t** d_urec, const uint64_t** d_ulptr,
                                         const int32_t** d_ulab, uint64_t* n_records,
                                         uint64_t* n_label_words);

/* ---- what-if batches: one source, every single-link failure -------------- */
/* For each failed link l of the list: the reference's
 * runSpf(src, true, {l}) (LinkState.cpp:808-882 with linksToIgnore = {l}),
 * reduced to a digest against the unfailed runSpf(src):
 *   n_dist_changed  nodes whose metric changed (incl. becoming unreachable)
 *   n_nh_changed    nodes whose nextHops() changed (incl. becoming unreachable)
 *   hash            sum over reachable v of
 *                     mix(mix(v + 1) + metric(v)) ^ fnv1a64(nh(v) as u32 words)
 *                   mod 2^64, mix = splitmix64's finaliser, nh(v) = bitset over
 *                   the distinct up neighbours of src in the unfailed graph
 *                   (ascending id), ceil(k/32) words.
 * The unfailed result's digest is {0, 0, hash}.  Global-memory kernels, no
 * LDS size limit: repair scratch is sized from fixed HBM budgets (8 GB of
 * wave teams, 8 GB of workgroup teams, fewer teams on bigger graphs) plus
 * O(N) per plan; an allocation failure returns SPF_E_NOMEM.  Graphs with a
 * metric <= 0 or u64 labels run on the exact kernel: the unfailed run
 * replayed in pop order, and for every failure one of whose directions is a
 * pathLink of it, runSpf(src, true, {l}) replayed by one wavefront (the
 * others keep the unfailed digest). */
typedef struct spf_whatif_digest {
  uint32_t n_dist_changed;
  uint32_t n_nh_changed;
  uint64_t hash;
} spf_whatif_digest;

typedef struct spf_whatif_plan spf_whatif_plan;
/* fail_links: undirected link ids (spf_graph.link_id) of up links; NULL =
 * every up link of the graph in ascending id order. */
spf_status spf_whatif_plan_create(spf_ctx* ctx, uint32_t src, const uint32_t* fail_links,
                                  uint32_t n_fail, spf_whatif_plan** out);
void spf_whatif_plan_destroy(spf_whatif_plan* plan);
uint32_t spf_whatif_plan_failures(const spf_whatif_plan* plan);
spf_status spf_whatif_plan_links(const spf_whatif_plan* plan, uint32_t* links /* [n_fail] */);
/* ---- what-if batches for node failures and node drains.
 * "Failure i" of the plan is a node x_i instead of a link:
 *   SPF_WHATIF_NODE_DOWN   runSpf(src, true, linksFromNode(x)): every link of x
 *                          ignored, the result of x's adjacency database being
 *                          deleted;
 *   SPF_WHATIF_NODE_DRAIN  runSpf(src) with x overloaded: x is recorded but not
 *                          expanded (LinkState.cpp:831-838).
 * The result is an ordinary spf_whatif_plan: spf_whatif_execute, _changes,
 * _changes_db / _read / _buffers / _timing, _base, _stats, _enable_timing,
 * _timing, _plan_failures and _plan_destroy work on it unchanged.  The digest
 * and the list entry are the link plans': the next-hop bitset is over the
 * distinct up neighbours of src in the UNFAILED graph, a failed neighbour's
 * bit is simply never set.
 *   DOWN x, x reachable in the unfailed run: x becomes unreachable -- it counts
 *     in n_dist_changed and n_nh_changed and is listed with dist = UINT64_MAX
 *     and zero words; only DAG descendants of x can change.
 *   DOWN x, x unreachable: cold, digest {0, 0, hash}, no entries.
 *   DRAIN x: x keeps its metric and next hops and is never listed or counted;
 *     nothing is relaxed out of x; only the descendants of x's tight children
 *     can change.  Cold when x is overloaded already, unreachable, or has no
 *     tight out-edge.
 * The repairs keep x in the affected set D as its root (D = x and its DAG
 * descendants) for both kinds: down, x takes no distance; drained, x is a
 * fixed node that settles at its unfailed metric and row and is neither a
 * transit nor a predecessor (so it never differs from the base).
 * fail_nodes: csr ids; NULL = every node except src, ascending (n_fail =
 * n_nodes - 1).  The list's order is kept; a node may appear twice.
 * SPF_E_INVALID: src in the list (failing the source is not a question this
 * call answers), a node id >= n_nodes, an unknown kind.  SPF_E_UNSUPPORTED:
 * graphs that take the exact path (a metric <= 0 or u64 labels) -- the exact
 * replay would need a per-wave ignore bitmap.  SPF_WHATIF_PROF is ignored by
 * node plans. */
#define SPF_WHATIF_NODE_DOWN 1u  /* every link of the node ignored            */
#define SPF_WHATIF_NODE_DRAIN 2u /* the node overloaded: reached, not transit */
spf_status spf_whatif_plan_create_nodes(spf_ctx* ctx, uint32_t src, uint32_t kind,
                                        const uint32_t* fail_nodes, uint32_t n_fail,
                                        spf_whatif_plan** out);
/* The plan's nodes; SPF_E_STATE on a link plan (as spf_whatif_plan_links is on
 * a node plan). */
spf_status spf_whatif_plan_nodes(const spf_whatif_plan* plan, uint32_t* nodes /* [n_fail] */);
/* ---- what-if batches for link-set failures (shared-risk link groups: a fibre
 * bundle, a line card, both links of a LAG, a conduit).
 * "Failure i" of the plan is a set of links, all ignored at once:
 *   runSpf(src, true, {set_links[set_ptr[i] .. set_ptr[i + 1])})
 * against the unfailed runSpf(src) -- the reference's own primitive with more
 * than one link in linksToIgnore (LinkState.cpp:808-882).  The result is an
 * ordinary spf_whatif_plan: spf_whatif_execute, _changes, _changes_db / _read /
 * _buffers / _timing, _base, _stats, _enable_timing, _timing, _plan_failures
 * and _plan_destroy work on it unchanged, and spf_whatif_plan_kind returns
 * SPF_WHATIF_LINK_SET.  The digest and the list entry are the link plans': the
 * next-hop bitset is over the distinct up neighbours of src in the UNFAILED
 * graph.
 *   A set is a set: the plan sorts each one and drops duplicates
 *     (spf_whatif_plan_sets returns them so).  The order of the sets is kept,
 *     and the same set may appear twice.
 *   The empty set is allowed and cold: digest {0, 0, hash}, no entries.
 *   A member that is down, or not tight in the unfailed shortest-path DAG, has
 *     no effect; a set none of whose members is tight is cold.
 *   Links of src are allowed, all of them included: every other node then
 *     becomes unreachable.  Unlike node plans, nothing about src is refused.
 *   A single link is a set of one (digests and lists equal the link plan's);
 *     linksFromNode(x) as a set equals SPF_WHATIF_NODE_DOWN of x.
 * The repairs take the heads of the set's tight members as the roots of the
 * affected set D (D = the roots and their DAG descendants; two members with
 * one head give one root), and test "is this edge failed" by membership of
 * its link id in the sorted set: compares against registers up to 4 members,
 * a binary search of the set in memory beyond.
 * SPF_E_INVALID: set_ptr[0] != 0, set_ptr not non-decreasing, a link id that is
 * not a link id of the graph (> the largest link id loaded), NULL arrays with
 * n_sets > 0 (set_links may be NULL when every set is empty).
 * SPF_E_UNSUPPORTED: graphs that take the exact path (a metric <= 0 or u64
 * labels), as for node plans.  SPF_WHATIF_PROF is ignored by set plans. */
#define SPF_WHATIF_LINK_SET 3u   /* failure i = a set of links, all ignored */
spf_status spf_whatif_plan_create_sets(spf_ctx* ctx, uint32_t src,
                                       const uint32_t* set_ptr /* [n_sets + 1] */,
                                       const uint32_t* set_links /* [set_ptr[n_sets]] */,
                                       uint32_t n_sets, spf_whatif_plan** out);
/* The plan's sets as it holds them: each ascending, duplicates removed.
 * set_ptr [n_fail + 1]; set_links [set_ptr[n_fail]], NULL to read set_ptr
 * alone.  SPF_E_STATE on a link or node plan (as spf_whatif_plan_links and
 * _plan_nodes are on a set plan). */
spf_status spf_whatif_plan_sets(const spf_whatif_plan* plan, uint32_t* set_ptr, uint32_t* set_links);
/* ---- what-if batches for link metric changes (cost-out and undrain: the
 * reference's LinkMonitor setLinkMetric / setAdjacencyMetric, `breeze lm
 * set-link-metric`).
 * "Failure i" of the plan is a change (links[i], m_lo[i], m_hi[i]): runSpf(src)
 * on the graph in which that link's direction from its endpoint with the
 * smaller csr id to the larger weighs m_lo[i] and the opposite direction
 * m_hi[i], against the unchanged runSpf(src).  SPF_WHATIF_METRIC_KEEP (0, no
 * metric of the positive envelope) keeps a direction's metric.  The link stays
 * usable: no failure of the other kinds expresses this, nor the way back
 * (lowering a metric to put traffic back on a link).  The result is an
 * ordinary spf_whatif_plan: spf_whatif_execute, _changes, _changes_db / _read /
 * _buffers / _timing, _base, _stats, _enable_timing, _timing, _plan_failures
 * and _plan_destroy work on it unchanged, and spf_whatif_plan_kind returns
 * SPF_WHATIF_LINK_METRIC.  The digest and the list entry are the link plans':
 * the next-hop bitset is over the distinct up neighbours of src in the
 * unchanged graph.  A metric change never alters that neighbour set or anyone's
 * reachability, so no entry carries dist == UINT64_MAX.
 *   One direction at most can matter, because metrics are positive: if u -> v
 *     is tight, or becomes useful (d(u) + w' <= d(v)), then d(u) < d(v), and the
 *     reverse direction cannot reach u at or below d(u) whatever it weighs.
 *   Cold (digest {0, 0, hash}, no entries): the link is down; both directions
 *     kept or equal to the current metric; a raised direction that is not
 *     tight; a lowered u -> v with d(u) + w' > d(v), or u unreachable, or u not
 *     expanded (overloaded and not src).
 *   Hot: a raise of a tight u -> v repairs the DAG descendants of v, the link
 *     plan's affected set, with the edge kept at its new weight; a lower with
 *     delta = d(v) - d(u) - w' >= 0 repairs the nodes reached from v over
 *     edges of slack <= delta, a superset of what can change (delta = 0: a new
 *     equal-cost tie, distances stay and next hops grow).
 * The order of the list is kept, and a link may appear several times with
 * different metrics (one link swept over ten metrics is one plan).
 * SPF_E_INVALID: a link id that is not a link id of the graph (> the largest
 * link id loaded), NULL arrays with n > 0, a metric so large that metric x
 * n_nodes >= 2^32 - 1 (the bound past which a loaded graph leaves 32-bit
 * distances).  SPF_E_UNSUPPORTED: graphs that take the exact path (a metric <= 0
 * or u64 labels), as for node and set plans.  SPF_WHATIF_PROF is ignored by
 * metric plans. */
#define SPF_WHATIF_LINK_METRIC 4u /* failure i = one link's metrics changed */
#define SPF_WHATIF_METRIC_KEEP 0u /* m_lo / m_hi: keep this direction's metric */
spf_status spf_whatif_plan_create_metrics(spf_ctx* ctx, uint32_t src, const uint32_t* links /* [n] */,
                                          const uint32_t* m_lo /* [n] */,
                                          const uint32_t* m_hi /* [n] */, uint32_t n,
                                          spf_whatif_plan** out);
/* The plan's changes as given, [n_fail] each; any output may be NULL.
 * SPF_E_STATE on a link, node or set plan (as spf_whatif_plan_links, _plan_nodes
 * and _plan_sets are on a metric plan). */
spf_status spf_whatif_plan_metrics(const spf_whatif_plan* plan, uint32_t* links, uint32_t* m_lo,
                                   uint32_t* m_hi);
/* 0 = link plan, SPF_WHATIF_NODE_*, SPF_WHATIF_LINK_SET or SPF_WHATIF_LINK_METRIC */
spf_status spf_whatif_plan_kind(const spf_whatif_plan* plan, uint32_t* kind);
/* d_out = [n_fail] digests, d_base = 1 digest (may be NULL).  Enqueued on
 * `stream` (a grid-resident launch for the unfailed solve); no host
 * synchronisation.  Failures with a large affected region are repaired on a
 * side stream owned by the ctx, forked from and joined back into `stream`
 * with events, so all work is ordered after earlier work on `stream` and
 * complete before later work on it.  Executes of plans sharing one ctx must
 * not overlap (one host thread per ctx, as elsewhere). */
spf_status spf_whatif_execute(spf_whatif_plan* plan, spf_whatif_digest* d_out,
                              spf_whatif_digest* d_base, void* stream);
/* After an execute: failures that needed a re-solve (tight links) and those
 * re-solved by whole workgroups (large affected region).  Waits for the last
 * execute's stream (SPF_E_STATE before the first execute). */
spf_status spf_whatif_stats(spf_whatif_plan* plan, uint32_t* n_hot, uint32_t* n_big);
spf_status spf_whatif_enable_timing(spf_whatif_plan* plan, uint32_t max_executes);
/* summed ms of the unfailed solve (SPF + next hops + hash) and of the failures */
spf_status spf_whatif_timing(spf_whatif_plan* plan, double* base_ms, double* fail_ms,
                             uint32_t* n);
/* ---- what-if change lists: what each failure changes, not only its digest.
 * For failure i of the plan's list: the nodes v whose metric changed, whose
 * nextHops() changed or which became unreachable under runSpf(src, true,
 * {l_i}) against the unfailed runSpf(src) -- the union of what n_dist_changed
 * and n_nh_changed count.  Per entry:
 *   node      u32  csr id
 *   dist      u64  the new metric, UINT64_MAX when v is now unreachable (u64 so
 *                  that exact / u64-label plans share the layout)
 *   nh[W]     u32  the new next-hop set, the digest's bitset (bits over the
 *                  distinct up neighbours of src in the unfailed graph,
 *                  ascending id), W = max(1, ceil(k / 32)); all zero when v is
 *                  unreachable
 * One exactly sized set per plan, on the device until the next call:
 *   cptr[n_fail + 1]   u64  failure i owns entries cptr[i] .. cptr[i + 1]
 *   cnode[total]       u32
 *   cdist[total]       u64
 *   cnh[total * W]     u32
 * A cold failure owns none.  The order of a failure's entries on the device
 * is unspecified (spf_whatif_changes_db sorts).  Built as count, exclusive
 * scan, fill: the repairs run twice, the second time writing entry k of
 * failure i at cptr[i] + k; a repair that meets more entries than were
 * counted for it drops them and the call reports SPF_E_HIP.
 *
 * spf_whatif_changes does what spf_whatif_execute does plus the lists: d_out
 * ([n_fail]) and d_base are optional device digests, equal to
 * spf_whatif_execute's.  *n_entries = total, *pool_bytes = 8 (n_fail + 1) +
 * total (12 + 4 W), *kernel_ms = count + scan + fill (spf_whatif_changes_timing:
 * apart); the outputs are optional.  Waits (the scan's total is read to size
 * the pools, which are kept while they are large enough).  SPF_E_NOMEM: the
 * pools do not fit beside the repair scratch; SPF_E_STATE: the graph changed
 * since the plan was created.  After a failed call the plan holds no lists. */
spf_status spf_whatif_changes(spf_whatif_plan* plan, spf_whatif_digest* d_out,
                              spf_whatif_digest* d_base, uint64_t* n_entries,
                              uint64_t* pool_bytes, double* kernel_ms, void* stream);
/* ms[3] = count pass, scan, fill pass of the last spf_whatif_changes. */
spf_status spf_whatif_changes_timing(const spf_whatif_plan* plan, double* ms);
/* Failure i's entries, ascending by node (sorted on the host): *n of them;
 * node[cap], dist[cap], nh[cap * W] are filled when cap >= *n, SPF_E_NOMEM
 * (with *n set) otherwise.  Every output may be NULL.  SPF_E_STATE when the
 * plan holds no lists. */
spf_status spf_whatif_changes_db(spf_whatif_plan* plan, uint32_t i, uint32_t* node, uint64_t* dist,
                                 uint32_t* nh, uint64_t cap, uint64_t* n);
/* The whole set in one copy per array, in device order: ptr[n_fail + 1],
 * node[total], dist[total], nh[total * W], total = a previous call's
 * n_entries.  Every output may be NULL.  SPF_E_STATE when the plan holds no
 * lists. */
spf_status spf_whatif_changes_read(spf_whatif_plan* plan, uint64_t* ptr, uint32_t* node,
                                   uint64_t* dist, uint32_t* nh);
/* The device arrays, for device-side consumers (valid until the next
 * spf_whatif_changes on the plan); every output may be NULL. */
spf_status spf_whatif_changes_buffers(spf_whatif_plan* plan, const uint64_t** d_ptr,
                                      const uint32_t** d_node, const uint64_t** d_dist,
                                      const uint32_t** d_nh, uint32_t* W, uint64_t* n_entries);
/* The unfailed result the lists are a patch against: dist[n_nodes] (UINT64_MAX
 * = unreachable), nh[n_nodes * W] in the same bitset (zero rows for
 * unreachable nodes), *W; every output may be NULL.  Waits for the last
 * execute / changes call; SPF_E_STATE before the first. */
spf_status spf_whatif_base(spf_whatif_plan* plan, uint64_t* dist, uint32_t* nh, uint32_t* W);
/* ---- what-if route impact: which ROUTES of src each failure changes.
 * A route belongs to a prefix, a prefix is advertised by a set of nodes
 * (anycast, a default route, a VIP).  Set s = set_nodes[set_ptr[s] ..
 * set_ptr[s + 1]) is given exactly as for spf_routes: the advertisers of one
 * prefix, already filtered by the caller for reachability / drain as
 * buildRouteDb does.  A what-if drain does NOT re-filter them: a set keeps a
 * member the failure drains.  The route of set s is (min_metric, nh):
 *   min_metric  u64  getMinCostNodes (Decision.cpp:1082-1105): the min of
 *                    dist(v) over the reachable members, UINT64_MAX when none
 *                    is reachable
 *   nh[W]       u32  the OR of nh(v) over the members at that min
 *                    (getNextHopsWithMetric without LFA, :1107-1155), in the
 *                    change lists' own bitset: bits over the distinct up
 *                    neighbours of src in the unfailed graph, W words
 * A repeated member counts once; a set that holds src is src's own prefix,
 * metric 0 and no next hops whatever else it holds.
 * For failure i of the plan: the sets whose route under failure i differs from
 * the base route in min_metric or in any word.  One exactly sized set per
 * plan, on the device until the next call:
 *   rptr[n_fail + 1]   u64  failure i owns entries rptr[i] .. rptr[i + 1]
 *   rset[total]        u32  set id (two identical sets are two entries)
 *   rmetric[total]     u64  the new min_metric; a withdrawn route is listed
 *                           with UINT64_MAX and zero words
 *   rnh[total * W]     u32
 * Empty sets, sets unreachable in the base and sets that hold src are never
 * listed.  The order of a failure's entries on the device is unspecified
 * (spf_whatif_routes_db sorts).  *n_entries = total, *pool_bytes =
 * 8 (n_fail + 1) + total (12 + 4 W), *kernel_ms = the four phases of
 * spf_whatif_routes_timing together; the outputs are optional.  n_sets == 0 is
 * allowed: zero entries.
 *
 * A device-side consumer of the resident change lists: it needs
 * spf_whatif_changes on the plan first, reads only the lists and the unfailed
 * result, and so works on every plan kind (links, nodes down / drained, link
 * sets, metric changes, and link plans on exact-path graphs).  Built as the
 * lists are: the base routes and a lookup table over the list entries, a
 * count pass driven by the entries, a scan, a fill pass into the exactly sized
 * pools (kept while they are large enough).  Waits.
 * SPF_E_INVALID: a NULL plan, set_ptr[0] != 0, set_ptr decreasing, a node id
 * >= n_nodes, NULL arrays with members.  SPF_E_STATE: the plan holds no lists;
 * the graph changed since the plan was created.  SPF_E_NOMEM: the pools or
 * the table do not fit.  SPF_E_HIP: a fill pass that meets more entries than
 * were counted drops them, as the lists do.  After a failed call the plan
 * holds no route lists, and a new spf_whatif_changes on the plan invalidates
 * them.
 * These lists are node-level: the expansion over src's own links
 * (getNextHopsThrift) is spf_whatif_route_update's, below; LFA and SpfSolver's
 * prefix bookkeeping stay with the caller. */
spf_status spf_whatif_routes(spf_whatif_plan* plan, const uint32_t* set_ptr /* [n_sets + 1] */,
                             const uint32_t* set_nodes /* [set_ptr[n_sets]] */, uint32_t n_sets,
                             uint64_t* n_entries, uint64_t* pool_bytes, double* kernel_ms,
                             void* stream);
/* Every set's base route: min_metric[n_sets], nh[n_sets * W]; either may be
 * NULL.  This and the calls below: SPF_E_STATE when the plan holds no route
 * lists (before a successful spf_whatif_routes). */
spf_status spf_whatif_routes_base(spf_whatif_plan* plan, uint64_t* min_metric, uint32_t* nh);
/* Failure i's entries, ascending by set id (sorted on the host): *n of them;
 * set[cap], min_metric[cap], nh[cap * W] are filled when cap >= *n,
 * SPF_E_NOMEM (with *n set) otherwise.  Every output may be NULL. */
spf_status spf_whatif_routes_db(spf_whatif_plan* plan, uint32_t i, uint32_t* set, uint64_t* min_metric,
                                uint32_t* nh, uint64_t cap, uint64_t* n);
/* The whole set in one copy per array, in device order: ptr[n_fail + 1],
 * set[total], min_metric[total], nh[total * W].  Every output may be NULL. */
spf_status spf_whatif_routes_read(spf_whatif_plan* plan, uint64_t* ptr, uint32_t* set,
                                  uint64_t* min_metric, uint32_t* nh);
/* The device arrays, for device-side consumers (valid until the next
 * spf_whatif_routes or spf_whatif_changes on the plan); every output may be
 * NULL. */
spf_status spf_whatif_routes_buffers(spf_whatif_plan* plan, const uint64_t** d_ptr,
                                     const uint32_t** d_set, const uint64_t** d_metric,
                                     const uint32_t** d_nh, uint32_t* W, uint64_t* n_entries);
/* ms[4] = base routes + table, count pass, scan, fill pass of the last
 * spf_whatif_routes. */
spf_status spf_whatif_routes_timing(const spf_whatif_plan* plan, double* ms);
/* ---- what-if route updates: each failure's LINK-LEVEL next hops.
 * What a FIB would be told under failure i: for a set s of the last
 * spf_whatif_routes, with (min', nh') its route under failure i (the route-list
 * entry when (i, s) is listed, the base route otherwise) and d'(x) the metric of
 * node x under failure i (the change-list entry when listed, the unfailed metric
 * otherwise), the slots q of src's CSR row, in row order (linksFromNode order),
 * that are
 *   live      not a dead self-loop (a link that is not up);
 *   surviving link plans: link_id[q] != l_i; node down: col[q] != x_i; node
 *             drain: always; link sets: link_id[q] not in set i; metric changes:
 *             always, weighing w'(q) = the substituted metric of its direction
 *             when link_id[q] == l_i and that direction is not kept;
 *   wanted    the bit of col[q] is set in nh';
 *   tight     w'(q) == d'(col[q])  (getNextHopsThrift's distOverLink ==
 *             minMetric, Decision.cpp:1198-1305, without LFA).
 * A record is q | min' << 32, the record of spf_routes and
 * spf_mplan_route_records; a withdrawn route (min' == UINT64_MAX) has none.
 * The update list of failure i holds every set whose record sequence under
 * failure i differs from its base sequence (no failure).  It is the route list
 * plus what node-level lists cannot see: a failure that removes or re-weighs a
 * slot of src's own row -- one member of a bundle, a member's metric raised, a
 * heavier parallel link lowered onto the tie -- changes the records of every
 * route through that neighbour while no node's metric or neighbour set moves.
 * Empty sets, sets that hold src and sets unreachable in the base are never
 * listed.  One exactly sized set per plan, on the device until the next call:
 *   uptr[n_fail + 1]      u64  failure i owns entries uptr[i] .. uptr[i + 1]
 *   uset[total]           u32  set id
 *   umetric[total]        u64  min' (UINT64_MAX: withdrawn, no records)
 *   urec_ptr[total + 1]   u64  entry e owns records urec_ptr[e] .. urec_ptr[e + 1]
 *   urec[records]         u64  contiguous per entry, in slot order
 * The order of a failure's entries on the device is unspecified (_db sorts).
 * *n_entries = total, *n_records = records, *pool_bytes = 8 (n_fail + 1) +
 * 12 total + 8 (total + 1) + 8 records, *kernel_ms = the phases of
 * spf_whatif_route_update_timing together; the outputs are optional.  n_sets
 * == 0 and zero failures are allowed.
 *
 * A device-side consumer of the change lists and the route lists: every set's
 * base records; a pass over the failures that finds those touching src's row,
 * each with the mask of the neighbours whose slots it changes; a count pass
 * with a lane per route-list entry walking the row, and for the touched
 * failures a sweep over the sets their route lists do not hold (the row is
 * walked where a base route's words meet the mask); the pools' scan; a fill
 * pass; the scan again over the entries' record counts; a pass that writes the
 * records.  No buffer is n_fail x n_sets or n_fail x n_nodes.  Waits.
 * SPF_E_INVALID: a NULL plan.  SPF_E_STATE: the plan holds no route lists
 * (spf_whatif_changes, then spf_whatif_routes over the sets in question, first);
 * the graph changed since the plan was created.  SPF_E_UNSUPPORTED: the plan
 * runs on the exact path (a metric <= 0 or u64 labels), where a record could
 * not hold the metric; nothing is launched.  SPF_E_NOMEM: the pools do not
 * fit.  SPF_E_HIP: a fill that meets more than was counted drops the excess,
 * as the lists do.  After a failed call the plan holds no update lists; a new
 * spf_whatif_changes or spf_whatif_routes invalidates them; a new
 * spf_whatif_route_update leaves the spf_whatif_by_set results valid. */
spf_status spf_whatif_route_update(spf_whatif_plan* plan, uint64_t* n_entries, uint64_t* n_records,
                                   uint64_t* pool_bytes, double* kernel_ms, void* stream);
/* Failure i's entries, ascending by set id (sorted on the host): *n of them
 * with *n_rec records; set[cap_entries], min_metric[cap_entries],
 * rec_ptr[cap_entries + 1] (offsets into rec, from 0) and rec[cap_records] are
 * filled when both capacities suffice, SPF_E_NOMEM (with *n and *n_rec set)
 * otherwise.  Every output may be NULL.  This and the calls below: SPF_E_STATE
 * when the plan holds no update lists. */
spf_status spf_whatif_route_update_db(spf_whatif_plan* plan, uint32_t i, uint32_t* set,
                                      uint64_t* min_metric, uint64_t* rec_ptr, uint64_t* rec,
                                      uint64_t cap_entries, uint64_t cap_records, uint64_t* n,
                                      uint64_t* n_rec);
/* The whole set in one copy per array, in device order: ptr[n_fail + 1],
 * set[total], min_metric[total], rec_ptr[total + 1], rec[records].  Every
 * output may be NULL. */
spf_status spf_whatif_route_update_read(spf_whatif_plan* plan, uint64_t* ptr, uint32_t* set,
                                        uint64_t* min_metric, uint64_t* rec_ptr, uint64_t* rec);
/* The device arrays, for device-side consumers (valid until the next
 * spf_whatif_route_update, spf_whatif_routes or spf_whatif_changes on the
 * plan); every output may be NULL. */
spf_status spf_whatif_route_update_buffers(spf_whatif_plan* plan, const uint64_t** d_ptr,
                                           const uint32_t** d_set, const uint64_t** d_metric,
                                           const uint64_t** d_rec_ptr, const uint64_t** d_rec,
                                           uint64_t* n_entries, uint64_t* n_records);
/* Every set's base records: rec_ptr[n_sets + 1], rec[rec_ptr[n_sets]]; either
 * may be NULL (read rec_ptr first to size rec). */
spf_status spf_whatif_route_update_base(spf_whatif_plan* plan, uint64_t* rec_ptr, uint64_t* rec);
/* ms[7] = base records, touch pass, count pass, scan, fill pass, the records'
 * scan, record pass of the last spf_whatif_route_update. */
spf_status spf_whatif_route_update_timing(const spf_whatif_plan* plan, double* ms);
/* The failures of the plan that change a slot of src's row (the ones swept) and
 * the number of base records; either may be NULL. */
spf_status spf_whatif_route_update_stats(spf_whatif_plan* plan, uint32_t* n_touched,
                                         uint64_t* base_records);
/* Launch constants the tests cross: the sets a workgroup of the sweep takes per
 * round, the counts the pools' scan takes per round, and the longest row of
 * src that the walking kernels stage in LDS (a longer one is read from L2). */
uint32_t spf_whatif_route_update_sweep_sets(void);
uint32_t spf_whatif_route_update_lds_slots(void);
uint32_t spf_whatif_scan_tile(void);
/* ---- what-if impact by destination: the lists above, keyed by what is hit.
 * The change and route lists are keyed by the failure.  "Which failures touch
 * node v (or prefix s), which of them cut it off, which is the worst and how
 * narrow does its ECMP get" is keyed by the destination: the resident lists
 * transposed on the device, and a summary per key.  Keys are nodes over the
 * change lists (spf_whatif_by_node: n_keys = n_nodes, base = what
 * spf_whatif_base returns) and set ids over the route lists
 * (spf_whatif_by_set: n_keys = the n_sets of the last spf_whatif_routes, base =
 * spf_whatif_routes_base).  An "entry of key k" is a list entry whose node /
 * set is k; a plan that lists a failure twice gives k two entries. */
#define SPF_WHATIF_NONE 0xFFFFFFFFu
#define SPF_WHATIF_BY_NODE 0u /* `which` of spf_whatif_impact_timing */
#define SPF_WHATIF_BY_SET 1u
typedef struct spf_whatif_impact { /* 32 bytes, one per key (node or set) */
  uint32_t n_changed;     /* failures of the plan whose list holds the key            */
  uint32_t n_unreachable; /* ... with the new metric UINT64_MAX (cut off / withdrawn) */
  uint32_t n_metric;      /* ... with the new metric != the base metric (incl. those) */
  uint32_t min_width;     /* smallest popcount of the next-hop words over the key's
                             entries with a finite metric; the base popcount when none */
  uint64_t max_metric;    /* max(base metric, largest finite new metric of an entry)  */
  uint32_t max_fail;      /* smallest failure index i whose entry has that metric, when
                             it is > the base metric; SPF_WHATIF_NONE otherwise        */
  uint32_t reserved;      /* 0 */
} spf_whatif_impact;
/* One exactly sized set per plan and flavour, on the device until the next
 * call of that flavour:
 *   tptr[n_keys + 1]   u64  key k owns transposed entries tptr[k] .. tptr[k + 1]
 *   tfail[total]       u32  the failure index i
 *   tent[total]        u64  the index e of that entry in the list pools, so a
 *                           consumer reads cdist[e] and cnh[e * W] (rmetric[e],
 *                           rnh[e * W]) without a search
 *   imp[n_keys]             the summaries
 * total equals the lists' n_entries.  *pool_bytes = 8 (n_keys + 1) + 12 total +
 * 32 n_keys, *kernel_ms = the three phases of spf_whatif_impact_timing
 * together; the outputs are optional.  The order of a key's entries on the
 * device is unspecified (the _db calls sort).  A key with no entry -- by set:
 * also the sets never listed, empty, holding src or unreachable in the base --
 * has n_* = 0, min_width = the base popcount, max_metric = the base metric
 * (UINT64_MAX when unreachable in the base) and max_fail = SPF_WHATIF_NONE.
 * Zero entries (or zero keys) is allowed.
 *
 * Device-side consumers of the resident lists, as spf_whatif_routes is: they
 * read only the lists and the base, and so work on every plan kind and on link
 * plans on exact-path graphs.  Built as the lists are: the summaries start as
 * the base; a count pass with a lane per entry adds to the three counts, takes
 * the 64-bit max of the finite metrics and the min of their popcounts (device-
 * scope atomics); the change lists' scan turns n_changed into tptr; a fill pass
 * finds each entry's failure by bisecting cptr / rptr and places (i, e) at
 * tptr[k] + a per-key cursor.  No buffer is n_fail x n_keys.  Waits.
 * SPF_E_INVALID: a NULL plan.  SPF_E_STATE: the plan holds no change lists
 * (by_node) or no route lists (by_set: spf_whatif_routes first); the graph
 * changed since the plan was created.  SPF_E_NOMEM: the pools do not fit.
 * SPF_E_HIP: an entry placed past its key's count is dropped, as in the lists.
 * After a failed call the plan holds none of that flavour; a new
 * spf_whatif_changes invalidates both flavours, a new spf_whatif_routes by_set. */
spf_status spf_whatif_by_node(spf_whatif_plan* plan, uint64_t* n_entries, uint64_t* pool_bytes,
                              double* kernel_ms, void* stream);
spf_status spf_whatif_by_set(spf_whatif_plan* plan, uint64_t* n_entries, uint64_t* pool_bytes,
                             double* kernel_ms, void* stream);
/* The summaries: out[n_keys], may be NULL.  This and the calls below:
 * SPF_E_STATE before a successful spf_whatif_by_node / _by_set. */
spf_status spf_whatif_by_node_impact(spf_whatif_plan* plan, spf_whatif_impact* out);
spf_status spf_whatif_by_set_impact(spf_whatif_plan* plan, spf_whatif_impact* out);
/* Key `key`'s entries, ascending by failure index (sorted on the host): *n of
 * them; fail[cap], ent[cap] are filled when cap >= *n, SPF_E_NOMEM (with *n
 * set) otherwise.  Every output may be NULL.  SPF_E_INVALID: key >= n_keys. */
spf_status spf_whatif_by_node_db(spf_whatif_plan* plan, uint32_t key, uint32_t* fail, uint64_t* ent,
                                 uint64_t cap, uint64_t* n);
spf_status spf_whatif_by_set_db(spf_whatif_plan* plan, uint32_t key, uint32_t* fail, uint64_t* ent,
                                uint64_t cap, uint64_t* n);
/* The whole set in one copy per array, in device order: ptr[n_keys + 1],
 * fail[total], ent[total], imp[n_keys].  Every output may be NULL. */
spf_status spf_whatif_by_node_read(spf_whatif_plan* plan, uint64_t* ptr, uint32_t* fail, uint64_t* ent,
                                   spf_whatif_impact* imp);
spf_status spf_whatif_by_set_read(spf_whatif_plan* plan, uint64_t* ptr, uint32_t* fail, uint64_t* ent,
                                  spf_whatif_impact* imp);
/* The device arrays, for device-side consumers (valid until the next call of
 * the flavour or of what invalidates it); every output may be NULL. */
spf_status spf_whatif_by_node_buffers(spf_whatif_plan* plan, const uint64_t** d_ptr,
                                      const uint32_t** d_fail, const uint64_t** d_ent,
                                      const spf_whatif_impact** d_imp, uint32_t* n_keys,
                                      uint64_t* n_entries);
spf_status spf_whatif_by_set_buffers(spf_whatif_plan* plan, const uint64_t** d_ptr,
                                     const uint32_t** d_fail, const uint64_t** d_ent,
                                     const spf_whatif_impact** d_imp, uint32_t* n_keys,
                                     uint64_t* n_entries);
/* ms[3] = count pass (with the summaries' initialisation), scan, fill pass of
 * the last spf_whatif_by_node (which = SPF_WHATIF_BY_NODE) or _by_set. */
spf_status spf_whatif_impact_timing(const spf_whatif_plan* plan, uint32_t which, double* ms);
/* Convenience: plan + execute + copy back. out = [n_fail] (n_fail = number of
 * up links when fail_links is NULL), base may be NULL. */
spf_status spf_whatif_solve(spf_ctx* ctx, uint32_t src, const uint32_t* fail_links,
                            uint32_t n_fail, spf_whatif_digest* out, spf_whatif_digest* base);

/* ---- SpfSolver next-hop selection (Decision.cpp:1082-1305) -------------- */
/* For node `me` and n_sets destination sets (set i = set_nodes[set_ptr[i] ..
 * set_ptr[i+1]), the advertisers of one prefix or the owner of one node
 * label, already filtered for reachability / drain as buildRouteDb does):
 *   getMinCostNodes      -> min_metric[i] (UINT64_MAX: no member reachable)
 *   getNextHopsWithMetric + getNextHopsThrift (single area, perDestination
 *   false) -> nh_count[i] next hops, each an up link of me (nh_edge = the
 *   directed CSR edge me -> neighbour, so link_id[] and the metric advertised
 *   by me come with it) and its metric w(link) + dist(neighbour, dst)
 *   (nh_metric).  Without SPF_ROUTE_LFA only links on shortest paths are
 *   kept; with it every neighbour passing the RFC 5286 condition of
 *   Decision.cpp:1180 is added.
 * nh_edge / nh_metric hold deg(me) entries per set: [n_sets * deg(me)], where
 * deg(me) = row_ptr[me+1] - row_ptr[me]. */
#define SPF_ROUTE_LFA 0x1u
spf_status spf_routes(spf_ctx* ctx, uint32_t me, const uint32_t* set_ptr,
                      const uint32_t* set_nodes, uint32_t n_sets, uint32_t flags,
                      uint64_t* min_metric, uint32_t* nh_count, uint32_t* nh_edge,
                      uint64_t* nh_metric);

/* ---- multi-device context: several GPUs behind one host thread ----------- */
/* SURVEY.md §8(b)'s spf_ctx_create(gpu_ids, ngpu): Open/R's Decision runs in
 * one process on one event-base thread (Decision.cpp:1484), so the GPUs of a
 * node are reached from one context, not a process per GPU.  An spf_mctx
 * holds one member engine context per listed device id (ids may repeat: the
 * members of one device share its execute stream and run one after another
 * there), each with a replica of the graph.  An spf_mplan splits a batch of
 * sources over the members and keeps each member's distance rows and
 * next-hop bitmaps resident in that member's HBM; queries are answered by the
 * owning member.  Results are bit-identical to one spf_plan over the batch.
 *
 * Partition of the sources (also usable on its own, host only):
 *   SPF_PARTITION_CONTIGUOUS  blocks of the request order balanced by the
 *                             bytes each source's results take (k + 40
 *                             bitmaps, k = distinct up neighbours)
 *   SPF_PARTITION_LOCALITY    a streaming partition keeping each member's
 *                             closure (sources + their neighbours, whose rows
 *                             the next-hop pass reads) small: a fabric's pods
 *                             and planes stay together
 *   SPF_PARTITION_AUTO        locality when its largest closure is smaller
 *                             (graphs up to 65,536 nodes), else contiguous */
#define SPF_PARTITION_AUTO 0u
#define SPF_PARTITION_CONTIGUOUS 1u
#define SPF_PARTITION_LOCALITY 2u
/* nb_ptr/nb_id: distinct up neighbours per node (spf_src_neighbors of every
 * node, CSR form); part_out[i] = part of srcs[i]; *mode_used = the rule taken. */
spf_status spf_partition_sources(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                                 const uint32_t* srcs, uint32_t n_src, uint32_t n_parts,
                                 uint32_t mode, uint32_t* part_out, uint32_t* mode_used);

typedef struct spf_mctx spf_mctx;
typedef struct spf_mplan spf_mplan;
spf_status spf_mctx_create(const int* gpu_ids, uint32_t n, spf_mctx** out);
void spf_mctx_destroy(spf_mctx* m);
const char* spf_mctx_last_error(const spf_mctx* m);
uint32_t spf_mctx_size(const spf_mctx* m);
/* member i's engine context (owned by the mctx; every single-context call
 * works on it) and its device id */
spf_ctx* spf_mctx_member(spf_mctx* m, uint32_t i);
int spf_mctx_device(const spf_mctx* m, uint32_t i);
/* graph replicated to every member; patches applied to every replica */
spf_status spf_mctx_graph_load(spf_mctx* m, const spf_graph* g);
spf_status spf_mctx_graph_set_overload(spf_mctx* m, const uint32_t* nodes,
                                       const uint8_t* overloaded, uint32_t n);
spf_status spf_mctx_graph_patch_rows(spf_mctx* m, const uint32_t* nodes, uint32_t n,
                                     const uint32_t* col, const int32_t* metric, const uint32_t* link);
spf_status spf_mctx_graph_set_metric(spf_mctx* m, const uint32_t* edges, const int32_t* metric,
                                     uint32_t n);

/* A batch of sources split over the members (partition `mode`), result
 * buffers owned by the plan on each member's device. */
spf_status spf_mplan_create(spf_mctx* m, const uint32_t* srcs, uint32_t n_src, uint32_t flags,
                            uint32_t mode, spf_mplan** out);
void spf_mplan_destroy(spf_mplan* mp);
uint32_t spf_mplan_partition(const spf_mplan* mp);   /* SPF_PARTITION_* taken */
/* request index i (srcs[i]) -> owning member, row in that member's plan */
spf_status spf_mplan_owner(const spf_mplan* mp, uint32_t i, uint32_t* member, uint32_t* row);
/* member's share: its plan (spf_plan_nh_layout etc.), its resident device
 * buffers ([n][pitch] rows, next-hop words) -- for device-side consumers */
spf_status spf_mplan_shard(spf_mplan* mp, uint32_t member, uint32_t* n_src, spf_plan** plan,
                           void** d_dist, uint32_t** d_nh);
uint32_t spf_mplan_closure_rows(const spf_mplan* mp, uint32_t member);
/* enable != 0: each member's execute is captured into a hipGraph after the
 * first execute of a graph epoch and replayed after that (re-captured after
 * an in-place patch) */
spf_status spf_mplan_set_graphs(spf_mplan* mp, int enable);
/* Host enqueue threads: mode 1 issues each member's execute from its own host
 * thread (spinning briefly between back-to-back executes, then sleeping), 0
 * from the caller's thread one member after another, -1 (default) threads
 * when the members with work sit on two or more distinct devices. */
spf_status spf_mplan_set_enqueue_threads(spf_mplan* mp, int mode);
/* The last execute's host enqueue: out[i] = ns from the execute's start until
 * member i's launches were enqueued (0 for members without work); *threaded =
 * 1 when it used the enqueue threads.  The spread of out[] is the start
 * stagger the members' GPUs see. */
spf_status spf_mplan_enqueue_ns(const spf_mplan* mp, uint64_t* out, uint32_t n, int* threaded);
/* Enqueue every member's execute on its device's stream; no host wait. */
spf_status spf_mplan_execute(spf_mplan* mp);
/* Wait for every member and check its grid / team barriers (spf_device_check). */
spf_status spf_mplan_synchronize(spf_mplan* mp);
/* Per-source digests (spf_plan_digest's hash) in request order, computed on
 * each owning device; waits. */
spf_status spf_mplan_digest(spf_mplan* mp, uint64_t* out);
/* Source i's result from its owner: dist = [n_nodes] (u32, u64 with
 * SPF_FLAG_DIST64), nh = k bitmaps of spf_row_pitch/32 words (k = distinct up
 * neighbours of srcs[i]); either may be NULL.  Waits for the owner's stream. */
spf_status spf_mplan_read(spf_mplan* mp, uint32_t i, void* dist, uint32_t* nh);
/* pathLinks of source i (spf_preds' output) from the resident row on its
 * owning device; SPF_E_UNSUPPORTED for zero / negative metrics and u64 rows. */
spf_status spf_mplan_preds(spf_mplan* mp, uint32_t i, uint32_t* pred_ptr, uint32_t* pred_edge,
                           uint32_t cap, uint32_t* n_preds);
/* Route selection of many nodes from the resident pass (no new SPF): the
 * reference's getNextHopsWithMetric + getNextHopsThrift (Decision.cpp:
 * 1082-1305, perDestination = false, one area) of every me = srcs[me_req[t]]
 * towards every destination set p (set_ptr / set_nodes as spf_routes),
 * evaluated on me's owning device from its resident row and bitmaps (LFA:
 * every neighbour's resident row, read over peer access when it lives on
 * another device).  What Decision::getDecisionRouteDb(node) for every node
 * (Decision.cpp:1480-1500) computes, minus the thrift formatting.
 * spf_mplan_route_digests: per me, digests[t] = sum over sets p with a kept
 * next hop of mix(mix(0x9e3779b97f4a7c15 (p+1) + shortest) + sum over kept
 * links of mix(link_hash[link id] + (u32) metric) + p) (mix = splitmix64's
 * finaliser; link_hash[id] identifies link `id` by value, as for
 * spf_ksp2_digest); *kernel_ms (optional) = the slowest member's kernel time.
 * spf_mplan_routes: one me's records in spf_routes' layout.  Rows must be u32
 * link-metric rows (not SPF_FLAG_HOP_COUNT / SPF_FLAG_DIST64). */
spf_status spf_mplan_route_digests(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* set_ptr, const uint32_t* set_nodes,
                                   uint32_t n_sets, uint32_t flags, const uint64_t* link_hash,
                                   uint32_t n_links, uint64_t* digests, double* kernel_ms);
spf_status spf_mplan_routes(spf_mplan* mp, uint32_t me_req, const uint32_t* set_ptr,
                            const uint32_t* set_nodes, uint32_t n_sets, uint32_t flags,
                            uint64_t* min_metric, uint32_t* nh_count, uint32_t* nh_edge,
                            uint64_t* nh_metric);
/* Every me's route database materialised on its owning device (the same
 * selection as spf_mplan_route_digests, written out instead of hashed): what
 * Decision::getDecisionRouteDb(node) returns for every node (Decision.cpp:
 * 1480-1500 -> buildRouteDb :556-722, one area), in device memory.  Per me t
 * and set p a header word = offset | count << 32 | stride << 48: the route's
 * k-th next hop (k < count) is record offset + k * stride of me's region, a
 * u64 = CSR edge (me -> neighbour: link id, interface, neighbour and the
 * metric me advertises come with it) | metric << 32 (w(link) +
 * dist(neighbour, dst)), in me's link order -- getNextHopsThrift's next
 * hops.  Device layout: me's region is one [deg(me)][1024] tile per 1024
 * sets (stride 1024), so consecutive routes' k-th next hops are adjacent; a
 * region holds ceil(n_sets / 1024) * 1024 * deg(me) record slots (unused ones
 * are never written).  Sets without a kept next hop have count 0.
 * SPF_E_UNSUPPORTED when a metric exceeds 2^32 - 1 or a region 2^32 slots,
 * and -- before anything is uploaded or launched, the error naming the node --
 * for a me whose CSR row has 65536 or more slots (dead ones included): the
 * header's count has 16 bits and a route keeps up to one next hop per slot.
 * (spf_mplan_label_routes has 64-bit offsets and no such limit.)
 * *n_records (optional) = records over every me; *kernel_ms (optional) = the
 * slowest member's kernel.  The databases stay resident until the next call.
 *
 * SPF_ROUTE_COMPACT (alone or with SPF_ROUTE_LFA): the same headers' fields
 * and the same records in an exactly sized pool.  Per member the routes of its
 * me slots lie in one contiguous pool of exactly `records` u64, in slot order
 * and within a me in set order: route (slot k, p) holds pool[base[k] + offset
 * .. + count), its header = offset | count << 32 | 1 << 48 (stride 1), offset
 * relative to me's region, which is exactly its records; a route without next
 * hops has count 0 and the offset where it would start, so base[k] + offset
 * over (k, p) is the exclusive scan of the counts.  Built by a count walk, a
 * scan and a fill walk (as spf_mplan_label_routes); *kernel_ms = the three
 * together.  The 65536-slot and the metric refusals hold as above; the region
 * limit becomes: SPF_E_UNSUPPORTED when one me has 2^32 records or more.
 * After a call that failed the plan holds no database. */
#define SPF_ROUTE_COMPACT 0x2u
spf_status spf_mplan_route_records(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* set_ptr, const uint32_t* set_nodes, uint32_t n_sets,
                                   uint32_t flags, uint64_t* n_records, double* kernel_ms);
/* The last spf_mplan_route_records' pools: *layout = 0 tiled, 1 compact;
 * *pool_bytes = the device bytes of the record pools over the members that
 * hold a me (tiled: 8 x the regions' slots; compact: 8 x max(records, 1) each
 * -- a pool left by an earlier compact call is kept while it is large enough,
 * and counts as allocated); *record_bytes = 8 x records.  Every output may be
 * NULL.  SPF_E_STATE when the plan holds no database (no call yet, or a
 * snapshot took it).  spf_mplan_route_records_timing: ms[3] = the count, scan
 * and fill of the last SPF_ROUTE_COMPACT call that asked for kernel_ms (the
 * slowest member each). */
spf_status spf_mplan_route_record_pool(spf_mplan* mp, uint32_t* layout, uint64_t* pool_bytes,
                                       uint64_t* record_bytes);
spf_status spf_mplan_route_records_timing(const spf_mplan* mp, double* ms);
/* A member's share of the last spf_mplan_route_records, for device-side
 * consumers, in either layout: its header array ([n_slots * n_sets], slot
 * major), base[n_slots] (where each slot's region starts in the pool) and the
 * record pool as device arrays (NULL when it holds no me, or a snapshot took
 * them), its record count, and slots[k] = the index t (into that call's
 * me_req) of its k-th me slot (cap entries; SPF_E_NOMEM when fewer than
 * *n_slots).  Route (k, p)'s j-th next hop is pool[base[k] + offset + j *
 * stride] with offset, count and stride from hdr[k * n_sets + p].  Every
 * output may be NULL. */
spf_status spf_mplan_route_record_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_hdr,
                                          const uint64_t** d_base, const uint64_t** d_pool,
                                          uint64_t* n_records, uint32_t* slots, uint32_t cap,
                                          uint32_t* n_slots);
/* Records a block of the SPF_ROUTE_COMPACT fill assembles on chip before it
 * stores them; a block whose routes hold more stores them one by one. */
uint32_t spf_route_compact_stage(void);
/* me t's database from the last spf_mplan_route_records, compacted on the
 * host: hdr = [n_sets] headers offset | count << 32 (stride 1: route p's next
 * hops contiguous, routes in set order; may be NULL), rec = its records (cap
 * entries; SPF_E_NOMEM when fewer than *n; may be NULL), *n = its record
 * count.  Waits. */
spf_status spf_mplan_route_db(spf_mplan* mp, uint32_t t, uint64_t* hdr, uint64_t* rec, uint64_t cap,
                              uint64_t* n);
/* Node-label MPLS routes (Decision.cpp:586-674) of every me from the resident
 * pass.  node_label[v] = node v's segment label; 0 or a label outside the
 * 20-bit space (isMplsLabelValid) = v advertises none (:592-603).
 * spf_label_groups (host only): the distinct advertised labels in ascending
 * order, labels[g], each with the nodes that advertise it in ascending id
 * (= name): grp_nodes[grp_ptr[g] .. grp_ptr[g+1]).  This order is the public
 * group index g of the calls below.  labels / grp_nodes = [n_nodes], grp_ptr =
 * [n_nodes + 1] (any may be NULL); *n_groups = G. */
spf_status spf_label_groups(const int32_t* node_label, uint32_t n_nodes, int32_t* labels,
                            uint32_t* grp_ptr, uint32_t* grp_nodes, uint32_t* n_groups);
/* Per me = srcs[me_req[t]] and label group g, on me's owning device:
 *   owner  the candidate with the smallest name that is me itself or has a
 *          finite distance in me's row; SPF_UNREACHABLE: none, no route.  (The
 *          reference's collision loop, :605-618 with the no-route skip at
 *          :641-647, gives this whatever order it visits the nodes in: a
 *          smaller name replaces the holder only when it has a route.  The
 *          host SpfSolvers' buildRouteDb resolves a collision the same way.)
 *   owner == me: POP_AND_LOOKUP (:620-633), no records.
 *   otherwise the next hops of getNextHopsWithMetric(me, {owner}) +
 *          getNextHopsThrift (:635-668; the selection of spf_mplan_route_records
 *          for the set {owner}, SPF_ROUTE_LFA included), one u64 record each =
 *          CSR edge | metric << 32 in me's link order.  The action is not
 *          stored: PHP when the edge ends at the owner, SWAP to the label
 *          otherwise (:1247-1257).
 * Layout per member (CSR, no packed count): owner[n * G] u32, ptr[n * G + 1]
 * u64, rec[ptr[n * G]] u64, n = the member's me slots; route (slot k, g) holds
 * rec[ptr[k * G + g] .. ptr[k * G + g + 1]).  Built by three passes -- count,
 * an exclusive scan, fill -- so the pool is sized exactly: *pool_bytes
 * (optional) = over the members with a me, 8 records + 8 (n G + 1) + 4 n G.
 * *n_labels = G, *n_records = records over every me, *kernel_ms = the slowest
 * member's kernels (all optional).  SPF_E_UNSUPPORTED for SPF_FLAG_HOP_COUNT /
 * SPF_FLAG_DIST64 plans and when a metric exceeds 2^32 - 1.  The databases
 * stay resident until the next call.  Adjacency-label routes (:676-698: every
 * link of me, no SPF) and static routes are the host's. */
spf_status spf_mplan_label_routes(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                  const int32_t* node_label /* [n_nodes] */, uint32_t flags,
                                  uint32_t* n_labels, uint64_t* n_records, uint64_t* pool_bytes,
                                  double* kernel_ms);
/* me t's label routes from the last spf_mplan_label_routes: owner = [G], ptr =
 * [G + 1] rebased to 0, rec = its records (cap entries; SPF_E_NOMEM when fewer
 * than *n); any may be NULL; *n = its record count.  Waits. */
spf_status spf_mplan_label_route_db(spf_mplan* mp, uint32_t t, uint32_t* owner, uint64_t* ptr,
                                    uint64_t* rec, uint64_t cap, uint64_t* n);
/* A member's share of the last spf_mplan_label_routes, for device-side
 * consumers: its owner / ptr / rec device arrays (NULL when it holds no me),
 * its record count, and slots[k] = the index t (into that call's me_req) of
 * its k-th me slot (cap entries; SPF_E_NOMEM when fewer than *n_slots).  Every
 * output may be NULL. */
spf_status spf_mplan_label_route_buffers(spf_mplan* mp, uint32_t member, const uint32_t** d_owner,
                                         const uint64_t** d_ptr, const uint64_t** d_rec,
                                         uint64_t* n_records, uint32_t* slots, uint32_t cap,
                                         uint32_t* n_slots);
/* ---- prefix routes: the unicast route decision from prefix entries --------- */
/* Every me's SP_ECMP / IP unicast route decision from the resident pass: what
 * createRouteForPrefix (Decision.cpp:390-554) decides per me, which a fixed
 * destination set per prefix (spf_mplan_route_records) cannot express.  One
 * area, perDestination = false, no prepend labels.
 * The prefix table is a CSR: prefix p's entries are [pfx_ptr[p], pfx_ptr[p+1])
 * of ent_node (advertiser), ent_pp / ent_sp / ent_dist (PrefixMetrics'
 * path_preference, source_preference, distance) and ent_min_nh (minNexthop;
 * <= 0: none); overloaded[n_nodes] marks the drained nodes.  n_pfx == 0 and
 * empty prefixes are valid (the arrays of a table without entries may be NULL).
 * Per me = srcs[me_req[t]] and prefix p, on me's owning device:
 *   R   the entries whose node is me or has a finite distance in me's row
 *       (:411-424)
 *   B0  the entries of R with the greatest (path_preference,
 *       source_preference, -distance) that is >= (0, 0, 0) (selectBestRoutes
 *       :725-752, selectBestPrefixMetrics Util.h:541-570: an entry under that
 *       floor never enters, :544, 555); with SPF_PREFIX_ALL_BEST (best-route
 *       selection off, :743-748) B0 = R
 *   best  me when me is in B0, else B0's smallest id (selectBestNodeArea); with
 *       SPF_PREFIX_ALL_BEST B0's smallest id (:747).  The drained filter never
 *       moves it (:786-789 compares a copy with its source).
 *   B   B0 without its overloaded nodes, or B0 when that would be empty
 *       (maybeFilterDrainedNodes :771-792)
 *   status, in this order:
 *       SPF_PREFIX_NONE         B0 is empty
 *       SPF_PREFIX_SELF         me is in B (:510-513; B, not B0: a drained me
 *                               beside undrained peers routes to them, best = me)
 *       SPF_PREFIX_NO_NEXTHOP   no next hop towards B
 *       SPF_PREFIX_MIN_NEXTHOP  fewer next hops than the largest positive
 *                               ent_min_nh over B (getMinNextHopThreshold
 *                               :755-768, addBestPaths :1031-1041)
 *       SPF_PREFIX_ROUTE        the next hops of spf_mplan_route_records'
 *                               selection for the set B (SPF_ROUTE_LFA
 *                               included), one u64 record each = CSR edge |
 *                               metric << 32 in me's link order
 *   Only SPF_PREFIX_ROUTE has records.
 * Layout per member (CSR, as spf_mplan_label_routes): info[n * P] u64 = best |
 * |B| << 32 | status << 56 (best = SPF_UNREACHABLE for SPF_PREFIX_NONE),
 * ptr[n * P + 1] u64, rec[ptr[n * P]] u64, n = the member's me slots, P =
 * n_pfx; route (slot k, p) holds rec[ptr[k * P + p] .. ptr[k * P + p + 1]).
 * Built by three passes -- count, an exclusive scan, fill -- so the pool is
 * sized exactly: *pool_bytes (optional) = over the members with a me, 8
 * records + 8 (n P + 1) + 8 n P.  *n_records = records over every me,
 * *kernel_ms = the slowest member's kernels (optional).  flags: SPF_ROUTE_LFA,
 * SPF_PREFIX_ALL_BEST.
 * SPF_E_INVALID, before anything is uploaded or launched and with the prefix
 * named in the error: pfx_ptr not starting at 0 or decreasing, a node id >=
 * n_nodes, the same node twice in one prefix, a distance of INT32_MIN.
 * SPF_E_UNSUPPORTED for SPF_FLAG_HOP_COUNT / SPF_FLAG_DIST64 plans, a prefix
 * of 2^24 entries or more, and when a metric exceeds 2^32 - 1.  After a call
 * that failed the plan holds no prefix database.  The call leaves the plan's
 * other databases (route records, label routes, snapshots, deltas) alone; the
 * databases stay resident until the next call. */
#define SPF_PREFIX_ALL_BEST 0x4u
#define SPF_PREFIX_NONE 0u
#define SPF_PREFIX_SELF 1u
#define SPF_PREFIX_NO_NEXTHOP 2u
#define SPF_PREFIX_MIN_NEXTHOP 3u
#define SPF_PREFIX_ROUTE 4u
spf_status spf_mplan_prefix_routes(spf_mplan* mp, const uint32_t* me_req, uint32_t n_me,
                                   const uint32_t* pfx_ptr /* [n_pfx + 1] */, const uint32_t* ent_node,
                                   const int32_t* ent_pp, const int32_t* ent_sp, const int32_t* ent_dist,
                                   const int64_t* ent_min_nh, uint32_t n_pfx,
                                   const uint8_t* overloaded /* [n_nodes] */, uint32_t flags,
                                   uint64_t* n_records, uint64_t* pool_bytes, double* kernel_ms);
/* me t's prefix routes from the last spf_mplan_prefix_routes: info = [P], ptr =
 * [P + 1] rebased to 0, rec = its records (cap entries; SPF_E_NOMEM when fewer
 * than *n); any may be NULL; *n = its record count.  SPF_E_INVALID when the
 * plan holds no prefix database or t is not one of its me.  Waits. */
spf_status spf_mplan_prefix_route_db(spf_mplan* mp, uint32_t t, uint64_t* info, uint64_t* ptr,
                                     uint64_t* rec, uint64_t cap, uint64_t* n);
/* A member's share of the last spf_mplan_prefix_routes, for device-side
 * consumers: its info / ptr / rec device arrays (NULL when it holds no me),
 * its record count, and slots[k] = the index t (into that call's me_req) of
 * its k-th me slot (cap entries; SPF_E_NOMEM when fewer than *n_slots).  Every
 * output may be NULL. */
spf_status spf_mplan_prefix_route_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_info,
                                          const uint64_t** d_ptr, const uint64_t** d_rec,
                                          uint64_t* n_records, uint32_t* slots, uint32_t cap,
                                          uint32_t* n_slots);
/* ms[3] = count, scan, fill of the last spf_mplan_prefix_routes that asked for
 * kernel_ms (the slowest member each); SPF_E_STATE without a prefix database. */
spf_status spf_mplan_prefix_routes_timing(const spf_mplan* mp, double* ms);
/* The prefixes of one block of the prefix-routes kernel, the links of me it
 * stages on chip at a time, and the entries of one tile of the scan. */
uint32_t spf_prefix_routes_threads(void);
uint32_t spf_prefix_routes_links(void);
uint32_t spf_prefix_routes_scan_tile(void);
/* ---- route-database delta between two passes ------------------------------ */
/* What Decision publishes after a rebuild is not the database but its
 * difference from the previous one: DecisionRouteDb::calculateUpdate
 * (Decision.cpp:111-146) -- routes to update (new, or the entry differs) and
 * routes to delete.  For every me at once, on the devices that hold the
 * databases:
 *
 * spf_mplan_route_snapshot: the old generation, kept.  The device pools of the
 * last spf_mplan_route_records (headers, record regions of either layout: a
 * delta compares tiled with compact generations freely) and, when there
 * was one, of the last spf_mplan_label_routes (owner / ptr / rec) are MOVED
 * into the snapshot, nothing is copied: the plan holds no database afterwards
 * (spf_mplan_route_db / _label_route_db / _label_route_buffers' pools:
 * SPF_E_STATE / none until the next materialising call, which allocates
 * afresh).  The snapshot also keeps, by value, what reads them later: the me
 * list (node ids), n_nodes, n_sets, the route flags, the labels, each member's
 * slot tables, the row starts, and on every member's device key_old[e] =
 * link_hash[link_id[e]] for every CSR edge of the graph as it is now.
 * link_hash[id] identifies link `id` by value (as for spf_mplan_route_digests;
 * n_links entries covering every link id): records name CSR edges, a row patch
 * reorders slots and a reload may re-issue link ids, so only this key compares
 * across generations.  The snapshot belongs to the plan's spf_mctx: it
 * outlives the plan (spf_mplan_destroy, graph patches and reloads) and is
 * destroyed by spf_route_snapshot_destroy or, at the latest, with the mctx.
 * SPF_E_STATE when the plan holds no route records; SPF_E_INVALID when the
 * label routes were materialised for another me list than the records.
 * spf_route_snapshot_bytes: the device memory it holds. */
typedef struct spf_route_snapshot spf_route_snapshot;
spf_status spf_mplan_route_snapshot(spf_mplan* mp, const uint64_t* link_hash, uint32_t n_links,
                                    spf_route_snapshot** out);
void spf_route_snapshot_destroy(spf_route_snapshot* snap);
uint64_t spf_route_snapshot_bytes(const spf_route_snapshot* snap);
/* spf_mplan_route_delta: the plan's current databases (new; the last
 * spf_mplan_route_records and spf_mplan_label_routes) against the snapshot
 * (old), per me on the device that owns it now; an old database on another
 * member is read in place (over peer access when that is another device).
 * A route's value is its set of next hops, each a (link identity, metric)
 * pair -- interface, neighbour, address and area follow from the link as seen
 * from me.
 *   IP route (me, set p): unchanged when both have no next hop or the two
 *     sets are equal; DELETE when only the old one has next hops; UPDATE when
 *     the new one has and the route is new or its set differs.
 *   Label route (me, label): the same with the owner part of the value (the
 *     PHP / SWAP action follows from it): owner SPF_UNREACHABLE = no route, an
 *     owner change is an UPDATE whatever the next hops, owner == me on both
 *     sides (POP_AND_LOOKUP) is unchanged.  Labels are matched by value, not
 *     by group index; a label of one generation only is a DELETE or an UPDATE.
 * A me whose CSR row has the same key sequence in both generations compares
 * records position by position; any other me by set equality on (key, metric).
 * Output per member (CSR, exactly sized, built by count / scan / fill, no
 * atomics per route), one pair for IP routes and one for labels: dptr[n + 1]
 * u64 offsets over the member's n me slots and dset[] u32 entries = the set
 * index (IP) or the label, | SPF_DELTA_DELETE on a delete, ascending within a
 * me.  totals (optional) = [5]: IP updates, IP deletes, label updates, label
 * deletes, me that took the set path; *kernel_ms (optional) = the slowest
 * member's kernels.  The snapshot is only read: a second call gives the same
 * lists.  SPF_E_INVALID when the me list, n_nodes, n_sets, the LFA flag or the
 * presence of label routes differ from the snapshot (a changed node set shifts
 * node ids: out of scope); SPF_E_STATE when the plan holds no databases;
 * SPF_E_UNSUPPORTED for SPF_FLAG_HOP_COUNT / SPF_FLAG_DIST64 plans and for
 * members on distinct devices without peer access.  The lists stay resident
 * until the next call. */
#define SPF_DELTA_DELETE 0x80000000u
spf_status spf_mplan_route_delta(spf_mplan* mp, const spf_route_snapshot* snap, const uint64_t* link_hash,
                                 uint32_t n_links, uint64_t* totals /* [5] */, double* kernel_ms);
/* me t's lists from the last spf_mplan_route_delta: ip / label = its entries
 * (cap entries each; SPF_E_NOMEM when fewer than *n_ip / *n_label; may be
 * NULL).  Waits. */
spf_status spf_mplan_route_delta_db(spf_mplan* mp, uint32_t t, uint32_t* ip, uint64_t ip_cap,
                                    uint64_t* n_ip, uint32_t* label, uint64_t label_cap,
                                    uint64_t* n_label);
/* A member's share of the last spf_mplan_route_delta, for device-side
 * consumers: its dptr / dset device arrays for IP routes and for labels (NULL
 * when it holds no me) and slots[k] = the index t (into the records call's
 * me_req) of its k-th me slot (cap entries; SPF_E_NOMEM when fewer than
 * *n_slots).  Every output may be NULL. */
spf_status spf_mplan_route_delta_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_ip_ptr,
                                         const uint32_t** d_ip_set, const uint64_t** d_label_ptr,
                                         const uint32_t** d_label_set, uint32_t* slots, uint32_t cap,
                                         uint32_t* n_slots);
/* spf_mplan_route_update: the payload of the last spf_mplan_route_delta -- what
 * a DecisionRouteUpdate carries besides the routes' names (Decision.cpp:111-146):
 * the next hops of every listed route, for a label route its owner too --
 * gathered per member on its device out of the plan's CURRENT databases (the
 * new generation; the snapshot is not read) into exactly sized, contiguous
 * pools parallel to the delta's lists.  Per member and kind (IP, labels), over
 * its `entries` list entries in list order:
 *   uptr[entries + 1]  u64 offsets; entry j's records are urec[uptr[j] ..
 *                      uptr[j + 1]): an UPDATE's next hops as its database holds
 *                      them (u64 = CSR edge | metric << 32 of the current graph,
 *                      in me's link order), none for a DELETE
 *   uowner[entries]    labels only: the label's new owner (csr id; me itself:
 *                      POP_AND_LOOKUP, no records), SPF_UNREACHABLE for a DELETE
 * Built by count / scan / fill over ordinary launches, no atomics per route;
 * the pools are allocated from the scan's totals and kept while large enough.
 * totals (optional) = [4]: IP update entries, IP records, label update entries,
 * label records; *pool_bytes (optional) = over the members that hold a me,
 * 8 x records + 8 x (entries + 1) for IP plus the same + 4 x entries for labels;
 * *kernel_ms (optional) = the slowest member's count + scan + fill
 * (spf_mplan_route_update_timing: the three apart, ms[3], of the last call that
 * asked for kernel_ms).  A second call gives identical arrays; a delta without
 * label routes gives empty label outputs.  SPF_E_STATE when there is no delta,
 * or when the plan's databases are no longer the ones it compared: a later
 * spf_mplan_route_records or spf_mplan_label_routes, or a
 * spf_mplan_route_snapshot that moved the pools away (call the delta again).
 * The delta's SPF_E_UNSUPPORTED cases are the delta's.  Waits. */
spf_status spf_mplan_route_update(spf_mplan* mp, uint64_t* totals /* [4] */, uint64_t* pool_bytes,
                                  double* kernel_ms);
spf_status spf_mplan_route_update_timing(const spf_mplan* mp, double* ms /* [3]: count, scan, fill */);
/* me t's payload from the last spf_mplan_route_update, parallel to
 * spf_mplan_route_delta_db's lists (n_ip / n_label entries come from there):
 * ip_ptr[n_ip + 1] / label_ptr[n_label + 1] rebased to 0, label_owner[n_label],
 * the records (ip_cap / label_cap records; SPF_E_NOMEM when fewer than
 * *n_ip_rec / *n_label_rec).  Every output may be NULL.  SPF_E_STATE without an
 * update of the last delta.  Waits. */
spf_status spf_mplan_route_update_db(spf_mplan* mp, uint32_t t, uint64_t* ip_ptr, uint64_t* ip_rec,
                                     uint64_t ip_cap, uint64_t* n_ip_rec, uint32_t* label_owner,
                                     uint64_t* label_ptr, uint64_t* label_rec, uint64_t label_cap,
                                     uint64_t* n_label_rec);
/* A member's whole share of the last delta and update in one copy per array
 * (a flap's payload is a few MB; reading it me by me costs a round trip per
 * me): n (optional) = [5]: its me slots, IP entries, IP records, label entries,
 * label records -- known on the host, so a first call with every array NULL
 * sizes the second --, then the delta's dptr[slots + 1] / dset[entries] and the
 * update's uptr[entries + 1] / urec[records] for IP routes and for labels, and
 * uowner[label entries]; offsets are the member's (not rebased), slot k's me is
 * spf_mplan_route_delta_buffers' slots[k].  Every output may be NULL; the
 * caller's arrays hold at least what n says.  SPF_E_STATE without an update of
 * the last delta.  Waits. */
spf_status spf_mplan_route_update_read(spf_mplan* mp, uint32_t member, uint64_t* n /* [5] */,
                                       uint64_t* ip_dptr, uint32_t* ip_dset, uint64_t* ip_uptr,
                                       uint64_t* ip_urec, uint64_t* label_dptr, uint32_t* label_dset,
                                       uint32_t* label_uowner, uint64_t* label_uptr, uint64_t* label_urec);
/* A member's share of the last spf_mplan_route_update, for device-side
 * consumers: its uptr / urec device arrays for IP routes, uowner / uptr / urec
 * for labels (over the entries of spf_mplan_route_delta_buffers' lists; NULL
 * when it holds no me) and its record totals.  Every output may be NULL. */
spf_status spf_mplan_route_update_buffers(spf_mplan* mp, uint32_t member, const uint64_t** d_ip_uptr,
                                          const uint64_t** d_ip_urec, const uint32_t** d_label_uowner,
                                          const uint64_t** d_label_uptr, const uint64_t** d_label_urec,
                                          uint64_t* n_ip_rec, uint64_t* n_label_rec);
/* HIP-event time of each member's executes: ms[member] summed over the last
 * executes since enable / the last call, *n = executes. */
spf_status spf_mplan_enable_timing(spf_mplan* mp, uint32_t max_executes);
spf_status spf_mplan_timing(spf_mplan* mp, double* ms, uint32_t* n);

/* ---- diagnostics ---------------------------------------------------------- */
/* With SPF_STAMPS set in the environment, the multi-source BFS kernel records
 * s_memtime clocks of workgroup 0 at its phase boundaries (init, then per level:
 * distance stores, pull sweep, barrier; end), per wave: out[w*64] = count,
 * out[w*64 + 1 ..] = clocks of wave w (16 waves).  Copies up to cap words. */
spf_status spf_debug_stamps(spf_ctx* ctx, uint64_t* out, uint32_t cap, uint32_t* n);
/* The device's practical HBM ceiling: a 16-byte grid-stride copy of `bytes`
 * (read + written per rep, `reps` reps timed with HIP events) -> *gbs in
 * GB/s of bytes moved.  What bench.py reports beside the 8 TB/s peak
 * (BASELINE.md §4).  No reference counterpart. */
spf_status spf_debug_copy_bandwidth(spf_ctx* ctx, uint64_t bytes, uint32_t reps, double* gbs);

/* Waits for every launch on the context's device and reports whether a
 * grid-resident kernel's barrier of THIS context (spf_big_kernel, the
 * what-if unfailed pass, the global-memory SSSP, the what-if group teams,
 * the team BFS) gave up waiting: its spin is bounded so a block that never
 * arrives cannot hang the GPU, and the outputs of that launch are then
 * invalid.  Each context has its own fault word, so another context's
 * timeout is neither reported nor cleared here.  SPF_E_HIP (and the word is
 * cleared) when one did; SPF_OK otherwise.  Such launches of one process
 * are serialised per device (one cannot starve another of CUs), so a timeout
 * means a fault or a foreign process holding the CUs.  The synchronous
 * convenience calls (spf_solve, spf_whatif_solve, spf_whatif_stats, ...)
 * check it themselves.  No reference counterpart. */
spf_status spf_device_check(spf_ctx* ctx);

/* ---- counters ----------------------------------------------------------- */
/* Logical single-source solves executed (the reference's decision.spf_runs,
 * LinkState.cpp:815) and kernel time of the last execute in ms. */
uint64_t spf_solves(const spf_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* OPENR_SPF_H_ */
