// ============================================================================
//  graph_host.cpp -- the loaded graph's host state (graph_host.h): a load
//  derives every table for every node, a row patch derives the same tables
//  for the touched nodes with the same per-node helpers.
// ============================================================================
#include "graph_host.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <numeric>

namespace spfi {

namespace {

spf_status refuse(std::string* err, spf_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return st;
}

// ---- metric facts (nonpos, needs64, max_metric, unit) over the live edges ----
void metric_flags(GraphHost& g) {
  g.nonpos = g.n_nonpos > 0;
  // i32 -> u64 wraps (LinkState.h:22); the longest possible path beyond 32
  // bits takes the exact kernel's u64 labels (SPF_FLAG_DIST64).  The bound is
  // on max metric x N, not x (N - 1): the u32 kernels form d(u) + w(u, v) for
  // every edge of a settled u, d(u) <= max metric x (N - 1), before they
  // compare it, and that sum must neither wrap nor reach kInf (a 50-node
  // chain at 87,652,393 per link has d = 2^32 - 39 at its far end, and the
  // relaxation back from there wrapped to a "shorter" distance)
  g.needs64 = g.n_neg > 0 || metric_past_u32(g.max_metric, g.N);
  g.unit = !g.nonpos && g.max_metric <= 1;
}
// the counts gain / lose the live edges of u's row
void add_row_facts(GraphHost& g, uint32_t u) {
  for (uint32_t e = g.row_ptr[u]; e < g.row_ptr[u + 1]; ++e) {
    if (g.col[e] == u) continue;  // dead slot
    g.n_nonpos += g.met[e] <= 0;
    g.n_neg += g.met[e] < 0;
    if (g.wt[e] > g.max_metric) {
      g.max_metric = g.wt[e];
      g.n_at_max = 1;
    } else if (g.wt[e] == g.max_metric) {
      ++g.n_at_max;
    }
  }
}
void remove_row_facts(GraphHost& g, uint32_t u) {
  for (uint32_t e = g.row_ptr[u]; e < g.row_ptr[u + 1]; ++e) {
    if (g.col[e] == u) continue;
    g.n_nonpos -= g.met[e] <= 0;
    g.n_neg -= g.met[e] < 0;
    g.n_at_max -= g.wt[e] == g.max_metric;
  }
}
// from a scan of the graph
void metric_facts(GraphHost& g) {
  g.n_nonpos = g.n_neg = g.n_at_max = 0;
  g.max_metric = 0;
  for (uint32_t u = 0; u < g.N; ++u) add_row_facts(g, u);
  metric_flags(g);
}

// ---- one derivation per table, per node ----
using NbList = std::vector<std::pair<uint32_t, uint32_t>>;  // (neighbour, metric)

// u's distinct up neighbours, ascending id, min metric
void derive_neighbours(const GraphHost& g, uint32_t u, NbList* out) {
  out->clear();
  for (uint32_t e = g.row_ptr[u]; e < g.row_ptr[u + 1]; ++e)
    if (g.col[e] != u) out->emplace_back(g.col[e], g.wt[e]);
  std::sort(out->begin(), out->end());  // first of an id = its min metric
  out->erase(std::unique(out->begin(), out->end(),
                         [](const auto& a, const auto& b) { return a.first == b.first; }),
             out->end());
}

// per edge of u: the head's index among u's distinct neighbours (the route
// selection's next-hop bitmap of that neighbour)
void derive_edge_nb(GraphHost& g, uint32_t u) {
  const auto b = g.nb_id.begin() + g.nb_ptr[u], e = g.nb_id.begin() + g.nb_ptr[u + 1];
  for (uint32_t q = g.row_ptr[u]; q < g.row_ptr[u + 1]; ++q)
    g.edge_nb[q] = g.col[q] == u ? kInf : (uint32_t)(std::lower_bound(b, e, g.col[q]) - b);
}

// v's lane of its slice's sliced-ELL columns (a dead slot: padding, node N),
// and of the packed u16x4 copy: byte offsets into the BFS frontier array (4 B
// per node)
void write_sell_columns(GraphHost& g, uint32_t v) {
  const uint32_t N = g.N, sl = v / kSliceW, ln = v % kSliceW;
  const uint32_t deg = g.row_ptr[v + 1] - g.row_ptr[v];
  for (uint32_t j = 0; j < deg; ++j) {
    const uint32_t x = g.col[g.row_ptr[v] + j];
    g.sell_col[g.sell_ptr[sl] + j * kSliceW + ln] = x == v ? N : x;
  }
  if (g.sell4.empty()) return;
  const uint32_t w = (g.sell_ptr[sl + 1] - g.sell_ptr[sl]) / kSliceW;
  const uint32_t groups = (g.sell4_ptr[sl + 1] - g.sell4_ptr[sl]) / kSliceW;
  for (uint32_t k = 0; k < groups; ++k) {
    uint32_t id[4];
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t j = 4 * k + i;
      id[i] = j < w ? g.sell_col[g.sell_ptr[sl] + j * kSliceW + ln] : N;
    }
    const size_t e = 2ull * (g.sell4_ptr[sl] + k * kSliceW + ln);
    g.sell4[e] = 4 * id[0] | (4 * id[1] << 16);
    g.sell4[e + 1] = 4 * id[2] | (4 * id[3] << 16);
  }
}

// a neighbour set changed: its twin class may split or merge
void neighbour_sets_changed(GraphHost& g) { g.qt.stale = true; }

uint32_t tail_of(const GraphHost& g, uint32_t e) {
  return (uint32_t)(std::upper_bound(g.row_ptr.begin(), g.row_ptr.end(), e) - g.row_ptr.begin()) - 1;
}

// msbfs_kernel's slices per wave: a level's pull sweep costs each wave the
// column groups of its slices and the workgroup waits for the slowest, so
// slices are dealt widest first to the wave with the fewest groups that
// still has a free slot (OWN slots per wave; unused slots = kNoSlice)
void derive_ms_smap(GraphHost& g) {
  g.ms_smap.clear();
  if (g.N > kMsMaxNodes) return;
  const uint32_t n_slices = (uint32_t)g.sell_ptr.size() - 1;
  const uint32_t own = ms_own(g.N), waves = kMsThreads / 64;
  std::vector<uint32_t> order(n_slices), load(waves, 0), used(waves, 0);
  std::iota(order.begin(), order.end(), 0u);
  auto width = [&](uint32_t sl) { return (g.sell_ptr[sl + 1] - g.sell_ptr[sl]) / kSliceW; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return width(a) > width(b); });
  g.ms_smap.assign((size_t)waves * own, kNoSlice);
  for (uint32_t sl : order) {
    uint32_t best = waves;
    for (uint32_t w = 0; w < waves; ++w)
      if (used[w] < own && (best == waves || load[w] < load[best])) best = w;
    g.ms_smap[(size_t)best * own + used[best]++] = sl;
    load[best] += std::max(1u, width(sl));
  }
  if (std::getenv("SPF_SMAP_STRIDED"))  // A/B: slot i of wave w = slice 16 i + w
    for (uint32_t w = 0; w < waves; ++w)
      for (uint32_t i = 0; i < own; ++i) {
        const uint32_t sl = i * waves + w;
        g.ms_smap[(size_t)w * own + i] = sl < n_slices ? sl : kNoSlice;
      }
}

}  // namespace

spf_status graph_host_load(GraphHost* gp, const spf_graph* in, GraphDirty* dirty, std::string* err) {
  GraphHost& g = *gp;
  const uint32_t N = in->n_nodes, E = in->n_edges;
  if (N == 0) return refuse(err, SPF_E_INVALID, "graph has no nodes");
  if (!in->row_ptr || (E && (!in->col || !in->metric || !in->link_id)) || !in->overloaded)
    return refuse(err, SPF_E_INVALID, "graph arrays missing");
  if (in->row_ptr[0] != 0 || in->row_ptr[N] != E)
    return refuse(err, SPF_E_INVALID, "row_ptr must start at 0 and end at n_edges");
  g.loaded = false;
  for (uint32_t u = 0; u < N; ++u)
    if (in->row_ptr[u] > in->row_ptr[u + 1]) return refuse(err, SPF_E_INVALID, "row_ptr not monotone at %u", u);
  for (uint32_t u = 0; u < N; ++u)
    for (uint32_t e = in->row_ptr[u]; e < in->row_ptr[u + 1]; ++e) {
      if (in->col[e] >= N) return refuse(err, SPF_E_INVALID, "edge %u head %u out of range", e, in->col[e]);
      if (in->col[e] == u && in->metric[e] != 1)  // a dead slot (see openr_spf.h): no edge
        return refuse(err, SPF_E_INVALID, "dead slot %u (a self-loop) must carry metric 1", e);
    }
  g.N = N;
  g.E = E;
  // dist rows / bitmap rows: whole 1024-node chunks, so every next-hop
  // bitmap (pitch / 8 bytes) starts on a 128-byte line and no line of the
  // output is written partially by two waves (SPF_PITCH_ALIGN: A/B only)
  {
    const char* e = std::getenv("SPF_PITCH_ALIGN");
    const uint32_t a = e ? (uint32_t)atoi(e) : 1024u;  // a power of two >= 64
    g.pitch = (N + a - 1) & ~(a - 1);
  }
  g.npitch = (N + 1023) & ~1023u;  // narrow rows: whole 1024-node chunks
  g.row_ptr.assign(in->row_ptr, in->row_ptr + N + 1);
  g.col.assign(in->col, in->col + E);
  g.link.assign(in->link_id, in->link_id + E);
  g.ovl.assign(in->overloaded, in->overloaded + N);
  g.met.assign(in->metric, in->metric + E);
  g.wt.resize(E);
  for (uint32_t e = 0; e < E; ++e) g.wt[e] = g.met[e] > 0 ? (uint32_t)g.met[e] : 0u;
  metric_facts(g);
  // reverse edge of every directed edge (same link id, swapped ends)
  g.max_link = 0;
  for (uint32_t e = 0; e < E; ++e) g.max_link = std::max(g.max_link, g.link[e]);
  g.rev.assign(E, kInf);
  g.link_slot.assign(2 * ((size_t)g.max_link + 1), kInf);
  for (uint32_t e = 0; e < E; ++e) {
    uint32_t* ls = &g.link_slot[2 * (size_t)g.link[e]];
    if (ls[0] == kInf) {
      ls[0] = e;
    } else {
      ls[1] = e;
      g.rev[e] = ls[0];
      g.rev[ls[0]] = e;
    }
  }
  for (uint32_t e = 0; e < E; ++e)
    if (g.rev[e] == kInf) return refuse(err, SPF_E_INVALID, "edge %u (link %u) has no reverse edge", e, g.link[e]);
  // distinct up neighbours per node, and each edge's index among them
  g.nb_ptr.assign(N + 1, 0);
  g.nb_id.clear();
  g.nb_w.clear();
  g.big_nodes = 0;
  NbList nb;
  for (uint32_t u = 0; u < N; ++u) {
    if (g.row_ptr[u + 1] - g.row_ptr[u] > kBigDeg) ++g.big_nodes;
    derive_neighbours(g, u, &nb);
    for (const auto& x : nb) {
      g.nb_id.push_back(x.first);
      g.nb_w.push_back(x.second);
    }
    g.nb_ptr[u + 1] = (uint32_t)g.nb_id.size();
  }
  neighbour_sets_changed(g);
  g.edge_nb.assign(std::max<uint32_t>(E, 1), kInf);
  for (uint32_t u = 0; u < N; ++u) derive_edge_nb(g, u);
  // sliced ELL (SELL-64): slice = 64 consecutive nodes, width = max degree in
  // the slice, entry (slice, j, lane) = j-th neighbour of node slice*64+lane,
  // padded with N (F[N] == 0 in the BFS kernel)
  const uint32_t n_slices = (N + kSliceW - 1) / kSliceW;
  g.sell_ptr.assign(n_slices + 1, 0);
  for (uint32_t sl = 0; sl < n_slices; ++sl) {
    uint32_t w = 0;
    for (uint32_t v = sl * kSliceW; v < std::min(N, (sl + 1) * kSliceW); ++v)
      w = std::max(w, g.row_ptr[v + 1] - g.row_ptr[v]);
    g.sell_ptr[sl + 1] = g.sell_ptr[sl] + w * kSliceW;
  }
  // + padding columns (node N): the trailing all-padding group the team
  // kernel's stream pads with, and the BFS kernels' unconditional loads up
  // to three groups of 8 columns past a slice's last column
  g.sell_col.assign(g.sell_ptr[n_slices] + 32 * kSliceW, N);
  // the same columns packed four u16 ids per lane (groups of 4 per slice,
  // at least one), for msbfs_planes_kernel (N <= 10240)
  g.sell4_ptr.assign(n_slices + 1, 0);
  g.sell4.clear();
  if (4ull * N < 65536) {
    for (uint32_t sl = 0; sl < n_slices; ++sl) {
      const uint32_t w = (g.sell_ptr[sl + 1] - g.sell_ptr[sl]) / kSliceW;
      g.sell4_ptr[sl + 1] = g.sell4_ptr[sl] + std::max(1u, (w + 3) / 4) * kSliceW;
    }
    g.sell4.assign(2ull * g.sell4_ptr[n_slices], 4 * N | (4 * N << 16));  // all padding
  }
  for (uint32_t v = 0; v < N; ++v) write_sell_columns(g, v);
  derive_ms_smap(g);
  g.loaded = true;
  ++g.sell_ver;
  ++g.shape;
  ++g.layout;
  *dirty = GraphDirty{};
  dirty->all = true;
  return SPF_OK;
}

spf_status graph_host_set_overload(GraphHost* gp, const uint32_t* nodes, const uint8_t* overloaded,
                                   uint32_t n, GraphDirty* dirty, std::string* err) {
  GraphHost& g = *gp;
  *dirty = GraphDirty{};
  if (!g.loaded) return refuse(err, SPF_E_STATE, "no graph loaded");
  for (uint32_t i = 0; i < n; ++i)
    if (nodes[i] >= g.N) return refuse(err, SPF_E_INVALID, "node %u out of range", nodes[i]);
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t v = overloaded[i] ? 1 : 0;
    dirty->changed |= g.ovl[nodes[i]] != v;
    g.ovl[nodes[i]] = v;
  }
  return SPF_OK;
}

spf_status graph_host_set_metric(GraphHost* gp, const uint32_t* edges, const int32_t* metric, uint32_t n,
                                 GraphDirty* dirty, std::string* err) {
  GraphHost& g = *gp;
  *dirty = GraphDirty{};
  if (!g.loaded) return refuse(err, SPF_E_STATE, "no graph loaded");
  for (uint32_t i = 0; i < n; ++i)
    if (edges[i] >= g.E) return refuse(err, SPF_E_INVALID, "edge %u out of range", edges[i]);
  std::vector<uint32_t> tails;
  for (uint32_t i = 0; i < n; ++i) {
    dirty->changed |= g.met[edges[i]] != metric[i];
    g.met[edges[i]] = metric[i];
    g.wt[edges[i]] = metric[i] > 0 ? (uint32_t)metric[i] : 0u;
    tails.push_back(tail_of(g, edges[i]));
  }
  if (!dirty->changed) return SPF_OK;
  metric_facts(g);
  // min metric per distinct neighbour of every tail touched
  std::sort(tails.begin(), tails.end());
  tails.erase(std::unique(tails.begin(), tails.end()), tails.end());
  NbList nb;
  for (uint32_t u : tails) {
    derive_neighbours(g, u, &nb);
    for (size_t k = 0; k < nb.size(); ++k) g.nb_w[g.nb_ptr[u] + k] = nb[k].second;
  }
  return SPF_OK;
}

// Every check runs on the incoming rows and the untouched ones before the
// first write: a refused patch changes nothing.
spf_status graph_host_patch_rows(GraphHost* gp, const uint32_t* nodes, uint32_t n, const uint32_t* col,
                                 const int32_t* metric, const uint32_t* link, GraphDirty* dirty,
                                 std::string* err) {
  GraphHost& g = *gp;
  *dirty = GraphDirty{};
  if (!g.loaded) return refuse(err, SPF_E_STATE, "no graph loaded");
  const uint32_t N = g.N;
  std::vector<uint8_t> touched(N, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (nodes[i] >= N) return refuse(err, SPF_E_INVALID, "node %u out of range", nodes[i]);
    if (touched[nodes[i]]++) return refuse(err, SPF_E_INVALID, "node %u listed twice", nodes[i]);
  }
  if (!n) return SPF_OK;
  // the links with a slot in a touched row, before or after: (link, slot, its
  // tail, its new head), a link that only leaves with slot kInf
  struct Slot {
    uint32_t link, slot, tail, head;
    bool operator<(const Slot& o) const { return link != o.link ? link < o.link : slot < o.slot; }
  };
  std::vector<Slot> moved;
  {
    size_t o = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t u = nodes[i];
      for (uint32_t e = g.row_ptr[u]; e < g.row_ptr[u + 1]; ++e, ++o) {
        if (col[o] >= N) return refuse(err, SPF_E_INVALID, "row of %u: head %u out of range", u, col[o]);
        if (link[o] > g.max_link)
          return refuse(err, SPF_E_INVALID, "row of %u: link %u is not a link of the loaded graph", u, link[o]);
        if (col[o] == u && metric[o] != 1)
          return refuse(err, SPF_E_INVALID, "row of %u: a dead slot (self-loop) must carry metric 1", u);
        moved.push_back({link[o], e, u, col[o]});
        if (g.link[e] != link[o]) moved.push_back({g.link[e], kInf, u, 0});
      }
    }
  }
  std::sort(moved.begin(), moved.end());
  // link slots and reverse edges: a link's slot in an untouched row keeps its
  // position; its slots in touched rows are where the new rows put them
  struct Pair {
    uint32_t link, a, b;  // its two slots after the patch (kInf, kInf: the link left the graph)
  };
  std::vector<Pair> pairs;
  for (size_t i = 0; i < moved.size();) {
    const uint32_t l = moved[i].link;
    Slot s[2];
    size_t k = 0;
    for (; i < moved.size() && moved[i].link == l; ++i)
      if (moved[i].slot != kInf) {
        if (k < 2) s[k] = moved[i];
        ++k;
      }
    for (int j = 0; j < 2; ++j) {  // its slot in an untouched row, if any, stays
      const uint32_t e = g.link_slot[2 * (size_t)l + j];
      if (e == kInf || g.link[e] != l) continue;
      const uint32_t t = tail_of(g, e);
      if (touched[t]) continue;
      if (k < 2) s[k] = {l, e, t, g.col[e]};
      ++k;
    }
    if (k == 0) {
      pairs.push_back({l, kInf, kInf});
      continue;
    }
    if (k != 2) return refuse(err, SPF_E_INVALID, "link %u has %zu slots after the patch (2 needed)", l, k);
    const bool dead0 = s[0].head == s[0].tail, dead1 = s[1].head == s[1].tail;
    if (dead0 != dead1 || (!dead0 && (s[0].head != s[1].tail || s[1].head != s[0].tail)))
      return refuse(err, SPF_E_INVALID, "link %u: its two slots are not one link in both directions", l);
    pairs.push_back({l, s[0].slot, s[1].slot});
  }

  // ---- the patch is valid: apply it ----
  std::vector<uint32_t>& order = dirty->nodes;
  order.assign(nodes, nodes + n);
  std::sort(order.begin(), order.end());
  std::vector<uint32_t> old_nb(n);
  for (uint32_t i = 0; i < n; ++i) old_nb[i] = g.nb_ptr[nodes[i] + 1] - g.nb_ptr[nodes[i]];
  // rows (the metric-fact counts lose the old rows' live edges and gain the
  // new ones')
  for (uint32_t i = 0; i < n; ++i) remove_row_facts(g, nodes[i]);
  {
    size_t o = 0;
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t e = g.row_ptr[nodes[i]]; e < g.row_ptr[nodes[i] + 1]; ++e, ++o) {
        g.col[e] = col[o];
        g.met[e] = metric[o];
        g.wt[e] = metric[o] > 0 ? (uint32_t)metric[o] : 0u;
        g.link[e] = link[o];
      }
  }
  for (uint32_t i = 0; i < n; ++i) add_row_facts(g, nodes[i]);
  // graph-wide metric facts over live edges: from the counts, unless every
  // edge at the old maximum left (then the maximum fell: one scan)
  if (g.n_at_max == 0) metric_facts(g);
  else metric_flags(g);
  std::vector<uint32_t> rev_dirty;  // reverse-edge entries whose value changed
  auto set_rev = [&](uint32_t e, uint32_t r) {
    if (g.rev[e] != r) {
      g.rev[e] = r;
      rev_dirty.push_back(e);
    }
  };
  for (const Pair& p : pairs) {
    g.link_slot[2 * (size_t)p.link] = p.a;
    g.link_slot[2 * (size_t)p.link + 1] = p.b;
    if (p.a == kInf) continue;
    set_rev(p.a, p.b);
    set_rev(p.b, p.a);
  }
  // distinct up neighbours of the touched nodes; the lists are rebuilt (every
  // untouched node's range copied) when a count changes
  std::vector<NbList> fresh(n);
  bool sets = false;
  for (uint32_t i = 0; i < n; ++i) {
    derive_neighbours(g, nodes[i], &fresh[i]);
    dirty->counts |= fresh[i].size() != old_nb[i];
  }
  if (dirty->counts) {
    // the untouched nodes' lists move as whole blocks between touched nodes
    std::vector<uint32_t> by_node(n);
    std::iota(by_node.begin(), by_node.end(), 0u);
    std::sort(by_node.begin(), by_node.end(), [&](uint32_t a, uint32_t b) { return nodes[a] < nodes[b]; });
    std::vector<uint32_t> ptr(N + 1, 0), id, w;
    id.reserve(g.nb_id.size() + 16);
    w.reserve(g.nb_id.size() + 16);
    uint32_t next = 0;  // first node not yet placed
    auto block = [&](uint32_t to) {  // untouched nodes next .. to - 1
      const uint32_t b = g.nb_ptr[next], e = g.nb_ptr[to];
      const int64_t shift = (int64_t)id.size() - (int64_t)b;
      id.insert(id.end(), g.nb_id.begin() + b, g.nb_id.begin() + e);
      w.insert(w.end(), g.nb_w.begin() + b, g.nb_w.begin() + e);
      for (uint32_t u = next; u < to; ++u) ptr[u + 1] = (uint32_t)((int64_t)g.nb_ptr[u + 1] + shift);
    };
    for (uint32_t oi : by_node) {
      const uint32_t u = nodes[oi];
      block(u);
      for (const auto& x : fresh[oi]) {
        id.push_back(x.first);
        w.push_back(x.second);
      }
      ptr[u + 1] = (uint32_t)id.size();
      next = u + 1;
    }
    block(N);
    g.nb_ptr.swap(ptr);
    g.nb_id.swap(id);
    g.nb_w.swap(w);
    ++g.layout;
    sets = true;
  } else {
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t b = g.nb_ptr[nodes[i]];
      for (size_t k = 0; k < fresh[i].size(); ++k) {
        sets |= g.nb_id[b + k] != fresh[i][k].first;
        g.nb_id[b + k] = fresh[i][k].first;
        g.nb_w[b + k] = fresh[i][k].second;
      }
    }
  }
  if (sets) neighbour_sets_changed(g);
  for (uint32_t i = 0; i < n; ++i) {
    derive_edge_nb(g, nodes[i]);
    write_sell_columns(g, nodes[i]);
  }
  ++g.sell_ver;  // (msbfs_team_prepare's cached tables read sell_col)
  // what changed: the touched rows (merged when adjacent), the partner slots
  // their reverse edges point at, and the touched slices
  auto& runs = dirty->runs;
  for (uint32_t u : order) {
    if (dirty->slices.empty() || dirty->slices.back() != u / kSliceW) dirty->slices.push_back(u / kSliceW);
    const uint32_t b = g.row_ptr[u], e = g.row_ptr[u + 1];
    if (b == e) continue;
    if (!runs.empty() && runs.back().second == b)
      runs.back().second = e;
    else
      runs.emplace_back(b, e);
  }
  std::sort(rev_dirty.begin(), rev_dirty.end());
  auto in_runs = [&](uint32_t q) {
    auto it = std::upper_bound(runs.begin(), runs.end(), std::make_pair(q, ~0u));
    return it != runs.begin() && q < std::prev(it)->second;
  };
  for (uint32_t q : rev_dirty) {
    if (in_runs(q)) continue;
    auto& rr = dirty->rev_runs;
    if (!rr.empty() && rr.back().first + rr.back().second == q)
      ++rr.back().second;
    else
      rr.emplace_back(q, 1u);
  }
  return SPF_OK;
}

// Lists are hashed, then compared within a hash bucket.
uint32_t twin_classes(uint32_t N, const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t* cls) {
  std::vector<uint64_t> h(N);
  for (uint32_t v = 0; v < N; ++v) {
    uint64_t x = 0x9E3779B97F4A7C15ull ^ (nb_ptr[v + 1] - nb_ptr[v]);
    for (uint32_t e = nb_ptr[v]; e < nb_ptr[v + 1]; ++e) {
      x ^= nb_id[e] + 0x9E3779B97F4A7C15ull + (x << 6) + (x >> 2);
      x *= 0xFF51AFD7ED558CCDull;
    }
    h[v] = x;
  }
  std::vector<uint32_t> order(N), rep(N);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(),
            [&](uint32_t a, uint32_t b) { return h[a] != h[b] ? h[a] < h[b] : a < b; });
  auto same = [&](uint32_t a, uint32_t b) {
    const uint32_t k = nb_ptr[a + 1] - nb_ptr[a];
    return k == nb_ptr[b + 1] - nb_ptr[b] &&
           std::equal(nb_id + nb_ptr[a], nb_id + nb_ptr[a] + k, nb_id + nb_ptr[b]);
  };
  std::vector<uint32_t> reps;  // first members of the classes in one hash bucket
  for (size_t i = 0; i < N;) {
    size_t j = i;
    reps.clear();
    for (; j < N && h[order[j]] == h[order[i]]; ++j) {
      const uint32_t v = order[j];
      rep[v] = v;
      for (uint32_t r : reps)
        if (same(r, v)) {
          rep[v] = r;
          break;
        }
      if (rep[v] == v) reps.push_back(v);
    }
    i = j;
  }
  uint32_t n_cls = 0;
  for (uint32_t v = 0; v < N; ++v) cls[v] = rep[v] == v ? n_cls++ : cls[rep[v]];  // rep[v] <= v
  return n_cls;
}

// A node's neighbours are whole classes (links are up in both directions or
// neither), so the quotient row of a class is the set of classes of its first
// member's neighbours; rows are cut into chunks of kQChunk columns padded with
// n_cls.
bool graph_host_quotient(GraphHost* gp) {
  GraphHost& g = *gp;
  GraphHost::Quotient& q = g.qt;
  if (!q.stale) return false;
  const uint32_t N = g.N;
  q.n_cls = q.n_vrow = 0;
  q.n_edge = 0;
  q.stale = false;
  if (N > kMsMaxNodes) return false;  // (msbfs_kernel does not run on such graphs)
  std::vector<uint32_t> cls(N);
  q.n_cls = twin_classes(N, g.nb_ptr.data(), g.nb_id.data(), cls.data());
  q.cls.assign(cls.begin(), cls.end());
  std::vector<uint32_t> row_of, cols, qn;  // per chunk: its row; kQChunk columns
  std::vector<uint8_t> seen(N, 0);         // (first members only)
  for (uint32_t v = 0; v < N; ++v) {
    if (seen[cls[v]]) continue;
    seen[cls[v]] = 1;
    qn.clear();
    for (uint32_t e = g.nb_ptr[v]; e < g.nb_ptr[v + 1]; ++e) qn.push_back(cls[g.nb_id[e]]);
    std::sort(qn.begin(), qn.end());
    qn.erase(std::unique(qn.begin(), qn.end()), qn.end());
    q.n_edge += qn.size();
    for (size_t b = 0; b < qn.size(); b += kQChunk) {
      row_of.push_back(cls[v]);
      for (size_t j = 0; j < kQChunk; ++j) cols.push_back(b + j < qn.size() ? qn[b + j] : q.n_cls);
    }
  }
  q.n_vrow = (uint32_t)row_of.size();
  const size_t nvp = (q.n_vrow + 7u) & ~7u;
  q.tab.assign((1 + kQChunk) * nvp, (uint16_t)q.n_cls);
  for (uint32_t r = 0; r < q.n_vrow; ++r) {
    q.tab[r] = (uint16_t)row_of[r];
    for (uint32_t j = 0; j < kQChunk; ++j) q.tab[nvp + j * nvp + r] = (uint16_t)cols[(size_t)r * kQChunk + j];
  }
  for (size_t r = q.n_vrow; r < nvp; ++r) q.tab[r] = 0;  // (chunks past n_vrow are not read)
  return true;
}

}  // namespace spfi
