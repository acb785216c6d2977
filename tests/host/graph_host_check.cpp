// The graph's host state (openr_amd/csrc/graph_host.h) on the CPU, no device:
//  * after every row patch each derived table equals a fresh load of the
//    same CSR;
//  * a refused patch leaves the struct as it was, field for field.
// Built with the sanitizers and run by tests/test_graph_host.py; exit status
// 0 = every check held.
#include "graph_host.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

using namespace spfi;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                  \
    }                                                              \
  } while (0)

// A graph as links; every node's row holds its links' slots in `slots` order,
// a down link's slot dead (a self-loop of metric 1).
struct Link {
  uint32_t id, a, b;
  int32_t m_ab, m_ba;
  bool up;
};
struct Model {
  uint32_t N = 0;
  std::vector<Link> links;
  std::vector<std::vector<uint32_t>> slots;  // per node: indices into links
  uint32_t add(uint32_t id, uint32_t a, uint32_t b, int32_t m_ab, int32_t m_ba) {
    links.push_back({id, a, b, m_ab, m_ba, true});
    slots[a].push_back((uint32_t)links.size() - 1);
    slots[b].push_back((uint32_t)links.size() - 1);
    return (uint32_t)links.size() - 1;
  }
};
struct Rows {  // rows back to back
  std::vector<uint32_t> ptr, col, link;
  std::vector<int32_t> met;
};
void append_row(const Model& m, uint32_t u, Rows* r) {
  for (uint32_t li : m.slots[u]) {
    const Link& l = m.links[li];
    r->col.push_back(l.up ? (l.a == u ? l.b : l.a) : u);
    r->met.push_back(l.up ? (l.a == u ? l.m_ab : l.m_ba) : 1);
    r->link.push_back(l.id);
  }
}

spf_status load(const Model& m, GraphHost* g, std::string* err) {
  Rows r;
  r.ptr.push_back(0);
  for (uint32_t u = 0; u < m.N; ++u) {
    append_row(m, u, &r);
    r.ptr.push_back((uint32_t)r.col.size());
  }
  const std::vector<uint8_t> ovl(m.N, 0);
  spf_graph in;
  in.n_nodes = m.N;
  in.n_edges = (uint32_t)r.col.size();
  in.row_ptr = r.ptr.data();
  in.col = r.col.data();
  in.metric = r.met.data();
  in.link_id = r.link.data();
  in.overloaded = ovl.data();
  GraphDirty d;
  const spf_status st = graph_host_load(g, &in, &d, err);
  if (st == SPF_OK) CHECK(d.all);
  return st;
}

spf_status patch(const Model& m, const std::vector<uint32_t>& nodes, GraphHost* g, GraphDirty* d,
                 std::string* err) {
  Rows r;
  for (uint32_t u : nodes) append_row(m, u, &r);
  return graph_host_patch_rows(g, nodes.data(), (uint32_t)nodes.size(), r.col.data(), r.met.data(),
                               r.link.data(), d, err);
}

std::vector<std::pair<uint32_t, uint32_t>> slot_pairs(const GraphHost& g) {
  std::vector<std::pair<uint32_t, uint32_t>> p;
  for (size_t l = 0; l + 1 < g.link_slot.size(); l += 2)
    p.emplace_back(std::min(g.link_slot[l], g.link_slot[l + 1]), std::max(g.link_slot[l], g.link_slot[l + 1]));
  return p;
}

#define SAME(f) CHECK(a.f == b.f)
// the graph and every table derived from it (not the version counters)
void same_tables(const GraphHost& a, const GraphHost& b) {
  SAME(loaded); SAME(N); SAME(E); SAME(pitch); SAME(npitch);
  SAME(row_ptr); SAME(col); SAME(met); SAME(wt); SAME(link); SAME(rev); SAME(ovl);
  SAME(nb_ptr); SAME(nb_id); SAME(nb_w); SAME(edge_nb);
  SAME(sell_ptr); SAME(sell_col); SAME(sell4_ptr); SAME(sell4); SAME(ms_smap);
  SAME(n_nonpos); SAME(n_neg); SAME(n_at_max);
  SAME(nonpos); SAME(needs64); SAME(unit); SAME(max_metric); SAME(max_link); SAME(big_nodes);
  CHECK(slot_pairs(a) == slot_pairs(b));
}
void same_quotient(const GraphHost& a, const GraphHost& b) {
  SAME(qt.stale); SAME(qt.n_cls); SAME(qt.n_vrow); SAME(qt.n_edge); SAME(qt.cls); SAME(qt.tab);
}
// field for field, counters included
void same_struct(const GraphHost& a, const GraphHost& b) {
  same_tables(a, b);
  same_quotient(a, b);
  SAME(link_slot); SAME(shape); SAME(epoch); SAME(layout); SAME(sell_ver);
}
#undef SAME

// One accepted patch: the touched rows go in, the tables equal a reload's, the
// layout moved iff a neighbour count changed, the quotient went stale iff a
// neighbour set changed (and rebuilds to the reload's).
void step(const char* what, const Model& m, std::vector<uint32_t> nodes, GraphHost* g, bool counts,
          bool sets) {
  std::printf("  %s\n", what);
  graph_host_quotient(g);
  CHECK(!g->qt.stale);
  const uint64_t layout = g->layout, sell_ver = g->sell_ver, epoch = g->epoch;
  GraphDirty d;
  std::string err;
  const spf_status st = patch(m, nodes, g, &d, &err);
  if (st != SPF_OK) std::printf("    refused: %s\n", err.c_str());
  CHECK(st == SPF_OK);
  CHECK(g->layout == layout + (counts ? 1 : 0));
  CHECK(g->sell_ver == sell_ver + 1);
  CHECK(g->epoch == epoch);  // the caller's, once the device copy followed
  CHECK(g->qt.stale == sets);
  CHECK(d.counts == counts && !d.all);
  std::sort(nodes.begin(), nodes.end());
  CHECK(d.nodes == nodes);
  for (const auto& r : d.rev_runs)  // outside the touched rows' runs
    for (const auto& run : d.runs) CHECK(r.first + r.second <= run.first || r.first >= run.second);
  GraphHost fresh;
  CHECK(load(m, &fresh, &err) == SPF_OK);
  same_tables(*g, fresh);
  graph_host_quotient(g);
  graph_host_quotient(&fresh);
  same_quotient(*g, fresh);
}

void swap_slots(Model* m, uint32_t u, size_t i, size_t j) { std::swap(m->slots[u][i], m->slots[u][j]); }

// 130-node ring with chords and two parallel links; link id 130 is unused.
// Nodes 63 | 64 straddle a slice boundary, 129 sits in the last, partial slice.
struct Ring {
  Model m;
  uint32_t chord_64_101, chord_5_70, par_63_64, par_129_0, ring_129_0;
  Ring() {
    m.N = 130;
    m.slots.resize(m.N);
    for (uint32_t i = 0; i < 130; ++i) m.add(i, i, (i + 1) % 130, 1 + (int32_t)(i % 3), 1 + (int32_t)(i % 5));
    ring_129_0 = 129;
    chord_64_101 = m.add(131, 64, 101, 4, 6);
    chord_5_70 = m.add(132, 5, 70, 1000, 1000);  // the only links at the maximum metric
    m.add(133, 129, 30, 2, 2);
    m.add(134, 63, 20, 3, 1);
    par_63_64 = m.add(135, 63, 64, 5, 2);
    par_129_0 = m.add(136, 129, 0, 1, 1);
  }
};

void ring_patches() {
  std::printf("ring130\n");
  Ring r;
  Model& m = r.m;
  GraphHost g;
  std::string err;
  CHECK(load(m, &g, &err) == SPF_OK);
  CHECK(!g.sell4.empty() && g.sell_ptr.size() == 4);
  m.links[r.chord_64_101].up = false;
  step("a link down (both slots dead): a neighbour count changes", m, {64, 101}, &g, true, true);
  m.links[r.chord_64_101].up = true;
  step("the link up again", m, {101, 64}, &g, true, true);
  m.links[r.par_63_64].m_ab = 1;
  m.links[r.par_63_64].m_ba = 9;
  step("a parallel link's metric changes", m, {63, 64}, &g, false, false);
  swap_slots(&m, 129, 0, 3);
  {
    const std::vector<uint32_t> rev = g.rev;
    step("a link moved to another slot of its row", m, {129}, &g, false, false);
    CHECK(rev != g.rev);  // the partners in untouched rows follow
  }
  m.links[r.par_129_0].up = false;
  step("one of two parallel links down: the neighbour stays", m, {129, 0}, &g, false, false);
  m.links[r.ring_129_0].up = false;
  step("the other one down", m, {0, 129}, &g, true, true);
  m.links[r.chord_5_70].up = false;
  step("the only link at the maximum metric down: the maximum falls", m, {5, 70}, &g, true, true);
  CHECK(g.max_metric == 9);
  m.links[r.chord_5_70].up = true;
  m.links[r.ring_129_0].up = true;
  m.links[r.par_129_0].up = true;
  step("three links up in one patch", m, {129, 70, 5, 0}, &g, true, true);
}

void ring_refusals() {
  std::printf("ring130 refusals\n");
  Ring r;
  const Model& m = r.m;
  GraphHost g;
  std::string err;
  CHECK(load(m, &g, &err) == SPF_OK);
  graph_host_quotient(&g);
  const GraphHost before = g;
  // node 64's row: ring 63-64, ring 64-65, the chord to 101, the parallel 63-64
  Rows row;
  append_row(m, 64, &row);
  CHECK(row.col.size() == 4 && row.col[2] == 101);
  const uint32_t node = 64;
  auto refused = [&](const char* what, Rows t) {
    std::printf("  %s\n", what);
    GraphDirty d;
    err.clear();
    CHECK(graph_host_patch_rows(&g, &node, 1, t.col.data(), t.met.data(), t.link.data(), &d, &err) ==
          SPF_E_INVALID);
    CHECK(!err.empty());
    std::printf("    -> %s\n", err.c_str());
    same_struct(g, before);
  };
  Rows t = row;
  t.col[2] = g.N;
  refused("a head out of range", t);
  t = row;
  t.link[2] = g.max_link + 1;
  refused("a link id above max_link", t);
  t = row;
  t.col[2] = node;
  t.met[2] = 2;
  refused("a dead slot with metric 2", t);
  t = row;
  t.col[2] = node;
  t.met[2] = 1;
  refused("one slot of a link dead, the other live", t);
  t = row;
  t.link[2] = t.link[1];
  refused("a link left with three slots", t);
  t = row;
  t.link[2] = 130;
  refused("a link left with one slot", t);
  Model down = m;
  down.links[r.chord_64_101].up = false;
  step("a valid patch afterwards", down, {64, 101}, &g, true, true);
}

// ssw_per_plane = 2, fsw_per_pod = 2, rsw_per_pod = 3, three pods: 19 nodes.
// Twin classes: the spines of a plane, the rack switches of a pod, every
// fabric switch alone.
void fabric_patches() {
  std::printf("fabric19\n");
  Model m;
  m.N = 19;
  m.slots.resize(m.N);
  uint32_t id = 0;
  for (uint32_t pod = 0; pod < 3; ++pod)
    for (uint32_t j = 0; j < 2; ++j) {
      const uint32_t fsw = 4 + 5 * pod + j;
      for (uint32_t i = 0; i < 2; ++i) m.add(id++, fsw, 2 * j + i, 1, 1);
      for (uint32_t k = 0; k < 3; ++k) m.add(id++, fsw, 4 + 5 * pod + 2 + k, 1, 1);
    }
  GraphHost g;
  std::string err;
  CHECK(load(m, &g, &err) == SPF_OK);
  CHECK(g.unit);
  graph_host_quotient(&g);
  CHECK(g.qt.n_cls == 2 + 3 * 2 + 3);
  const uint32_t fsw = 4, rsw = 6;
  const uint32_t l = m.slots[rsw][0];
  CHECK(m.links[l].a == fsw && m.links[l].b == rsw);
  m.links[l].up = false;
  step("a rack switch loses a fabric switch: its class splits", m, {fsw, rsw}, &g, true, true);
  CHECK(g.qt.n_cls == 12);
  m.links[l].up = true;
  step("and joins it again", m, {rsw, fsw}, &g, true, true);
  CHECK(g.qt.n_cls == 11);
  m.links[l].m_ab = 3;
  step("a metric ends unit metrics", m, {fsw}, &g, false, false);
  CHECK(!g.unit && g.max_metric == 3);
  swap_slots(&m, fsw, 1, 4);
  step("a link moved to another slot of its row", m, {fsw}, &g, false, false);
}

// 16,384 nodes: the largest msbfs_kernel graph, too large for the packed
// u16x4 columns (4 N >= 65536).
void chain_patches() {
  std::printf("chain16384\n");
  Model m;
  m.N = 16384;
  m.slots.resize(m.N);
  for (uint32_t i = 0; i + 1 < m.N; ++i) m.add(i, i, i + 1, 1, 1);
  GraphHost g;
  std::string err;
  CHECK(load(m, &g, &err) == SPF_OK);
  CHECK(g.sell4.empty() && !g.ms_smap.empty());
  m.links[8191].up = false;
  step("a link down", m, {8191, 8192}, &g, true, true);
  m.links[8191].up = true;
  step("up again", m, {8192, 8191}, &g, true, true);
  swap_slots(&m, 100, 0, 1);
  step("a link moved to another slot of its row", m, {100}, &g, false, false);
  m.links[16382].m_ba = 7;
  step("the last node's metric", m, {16383}, &g, false, false);
}

}  // namespace

int main() {
  ring_patches();
  ring_refusals();
  fabric_patches();
  chain_patches();
  if (g_failed) std::printf("%d checks failed\n", g_failed);
  else std::printf("ok\n");
  return g_failed ? 1 : 0;
}
