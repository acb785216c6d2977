// The prefix table of spf_mplan_prefix_routes on the CPU
// (openr_amd/csrc/prefix_table_host.h), no device:
//  * prefix_table_build's refusals (SPF_E_INVALID, the prefix named): a
//    pfx_ptr that decreases or does not start at 0, a node id >= n_nodes, the
//    same node twice in one prefix, distance == INT32_MIN; what it accepts: no
//    prefixes, an empty prefix, the same node in two prefixes;
//  * the ranks and the saturation of min_nexthop;
//  * prefix_select on cases written by hand: the floor (distance 5 with zero
//    preferences never enters, distance 0 does), a preference tie broken by
//    distance, all drained / some drained / me drained among undrained peers,
//    unreachable advertisers, min_nexthop taken from B only, and all_best.
// Built with the sanitizers and run by tests/test_prefix_table_host.py; exit
// status 0 = every check held.
#include "prefix_table_host.h"

#include <climits>
#include <cstdio>
#include <cstring>

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

struct Ent {
  uint32_t node;
  int32_t pp, sp, dist;
  int64_t min_nh;
};

struct Input {
  std::vector<uint32_t> ptr{0}, node;
  std::vector<int32_t> pp, sp, dist;
  std::vector<int64_t> mn;
  void prefix(const std::vector<Ent>& es) {
    for (const Ent& e : es) {
      node.push_back(e.node);
      pp.push_back(e.pp);
      sp.push_back(e.sp);
      dist.push_back(e.dist);
      mn.push_back(e.min_nh);
    }
    ptr.push_back((uint32_t)node.size());
  }
  spf_status build(const std::vector<uint8_t>& ovl, bool all_best, PrefixTable* t, std::string* err) const {
    return prefix_table_build(ptr.data(), node.data(), pp.data(), sp.data(), dist.data(), mn.data(),
                              (uint32_t)ptr.size() - 1, ovl.data(), (uint32_t)ovl.size(), all_best, t, err);
  }
};

constexpr uint32_t INF = SPF_UNREACHABLE;
using V = std::vector<uint32_t>;

void refusals() {
  const std::vector<uint8_t> ovl(4, 0);
  PrefixTable t;
  std::string err;
  {  // pfx_ptr decreases at prefix 1
    Input in;
    in.prefix({{0, 0, 0, 0, 0}, {1, 0, 0, 0, 0}});
    in.prefix({{2, 0, 0, 0, 0}});
    in.ptr = {0, 2, 1, 3};
    CHECK(in.build(ovl, false, &t, &err) == SPF_E_INVALID);
    CHECK(err.find("prefix 1") != std::string::npos);
  }
  {  // ... does not start at 0
    Input in;
    in.prefix({{0, 0, 0, 0, 0}});
    in.ptr = {1, 1};
    CHECK(in.build(ovl, false, &t, &err) == SPF_E_INVALID);
    CHECK(err.find("prefix 0") != std::string::npos);
  }
  {  // a node id out of range, in prefix 2
    Input in;
    in.prefix({{0, 0, 0, 0, 0}});
    in.prefix({});
    in.prefix({{3, 0, 0, 0, 0}, {4, 0, 0, 0, 0}});
    CHECK(in.build(ovl, false, &t, &err) == SPF_E_INVALID);
    CHECK(err.find("prefix 2") != std::string::npos && err.find("node 4") != std::string::npos);
  }
  {  // the same node twice in prefix 1 (twice over two prefixes is fine)
    Input in;
    in.prefix({{1, 0, 0, 0, 0}});
    in.prefix({{1, 0, 0, 0, 0}, {2, 0, 0, 0, 0}, {1, 1, 0, 0, 0}});
    CHECK(in.build(ovl, false, &t, &err) == SPF_E_INVALID);
    CHECK(err.find("prefix 1") != std::string::npos && err.find("twice") != std::string::npos);
    in = Input();
    in.prefix({{1, 0, 0, 0, 0}});
    in.prefix({{1, 0, 0, 0, 0}, {2, 0, 0, 0, 0}});
    CHECK(in.build(ovl, false, &t, &err) == SPF_OK);
  }
  for (const bool all_best : {false, true}) {  // distance INT32_MIN, under the floor or not
    Input in;
    in.prefix({{0, 5, 0, INT32_MIN, 0}});
    CHECK(in.build(ovl, all_best, &t, &err) == SPF_E_INVALID);
    CHECK(err.find("prefix 0") != std::string::npos && err.find("INT32_MIN") != std::string::npos);
  }
  {  // no prefixes; NULL arrays
    CHECK(prefix_table_build(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, ovl.data(), 4, false,
                             &t, &err) == SPF_OK);
    CHECK(t.n_pfx == 0 && t.ptr == V{0} && t.ent.empty());
    const uint32_t ptr[3] = {0, 0, 0};  // two empty prefixes
    CHECK(prefix_table_build(ptr, nullptr, nullptr, nullptr, nullptr, nullptr, 2, ovl.data(), 4, false, &t,
                             &err) == SPF_OK);
    CHECK(t.n_pfx == 2 && t.ptr == (V{0, 0, 0}));
    const uint32_t dist[4] = {0, 0, 0, 0};
    const PrefixChoice c = prefix_select(t, 1, 0, dist, false);
    CHECK(c.status == SPF_PREFIX_NONE && c.best == INF && c.B.empty());
  }
}

void ranks() {
  const std::vector<uint8_t> ovl{0, 1, 0, 0, 0, 0};
  Input in;
  // tuples: (1,0,-3) (1,0,-1) (0,7,0) (1,0,-1) (0,0,-5: under the floor) (-1,9,0: under it)
  in.prefix({{0, 1, 0, 3, -4}, {1, 1, 0, 1, 0}, {2, 0, 7, 0, 2}, {3, 1, 0, 1, (int64_t)1 << 40},
             {4, 0, 0, 5, 1}, {5, -1, 9, 0, 1}});
  in.prefix({{4, 0, 0, 0, 9}, {5, 0, 0, -2, INT64_MIN}});  // (0,0,0) and (0,0,2)
  PrefixTable t;
  std::string err;
  CHECK(in.build(ovl, false, &t, &err) == SPF_OK);
  CHECK(t.ptr == (V{0, 4, 6}));
  if (t.ent.size() == 6) {
    const uint32_t node[6] = {0, 1, 2, 3, 4, 5}, rank[6] = {1, 2, 0, 2, 0, 1};
    const uint32_t need[6] = {0, 0, 2, UINT32_MAX, 9, 0}, dr[6] = {0, 1, 0, 0, 0, 0};
    for (int i = 0; i < 6; ++i)
      CHECK(t.ent[i].node == node[i] && t.ent[i].rank == rank[i] && t.ent[i].min_nh == need[i] &&
            t.ent[i].drained == dr[i]);
  } else {
    CHECK(t.ent.size() == 6);
  }
  // all_best keeps the entries under the floor, every rank 0
  CHECK(in.build(ovl, true, &t, &err) == SPF_OK);
  CHECK(t.ptr == (V{0, 6, 8}));
  for (const PrefixEnt& e : t.ent) CHECK(e.rank == 0);
}

void selection() {
  // nodes 0..7; 6 and 7 are drained
  const std::vector<uint8_t> ovl{0, 0, 0, 0, 0, 0, 1, 1};
  Input in;
  in.prefix({{1, 0, 0, 5, 0}, {2, 0, 0, 0, 0}});                  // 0 the floor: 1 never enters
  in.prefix({{1, 0, 0, 5, 0}});                                    // 1 ... alone: no route
  in.prefix({{1, 2, 1, 4, 0}, {2, 2, 1, 3, 0}, {3, 2, 0, 0, 0}});  // 2 a tie on preferences: distance
  in.prefix({{6, 0, 0, 0, 0}, {7, 0, 0, 0, 0}});                  // 3 all drained
  in.prefix({{6, 0, 0, 0, 0}, {3, 0, 0, 0, 0}, {7, 0, 0, 0, 0}});  // 4 some drained
  in.prefix({{3, 0, 0, 0, 1}, {6, 0, 0, 0, 3}, {4, 1, 0, 0, 7}});  // 5 min_nexthop: B only
  in.prefix({{5, 3, 0, 0, 0}, {2, 1, 0, 0, 0}});                  // 6 the best one unreachable
  PrefixTable t;
  std::string err;
  CHECK(in.build(ovl, false, &t, &err) == SPF_OK);
  uint32_t d[8] = {0, 3, 1, 2, INF, INF, 1, 4};  // me = 0: nodes 4 and 5 out of reach
  PrefixChoice c = prefix_select(t, 0, 0, d, false);
  CHECK(c.B == V{2} && c.best == 2 && c.status == SPF_PREFIX_ROUTE && c.need == 0);
  c = prefix_select(t, 1, 0, d, false);
  CHECK(c.B.empty() && c.best == INF && c.status == SPF_PREFIX_NONE);
  c = prefix_select(t, 2, 0, d, false);
  CHECK(c.B == V{2} && c.best == 2 && c.status == SPF_PREFIX_ROUTE);
  c = prefix_select(t, 3, 0, d, false);  // all drained: kept
  CHECK(c.B == (V{6, 7}) && c.best == 6 && c.status == SPF_PREFIX_ROUTE);
  c = prefix_select(t, 4, 0, d, false);  // some drained: the best node stays the smallest of B0
  CHECK(c.B == V{3} && c.best == 3 && c.status == SPF_PREFIX_ROUTE);
  c = prefix_select(t, 5, 0, d, false);  // 4 (the best tuple) unreachable; 6 drained: its 3 does not count
  CHECK(c.B == V{3} && c.best == 3 && c.need == 1);
  c = prefix_select(t, 6, 0, d, false);
  CHECK(c.B == V{2} && c.best == 2);
  d[4] = 9;  // 4 reachable: it alone is best, its min_nexthop counts
  c = prefix_select(t, 5, 0, d, false);
  CHECK(c.B == V{4} && c.best == 4 && c.need == 7);
  // me among the advertisers
  uint32_t d6[8] = {1, 4, 2, 3, INF, INF, 0, 5};  // me = 6 (drained)
  c = prefix_select(t, 3, 6, d6, false);  // all drained, me among them: SELF
  CHECK(c.B == (V{6, 7}) && c.best == 6 && c.status == SPF_PREFIX_SELF);
  c = prefix_select(t, 4, 6, d6, false);  // me drained beside an undrained peer: a route to it, best = me
  CHECK(c.B == V{3} && c.best == 6 && c.status == SPF_PREFIX_ROUTE);
  c = prefix_select(t, 4, 6, d6, true);  // (the same table read with all_best: the smallest id)
  CHECK(c.B == V{3} && c.best == 3 && c.status == SPF_PREFIX_ROUTE);
  uint32_t d7[8] = {4, 1, 2, 3, INF, INF, 5, INF};  // me = 7, its own row entry not even 0
  c = prefix_select(t, 4, 7, d7, false);
  CHECK(c.B == V{3} && c.best == 7 && c.status == SPF_PREFIX_ROUTE);
  uint32_t d3[8] = {2, 5, 3, 0, INF, INF, 3, 6};  // me = 3 (undrained)
  c = prefix_select(t, 4, 3, d3, false);
  CHECK(c.B == V{3} && c.best == 3 && c.status == SPF_PREFIX_SELF);
  c = prefix_select(t, 2, 3, d3, false);  // me advertises, under the best tuple: a route to 2
  CHECK(c.B == V{2} && c.best == 2 && c.status == SPF_PREFIX_ROUTE);
  // all_best: every reachable entry, the floor included
  CHECK(in.build(ovl, true, &t, &err) == SPF_OK);
  c = prefix_select(t, 0, 0, d, true);
  CHECK(c.B == (V{1, 2}) && c.best == 1 && c.status == SPF_PREFIX_ROUTE);
  c = prefix_select(t, 2, 3, d3, true);  // me among them: SELF, best the smallest id
  CHECK(c.B == (V{1, 2, 3}) && c.best == 1 && c.status == SPF_PREFIX_SELF);
  c = prefix_select(t, 5, 0, d, true);  // 3, 4 (d[4] = 9), 6 drained: min_nexthop from 3 and 4
  CHECK(c.B == (V{3, 4}) && c.best == 3 && c.need == 7);
}

}  // namespace

int main() {
  refusals();
  ranks();
  selection();
  if (g_failed) std::printf("%d checks failed\n", g_failed);
  return g_failed ? 1 : 0;
}
