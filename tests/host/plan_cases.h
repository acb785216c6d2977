// The graphs, requests and knob values of tests/host/plan_host_check.cpp, each
// with the digest of the tables build_plan uploaded for it before its
// derivations moved to plan_host.cpp (commit cb07bca: the same graphs loaded
// through spf_graph_load on an MI355X, the knobs set through SPF_NARROW,
// SPF_ECMP_RUNS, SPF_SLICED_UNIT and SPF_SLICED_GROUP with SPF_MSBFS=masks,
// the digest printed where the tables were uploaded).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace plan_cases {

// Unit-metric graph as links; a node's row holds its links in the order given.
struct Graph {
  uint32_t N = 0;
  std::vector<uint32_t> row_ptr, col, link;
  std::vector<int32_t> met;
  std::vector<uint8_t> ovl;
};

inline Graph from_links(uint32_t N, const std::vector<std::pair<uint32_t, uint32_t>>& links,
                        const std::vector<uint32_t>& drained = {}) {
  Graph g;
  g.N = N;
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> rows(N);  // (head, link id)
  for (uint32_t l = 0; l < links.size(); ++l) {
    rows[links[l].first].emplace_back(links[l].second, l);
    rows[links[l].second].emplace_back(links[l].first, l);
  }
  g.row_ptr.push_back(0);
  for (uint32_t u = 0; u < N; ++u) {
    for (const auto& e : rows[u]) {
      g.col.push_back(e.first);
      g.link.push_back(e.second);
      g.met.push_back(1);
    }
    g.row_ptr.push_back((uint32_t)g.col.size());
  }
  g.ovl.assign(N, 0);
  for (uint32_t d : drained) g.ovl[d] = 1;
  return g;
}

// Two pods under four planes of four spines: spines 0 .. 15 (plane j: 4j ..
// 4j + 3), then per pod its four fabric switches (one per plane) and twenty
// rack switches: 64 nodes.  A fabric switch's neighbours are [its plane's
// spines][its pod's rack switches]: the first segment of kSlSeg positions is
// its plane's, the rest its pod's.  The rack switches of a pod are twins, and
// so are the spines of a plane.  `tail` more nodes hang off spine 0 as a chain.
constexpr uint32_t kFabricNodes = 64;
inline uint32_t fabric_fsw(uint32_t pod, uint32_t plane) { return 16 + 24 * pod + plane; }
inline Graph fabric(const std::vector<uint32_t>& drained = {}, uint32_t tail = 0) {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t pod = 0; pod < 2; ++pod)
    for (uint32_t plane = 0; plane < 4; ++plane) {
      const uint32_t fsw = fabric_fsw(pod, plane);
      for (uint32_t s = 0; s < 4; ++s) links.emplace_back(fsw, 4 * plane + s);
      for (uint32_t r = 0; r < 20; ++r) links.emplace_back(fsw, 16 + 24 * pod + 4 + r);
    }
  for (uint32_t t = 0; t < tail; ++t) links.emplace_back(t ? kFabricNodes + t - 1 : 0, kFabricNodes + t);
  return from_links(kFabricNodes + tail, links, drained);
}

inline Graph ring(uint32_t n) {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t i = 0; i < n; ++i) links.emplace_back(i, (i + 1) % n);
  return from_links(n, links);
}

// node 0 with `deg` leaves
inline Graph hub(uint32_t deg) {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t i = 1; i <= deg; ++i) links.emplace_back(0, i);
  return from_links(deg + 1, links);
}

inline std::vector<uint32_t> first(uint32_t n) {
  std::vector<uint32_t> v(n);
  for (uint32_t i = 0; i < n; ++i) v[i] = i;
  return v;
}

struct Case {
  const char* name;
  Graph g;
  std::vector<uint32_t> srcs;
  int rows;       // the rows the next-hop pass reads: 2 sliced, 1 u8, 0 u32 (as SPF_NARROW)
  uint32_t runs;  // plan_xcd_lists
  uint32_t unit;  // plan_sliced_units
  int group;
  uint64_t digest;  // of the tables at commit cb07bca
};

// Sources 0 .. 43 of the fabric: the spines, pod 0, pod 1's fabric switches
// (whose rack switches the closure adds).  Dealt round-robin (runs 0), the two
// fabric switches of a plane meet in one XCD list.
inline std::vector<Case> all() {
  const std::vector<uint32_t> two_spines{0, 4};  // of planes 0 and 1
  const Graph f = fabric(), fd = fabric(two_spines), big = fabric({}, 2036);
  const std::vector<uint32_t> most = first(44);
  std::vector<Case> c;
  c.push_back({"fabric64 group 2", f, most, 2, 2, 512, 2, 0x639a93c13c9a521bull});
  c.push_back({"fabric64 group 1", f, most, 2, 2, 512, 1, 0x639a93c13c9a521bull});
  c.push_back({"fabric64 group 0", f, most, 2, 2, 512, 0, 0x1ecc473699516e3full});
  c.push_back({"fabric64 one run per XCD, group 2", f, most, 2, 1, 512, 2, 0xc8501de09f407fd3ull});
  c.push_back({"fabric64 one run per XCD, group 1", f, most, 2, 1, 512, 1, 0xdd2f2600d251c5e5ull});
  c.push_back({"fabric64 one run per XCD, unit 16", f, most, 2, 1, 16, 2, 0x77e283994b866ddfull});
  c.push_back({"ring40", ring(40), first(20), 2, 2, 512, 2, 0x667afdd9b0ef6dfcull});
  c.push_back({"fabric64 drained, runs 0, group 2", fd, most, 2, 0, 512, 2, 0x73b944a985743395ull});
  c.push_back({"fabric64 drained, group 2", fd, most, 2, 2, 512, 2, 0xc057e4fcc56b903bull});
  c.push_back({"fabric64 drained, group 1", fd, most, 2, 2, 512, 1, 0xc057e4fcc56b903bull});
  c.push_back({"fabric64 drained, u8 rows", fd, most, 1, 2, 512, 2, 0x7b24dcc7a02c05b0ull});
  c.push_back({"fabric64 drained, u32 rows", fd, most, 0, 2, 512, 2, 0x190775875633ac20ull});
  c.push_back({"hub of degree 40, unit 16", hub(40), {0, 1, 2}, 2, 2, 16, 2, 0x6aaadac8078ead33ull});
  c.push_back({"fabric + chain of 2100 nodes, group 2", big, most, 2, 2, 512, 2, 0x1b1d3a8274f930b6ull});
  c.push_back({"fabric + chain of 2100 nodes, unit 32, group 0", big, most, 2, 2, 32, 0, 0xd1ffd1ba274b8f69ull});
  c.push_back({"fabric + chain of 2100 nodes, unit 32, runs 0", big, most, 2, 0, 32, 2, 0x53a574c47ec783bfull});
  c.push_back({"sources 5 1 5 0", f, {5, 1, 5, 0}, 2, 2, 512, 2, 0x2fad937c85b910b8ull});
  c.push_back({"every node a source", f, first(64), 2, 2, 512, 2, 0x6713c1c9c22e9cd4ull});
  c.push_back({"every node a source, runs 64", f, first(64), 2, 64, 512, 2, 0x4f5237232b053914ull});
  c.push_back({"one source", f, {fabric_fsw(0, 1)}, 2, 2, 512, 2, 0xd692c8eedaf53079ull});
  c.push_back({"fabric64 runs 0", f, most, 2, 0, 512, 2, 0x4ad8c0d6bcbfb221ull});
  c.push_back({"fabric64 runs 64", f, most, 2, 64, 512, 2, 0x910113286215ebedull});
  return c;
}

// FNV-1a over 32-bit words, least significant byte first; every table goes in
// as its length, then its words.
struct Digest {
  uint64_t h = 0xcbf29ce484222325ull;
  void word(uint32_t w) {
    for (int b = 0; b < 4; ++b) {
      h ^= (w >> (8 * b)) & 0xFFu;
      h *= 0x100000001b3ull;
    }
  }
  void table(const uint32_t* p, size_t n) {
    word((uint32_t)n);
    for (size_t i = 0; i < n; ++i) word(p[i]);
  }
  void table(const std::vector<uint32_t>& v) { table(v.data(), v.size()); }
  void table(const std::vector<uint64_t>& v) {  // low word, high word
    word((uint32_t)v.size());
    for (uint64_t x : v) word((uint32_t)x), word((uint32_t)(x >> 32));
  }
};

}  // namespace plan_cases
