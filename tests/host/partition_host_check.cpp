// The multi-device plans' host arithmetic (openr_amd/csrc/partition_host.h) on
// the CPU, no device:
//  * partition_sources on a 19-node fabric, a 5 x 5 grid, a star with 8
//    leaves, a ring with an isolated node among the sources and a source
//    subset (every third node of the fabric), each in all three modes with 1,
//    2, 3 and n_src + 1 parts (empty blocks): every source in a part, and
//    part[] and the rule taken word for word what spf_partition_sources
//    answered before the partition moved here;
//  * AUTO just past kLocalityMaxNodes answers CONTIGUOUS;
//  * label_groups without a labelled node, with one label on every node,
//    duplicates out of order and the ends of the 20-bit label space: what
//    spf_label_groups answered before its body moved here;
//  * label_union against expectations written by hand.
// The digests below are FNV-1a (plan_cases.h) of what commit 8a10051 answered:
// this program run with --print, its spfi:: calls bound to that commit's
// spf_partition_sources and spf_label_groups.  Built with the sanitizers and
// run by tests/test_partition_host.py; exit status 0 = every check held.
#include "partition_host.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>

#include "plan_cases.h"

using namespace spfi;

namespace {

int g_failed = 0;
bool g_print = false;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                  \
    }                                                              \
  } while (0)

// distinct neighbours per node, ascending (spf_src_neighbors' lists, CSR form)
struct Nbrs {
  uint32_t N = 0;
  std::vector<uint32_t> ptr, id;
};

Nbrs from_links(uint32_t N, const std::vector<std::pair<uint32_t, uint32_t>>& links) {
  std::vector<std::vector<uint32_t>> rows(N);
  for (const auto& l : links) {
    rows[l.first].push_back(l.second);
    rows[l.second].push_back(l.first);
  }
  Nbrs g;
  g.N = N;
  g.ptr.push_back(0);
  for (auto& r : rows) {
    std::sort(r.begin(), r.end());
    r.erase(std::unique(r.begin(), r.end()), r.end());
    g.id.insert(g.id.end(), r.begin(), r.end());
    g.ptr.push_back((uint32_t)g.id.size());
  }
  return g;
}

// Two planes of two spines (0 .. 3), then three pods of two fabric switches
// (one per plane) and three rack switches each: 19 nodes.
Nbrs fabric19() {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t pod = 0; pod < 3; ++pod)
    for (uint32_t plane = 0; plane < 2; ++plane) {
      const uint32_t fsw = 4 + 5 * pod + plane;
      for (uint32_t s = 0; s < 2; ++s) links.emplace_back(fsw, 2 * plane + s);
      for (uint32_t r = 0; r < 3; ++r) links.emplace_back(fsw, 4 + 5 * pod + 2 + r);
    }
  return from_links(19, links);
}

Nbrs grid(uint32_t n) {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t y = 0; y < n; ++y)
    for (uint32_t x = 0; x < n; ++x) {
      if (x + 1 < n) links.emplace_back(y * n + x, y * n + x + 1);
      if (y + 1 < n) links.emplace_back(y * n + x, (y + 1) * n + x);
    }
  return from_links(n * n, links);
}

Nbrs star(uint32_t leaves) {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t i = 1; i <= leaves; ++i) links.emplace_back(0, i);
  return from_links(leaves + 1, links);
}

// a ring of `n` nodes and node `n` without a link
Nbrs ring_and_isolated(uint32_t n) {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t i = 0; i < n; ++i) links.emplace_back(i, (i + 1) % n);
  return from_links(n + 1, links);
}

Nbrs chain(uint32_t n) {
  std::vector<std::pair<uint32_t, uint32_t>> links;
  for (uint32_t i = 0; i + 1 < n; ++i) links.emplace_back(i, i + 1);
  return from_links(n, links);
}

std::vector<uint32_t> every(uint32_t n, uint32_t step) {
  std::vector<uint32_t> v;
  for (uint32_t i = 0; i < n; i += step) v.push_back(i);
  return v;
}

void expect(const char* name, uint64_t got, uint64_t want) {
  if (g_print) {
    std::printf("  %-40s 0x%016llxull\n", name, (unsigned long long)got);
    return;
  }
  if (got != want) std::printf("%s: digest %016llx, expected %016llx\n", name, (unsigned long long)got,
                               (unsigned long long)want);
  CHECK(got == want);
}

// all three modes with 1, 2, 3 and n_src + 1 parts: one digest over every
// answer (the rule taken, then part[])
void partition_case(const char* name, const Nbrs& g, const std::vector<uint32_t>& srcs, uint64_t want) {
  const uint32_t n_src = (uint32_t)srcs.size();
  plan_cases::Digest d;
  for (const uint32_t n_parts : {1u, 2u, 3u, n_src + 1})
    for (const uint32_t mode : {SPF_PARTITION_AUTO, SPF_PARTITION_CONTIGUOUS, SPF_PARTITION_LOCALITY}) {
      std::vector<uint32_t> part(n_src, 0xFFFFFFFFu);
      const uint32_t used = partition_sources(g.ptr.data(), g.id.data(), g.N, srcs.data(), n_src, n_parts, mode,
                                              part.data());
      for (const uint32_t p : part) CHECK(p < n_parts);
      CHECK(used == SPF_PARTITION_CONTIGUOUS || used == SPF_PARTITION_LOCALITY);
      if (mode != SPF_PARTITION_AUTO) CHECK(used == (n_parts > 1 ? mode : SPF_PARTITION_CONTIGUOUS));
      if (used == SPF_PARTITION_CONTIGUOUS) CHECK(std::is_sorted(part.begin(), part.end()));
      d.word(used);
      d.table(part);
    }
  expect(name, d.h, want);
}

void partitions() {
  std::printf("partition_sources\n");
  const Nbrs f = fabric19(), ri = ring_and_isolated(6);
  partition_case("fabric of 19 nodes", f, plan_cases::first(19), 0x4529dbf0b4fd280dull);
  partition_case("grid 5 x 5", grid(5), plan_cases::first(25), 0x84d3b3ba35af45e6ull);
  partition_case("star with 8 leaves", star(8), plan_cases::first(9), 0x347128fd2c543be7ull);
  partition_case("ring of 6 and an isolated node", ri, plan_cases::first(7), 0x916957e7205b2847ull);
  partition_case("every third node of the fabric", f, every(19, 3), 0x0db7aa7c9d59fd04ull);
  // one node more than the locality partition takes on automatically
  const Nbrs big = chain(kLocalityMaxNodes + 1);
  const std::vector<uint32_t> srcs = every(big.N, 1024);
  std::vector<uint32_t> part(srcs.size(), 0xFFFFFFFFu);
  const uint32_t used = partition_sources(big.ptr.data(), big.id.data(), big.N, srcs.data(), (uint32_t)srcs.size(),
                                          2, SPF_PARTITION_AUTO, part.data());
  CHECK(used == SPF_PARTITION_CONTIGUOUS);
  plan_cases::Digest d;
  d.word(used);
  d.table(part);
  expect("chain of 65537 nodes, AUTO", d.h, 0x0c997ff5d8e4ec34ull);
}

void label_case(const char* name, const std::vector<int32_t>& node_label, uint32_t groups, uint64_t want) {
  const uint32_t n = (uint32_t)node_label.size();
  std::vector<int32_t> labels(n, -7);
  std::vector<uint32_t> gptr((size_t)n + 1, 0xFFFFFFFFu), gnodes(n, 0xFFFFFFFFu);
  const uint32_t G = label_groups(node_label.data(), n, labels.data(), gptr.data(), gnodes.data());
  CHECK(G == groups);
  CHECK(label_groups(node_label.data(), n, nullptr, nullptr, nullptr) == G);  // counting alone
  CHECK(G <= n && gptr[0] == 0);
  if (G > n) return;
  for (uint32_t g = 0; g < G; ++g) {
    CHECK(gptr[g] < gptr[g + 1] && gptr[g + 1] <= n);
    if (g) CHECK(labels[g - 1] < labels[g]);
    for (uint32_t i = gptr[g]; i < gptr[g + 1] && i < n; ++i) {
      CHECK(gnodes[i] < n && node_label[gnodes[i]] == labels[g]);
      if (i > gptr[g]) CHECK(gnodes[i - 1] < gnodes[i]);
    }
  }
  plan_cases::Digest d;
  d.word(G);
  d.table(reinterpret_cast<const uint32_t*>(labels.data()), G);
  d.table(gptr.data(), (size_t)G + 1);
  d.table(gnodes.data(), gptr[G] <= n ? gptr[G] : 0);
  expect(name, d.h, want);
}

void labels() {
  std::printf("label_groups\n");
  const int32_t top = (1 << 20) - 1;  // the largest label of the 20-bit space; 1 the smallest
  label_case("no node", {}, 0, 0xf942775cda7cd084ull);
  label_case("no labelled node", {0, 0, 0, 0, 0}, 0, 0xf942775cda7cd084ull);
  label_case("one label on every node", {777, 777, 777, 777}, 1, 0x58f80748e4e2fbffull);
  label_case("duplicates out of order", {300, 100, 300, 200, 100, 0, 300, 200}, 3, 0xf2febb0252f7ec2dull);
  label_case("ends of the label space", {top, 1, top + 1, 0, -1, 2147483647, (int32_t)-2147483647 - 1, 1, top}, 2,
             0x05da572e157590e2ull);
}

void union_case(const std::vector<int32_t>& a, const std::vector<int32_t>& b, const std::vector<uint32_t>& lab,
                const std::vector<uint32_t>& mold, const std::vector<uint32_t>& mnew) {
  const LabelUnion u = label_union(a, b);
  CHECK(u.lab == lab && u.mold == mold && u.mnew == mnew);
  CHECK(u.mold.size() == u.lab.size() && u.mnew.size() == u.lab.size());
  if (u.mold.size() != u.lab.size() || u.mnew.size() != u.lab.size()) return;
  for (size_t i = 0; i < u.lab.size(); ++i) {
    if (i) CHECK(u.lab[i - 1] < u.lab[i]);  // strictly ascending: every label once
    CHECK(u.mold[i] != 0xFFFFFFFFu || u.mnew[i] != 0xFFFFFFFFu);
    if (u.mold[i] != 0xFFFFFFFFu) CHECK(u.mold[i] < a.size() && (uint32_t)a[u.mold[i]] == u.lab[i]);
    else CHECK(std::find(a.begin(), a.end(), (int32_t)u.lab[i]) == a.end());
    if (u.mnew[i] != 0xFFFFFFFFu) CHECK(u.mnew[i] < b.size() && (uint32_t)b[u.mnew[i]] == u.lab[i]);
    else CHECK(std::find(b.begin(), b.end(), (int32_t)u.lab[i]) == b.end());
  }
}

void unions() {
  std::printf("label_union\n");
  const uint32_t no = 0xFFFFFFFFu;
  union_case({}, {}, {}, {}, {});
  union_case({5, 9}, {}, {5, 9}, {0, 1}, {no, no});
  union_case({}, {5, 9}, {5, 9}, {no, no}, {0, 1});
  union_case({1, 2, 1048575}, {1, 2, 1048575}, {1, 2, 1048575}, {0, 1, 2}, {0, 1, 2});
  union_case({1, 2, 3}, {10, 20}, {1, 2, 3, 10, 20}, {0, 1, 2, no, no}, {no, no, no, 0, 1});
  union_case({10, 20}, {1, 2, 3}, {1, 2, 3, 10, 20}, {no, no, no, 0, 1}, {0, 1, 2, no, no});
  union_case({1, 4, 6, 9}, {2, 4, 5, 9, 12}, {1, 2, 4, 5, 6, 9, 12}, {0, no, 1, no, 2, 3, no},
             {no, 0, 1, 2, no, 3, 4});
}

}  // namespace

int main(int argc, char** argv) {
  g_print = argc > 1 && std::strcmp(argv[1], "--print") == 0;
  partitions();
  labels();
  unions();
  if (g_failed) std::printf("%d checks failed\n", g_failed);
  else std::printf("ok\n");
  return g_failed ? 1 : 0;
}
