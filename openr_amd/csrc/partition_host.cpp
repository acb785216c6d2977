// ============================================================================
//  partition_host.cpp -- see partition_host.h.
// ============================================================================
#include "partition_host.h"

#include <algorithm>
#include <limits>
#include <numeric>
#include <utility>

namespace spfi {

std::vector<uint32_t> closure_sizes(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                                    const uint32_t* srcs, uint32_t n_src, const uint32_t* part,
                                    uint32_t n_parts) {
  std::vector<uint32_t> out(n_parts, 0);
  std::vector<uint32_t> mark(n_nodes, 0xFFFFFFFFu);
  for (uint32_t r = 0; r < n_parts; ++r) {
    uint32_t cnt = 0;
    auto add = [&](uint32_t x) {
      if (mark[x] != r) mark[x] = r, ++cnt;
    };
    for (uint32_t i = 0; i < n_src; ++i) {
      if (part[i] != r) continue;
      add(srcs[i]);
      for (uint32_t e = nb_ptr[srcs[i]]; e < nb_ptr[srcs[i] + 1]; ++e) add(nb_id[e]);
    }
    out[r] = cnt;
  }
  return out;
}

void contiguous_parts(const uint32_t* nb_ptr, const uint32_t* srcs, uint32_t n_src, uint32_t n_parts,
                      uint32_t* part) {
  std::vector<double> cum(n_src);
  double acc = 0;
  for (uint32_t i = 0; i < n_src; ++i) {
    acc += (double)(nb_ptr[srcs[i] + 1] - nb_ptr[srcs[i]]) + kRowCost;
    cum[i] = acc;
  }
  std::vector<uint32_t> bounds(n_parts + 1, 0);
  bounds[n_parts] = n_src;
  for (uint32_t r = 1; r < n_parts; ++r)
    bounds[r] = (uint32_t)(std::upper_bound(cum.begin(), cum.end(), acc * r / n_parts) - cum.begin());
  for (uint32_t r = 0; r < n_parts; ++r)
    for (uint32_t i = bounds[r]; i < std::max(bounds[r], bounds[r + 1]); ++i) part[i] = r;
}

// One-pass streaming partition (linear deterministic greedy): sources in
// ascending (degree, position), each to the part whose closure it grows
// least among the parts whose cost stays within 3 % of the mean, ties to
// the least loaded, then the lowest part.  Low-degree nodes first: a
// fabric's rack switches gather by pod, the fabric switches follow their
// pod, a plane's spines land together.  Same rule as sharding.py
// locality_partition (tests/test_partition.py checks they agree).
void locality_parts(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                    const uint32_t* srcs, uint32_t n_src, uint32_t n_parts, uint32_t* part) {
  std::vector<uint32_t> order(n_src);
  std::iota(order.begin(), order.end(), 0u);
  auto deg = [&](uint32_t i) { return nb_ptr[srcs[i] + 1] - nb_ptr[srcs[i]]; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return deg(a) < deg(b); });
  double total = 0;
  for (uint32_t i = 0; i < n_src; ++i) total += (double)deg(i) + kRowCost;
  const double cap = total / n_parts * (1.0 + 0.03);  // sharding.py: sum / world * (1 + slack)
  std::vector<uint8_t> clo((size_t)n_parts * n_nodes, 0);
  std::vector<double> load(n_parts, 0.0);
  std::vector<double> grow(n_parts);
  for (uint32_t i : order) {
    const uint32_t v = srcs[i];
    const double cost = (double)deg(i) + kRowCost;
    bool any_ok = false;
    for (uint32_t r = 0; r < n_parts; ++r) any_ok |= load[r] + cost <= cap;
    for (uint32_t r = 0; r < n_parts; ++r) {
      if (any_ok && !(load[r] + cost <= cap)) {
        grow[r] = std::numeric_limits<double>::infinity();
        continue;
      }
      const uint8_t* c = clo.data() + (size_t)r * n_nodes;
      uint32_t g = c[v] ? 0u : 1u;
      for (uint32_t e = nb_ptr[v]; e < nb_ptr[v + 1]; ++e) g += c[nb_id[e]] ? 0u : 1u;
      grow[r] = g;
    }
    const double best = *std::min_element(grow.begin(), grow.end());
    uint32_t pick = n_parts;
    for (uint32_t r = 0; r < n_parts; ++r)
      if (grow[r] == best && (pick == n_parts || load[r] < load[pick])) pick = r;
    part[i] = pick;
    uint8_t* c = clo.data() + (size_t)pick * n_nodes;
    c[v] = 1;
    for (uint32_t e = nb_ptr[v]; e < nb_ptr[v + 1]; ++e) c[nb_id[e]] = 1;
    load[pick] += cost;
  }
}

uint32_t partition_sources(const uint32_t* nb_ptr, const uint32_t* nb_id, uint32_t n_nodes,
                           const uint32_t* srcs, uint32_t n_src, uint32_t n_parts, uint32_t mode,
                           uint32_t* part) {
  contiguous_parts(nb_ptr, srcs, n_src, n_parts, part);
  if (mode == SPF_PARTITION_CONTIGUOUS || n_parts <= 1) return SPF_PARTITION_CONTIGUOUS;
  if (mode == SPF_PARTITION_AUTO && n_nodes > kLocalityMaxNodes) return SPF_PARTITION_CONTIGUOUS;
  std::vector<uint32_t> loc(n_src);
  locality_parts(nb_ptr, nb_id, n_nodes, srcs, n_src, n_parts, loc.data());
  if (mode == SPF_PARTITION_AUTO) {
    const auto a = closure_sizes(nb_ptr, nb_id, n_nodes, srcs, n_src, part, n_parts);
    const auto b = closure_sizes(nb_ptr, nb_id, n_nodes, srcs, n_src, loc.data(), n_parts);
    if (*std::max_element(b.begin(), b.end()) >= *std::max_element(a.begin(), a.end()))
      return SPF_PARTITION_CONTIGUOUS;
  }
  std::copy(loc.begin(), loc.end(), part);
  return SPF_PARTITION_LOCALITY;
}

uint32_t label_groups(const int32_t* node_label, uint32_t n_nodes, int32_t* labels, uint32_t* grp_ptr,
                      uint32_t* grp_nodes) {
  // buildRouteDb (Decision.cpp:592-603): label 0 = none advertised, a label
  // outside the 20-bit space (isMplsLabelValid) is skipped
  std::vector<std::pair<int32_t, uint32_t>> adv;
  for (uint32_t v = 0; v < n_nodes; ++v)
    if (node_label[v] > 0 && node_label[v] <= (1 << 20) - 1) adv.emplace_back(node_label[v], v);
  std::sort(adv.begin(), adv.end());
  uint32_t g = 0;
  for (size_t i = 0; i < adv.size(); ++i) {
    if (i == 0 || adv[i].first != adv[i - 1].first) {
      if (labels) labels[g] = adv[i].first;
      if (grp_ptr) grp_ptr[g] = (uint32_t)i;
      ++g;
    }
    if (grp_nodes) grp_nodes[i] = adv[i].second;
  }
  if (grp_ptr) grp_ptr[g] = (uint32_t)adv.size();
  return g;
}

LabelUnion label_union(const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
  LabelUnion u;
  size_t i = 0, j = 0;
  while (i < a.size() || j < b.size()) {
    const bool ta = j == b.size() || (i < a.size() && a[i] <= b[j]);
    const bool tb = i == a.size() || (j < b.size() && b[j] <= a[i]);
    u.lab.push_back((uint32_t)(ta ? a[i] : b[j]));
    u.mold.push_back(ta ? (uint32_t)i : 0xFFFFFFFFu);
    u.mnew.push_back(tb ? (uint32_t)j : 0xFFFFFFFFu);
    i += ta;
    j += tb;
  }
  return u;
}

}  // namespace spfi
