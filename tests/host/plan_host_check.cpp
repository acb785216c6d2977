// A plan's host tables (openr_amd/csrc/plan_host.h) on the CPU, no device,
// over the cases of plan_cases.h:
//  * the contract ecmp_sliced_kernel trusts: every (source, neighbour
//    position, chunk) in exactly one work unit, group members in the unit's
//    XCD list with equal, live neighbour rows over the unit's range, padded
//    and aligned row lists, a slot table holding every request once;
//  * the closure's rows and the next-hop layout;
//  * every table word for word what build_plan uploaded before the
//    derivations moved here (the digests of plan_cases.h);
//  * depth_bound's memo and ecc_estimate on graphs whose answers are known.
// Built with the sanitizers and run by tests/test_plan_host.py; exit status
// 0 = every check held.
#include "plan_host.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "plan_cases.h"

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

void load(const plan_cases::Graph& in, GraphHost* g) {
  spf_graph sg;
  sg.n_nodes = in.N;
  sg.n_edges = (uint32_t)in.col.size();
  sg.row_ptr = in.row_ptr.data();
  sg.col = in.col.data();
  sg.metric = in.met.data();
  sg.link_id = in.link.data();
  sg.overloaded = in.ovl.data();
  GraphDirty d;
  std::string err;
  const spf_status st = graph_host_load(g, &sg, &d, &err);
  if (st != SPF_OK) std::printf("load refused: %s\n", err.c_str());
  CHECK(st == SPF_OK);
}

void check_rows(const GraphHost& g, const std::vector<uint32_t>& srcs, const PlanRows& r) {
  const uint32_t n_src = (uint32_t)srcs.size();
  std::vector<uint8_t> is_src(g.N, 0), wanted(g.N, 0);
  bool distinct = true, closed = true;
  for (uint32_t s : srcs) {
    if (is_src[s]) distinct = false;
    is_src[s] = 1;
  }
  for (uint32_t s : srcs) {
    wanted[s] = 1;
    for (uint32_t e = g.nb_ptr[s]; e < g.nb_ptr[s + 1]; ++e) {
      const uint32_t x = g.nb_id[e];
      if (g.ovl[x]) continue;
      wanted[x] = 1;
      closed &= is_src[x] != 0;
      CHECK(r.row_of[x] != kInf);  // every non-drained neighbour of every source has a row
    }
  }
  CHECK(r.distinct == distinct);
  CHECK(r.direct == (distinct && closed));
  if (r.direct) CHECK(r.closure == srcs);
  CHECK(r.row_of.size() == g.N && r.req_rows.size() == n_src);
  for (uint32_t x = 0; x < g.N; ++x) {
    CHECK((r.row_of[x] != kInf) == (wanted[x] != 0));  // and nothing else has one
    if (r.row_of[x] != kInf) CHECK(r.row_of[x] < r.closure.size() && r.closure[r.row_of[x]] == x);
  }
  for (uint32_t row = 0; row < r.closure.size(); ++row) CHECK(r.row_of[r.closure[row]] == row);
  for (uint32_t i = 0; i < n_src; ++i) {
    CHECK(r.req_rows[i] == r.row_of[srcs[i]]);
    if (distinct) CHECK(r.closure[i] == srcs[i]);
  }
}

void check_layout(const GraphHost& g, const std::vector<uint32_t>& srcs, const NhLayout& l) {
  uint64_t off = 0;
  uint32_t wmax = 1;
  CHECK(l.words.size() == srcs.size() && l.nh_off.size() == srcs.size());
  for (size_t i = 0; i < srcs.size(); ++i) {
    const uint32_t k = g.nb_ptr[srcs[i] + 1] - g.nb_ptr[srcs[i]];
    CHECK(l.words[i] == k && l.nh_off[i] == off);
    off += (uint64_t)k * (g.pitch / 32);
    wmax = std::max(wmax, (k + 31) / 32);
  }
  CHECK(l.nh_total == off && l.wmax == wmax);
}

void check_nb_rows(const GraphHost& g, const std::vector<uint32_t>& srcs, const PlanRows& r,
                   const std::vector<uint32_t>& words, uint64_t stride, const NbRows& nb) {
  const uint32_t n_src = (uint32_t)srcs.size();
  CHECK(nb.dead == (stride ? (uint32_t)(r.closure.size() * stride) : kInf));
  CHECK(nb.nb_row_off.size() == n_src && nb.nb_drained.size() == n_src);
  for (uint32_t i = 0; i < n_src; ++i) {
    const uint32_t at = nb.nb_row_off[i];
    const size_t end = i + 1 < n_src ? nb.nb_row_off[i + 1] : nb.nb_row.size();
    CHECK(at % 8 == 0 && at + words[i] + 8 <= end);  // at least 8 dead words behind each list
    uint32_t drained = 0;
    for (uint32_t j = 0; j < words[i]; ++j) {
      const uint32_t x = g.nb_id[g.nb_ptr[srcs[i]] + j];
      if (g.ovl[x]) {
        CHECK(nb.nb_row[at + j] == nb.dead);
        ++drained;
      } else {
        CHECK(nb.nb_row[at + j] == (stride ? (uint32_t)(r.row_of[x] * stride) : r.row_of[x]));
        CHECK(nb.nb_row[at + j] != nb.dead);
      }
    }
    for (size_t j = at + words[i]; j < end; ++j) CHECK(nb.nb_row[j] == nb.dead);
    CHECK(nb.nb_drained[i] == drained);
  }
}

void check_lists(uint32_t n_src, const XcdLists& x) {
  std::vector<uint32_t> seen(n_src, 0);
  size_t most = 0;
  for (const auto& l : x.list) {
    most = std::max(most, l.size());
    CHECK(std::is_sorted(l.begin(), l.end()));  // the XCD's source order is the request's
    for (uint32_t i : l) {
      CHECK(i < n_src);
      if (i < n_src) ++seen[i];
    }
  }
  for (uint32_t i = 0; i < n_src; ++i) CHECK(seen[i] == 1);
  CHECK(x.slots == most * 8 && x.slot.size() == std::max<size_t>(x.slots, 1));
  size_t held = 0;
  for (size_t t = 0; t < most; ++t)
    for (int g = 0; g < 8; ++g) {
      const uint32_t v = x.slot[t * 8 + g];
      CHECK(v == (t < x.list[g].size() ? x.list[g][t] : kInf));
      held += v != kInf;
    }
  CHECK(held == n_src);  // every request index once (the lists hold each once), kInf elsewhere
}

struct UnitStats {
  uint32_t units = 0, groups = 0, largest_group = 0;
  uint32_t group_units = 0;  // units of groups
  uint32_t part_units = 0;   // ... over a part of their members' lists, not all of them
  uint32_t multi_chunk = 0;  // per-source units spanning more than one chunk
  uint32_t cut = 0;          // units (of either kind) over part of a longer run of positions
};

UnitStats check_units(const std::vector<uint32_t>& words, const NbRows& nb, const XcdLists& x,
                      uint32_t chunks, int group, const SlicedUnits& su) {
  UnitStats st;
  const uint32_t n_src = (uint32_t)words.size();
  CHECK(su.unit_off.size() == 9 && su.unit_off[0] == 0);
  uint32_t most = 0;
  for (int g = 0; g < 8; ++g) {
    CHECK(su.unit_off[g] <= su.unit_off[g + 1]);
    most = std::max(most, su.unit_off[g + 1] - su.unit_off[g]);
  }
  CHECK(su.max_xcd_units == most);
  if (su.unit_off[8]) CHECK((size_t)su.unit_off[8] * 4 == su.units.size());
  else CHECK(su.units == std::vector<uint32_t>(4, 0u));
  CHECK(!su.gtab.empty());
  if ((size_t)su.unit_off[8] * 4 > su.units.size()) return st;
  // cover[i][j * chunks + ch]: the units holding (source i, position j, chunk ch)
  std::vector<std::vector<uint8_t>> cover(n_src);
  for (uint32_t i = 0; i < n_src; ++i) cover[i].assign((size_t)words[i] * chunks, 0);
  auto add = [&](uint32_t i, uint32_t c0, uint32_t c1, uint32_t j0, uint32_t j1) {
    for (uint32_t j = j0; j < j1; ++j)
      for (uint32_t ch = c0; ch < c1; ++ch) ++cover[i][(size_t)j * chunks + ch];
  };
  bool any_group = false;
  for (int g = 0; g < 8; ++g) {
    const auto& list = x.list[g];
    auto in_list = [&](uint32_t i) { return std::binary_search(list.begin(), list.end(), i); };
    for (uint32_t u = su.unit_off[g]; u < su.unit_off[g + 1]; ++u) {
      const uint32_t ux = su.units[4 * u], uy = su.units[4 * u + 1], uz = su.units[4 * u + 2],
                     uw = su.units[4 * u + 3];
      ++st.units;
      CHECK(uz % kSlSeg == 0 && uz < uw);
      if (uy >> 31 == 0) {  // one source, chunks [uy & 0xFFFF, uy >> 16)
        const uint32_t c0 = uy & 0xFFFFu, c1 = uy >> 16;
        CHECK(ux < n_src && c0 < c1 && c1 <= chunks);
        if (!(ux < n_src && c1 <= chunks)) continue;
        CHECK(in_list(ux) && uw <= words[ux]);
        if (uw > words[ux]) continue;
        add(ux, c0, c1, uz, uw);
        st.multi_chunk += c1 - c0 > 1;
        st.cut += c1 - c0 < chunks;
        continue;
      }
      // a group: chunk uy & 0xFFFF for every member of gtab[ux]
      any_group = true;
      const uint32_t ch = uy & 0xFFFFu;
      CHECK((uy & 0x7FFF0000u) == 0 && ch < chunks);
      CHECK(ux < su.gtab.size());
      if (!(ux < su.gtab.size() && ch < chunks)) continue;
      const uint32_t gs = su.gtab[ux];
      CHECK(gs >= 2 && gs <= kSlGroup && (size_t)ux + 1 + gs <= su.gtab.size());
      if (!(gs >= 2 && gs <= kSlGroup && (size_t)ux + 1 + gs <= su.gtab.size())) continue;
      st.largest_group = std::max(st.largest_group, gs);
      ++st.group_units;
      const uint32_t* m = su.gtab.data() + ux + 1;
      bool ok = true;
      for (uint32_t a = 0; a < gs; ++a) {
        CHECK(m[a] < n_src);
        ok &= m[a] < n_src;
        if (!ok) break;
        CHECK(in_list(m[a]) && uw <= words[m[a]]);
        ok &= uw <= words[m[a]];
        for (uint32_t b = 0; b < a; ++b) CHECK(m[a] != m[b]);
      }
      if (!ok) continue;
      for (uint32_t a = 0; a < gs; ++a) {
        for (uint32_t j = uz; j < uw; ++j) {
          const uint32_t row = nb.nb_row[nb.nb_row_off[m[a]] + j];
          CHECK(row != nb.dead && row == nb.nb_row[nb.nb_row_off[m[0]] + j]);
        }
        add(m[a], ch, ch + 1, uz, uw);
      }
      st.part_units += uz > 0 || uw < words[m[0]];
    }
  }
  for (uint32_t i = 0; i < n_src; ++i) {
    bool once = true;
    for (uint8_t n : cover[i]) once &= n == 1;
    if (!once) std::printf("    source %u: a (position, chunk) not in exactly one unit\n", i);
    CHECK(once);
  }
  // the groups gtab lists, back to back
  for (size_t at = 0; any_group && at < su.gtab.size(); at += 1 + su.gtab[at]) ++st.groups;
  if (!any_group) CHECK(su.gtab == std::vector<uint32_t>(1, 0u));
  if (group == 0) CHECK(!any_group);
  return st;
}

void run_case(const plan_cases::Case& c) {
  std::printf("%s\n", c.name);
  GraphHost g;
  load(c.g, &g);
  if (!g.loaded) return;
  const uint32_t n_src = (uint32_t)c.srcs.size();
  const PlanRows rows = plan_rows(g, c.srcs.data(), n_src);
  check_rows(g, c.srcs, rows);
  const NhLayout nl = plan_nh_layout(g, c.srcs.data(), n_src);
  check_layout(g, c.srcs, nl);
  const uint32_t wpm = g.pitch / 32, chunks = (wpm + 63) / 64;
  const uint64_t stride = c.rows == 2 ? (uint64_t)kSlSlots * wpm : c.rows == 1 ? g.npitch : 0;
  const NbRows nb = plan_nb_rows(g, c.srcs.data(), n_src, rows.row_of, stride, rows.closure.size());
  check_nb_rows(g, c.srcs, rows, nl.words, stride, nb);
  const XcdLists xcd = plan_xcd_lists(nl.words, c.runs);
  check_lists(n_src, xcd);
  SlicedUnits su;
  UnitStats st;
  if (c.rows == 2) {
    su = plan_sliced_units(xcd.list, nl.words, nb, chunks, c.unit, c.group);
    st = check_units(nl.words, nb, xcd, chunks, c.group, su);
  }
  plan_cases::Digest d;
  d.table(rows.closure);
  d.table(rows.row_of);
  d.table(rows.req_rows);
  d.table(nl.nh_off);
  d.table(nl.words);
  d.table(nb.nb_row);
  d.table(nb.nb_row_off);
  d.table(nb.nb_drained);
  d.table(su.units);
  d.table(su.unit_off);
  d.table(su.gtab);
  d.table(xcd.slot);
  std::printf("  rows %zu%s, chunks %u, units %u (%u over several chunks, %u of one chunk of several), groups %u "
              "(largest %u) in %u units (%u over part of a list), digest %016llx\n", rows.closure.size(),
              rows.direct ? " (direct)" : "", chunks, st.units, st.multi_chunk, st.cut, st.groups,
              st.largest_group, st.group_units, st.part_units, (unsigned long long)d.h);
  CHECK(d.h == c.digest);

  // what each case is there for
  const std::string name = c.name;
  auto is = [&](const char* prefix) { return name.compare(0, std::strlen(prefix), prefix) == 0; };
  size_t lists_used = 0;
  for (const auto& l : xcd.list) lists_used += !l.empty();
  uint32_t drained = 0;
  for (uint32_t n : nb.nb_drained) drained += n;
  if (is("fabric64 group 2") || is("fabric64 group 1")) CHECK(st.groups > 0 && !rows.direct);
  // whole-list twins only: every group unit over its members' whole lists
  if (c.group == 1) CHECK(st.part_units == 0);
  // three fabric switches of pod 0 in one list share their pod's segments
  if (is("fabric64 one run per XCD, group 2")) CHECK(st.part_units > 0 && st.largest_group == kSlGroup);
  if (is("fabric64 one run per XCD, unit 16")) CHECK(st.group_units > st.groups);  // ranges cut
  if (is("ring40")) CHECK(st.groups == 0 && st.units == n_src);
  if (is("fabric64 drained")) CHECK(drained == 4);  // the fabric switches of planes 0 and 1 see one each
  if (is("hub of degree 40")) CHECK(chunks == 1 && st.units == 3 + 2 && st.groups == 0);  // 40 = 16 + 16 + 8
  if (is("fabric + chain of 2100 nodes")) CHECK(g.pitch > 2048 && chunks == 2);
  if (is("fabric + chain of 2100 nodes, group 2")) CHECK(st.multi_chunk > 0 && st.group_units >= 2 * st.groups);
  if (is("fabric + chain of 2100 nodes, unit 32, group 0")) CHECK(st.cut > 0 && st.multi_chunk > 0);
  if (is("sources 5 1 5 0")) CHECK(!rows.distinct && !rows.direct && rows.req_rows[0] == rows.req_rows[2]);
  if (is("every node a source")) CHECK(rows.direct && rows.closure.size() == g.N);
  if (is("one source")) CHECK(lists_used == 1 && xcd.slots == 8);
  if (is("fabric64 runs 0")) {
    // 16 + j and 40 + j, the fabric switches of plane j, are 24 apart: one list,
    // sharing their plane's segment; so do planes 2 and 3 with spines drained
    CHECK(xcd.list[3] == (std::vector<uint32_t>{3, 11, 19, 27, 35, 43}));
    CHECK(st.part_units >= 4);
  }
  if (is("fabric64 drained, runs 0")) CHECK(st.part_units >= 2);
}

// The bounds: known answers, the memo's rule (same sell_ver and drain bits,
// four entries), the depth order.
void bounds() {
  std::printf("bounds\n");
  GraphHost g;
  load(plan_cases::ring(40), &g);
  DepthCache m;
  CHECK(depth_bound(g, &m) == 2 + 2 * 20);
  CHECK(m.memo.size() == 1);
  const std::vector<uint32_t>& ecc = ecc_estimate(g, &m);
  CHECK(ecc.size() == 40 && ecc[0] == 20);
  for (uint32_t e : ecc) CHECK(e <= 20);
  // a drained node opens the ring: a path, measured from its lowest node
  g.ovl[7] = 1;
  ++g.epoch;
  CHECK(depth_bound(g, &m) == 2 + 2 * 32 && m.memo.size() == 2);  // node 0, the root, is 32 from node 8
  g.ovl[7] = 0;
  ++g.epoch;
  CHECK(depth_bound(g, &m) == 42 && m.memo.size() == 2);  // found again, no new entry
  for (uint32_t v = 10; v < 14; ++v) {
    g.ovl[v] = 1;
    ++g.epoch;
    depth_bound(g, &m);
  }
  CHECK(m.memo.size() == 4 && m.dbound == 2 + 2 * 26);  // 14 .. 39, 0 .. 9
  ++g.sell_ver;  // the structure moved: nothing remembered applies
  ++g.epoch;
  CHECK(depth_bound(g, &m) == 2 + 2 * 26 && m.memo.size() == 4 && m.memo.back().sell_ver == g.sell_ver);

  GraphHost f;
  load(plan_cases::fabric({0, 4}), &f);
  DepthCache mf;
  CHECK(depth_bound(f, &mf) == 2 + 2 * 4);  // spine - fsw - rsw - fsw - spine
  const std::vector<uint32_t> closure{20, 0, 16, 1, 12};
  const std::vector<uint32_t>& fe = ecc_estimate(f, &mf);
  const std::vector<uint32_t> order = plan_depth_order(closure, fe);
  CHECK(order.size() == closure.size());
  for (size_t i = 0; i + 1 < order.size(); ++i) {
    const uint32_t a = fe[closure[order[i]]], b = fe[closure[order[i + 1]]];
    CHECK(a > b || (a == b && order[i] < order[i + 1]));
  }
}

}  // namespace

int main() {
  for (const auto& c : plan_cases::all()) run_case(c);
  bounds();
  if (g_failed) std::printf("%d checks failed\n", g_failed);
  else std::printf("ok\n");
  return g_failed ? 1 : 0;
}
