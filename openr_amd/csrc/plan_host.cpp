// ============================================================================
//  plan_host.cpp -- a plan's host tables (plan_host.h), derived from the
//  graph's host state.  No device in here.
// ============================================================================
#include "plan_host.h"

#include <algorithm>
#include <map>
#include <numeric>
#include <utility>

namespace spfi {

PlanRows plan_rows(const GraphHost& g, const uint32_t* srcs, uint32_t n_src) {
  PlanRows r;
  r.row_of.assign(g.N, kInf);
  std::vector<uint32_t>& row_of = r.row_of;
  r.distinct = true;
  for (uint32_t i = 0; i < n_src; ++i) {
    if (row_of[srcs[i]] != kInf) r.distinct = false;
    else row_of[srcs[i]] = i;
  }
  // closure: every non-overloaded neighbour's distance row is needed
  bool closed = r.distinct;
  for (uint32_t i = 0; i < n_src && closed; ++i) {
    const uint32_t s = srcs[i];
    for (uint32_t j = g.nb_ptr[s]; j < g.nb_ptr[s + 1]; ++j) {
      const uint32_t x = g.nb_id[j];
      if (!g.ovl[x] && row_of[x] == kInf) {
        closed = false;
        break;
      }
    }
  }
  r.direct = closed;
  if (closed) {
    r.closure.assign(srcs, srcs + n_src);
  } else {
    std::fill(row_of.begin(), row_of.end(), kInf);
    auto add = [&](uint32_t x) {
      if (row_of[x] == kInf) {
        row_of[x] = (uint32_t)r.closure.size();
        r.closure.push_back(x);
      }
    };
    if (r.distinct)
      for (uint32_t i = 0; i < n_src; ++i) add(srcs[i]);
    for (uint32_t i = 0; i < n_src; ++i) {
      const uint32_t s = srcs[i];
      add(s);
      for (uint32_t j = g.nb_ptr[s]; j < g.nb_ptr[s + 1]; ++j)
        if (!g.ovl[g.nb_id[j]]) add(g.nb_id[j]);
    }
  }
  r.req_rows.resize(n_src);
  for (uint32_t i = 0; i < n_src; ++i) r.req_rows[i] = row_of[srcs[i]];
  return r;
}

NhLayout plan_nh_layout(const GraphHost& g, const uint32_t* srcs, uint32_t n_src) {
  NhLayout l;
  l.nh_off.resize(n_src);
  l.words.resize(n_src);
  uint64_t off = 0;
  for (uint32_t i = 0; i < n_src; ++i) {
    const uint32_t k = g.nb_ptr[srcs[i] + 1] - g.nb_ptr[srcs[i]];
    l.words[i] = k;  // one destination bitmap per distinct up neighbour
    l.nh_off[i] = off;
    off += (uint64_t)k * (g.pitch / 32);
    l.wmax = std::max(l.wmax, (k + 31) / 32);
  }
  l.nh_total = off;
  return l;
}

NbRows plan_nb_rows(const GraphHost& g, const uint32_t* srcs, uint32_t n_src,
                    const std::vector<uint32_t>& row_of, uint64_t stride, size_t rows) {
  NbRows nb;
  nb.nb_row_off.resize(n_src);
  nb.nb_drained.assign(n_src, 0);
  const uint32_t dead = stride ? (uint32_t)(rows * stride) : kInf;
  nb.dead = dead;
  std::vector<uint32_t>& nb_row = nb.nb_row;
  for (uint32_t i = 0; i < n_src; ++i) {
    nb.nb_row_off[i] = (uint32_t)nb_row.size();
    for (uint32_t e = g.nb_ptr[srcs[i]]; e < g.nb_ptr[srcs[i] + 1]; ++e) {
      const uint32_t x = g.nb_id[e];
      const bool dr = g.ovl[x] != 0;
      nb_row.push_back(dr ? dead : stride ? (uint32_t)(row_of[x] * stride) : row_of[x]);
      nb.nb_drained[i] += dr;
    }
    const size_t k = nb_row.size() - nb.nb_row_off[i];
    nb_row.resize(nb.nb_row_off[i] + (k + 7) / 8 * 8 + 8, dead);
  }
  return nb;
}

ClassRows plan_class_rows(const GraphHost& g, const std::vector<uint32_t>& closure) {
  ClassRows cr;
  const std::vector<uint16_t>& cls = g.qt.cls;
  cr.fwd.assign(g.qt.n_cls, 0);
  for (uint32_t v = 0; v < g.N; ++v)
    if (!g.ovl[v]) cr.fwd[cls[v]] = 1;
  std::vector<uint32_t> src_of(g.qt.n_cls, kInf);  // class -> its class source
  cr.crow_of.resize(closure.size());
  for (size_t r = 0; r < closure.size(); ++r) {
    uint32_t& k = src_of[cls[closure[r]]];
    if (k == kInf) {
      k = (uint32_t)cr.csrc.size();
      cr.csrc.push_back(closure[r]);
    }
    cr.crow_of[r] = k;
  }
  return cr;
}

ExpandGrid plan_expand_grid(uint32_t rows, uint32_t span, uint32_t resident) {
  ExpandGrid eg;
  eg.groups = (rows + kExRows - 1) / kExRows;
  eg.pieces = (span + kExPiece - 1) / kExPiece;
  resident = std::max(1u, resident);
  eg.pps = std::max(1u, eg.pieces);
  if (eg.groups >= resident) {
    eg.gper = (eg.groups + resident - 1) / resident;
    eg.wgs = (eg.groups + eg.gper - 1) / eg.gper;
  } else {
    eg.wgs = std::max(1u, eg.groups);
    const uint32_t want = std::min(eg.pps, resident / eg.wgs);
    eg.pps = (eg.pps + want - 1) / want;
    eg.splits = (std::max(1u, eg.pieces) + eg.pps - 1) / eg.pps;
  }
  return eg;
}

XcdLists plan_xcd_lists(const std::vector<uint32_t>& words, uint32_t runs) {
  XcdLists x;
  const uint32_t n_src = (uint32_t)words.size();
  if (runs == 0) {  // plain round-robin
    for (uint32_t i = 0; i < n_src; ++i) x.list[i % 8].push_back(i);
  } else {
    // (runs come in request order: the heavy spine and fabric switches first)
    uint64_t total = 0, load[8] = {};
    for (uint32_t i = 0; i < n_src; ++i) total += words[i] + 1;
    const uint64_t target = std::max<uint64_t>(1, total / (8ull * runs));
    for (uint32_t i = 0; i < n_src;) {
      uint32_t e = i;
      uint64_t w = 0;
      while (e < n_src && w < target) w += words[e++] + 1;
      const int g = (int)(std::min_element(load, load + 8) - load);
      load[g] += w;
      for (uint32_t t = i; t < e; ++t) x.list[g].push_back(t);
      i = e;
    }
  }
  size_t most = 0;
  for (const auto& l : x.list) most = std::max(most, l.size());
  x.slot.assign(most * 8, kInf);
  for (int g = 0; g < 8; ++g)
    for (size_t t = 0; t < x.list[g].size(); ++t) x.slot[t * 8 + g] = x.list[g][t];
  x.slots = x.slot.size();
  if (x.slot.empty()) x.slot.push_back(kInf);
  return x;
}

uint32_t plan_sliced_unit(const std::vector<uint32_t>& words, uint32_t chunks, uint32_t n_cu) {
  // small plans (a rank's share of a multi-GPU pass) get smaller units so
  // the waves still cover the chip
  uint64_t matches = 0;
  for (uint32_t k : words) matches += (uint64_t)k * chunks;
  return (uint32_t)std::min<uint64_t>(kSlUnit, std::max<uint64_t>(16, matches / (16ull * n_cu) / 8 * 8));
}

// Per XCD, in the XCD's source order: a source whose neighbour-chunk matches
// fit `unit` is one unit, a heavier one is cut per chunk and per neighbour
// range (multiples of kSlSeg: the row offset lists are read 16-byte aligned).
// Grouped units: neighbour positions are cut into segments of kSlSeg;
// sources of one XCD list whose segment q holds the same rows (none
// drained) share it -- one wave loads each of those rows once for up
// to kSlGroup sources.  Whole lists match for a pod's rack switches and
// a plane's spines; a fabric switch's list is [its plane's spines][its
// pod's rack switches], so the fabric switches of one plane share the
// first part and those of one pod the second.  Consecutive segments of
// one member set merge into one range; what no group takes stays with
// per-source units.
SlicedUnits plan_sliced_units(const std::vector<uint32_t> (&list)[8], const std::vector<uint32_t>& words,
                              const NbRows& nb, uint32_t chunks, uint32_t unit, int group) {
  SlicedUnits s;
  std::vector<uint32_t>& units = s.units;
  std::vector<uint32_t>& gtab = s.gtab;
  s.unit_off.assign(9, 0);
  const uint32_t dead = nb.dead;
  for (int g = 0; g < 8; ++g) {
    s.unit_off[g] = (uint32_t)(units.size() / 4);
    // per source of the list: which segments a group took
    std::map<uint32_t, std::vector<uint8_t>> taken;
    // member set -> segments (q, end position) it shares
    std::map<std::vector<uint32_t>, std::vector<std::pair<uint32_t, uint32_t>>> shared;
    if (group) {
      std::map<std::vector<uint32_t>, std::vector<uint32_t>> seg;
      for (uint32_t i : list[g]) {
        const uint32_t k = words[i];
        if (!k) continue;
        const uint32_t* r = nb.nb_row.data() + nb.nb_row_off[i];
        if (group == 1) {  // the whole list as one key
          if (nb.nb_drained[i]) continue;
          std::vector<uint32_t> key{0u, k};
          key.insert(key.end(), r, r + k);
          seg[key].push_back(i);
          continue;
        }
        for (uint32_t q = 0; q * kSlSeg < k; ++q) {
          const uint32_t j = q * kSlSeg, e = std::min(k, j + kSlSeg);
          bool dead_in = false;
          for (uint32_t jj = j; jj < e; ++jj) dead_in |= r[jj] == dead;
          if (dead_in) continue;
          std::vector<uint32_t> key{q, e};
          key.insert(key.end(), r + j, r + e);
          seg[key].push_back(i);
        }
      }
      for (auto& kv : seg) {
        const auto& src = kv.second;
        for (size_t a = 0; a + 1 < src.size(); a += kSlGroup) {
          const size_t b = std::min(src.size(), a + kSlGroup);
          if (b - a < 2) break;
          std::vector<uint32_t> m(src.begin() + a, src.begin() + b);
          const uint32_t q = kv.first[0], e = kv.first[1];
          if (group == 1) {  // whole list: every segment of it
            for (uint32_t qq = 0; qq * kSlSeg < e; ++qq)
              shared[m].emplace_back(qq, std::min(e, (qq + 1) * kSlSeg));
          } else {
            shared[m].emplace_back(q, e);
          }
          for (uint32_t i : m) {
            auto& t = taken[i];
            if (t.empty()) t.assign((words[i] + kSlSeg - 1) / kSlSeg, 0);
            if (group == 1)
              std::fill(t.begin(), t.end(), 1);
            else
              t[q] = 1;
          }
        }
      }
    }
    // group units: per member set, runs of consecutive segments, per
    // chunk, ranges of about `unit` matches (multiples of kSlSeg)
    for (auto& kv : shared) {
      auto& segs = kv.second;
      std::sort(segs.begin(), segs.end());
      const uint32_t gs = (uint32_t)kv.first.size();
      const uint32_t goff = (uint32_t)gtab.size();
      gtab.push_back(gs);
      gtab.insert(gtab.end(), kv.first.begin(), kv.first.end());
      for (size_t a = 0; a < segs.size();) {
        size_t b = a + 1;
        while (b < segs.size() && segs[b].first == segs[b - 1].first + 1) ++b;
        const uint32_t j0 = segs[a].first * kSlSeg, j1 = segs[b - 1].second;
        const uint32_t parts = (uint32_t)(((uint64_t)(j1 - j0) * gs + unit - 1) / unit);
        const uint32_t jstep = ((j1 - j0 + parts - 1) / parts + kSlSeg - 1) / kSlSeg * kSlSeg;
        for (uint32_t ch = 0; ch < chunks; ++ch)
          for (uint32_t j = j0; j < j1; j += jstep)
            units.insert(units.end(), {goff, ch | (1u << 31), j, std::min(j1, j + jstep)});
        a = b;
      }
    }
    // per-source units over what no group took
    for (uint32_t i : list[g]) {
      const uint32_t k = words[i];
      if (k == 0) continue;
      const auto it = taken.find(i);
      const std::vector<uint8_t>* t = it == taken.end() ? nullptr : &it->second;
      for (uint32_t q = 0; q * kSlSeg < k;) {
        if (t && (*t)[q]) {
          ++q;
          continue;
        }
        uint32_t q1 = q + 1;
        while (q1 * kSlSeg < k && !(t && (*t)[q1])) ++q1;
        const uint32_t j0 = q * kSlSeg, j1 = std::min(k, q1 * kSlSeg), kr = j1 - j0;
        if ((uint64_t)kr * chunks <= unit) {
          units.insert(units.end(), {i, 0u | (chunks << 16), j0, j1});
        } else {  // per chunk, equal ranges of <= unit neighbours (multiples of kSlSeg)
          const uint32_t parts = (kr + unit - 1) / unit;
          const uint32_t jstep = ((kr + parts - 1) / parts + kSlSeg - 1) / kSlSeg * kSlSeg;
          for (uint32_t ch = 0; ch < chunks; ++ch)
            for (uint32_t j = j0; j < j1; j += jstep)
              units.insert(units.end(), {i, ch | ((ch + 1) << 16), j, std::min(j1, j + jstep)});
        }
        q = q1;
      }
    }
    s.max_xcd_units = std::max(s.max_xcd_units, (uint32_t)(units.size() / 4) - s.unit_off[g]);
  }
  s.unit_off[8] = (uint32_t)(units.size() / 4);
  if (units.empty()) units.assign(4, 0);
  if (gtab.empty()) gtab.push_back(0);
  return s;
}

const std::vector<uint32_t>& ecc_estimate(const GraphHost& g, DepthCache* m) {
  if (m->ecc_epoch == g.epoch && m->ecc.size() == g.N) return m->ecc;
  const uint32_t N = g.N;
  std::vector<uint32_t> d(N), mind(N, kInf), q;
  m->ecc.assign(N, 0);
  auto bfs = [&](uint32_t r) {
    std::fill(d.begin(), d.end(), kInf);
    d[r] = 0;
    q.assign(1, r);
    for (size_t h = 0; h < q.size(); ++h) {
      const uint32_t u = q[h];
      for (uint32_t e = g.row_ptr[u]; e < g.row_ptr[u + 1]; ++e)
        if (d[g.col[e]] == kInf) {
          d[g.col[e]] = d[u] + 1;
          q.push_back(g.col[e]);
        }
    }
  };
  uint32_t land = 0;
  for (int j = 0; j < 9 && N; ++j) {
    bfs(land);
    uint32_t far = land, best = 0;
    for (uint32_t v = 0; v < N; ++v) {
      if (d[v] == kInf) continue;
      if (j > 0) m->ecc[v] = std::max(m->ecc[v], d[v]);  // landmark 0 (node 0's far end) onwards
      mind[v] = std::min(mind[v], d[v]);
      if (j == 0 ? d[v] > best : mind[v] > best) {
        best = j == 0 ? d[v] : mind[v];
        far = v;
      }
    }
    if (j == 0) std::fill(mind.begin(), mind.end(), kInf);  // node 0 is no landmark
    land = far;
  }
  m->ecc_epoch = g.epoch;
  return m->ecc;
}

std::vector<uint32_t> plan_depth_order(const std::vector<uint32_t>& closure, const std::vector<uint32_t>& ecc) {
  std::vector<uint32_t> order(closure.size());
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return ecc[closure[a]] > ecc[closure[b]]; });
  return order;
}

uint32_t depth_bound(const GraphHost& g, DepthCache* m) {
  if (m->dbound_epoch == g.epoch) return m->dbound;
  for (const auto& e : m->memo)  // the same structure and drain bits as a recent epoch
    if (e.sell_ver == g.sell_ver && e.ovl == g.ovl) {
      m->dbound = e.dbound;
      m->dbound_epoch = g.epoch;
      return m->dbound;
    }
  // one level-synchronous BFS per component over the distinct up neighbours;
  // drained nodes are neither roots nor transit, so they start out seen (one
  // byte test per edge -- recomputed after every patch, on the path of the
  // first plan build of a publication)
  const uint32_t N = g.N;
  std::vector<uint8_t> seen(N);
  for (uint32_t v = 0; v < N; ++v) seen[v] = g.ovl[v] != 0;
  std::vector<uint32_t> q(std::max<uint32_t>(N, 1));
  const uint32_t* nbp = g.nb_ptr.data();
  const uint32_t* nbi = g.nb_id.data();
  uint32_t worst = 0;
  for (uint32_t r = 0; r < N; ++r) {
    if (seen[r]) continue;
    seen[r] = 1;
    size_t head = 0, tail = 0, level_end = 1;
    q[tail++] = r;
    uint32_t ecc = 0;
    while (head < tail) {
      const uint32_t u = q[head++];
      for (uint32_t e = nbp[u]; e < nbp[u + 1]; ++e) {
        const uint32_t x = nbi[e];
        if (!seen[x]) {
          seen[x] = 1;
          q[tail++] = x;
        }
      }
      if (head == level_end && head < tail) {  // the next level starts
        ++ecc;
        level_end = tail;
      }
    }
    worst = std::max(worst, ecc);
  }
  m->dbound = 2 + 2 * worst;
  m->dbound_epoch = g.epoch;
  if (m->memo.size() >= 4) m->memo.erase(m->memo.begin());
  m->memo.push_back({g.sell_ver, g.ovl, m->dbound});
  return m->dbound;
}

}  // namespace spfi
