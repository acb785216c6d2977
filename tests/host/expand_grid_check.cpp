// plan_expand_grid (plan_host.cpp) on the CPU: the workgroups of the expansion
// kernel's grid cover every row group and every piece of the row width exactly
// once, whatever the rows, the width and the chip; a plan with fewer groups
// than the chip holds workgroups splits the width.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "plan_host.h"

using namespace spfi;

static int failures = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      std::printf("FAIL " __VA_ARGS__); \
      std::printf("\n");                \
      ++failures;                       \
    }                                   \
  } while (0)

static void one(uint32_t rows, uint32_t span, uint32_t cus, uint32_t per_cu) {
  const uint32_t resident = cus * per_cu;
  const ExpandGrid eg = plan_expand_grid(rows, span, resident);
  const uint32_t groups = (rows + kExRows - 1) / kExRows, pieces = (span + kExPiece - 1) / kExPiece;
  CHECK(eg.groups == groups && eg.pieces == pieces, "counts rows=%u span=%u", rows, span);
  CHECK(eg.wgs >= 1 && eg.splits >= 1 && eg.gper >= 1 && eg.pps >= 1, "empty grid rows=%u span=%u", rows, span);
  std::vector<uint32_t> hit((size_t)groups * pieces, 0), row_hit(rows, 0), node_hit(span, 0);
  for (uint32_t x = 0; x < eg.wgs; ++x)
    for (uint32_t y = 0; y < eg.splits; ++y) {
      // the kernel's ranges of workgroup (x, y)
      const uint32_t g0 = x * eg.gper, g1 = std::min(groups, g0 + eg.gper);
      const uint32_t p0 = y * eg.pps, p1 = std::min(pieces, p0 + eg.pps);
      CHECK(g0 < g1 && p0 < p1, "idle workgroup (%u, %u) rows=%u span=%u cus=%u", x, y, rows, span, cus);
      for (uint32_t g = g0; g < g1; ++g)
        for (uint32_t p = p0; p < p1; ++p) ++hit[(size_t)g * pieces + p];
      if (y == 0)
        for (uint32_t r = g0 * kExRows; r < std::min(rows, g1 * kExRows); ++r) ++row_hit[r];
      if (x == 0)
        for (uint32_t v = p0 * kExPiece; v < std::min(span, p1 * kExPiece); ++v) ++node_hit[v];
    }
  const auto once = [](uint32_t h) { return h == 1; };
  CHECK(std::all_of(hit.begin(), hit.end(), once), "group x piece cover rows=%u span=%u cus=%u", rows, span, cus);
  CHECK(std::all_of(row_hit.begin(), row_hit.end(), once), "row cover rows=%u span=%u cus=%u", rows, span, cus);
  CHECK(std::all_of(node_hit.begin(), node_hit.end(), once), "node cover rows=%u span=%u cus=%u", rows, span, cus);
  // one round: every workgroup resident from the start
  CHECK((uint64_t)eg.wgs * eg.splits <= resident, "more workgroups than the chip holds rows=%u span=%u cus=%u",
        rows, span, cus);
  if (groups >= resident) {
    CHECK(eg.splits == 1 && eg.wgs <= resident, "full-width grid rows=%u cus=%u", rows, cus);
    // the last round is full: every workgroup but the last owns gper groups
    CHECK((uint64_t)(eg.wgs - 1) * eg.gper < groups, "tail rows=%u cus=%u", rows, cus);
  } else if (pieces > 1 && 2 * groups <= resident) {
    CHECK(eg.splits > 1, "few rows keep the width whole rows=%u span=%u cus=%u", rows, span, cus);
  }
}

int main() {
  for (uint32_t rows : {1u, 7u, 8u, 9u, 200u, 9976u})
    for (uint32_t span : {32u, 1024u, 1056u, 2208u, 2240u, 9984u, 10240u})
      for (uint32_t cus : {1u, 256u})
        for (uint32_t per_cu : {1u, 3u}) one(rows, span, cus, per_cu);
  // fabric_full on a 256-CU chip, three workgroups per CU: two groups each
  const ExpandGrid eg = plan_expand_grid(9976, 10240, 768);
  CHECK(eg.wgs == 624 && eg.gper == 2 && eg.splits == 1 && eg.pps == 40, "fabric_full grid %u %u %u %u", eg.wgs,
        eg.gper, eg.splits, eg.pps);
  // 200 rows: 25 groups, the width split
  const ExpandGrid es = plan_expand_grid(200, 10240, 768);
  CHECK(es.wgs == 25 && es.splits == 20 && es.pps == 2, "200-row grid %u %u %u", es.wgs, es.splits, es.pps);
  if (failures) return 1;
  std::printf("expand_grid_check: ok\n");
  return 0;
}
