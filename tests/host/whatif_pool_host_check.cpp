// The device-free part of a list pool's _db call
// (openr_amd/csrc/whatif_pool_host.cpp) on the CPU: the checks of an owner's
// slice with their status codes, and the order its entries are returned in.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "whatif_pool_host.h"

using namespace spfi;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

using Order = std::vector<size_t>;

static Order order_of(const std::vector<uint32_t>& key, const std::vector<uint64_t>& val) {
  CHECK(key.size() == val.size());
  const Order o = pool_order(key.data(), val.data(), key.size());
  CHECK(o.size() == key.size());
  std::vector<int> seen(key.size(), 0);  // a permutation, ascending by (key, val)
  for (size_t k = 0; k < o.size(); ++k) {
    CHECK(o[k] < key.size() && !seen[o[k]]++);
    if (k) {
      const size_t a = o[k - 1], b = o[k];
      CHECK(key[a] < key[b] || (key[a] == key[b] && val[a] <= val[b]));
    }
  }
  return o;
}

int main() {
  const uint64_t kUntouched = 0xABCDull;
  uint64_t n = kUntouched;
  bool copy = true;
  // an empty slice: nothing to copy, whatever the room
  CHECK(pool_slice(7, 7, 20, true, 0, &n, &copy) == SPF_OK && n == 0 && !copy);
  CHECK(pool_order(nullptr, nullptr, 0).empty());
  // one entry
  CHECK(pool_slice(7, 8, 20, true, 1, &n, &copy) == SPF_OK && n == 1 && copy);
  CHECK(order_of({5}, {9}) == Order{0});
  // keys already sorted, keys reversed
  CHECK((order_of({1, 4, 6, 9}, {3, 2, 1, 0}) == Order{0, 1, 2, 3}));
  CHECK((order_of({9, 6, 4, 1}, {0, 1, 2, 3}) == Order{3, 2, 1, 0}));
  // equal keys: by value, also past 32 bits
  CHECK((order_of({2, 1, 2, 2, 1}, {1ull << 40, 7, 3, ~0ull, 6}) == Order{4, 1, 2, 0, 3}));
  // room one short of the count: SPF_E_NOMEM, the count still returned; exactly enough: fine
  n = kUntouched;
  CHECK(pool_slice(10, 15, 20, true, 4, &n, &copy) == SPF_E_NOMEM && n == 5 && !copy);
  CHECK(pool_slice(10, 15, 20, true, 5, &n, &copy) == SPF_OK && n == 5 && copy);
  // decreasing offsets, an end past the pool: SPF_E_HIP and no count
  n = kUntouched;
  CHECK(pool_slice(15, 10, 20, true, 100, &n, &copy) == SPF_E_HIP && n == kUntouched && !copy);
  CHECK(pool_slice(10, 21, 20, true, 100, &n, &copy) == SPF_E_HIP && n == kUntouched && !copy);
  CHECK(pool_slice(10, 21, 20, false, 0, &n, &copy) == SPF_E_HIP && n == kUntouched);
  CHECK(pool_slice(15, 20, 20, true, 5, &n, &copy) == SPF_OK && n == 5 && copy);  // the last owner
  // every output NULL: the count only, no room needed, nothing copied
  CHECK(pool_slice(10, 15, 20, false, 0, &n, &copy) == SPF_OK && n == 5 && !copy);
  CHECK(pool_slice(10, 15, 20, true, 5, nullptr, &copy) == SPF_OK && copy);  // no count asked for
  // seeded slices against the property
  std::mt19937_64 rng(3);
  for (int round = 0; round < 50; ++round) {
    std::vector<uint32_t> key(rng() % 200);
    std::vector<uint64_t> val(key.size());
    for (auto& k : key) k = (uint32_t)(rng() % 16);
    for (auto& v : val) v = rng() % 4 ? rng() : ~0ull;
    order_of(key, val);
  }
  std::puts("whatif_pool_host_check: ok");
  return 0;
}
