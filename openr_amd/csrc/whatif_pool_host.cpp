// whatif_pool_host.cpp -- see whatif_pool_host.h.
#include "whatif_pool_host.h"

#include <algorithm>
#include <numeric>

namespace spfi {

spf_status pool_slice(uint64_t lo, uint64_t hi, uint64_t total, bool want, uint64_t cap, uint64_t* n,
                      bool* copy) {
  *copy = false;
  if (hi < lo || hi > total) return SPF_E_HIP;
  if (n) *n = hi - lo;
  if (want && cap < hi - lo) return SPF_E_NOMEM;
  *copy = want && hi > lo;
  return SPF_OK;
}

std::vector<size_t> pool_order(const uint32_t* key, const uint64_t* val, size_t m) {
  std::vector<size_t> order(m);
  std::iota(order.begin(), order.end(), (size_t)0);
  // The device order is the fill pass's atomics'.  A change or route list holds
  // a key (node, set) once per owner, so this is ascending by key; an impact
  // list holds a failure once per entry it lists, in entry order.
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return key[a] != key[b] ? key[a] < key[b] : val[a] < val[b];
  });
  return order;
}

}  // namespace spfi
