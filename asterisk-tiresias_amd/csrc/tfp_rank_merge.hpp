// tfp_rank_merge.hpp — merge-and-keep-k of a device group's ranked search (tfp_group.cpp), as a
// plain host function with no GPU call (tests/native/check_rank_merge.cpp runs it under ASan/UBSan).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace tfp {

// keys[0, n) in any order, 0 = no row: the k greatest non-zero keys, descending, into out[0, k)
// (zero-filled past the last); returns how many rows there are. keys is reordered.
inline int32_t rank_merge_keep(unsigned long long* keys, int64_t n, int32_t k, unsigned long long* out) {
  int32_t m = 0;
  if (n > 0 && k > 0) {
    const int64_t top = std::min<int64_t>(k, n);
    std::partial_sort(keys, keys + top, keys + n, [](unsigned long long a, unsigned long long b) { return a > b; });
    while (m < top && keys[m] != 0ull) m++;
  }
  for (int32_t r = 0; r < k; r++) out[r] = r < m ? keys[r] : 0ull;
  return m;
}

}  // namespace tfp
