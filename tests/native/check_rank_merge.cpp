// check_rank_merge.cpp — the device group's merge-and-keep-k (csrc/tfp_rank_merge.hpp), host code
// with no GPU call, against a sort of the whole list; built with ASan + UBSan by
// tests/test_rank_merge.py. Prints OK.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "tfp_rank_merge.hpp"

static uint64_t rng_state = 0x7153A1ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

int main() {
  long cases = 0;
  for (int k = 1; k <= 32; k++) {
    for (int n = 0; n <= 3 * 32 + 1; n += (n < 6 ? 1 : 5)) {
      for (int zeros = 0; zeros < 3; zeros++) {
        // n keys as n / k shards would return them: distinct non-zero keys, some slots 0 (no row)
        std::vector<unsigned long long> keys(n);
        for (int i = 0; i < n; i++) {
          const bool z = zeros == 2 || (zeros == 1 && rnd() % 3 == 0);
          keys[i] = z ? 0ull : ((rnd() % 5 + 1) << 32) | (unsigned long long)(i + 1);  // few counts: many ties
        }
        std::vector<unsigned long long> ref(keys);
        std::sort(ref.begin(), ref.end(), std::greater<unsigned long long>());
        std::vector<unsigned long long> out(k, ~0ull);
        const int32_t m = tfp::rank_merge_keep(keys.data(), n, k, out.data());
        int32_t want = 0;
        while (want < k && want < n && ref[want]) want++;
        if (m != want) {
          printf("k %d n %d: %d rows, expected %d\n", k, n, m, want);
          return 1;
        }
        for (int r = 0; r < k; r++)
          if (out[r] != (r < want ? ref[r] : 0ull)) {
            printf("k %d n %d: row %d\n", k, n, r);
            return 1;
          }
        cases++;
      }
    }
  }
  unsigned long long none[1] = {~0ull};
  if (tfp::rank_merge_keep(nullptr, 0, 1, none) != 0 || none[0] != 0ull) return 1;
  printf("%ld cases OK\n", cases);
  return 0;
}
