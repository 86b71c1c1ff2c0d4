// check_neighbour.cpp — the host side of catalog neighbours (csrc/tfp_neighbour.hpp), stand-alone:
// "k + 1 rows minus self" (neighbour_drop_self) against a plain definition, with self at every
// position, absent, fewer than k + 1 rows and k = 32; the device group's merge (each shard's first k
// rows, only the owner deleting the clip's own row, merged by rank_merge_keep) against one engine over
// all the clips, cross-shard ties included; and the row-to-frame-value map at its special values.
// Built by tests/test_neighbours_host.py under AddressSanitizer + UndefinedBehaviorSanitizer. With --map it
// prints tfp::neighbour_frame_value of the integers on stdin, for the test's comparison with Python's text parse.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "tfp_neighbour.hpp"
#include "tfp_rank_merge.hpp"

static int failures = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      failures++;                                              \
    }                                                          \
  } while (0)

// The definition: delete self from the whole list, read the first k.
static std::vector<int32_t> plain(const std::vector<int32_t>& all, int32_t self, int32_t k) {
  std::vector<int32_t> out;
  for (const int32_t id : all)
    if (id != self && (int32_t)out.size() < k) out.push_back(id);
  return out;
}

static void check_drop(const std::vector<int32_t>& all, int32_t self, int32_t k) {
  const int32_t n = (int32_t)std::min<size_t>(all.size(), (size_t)k + 1);  // what a search at k + 1 returns
  std::vector<int32_t> keep((size_t)k), got;
  const int32_t m = tfp::neighbour_drop_self(all.data(), n, self, k, keep.data());
  CHECK(m >= 0 && m <= k);
  for (int32_t r = 0; r < m; r++) {
    CHECK(keep[r] >= 0 && keep[r] < n);
    got.push_back(all[keep[r]]);
  }
  CHECK(got == plain(all, self, k));
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--map")) {  // stdin: one int32 per line; stdout: the frame value as a hex float
    long long m;
    while (scanf("%lld", &m) == 1) printf("%a\n", tfp::neighbour_frame_value((int32_t)m));
    return 0;
  }
  // drop_self: lists of 0 .. 40 distinct clips, k = 1, 3, 31, 32, self at every position and absent
  for (const int32_t k : {1, 3, 31, 32})
    for (int32_t len = 0; len <= 40; len++) {
      std::vector<int32_t> all((size_t)len);
      for (int32_t i = 0; i < len; i++) all[i] = 100 + i;
      check_drop(all, 7, k);   // absent
      check_drop(all, -1, k);  // no clip to drop
      for (int32_t pos = 0; pos < len; pos++) check_drop(all, all[pos], k);
    }

  // the group merge: clips with (count, tie key) spread over 3 shards, counts tied across shards
  for (int trial = 0; trial < 200; trial++) {
    const int32_t nclips = 1 + (int32_t)(rnd() % 80), k = trial % 4 == 0 ? 32 : 1 + (int32_t)(rnd() % 32);
    std::vector<unsigned long long> key((size_t)nclips);
    std::vector<int> shard((size_t)nclips);
    for (int32_t c = 0; c < nclips; c++) {
      const uint32_t count = rnd() % 4;  // 0: the clip has no row; few values: ties everywhere
      key[c] = count ? ((unsigned long long)count << 32) | (uint32_t)(c * 7 + 1) : 0ull;
      shard[c] = (int)(rnd() % 3);
    }
    const int32_t self = (int32_t)(rnd() % (uint32_t)nclips);
    // one engine: every non-zero key but self's, descending, first k
    std::vector<unsigned long long> one;
    for (int32_t c = 0; c < nclips; c++)
      if (c != self && key[c]) one.push_back(key[c]);
    std::sort(one.begin(), one.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
    one.resize(std::min<size_t>(one.size(), (size_t)k));
    // the group: per shard its first k + 1 rows, the owner drops self, k kept; then the merge
    std::vector<unsigned long long> merged;
    for (int s = 0; s < 3; s++) {
      std::vector<unsigned long long> mine;
      std::vector<int32_t> ids;
      for (int32_t c = 0; c < nclips; c++)
        if (shard[c] == s && key[c]) mine.push_back(key[c]);
      std::sort(mine.begin(), mine.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
      mine.resize(std::min<size_t>(mine.size(), (size_t)k + 1));
      for (const unsigned long long q : mine) ids.push_back((int32_t)(((uint32_t)q - 1) / 7));
      std::vector<int32_t> keep((size_t)k);
      const int32_t m = tfp::neighbour_drop_self(ids.data(), (int32_t)ids.size(), shard[self] == s ? self : -1, k, keep.data());
      for (int32_t r = 0; r < m; r++) merged.push_back(mine[keep[r]]);
    }
    std::vector<unsigned long long> top((size_t)k);
    const int32_t m = tfp::rank_merge_keep(merged.data(), (int64_t)merged.size(), k, top.data());
    CHECK((size_t)m == one.size());
    for (int32_t r = 0; r < m && (size_t)r < one.size(); r++) CHECK(top[r] == one[r]);
  }

  // the frame value of a stored row
  CHECK(tfp::neighbour_frame_value(INT32_MIN) == -INFINITY);
  CHECK(tfp::neighbour_frame_value(0) == 0.0);
  CHECK(tfp::neighbour_frame_value(-37000000) == -37.0);
  CHECK(tfp::neighbour_frame_value(12345678) == strtod("12.345678", nullptr));
  CHECK(tfp::neighbour_frame_value(-1) == strtod("-0.000001", nullptr));
  CHECK(tfp::neighbour_frame_value(INT32_MAX) == strtod("2147.483647", nullptr));
  CHECK(tfp::neighbour_frame_value(INT32_MIN + 1) == strtod("-2147.483647", nullptr));
  // ... against strtod of the "%f" text on the whole input set: fractions 0, 1 and 999999 micro-units at
  // integer parts -120 .. 120 in both signs, the int32 extremes, and 100,000 seeded random int32; the key
  // (int) of the double is the decimal's truncation
  auto pin = [](int32_t m) {
    char text[32];
    const long long a = m < 0 ? -(long long)m : (long long)m;
    snprintf(text, sizeof text, "%s%lld.%06lld", m < 0 ? "-" : "", a / 1000000, a % 1000000);
    const double v = tfp::neighbour_frame_value(m);
    CHECK(v == strtod(text, nullptr));
    CHECK((long long)(int32_t)v == (m < 0 ? -(a / 1000000) : a / 1000000));
  };
  for (int32_t ip = -120; ip <= 120; ip++)
    for (const int32_t frac : {0, 1, 999999})
      for (const int32_t sign : {1, -1}) pin(ip * 1000000 + sign * frac);
  pin(INT32_MAX);
  pin(INT32_MIN + 1);
  for (int i = 0; i < 100000; i++) {
    const int32_t m = (int32_t)rnd();
    if (m != INT32_MIN) pin(m);
  }

  if (failures) return 1;
  printf("OK\n");
  return 0;
}
