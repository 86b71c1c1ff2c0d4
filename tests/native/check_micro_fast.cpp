// tfp_math.hpp micro_of_coef_fast() against this host's glibc: for a float c the stored micro-units are
// micro_of_db(10.0 * log10(fabs((double)c))) (fp_handler.c:651, db_ctx_handler.c:479-481). Wherever the
// fast finish decides, its value must be that one; with micro_of_db(db_of_coef(c)) (the kernels' slow
// branch) where it does not, the result must be that one everywhere. Walks every float bit pattern
// u = 0, stride, 2 stride, ... < 2^32 (stride 1: all of them; tests/test_micro_fast.py runs a sampled
// stride), then the patterns of micro_fast_subset.hpp. With stride 1 it also prints the patterns whose
// value lies nearest a half-micro boundary (the list file of later runs).
// usage: check_micro_fast <stride> [list-file]
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "../../asterisk-tiresias_amd/csrc/tfp_math.hpp"
#include "micro_fast_subset.hpp"

using namespace tfp;

struct Tally {
  uint64_t n = 0, finite = 0, undecided = 0, bad_decided = 0, bad_combined = 0, null_undecided = 0;
};

static inline void check_one(uint32_t u, Tally& t) {
  const float c = u2f(u);
  const int32_t want = micro_of_db(10.0 * log10(fabs((double)c)));
  bool und = true;
  const int32_t fast = micro_of_coef_fast(c, &und);
  const int32_t got = und ? micro_of_db(db_of_coef(c)) : fast;
  const uint32_t a = u & 0x7fffffffu;
  t.n++;
  t.finite += a != 0 && a < 0x7f800000u;
  t.undecided += und;
  t.bad_decided += !und && fast != want;
  t.bad_combined += got != want;
  t.null_undecided += und && (a == 0 || a >= 0x7f800000u);  // zeros, inf, NaN are decided from their bits
}

int main(int argc, char** argv) {
  const uint64_t stride = argc > 1 ? strtoull(argv[1], 0, 10) : 1;
  const char* list = argc > 2 ? argv[2] : nullptr;
  if (stride == 0) return 2;
  omp_set_num_threads(std::min(16, omp_get_max_threads()));
  const int64_t steps = (int64_t)((0xffffffffull / stride) + 1);
  uint64_t n = 0, finite = 0, undecided = 0, bad_decided = 0, bad_combined = 0, null_undecided = 0;
  std::vector<std::pair<double, uint32_t>> near;  // (distance from the boundary in micro-units, pattern)
#pragma omp parallel
  {
    Tally t;
    std::vector<std::pair<double, uint32_t>> mine;
#pragma omp for schedule(static)
    for (int64_t k = 0; k < steps; k++) {
      const uint32_t u = (uint32_t)((uint64_t)k * stride);
      check_one(u, t);
      if (stride == 1 && (u & 0x7fffffffu) - 0x00800000u < 0x7f000000u) {  // positive and negative normals
        // glibc's value times 10^6 as p + pe exactly (fmt6's two_prod); p - rint(p) is exact
        const double q = 10.0 * log10(fabs((double)u2f(u)));
        const double p = q * 1e6, pe = __builtin_fma(q, 1e6, -p);
        const double dd = p - rint(p);
        const double d = fabs((fabs(dd) - 0.5) + (dd < 0.0 ? -pe : pe));
        if (d < 0x1p-20) mine.push_back({d, u});
      }
    }
#pragma omp critical
    {
      n += t.n, finite += t.finite, undecided += t.undecided, bad_decided += t.bad_decided;
      bad_combined += t.bad_combined, null_undecided += t.null_undecided;
      near.insert(near.end(), mine.begin(), mine.end());
    }
  }
  printf("stride %lu: %lu patterns (%lu finite non-zero)\n", (unsigned long)stride, (unsigned long)n, (unsigned long)finite);
  printf("decided but != glibc : %lu\n", (unsigned long)bad_decided);
  printf("with the slow path where undecided, != glibc : %lu\n", (unsigned long)bad_combined);
  printf("undecided : %lu (%.3e of the finite non-zero), zeros/inf/NaN undecided : %lu\n", (unsigned long)undecided,
         finite ? (double)undecided / (double)finite : 0.0, (unsigned long)null_undecided);
  uint64_t bad = bad_decided + bad_combined + null_undecided;

  const std::vector<uint32_t> extra = micro_fast_extras(list);
  if (extra.empty()) bad++;
  Tally x;
  for (uint32_t u : extra) check_one(u, x);
  printf("listed patterns: %lu, decided but != glibc : %lu, combined != glibc : %lu, undecided : %lu\n",
         (unsigned long)x.n, (unsigned long)x.bad_decided, (unsigned long)x.bad_combined, (unsigned long)x.undecided);
  bad += x.bad_decided + x.bad_combined + x.null_undecided;

  if (stride == 1) {
    std::sort(near.begin(), near.end());
    const size_t keep = std::min<size_t>(near.size(), 64);
    printf("nearest a half-micro boundary (of %lu within 2^-20):\n", (unsigned long)near.size());
    for (size_t i = 0; i < keep; i++) printf("near 0x%08x %.3e\n", near[i].second, near[i].first);
  }
  printf("%s\n", bad ? "FAIL" : "OK");
  return bad ? 1 : 0;
}
