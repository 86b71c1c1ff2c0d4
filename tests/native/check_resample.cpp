// check_resample.cpp — the host routine and table builder of csrc/tfp_resample.hpp, stand-alone: the
// plan's shape, the table's sums, the per-sample routine against a plain restatement with bounds
// checked reads, at the clips' edges and with n * M beyond 2^31 and 2^40. Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all and run on the CPU: any finding aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfp_resample.hpp"

namespace tfp {
// (tfp_resample.cpp's cache is not linked here; the checks build their tables themselves)
std::shared_ptr<const ResampleTable> resample_table(int32_t, int32_t, bool*) { return nullptr; }
}  // namespace tfp

using namespace tfp;

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      return 1;                                                     \
    }                                                               \
  } while (0)

static bool table_of(int32_t rin, int32_t rout, ResampleTable* t) {
  bool bad = false;
  return resample_plan(rin, rout, &t->plan, &bad) && resample_build(t->plan, &t->taps);
}

// The definition, read by read: x(i) is 0 outside [0, n_in).
static int16_t restate(const ResampleTable& t, const std::vector<int16_t>& x, int64_t n) {
  const ResamplePlan& P = t.plan;
  const __int128 nm = (__int128)n * P.M;
  const int64_t i0 = (int64_t)(nm / P.L), p = (int64_t)(nm % P.L);
  __int128 acc = 0;
  for (int32_t j = 0; j < P.ntaps; j++) {
    const int64_t i = i0 + P.k_lo + j;
    const int64_t xv = i >= 0 && i < (int64_t)x.size() ? x.at((size_t)i) : 0;
    acc += (__int128)t.taps.at((size_t)(p * P.ntaps + j)) * xv;
  }
  __int128 y = (acc + 16384) >> 15;
  return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}

static uint32_t rng_state = 12345u;
static int16_t rnd16() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (int16_t)(rng_state >> 16);
}

int main() {
  // plans: the shapes of the issue's table, the refusals
  const int32_t shapes[][5] = {{16000, 8000, 1, 2, 97},   {48000, 8000, 1, 6, 289},   {96000, 8000, 1, 12, 577},
                               {8000, 16000, 2, 1, 49},   {44100, 8000, 80, 441, 266}, {11025, 8000, 320, 441, 68},
                               {44100, 48000, 160, 147, 49}, {8001, 8000, 8000, 8001, 50}};
  for (const auto& s : shapes) {
    ResamplePlan P;
    bool bad = true;
    CHECK(resample_plan(s[0], s[1], &P, &bad) && !bad);
    CHECK(P.L == s[2] && P.M == s[3] && P.ntaps == s[4]);
  }
  {
    ResamplePlan P;
    bool bad = false;
    CHECK(!resample_plan(7999, 44100, &P, &bad) && !bad);
    CHECK(!resample_plan(0, 8000, &P, &bad) && bad);
    CHECK(!resample_plan(8000, -1, &P, &bad) && bad);
    CHECK(!resample_plan(1, 1000000, &P, &bad) && !bad);
    CHECK(resample_plan(1000000, 1000000, &P, &bad) && P.L == 1 && P.M == 1 && P.ntaps == 49);
  }
  // counts: the edges, and the refusal where n_in L + M leaves int64
  {
    ResamplePlan P{80, 441, -132, 266};
    CHECK(resample_count(P, 0) == 0 && resample_count(P, -3) == 0 && resample_count(P, 1) == 1);
    CHECK(resample_count(P, 441) == 80 && resample_count(P, 442) == 81 && resample_count(P, 440) == 80);
    CHECK(resample_count(P, INT64_MAX / 80) == -1);
    CHECK(resample_count(P, (INT64_MAX - 441) / 80) > 0);
  }
  const int32_t pairs[][2] = {{16000, 8000}, {8000, 16000}, {44100, 8000}, {11025, 8000}, {96000, 8000}, {8001, 8000}};
  for (const auto& pr : pairs) {
    ResampleTable t;
    CHECK(table_of(pr[0], pr[1], &t));
    for (int32_t p = 0; p < t.plan.L; p++) {
      int64_t sum = 0;
      for (int32_t j = 0; j < t.plan.ntaps; j++) sum += t.taps.at((size_t)p * t.plan.ntaps + j);
      CHECK(sum == 32768);
    }
    const int64_t lens[] = {0, 1, 2, t.plan.ntaps - 1, t.plan.ntaps, 1500};
    for (int64_t n_in : lens) {
      std::vector<int16_t> x((size_t)n_in);  // exactly n_in samples: a read past either end is a finding
      for (auto& v : x) v = rnd16();
      if (n_in > 3) x[0] = -32768, x[1] = -32768, x[(size_t)n_in - 1] = 32767;
      const int64_t n_out = resample_count(t.plan, n_in);
      std::vector<int16_t> y((size_t)n_out);
      resample_clip(t, x.data(), n_in, y.data());
      for (int64_t n = 0; n < n_out; n++) CHECK(y[(size_t)n] == restate(t, x, n));
      // a staged span: the samples [lo, hi) of the clip with zeros past its ends, as the kernel stages them
      if (n_out > 0) {
        const int64_t n0 = n_out / 3, n1 = n_out;
        const int64_t lo = (n0 * t.plan.M) / t.plan.L + t.plan.k_lo, hi = ((n1 - 1) * t.plan.M) / t.plan.L + t.plan.k_lo + t.plan.ntaps;
        std::vector<int16_t> span((size_t)(hi - lo));
        for (int64_t s = lo; s < hi; s++) span[(size_t)(s - lo)] = s >= 0 && s < n_in ? x[(size_t)s] : (int16_t)0;
        for (int64_t n = n0; n < n1; n++) CHECK(resample_sample(t.plan, t.taps.data(), span.data(), lo, hi, n) == y[(size_t)n]);
      }
    }
  }
  // n * M beyond 2^31 and 2^40: a window of a virtual long clip. Only the samples [base, base + W) exist; the
  // routine is handed them as a span, and the restatement's clip is the same window shifted to 0 with the
  // output index shifted by a whole number of periods (n M = (n - dn) M + dn M, dn a multiple of L).
  for (const auto& pr : pairs) {
    ResampleTable t;
    CHECK(table_of(pr[0], pr[1], &t));
    const ResamplePlan& P = t.plan;
    for (int64_t target : {((int64_t)1 << 31) + 12345, ((int64_t)1 << 40) + 999}) {
      const int64_t periods = target / ((int64_t)P.M * P.L) + 1;
      const int64_t dn = periods * P.L, base = periods * P.M;  // output dn sits at input base, phase 0
      CHECK(dn * P.M > ((int64_t)1 << 31));
      const int64_t W = 4 * P.ntaps + 64;
      std::vector<int16_t> x((size_t)W);
      for (auto& v : x) v = rnd16();
      const int64_t n_out = resample_count(P, W);
      for (int64_t n = 0; n < n_out; n++)
        CHECK(resample_sample(P, t.taps.data(), x.data(), base, base + W, dn + n) == restate(t, x, n));
    }
  }
  // rounding and clamp
  CHECK(resample_round(0) == 0 && resample_round(16383) == 0 && resample_round(16384) == 1);
  CHECK(resample_round(-16384) == 0 && resample_round(-16385) == -1);
  CHECK(resample_round((int64_t)40000 << 15) == 32767 && resample_round(-((int64_t)40000 << 15)) == -32768);
  CHECK(resample_round((int64_t)70208 * 32768) == 32767 && resample_round(-(int64_t)70208 * 32768) == -32768);
  // tiles
  {
    const int64_t off[] = {0, 0, 1, 1 + kRsTile, 2 + 2 * kRsTile + 1 + kRsTile};
    std::vector<int32_t> toff, tclip;
    resample_tiles(off, 4, &toff, &tclip);
    CHECK(toff == (std::vector<int32_t>{0, 0, 1, 2, 5}));
    CHECK(tclip == (std::vector<int32_t>{1, 2, 3, 3, 3}));
  }
  std::printf("OK\n");
  return 0;
}
