// check_resample_wide.cpp — the wide (int32 Q31) routines of csrc/tfp_resample.hpp, stand-alone: the host clip
// routine against an independent __int128 sum with bounds checked reads (zero-length, one-frame and shorter-
// than-the-filter clips, full scale at 32 channels), the routine over a staged span (int32 samples for one
// channel, int64 sums for several: the kernel's staging arithmetic run on the host) against the routine over
// the whole clip for every tile of a 2-tile clip, the per-tap form, the widening identity against the int16
// routines, the rounding, the mean, the range bound and the float maps. Built with
// -fsanitize=address,undefined -fno-sanitize-recover=all and run on the CPU: any finding aborts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
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
  if (!resample_plan(rin, rout, &t->plan, &bad) || !resample_build(t->plan, &t->taps)) return false;
  t->abs_sum = resample_abs_sum(t->plan, t->taps);
  return true;
}

static int64_t floor_div(__int128 a, __int128 b) {  // b > 0
  __int128 q = a / b;
  if (a % b < 0) q--;
  return (int64_t)q;
}

static int16_t clamp16(int64_t y) { return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y); }

// The definition, read by read: frame i is 0 outside [0, n_in).
static int16_t restate(const ResampleTable& t, const std::vector<int32_t>& x, int32_t C, int64_t n) {
  const ResamplePlan& P = t.plan;
  const int64_t n_in = (int64_t)x.size() / C;
  const __int128 nm = (__int128)n * P.M;
  const int64_t i0 = (int64_t)(nm / P.L), p = (int64_t)(nm % P.L);
  __int128 acc = 0;
  for (int32_t j = 0; j < P.ntaps; j++) {
    const int64_t i = i0 + P.k_lo + j;
    __int128 S = 0;
    if (i >= 0 && i < n_in)
      for (int32_t c = 0; c < C; c++) S += x.at((size_t)(i * C + c));
    acc += (__int128)t.taps.at((size_t)(p * P.ntaps + j)) * S;
  }
  return clamp16(floor_div(acc + ((__int128)1 << 30) * C, ((__int128)1 << 31) * C));
}

static uint32_t rng_state = 4242u;
static int32_t rnd32() {
  rng_state = rng_state * 1664525u + 1013904223u;
  const uint32_t hi = rng_state;
  rng_state = rng_state * 1664525u + 1013904223u;
  return (int32_t)((hi & 0xffff0000u) | (rng_state >> 16));
}

// The kernel's staging of the frames [lo, hi) of a clip of n_in frames at x. One channel: the samples
// themselves, zeros past the clip's ends. Several: zeros, then word j of the clip's own run added to sum j / C.
static void stage_mono(const int32_t* x, int64_t n_in, int64_t lo, int64_t hi, std::vector<int32_t>* s) {
  s->assign((size_t)(hi - lo), 0);
  for (int64_t i = 0; i < hi - lo; i++) {
    const int64_t f = lo + i;
    (*s)[(size_t)i] = f >= 0 && f < n_in ? x[f] : 0;
  }
}
static void stage_sums(const int32_t* x, int64_t n_in, int32_t C, int64_t lo, int64_t hi, std::vector<int64_t>* sums) {
  sums->assign((size_t)(hi - lo), 0);
  const int64_t fa = lo > 0 ? lo : 0, fb = hi < n_in ? hi : n_in;
  if (fb <= fa) return;
  const int32_t* xs = x + fa * C;
  const int32_t total = (int32_t)(fb - fa) * C;
  for (int32_t j = 0; j < total; j++) {
    const int32_t f = (int32_t)((uint32_t)j / (uint32_t)C);
    if (f >= (int32_t)(fb - fa)) std::abort();
    sums->at((size_t)(fa - lo + f)) += (int64_t)xs[j];
  }
}

int main() {
  const int64_t two30 = (int64_t)1 << 30, two31 = (int64_t)1 << 31;
  // rounding: the floor, the tie, the clamp; against the int16 rounding on acc << 16
  CHECK(resample_wide_round(0, 2) == 0 && resample_wide_round(-5 * two31, 3) == -2 && resample_wide_round(-3 * two31, 2) == -1);
  CHECK(resample_wide_round(-1 * two31, 2) == 0 && resample_wide_round(1 * two31, 2) == 1 && resample_wide_round(5 * two31, 3) == 2);
  CHECK(resample_wide_round(two30 - 1, 1) == 0 && resample_wide_round(two30, 1) == 1 && resample_wide_round(-two30 - 1, 1) == -1);
  CHECK(resample_wide_round(((int64_t)1 << 61) - 1, 32) == 32767 && resample_wide_round(-((int64_t)1 << 61), 32) == -32768);
  CHECK(resample_wide_round(((int64_t)1 << 61) - 1, 1) == 32767 && resample_wide_round(-((int64_t)1 << 61), 1) == -32768);
  for (int64_t a = -200000; a <= 200000; a += 37)
    for (int32_t C : {1, 2, 3, 32}) CHECK(resample_wide_round(a * 65536, C) == resample_mix_round(a, C));
  // the mean: half up, the clamp at Q31 full scale, against the int16 mean on S << 16
  CHECK(resample_wide_mean(INT32_MAX, 1) == 32767 && resample_wide_mean(INT32_MIN, 1) == -32768);
  CHECK(resample_wide_mean((int64_t)32 * INT32_MAX, 32) == 32767 && resample_wide_mean((int64_t)32 * INT32_MIN, 32) == -32768);
  CHECK(resample_wide_mean(32768, 1) == 1 && resample_wide_mean(32767, 1) == 0 && resample_wide_mean(-32768, 1) == 0 &&
        resample_wide_mean(-32769, 1) == -1);
  for (int32_t S = -3000; S <= 3000; S += 7)
    for (int32_t C : {2, 3, 32}) CHECK(resample_wide_mean((int64_t)S * 65536, C) == resample_mix_mean(S, C));
  // the float maps
  CHECK(q31_from_f32(1.0f) == INT32_MAX && q31_from_f32(-1.0f) == INT32_MIN && q31_from_f32(0.5f) == (1 << 30));
  CHECK(q31_from_f32(std::numeric_limits<float>::quiet_NaN()) == 0 && q31_from_f32(std::numeric_limits<float>::infinity()) == INT32_MAX);
  CHECK(q31_from_f32(-std::numeric_limits<float>::infinity()) == INT32_MIN && q31_from_f32(std::numeric_limits<float>::denorm_min()) == 0);
  CHECK(q31_from_f32(3.4e38f) == INT32_MAX && q31_from_f32(-3.4e38f) == INT32_MIN);
  CHECK(q31_from_f64(1.0) == INT32_MAX && q31_from_f64(-1.0) == INT32_MIN && q31_from_f64(std::ldexp(3.0, -32)) == 2);
  CHECK(q31_from_f64(std::ldexp(1.0, -32)) == 0 && q31_from_f64(std::ldexp(5.0, -32)) == 2 && q31_from_f64(std::ldexp(-3.0, -32)) == -2);
  CHECK(q31_from_f64(std::numeric_limits<double>::quiet_NaN()) == 0 && q31_from_f64(1e300) == INT32_MAX && q31_from_f64(-1e300) == INT32_MIN);
  CHECK(q31_from_f64(1.0 - std::ldexp(1.0, -32)) == INT32_MAX && q31_from_f64(std::numeric_limits<double>::denorm_min()) == 0);

  const int32_t pairs[][2] = {{16000, 8000}, {8000, 16000}, {44100, 8000}, {11025, 8000}};
  const int32_t chans[] = {1, 2, 3, 6, 32};
  for (const auto& pr : pairs) {
    ResampleTable t;
    CHECK(table_of(pr[0], pr[1], &t));
    const ResamplePlan& P = t.plan;
    CHECK(t.abs_sum >= 32768 && resample_wide_in_range(t, 32));  // (every phase sums to 32768)
    const int64_t two_tiles = ((int64_t)(kRsTile + 37) * P.M) / P.L + 3;  // a clip of 2 tiles
    const int64_t lens[] = {0, 1, 2, P.ntaps - 1, P.ntaps, 700, two_tiles};
    for (int32_t C : chans) {
      for (int64_t n_in : lens) {
        for (int mode = 0; mode < 4; mode++) {  // noise, all INT32_MIN, all INT32_MAX, int16 noise << 16
          if ((mode == 1 || mode == 2) && C != 32 && C != 1) continue;
          std::vector<int32_t> buf((size_t)(n_in * C));  // exactly: a read past either end is a finding
          std::vector<int16_t> narrow((size_t)(n_in * C));
          for (size_t i = 0; i < buf.size(); i++) {
            narrow[i] = (int16_t)(rnd32() >> 16);
            buf[i] = mode == 0 ? rnd32() : mode == 1 ? INT32_MIN : mode == 2 ? INT32_MAX : (int32_t)narrow[i] * 65536;
          }
          const int32_t* x = buf.data();
          const int64_t n_out = resample_count(P, n_in);
          CHECK(n_in > 0 || n_out == 0);
          std::vector<int16_t> y((size_t)n_out);
          resample_wide_clip(t, x, n_in, C, y.data());
          for (int64_t n = 0; n < n_out; n++) {
            CHECK(y[(size_t)n] == restate(t, buf, C, n));
            CHECK(resample_wide_sample_frames(P, t.taps.data(), x, n_in, n, C) == y[(size_t)n]);
          }
          if (mode == 3) {  // the widening identity
            std::vector<int16_t> m((size_t)n_out);
            resample_mix_clip(t, narrow.data(), n_in, C, m.data());
            CHECK(m == y);
            if (C == 1) {
              resample_clip(t, narrow.data(), n_in, m.data());
              CHECK(m == y);
            }
          }
          // every tile: the staged span against the whole clip
          const int64_t ntiles = (n_out + kRsTile - 1) / kRsTile;
          CHECK(n_in != two_tiles || ntiles == 2);
          for (int64_t tile = 0; tile < ntiles; tile++) {
            const int64_t n0 = tile * kRsTile, n1 = n0 + kRsTile < n_out ? n0 + kRsTile : n_out;
            const int64_t lo = (n0 * P.M) / P.L + P.k_lo, hi = ((n1 - 1) * P.M) / P.L + P.k_lo + P.ntaps;
            CHECK(hi - lo <= ((int64_t)(kRsTile - 1) * P.M) / P.L + 1 + P.ntaps && hi - lo <= kRsWideSpanMax);
            if (C == 1) {
              std::vector<int32_t> s;
              stage_mono(x, n_in, lo, hi, &s);
              for (int64_t n = n0; n < n1; n++) CHECK(resample_wide_sample(P, t.taps.data(), s.data(), lo, hi, n, 1) == y[(size_t)n]);
            }
            std::vector<int64_t> sums;  // (one channel through the sums as well: the routine is one template)
            stage_sums(x, n_in, C, lo, hi, &sums);
            for (int64_t n = n0; n < n1; n++) CHECK(resample_wide_sample(P, t.taps.data(), sums.data(), lo, hi, n, C) == y[(size_t)n]);
          }
        }
      }
    }
  }
  // equal rates through the identity span the downmix launch uses
  {
    const ResamplePlan I{1, 1, 0, 1};
    const int64_t n_in = kRsTile + 5;
    for (int32_t C : {2, 3, 32}) {
      std::vector<int32_t> buf((size_t)(n_in * C));
      for (auto& v : buf) v = C == 32 ? INT32_MAX : rnd32();
      const int32_t* x = buf.data();
      for (int64_t n0 = 0; n0 < n_in; n0 += kRsTile) {
        const int64_t n1 = n0 + kRsTile < n_in ? n0 + kRsTile : n_in;
        const int64_t lo = (n0 * I.M) / I.L + I.k_lo, hi = ((n1 - 1) * I.M) / I.L + I.k_lo + I.ntaps;
        CHECK(lo == n0 && hi == n1);
        std::vector<int64_t> sums;
        stage_sums(x, n_in, C, lo, hi, &sums);
        for (int64_t n = n0; n < n1; n++) {
          __int128 S = 0;
          for (int32_t c = 0; c < C; c++) S += x[n * C + c];
          CHECK(sums[(size_t)(n - lo)] == (int64_t)S);
          CHECK(resample_wide_mean((int64_t)S, C) == clamp16(floor_div(S + ((__int128)1 << 15) * C, ((__int128)1 << 16) * C)));
        }
      }
    }
  }
  // a table whose absolute sum would leave the range is refused by the bound
  {
    ResampleTable big;
    big.abs_sum = ((int64_t)1 << 30) / 32;
    CHECK(!resample_wide_in_range(big, 32) && resample_wide_in_range(big, 31));
  }
  std::printf("OK\n");
  return 0;
}
