// check_resample_mix.cpp — the multichannel routines of csrc/tfp_resample.hpp, stand-alone: the routine over
// channel sums against a plain restatement with bounds checked reads (zero-length, one-frame and shorter-
// than-the-filter clips, full scale at 32 channels), the routine over a staged span against the routine
// over the whole clip for every tile of a 2-tile clip (the kernel's staging arithmetic, word walk included,
// run on the host), the per-tap form, the rounding and the mean. Built with -fsanitize=address,undefined
// -fno-sanitize-recover=all and run on the CPU: any finding aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static int64_t floor_div(__int128 a, int64_t b) {  // b > 0
  __int128 q = a / b;
  if (a % b < 0) q--;
  return (int64_t)q;
}

// The definition, read by read: frame i is 0 outside [0, n_in).
static int16_t restate(const ResampleTable& t, const std::vector<int16_t>& x, int32_t C, int64_t n) {
  const ResamplePlan& P = t.plan;
  const int64_t n_in = (int64_t)x.size() / C;
  const __int128 nm = (__int128)n * P.M;
  const int64_t i0 = (int64_t)(nm / P.L), p = (int64_t)(nm % P.L);
  __int128 acc = 0;
  for (int32_t j = 0; j < P.ntaps; j++) {
    const int64_t i = i0 + P.k_lo + j;
    int64_t S = 0;
    if (i >= 0 && i < n_in)
      for (int32_t c = 0; c < C; c++) S += x.at((size_t)(i * C + c));
    acc += (__int128)t.taps.at((size_t)(p * P.ntaps + j)) * S;
  }
  const int64_t y = floor_div(acc + (__int128)16384 * C, (int64_t)32768 * C);
  return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}

static uint32_t rng_state = 777u;
static int16_t rnd16() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (int16_t)(rng_state >> 16);
}

// The kernel's staging of the frames [lo, hi) of a clip of n_in frames at x (x inside a buffer that starts
// 4-byte aligned): zeros, then the clip's own run walked by aligned words, each sample added to its frame.
static void stage(const int16_t* x, int64_t n_in, int32_t C, int64_t lo, int64_t hi, std::vector<int32_t>* sums) {
  sums->assign((size_t)(hi - lo), 0);
  const int64_t fa = lo > 0 ? lo : 0, fb = hi < n_in ? hi : n_in;
  if (fb <= fa) return;
  const int16_t* xs = x + fa * C;
  const int32_t total = (int32_t)(fb - fa) * C;
  const int32_t head = (int32_t)((reinterpret_cast<uintptr_t>(xs) >> 1) & 1);
  const int32_t nwords = (head + total + 1) / 2;
  int32_t* dst = sums->data() + (fa - lo);
  for (int32_t j = 0; j < nwords; j++) {
    const int32_t s0 = 2 * j - head, s1 = s0 + 1;
    int32_t v0 = 0, v1 = 0;
    if (s0 >= 0 && s1 < total) {
      uint32_t u;
      std::memcpy(&u, xs - head + 2 * j, 4);  // (the aligned word)
      v0 = (int32_t)(int16_t)(u & 0xffffu);
      v1 = (int32_t)(int16_t)(u >> 16);
    } else {
      if (s0 >= 0) v0 = xs[s0];
      if (s1 < total) v1 = xs[s1];
    }
    const int32_t f0 = s0 >= 0 ? (int32_t)((uint32_t)s0 / (uint32_t)C) : 0;
    const int32_t f1 = s1 < total ? (int32_t)((uint32_t)s1 / (uint32_t)C) : f0;
    if (f0 >= (int32_t)(fb - fa) || f1 >= (int32_t)(fb - fa)) std::abort();
    dst[f0] += v0;
    dst[f1] += v1;
  }
}

int main() {
  // rounding: the floor, the tie, the clamp; the mean
  CHECK(resample_mix_round(0, 2) == 0 && resample_mix_round(-5 * 32768, 3) == -2 && resample_mix_round(-3 * 32768, 2) == -1);
  CHECK(resample_mix_round(-1 * 32768, 2) == 0 && resample_mix_round(1 * 32768, 2) == 1 && resample_mix_round(5 * 32768, 3) == 2);
  CHECK(resample_mix_round((int64_t)32 * 32767 * 32768, 32) == 32767 && resample_mix_round(-(int64_t)32 * 32768 * 32768, 32) == -32768);
  CHECK(resample_mix_round(((int64_t)1 << 37) - 1, 32) == 32767 && resample_mix_round(-((int64_t)1 << 37), 32) == -32768);
  CHECK(resample_mix_round(((int64_t)1 << 37) - 1, 1) == 32767 && resample_mix_round(-((int64_t)1 << 37), 1) == -32768);
  for (int64_t a = -200000; a <= 200000; a += 37) CHECK(resample_mix_round(a, 1) == resample_round(a));
  CHECK(resample_mix_mean(-3, 2) == -1 && resample_mix_mean(-1, 2) == 0 && resample_mix_mean(1, 2) == 1);
  CHECK(resample_mix_mean(-5, 3) == -2 && resample_mix_mean(32 * 32767, 32) == 32767 && resample_mix_mean(-32 * 32768, 32) == -32768);

  const int32_t pairs[][2] = {{16000, 8000}, {8000, 16000}, {44100, 8000}, {11025, 8000}};
  const int32_t chans[] = {1, 2, 3, 6, 32};
  for (const auto& pr : pairs) {
    ResampleTable t;
    CHECK(table_of(pr[0], pr[1], &t));
    const ResamplePlan& P = t.plan;
    const int64_t two_tiles = ((int64_t)(kRsTile + 37) * P.M) / P.L + 3;  // a clip of 2 tiles
    const int64_t lens[] = {0, 1, 2, P.ntaps - 1, P.ntaps, 700, two_tiles};
    for (int32_t C : chans) {
      for (int64_t n_in : lens) {
        for (int mode = 0; mode < 3; mode++) {  // noise, all -32768, all 32767
          if (mode && C != 32 && C != 3) continue;
          // the clip starts `lead` samples into an aligned buffer: both parities of the first sample
          for (int64_t lead = 0; lead < 2; lead++) {
            std::vector<int16_t> buf((size_t)(lead + n_in * C));  // exactly: a read past either end is a finding
            for (auto& v : buf) v = mode == 0 ? rnd16() : mode == 1 ? (int16_t)-32768 : (int16_t)32767;
            const int16_t* x = buf.data() + lead;
            const std::vector<int16_t> clip(x, x + n_in * C);
            const int64_t n_out = resample_count(P, n_in);
            CHECK(n_in > 0 || n_out == 0);
            std::vector<int16_t> y((size_t)n_out);
            resample_mix_clip(t, x, n_in, C, y.data());
            for (int64_t n = 0; n < n_out; n++) {
              CHECK(y[(size_t)n] == restate(t, clip, C, n));
              CHECK(resample_mix_sample_frames(P, t.taps.data(), x, n_in, n, C) == y[(size_t)n]);
            }
            if (C == 1) {
              std::vector<int16_t> m((size_t)n_out);
              resample_clip(t, x, n_in, m.data());
              CHECK(m == y);
            }
            // every tile: the staged span against the whole clip
            const int64_t ntiles = (n_out + kRsTile - 1) / kRsTile;
            CHECK(n_in != two_tiles || ntiles == 2);
            for (int64_t tile = 0; tile < ntiles; tile++) {
              const int64_t n0 = tile * kRsTile, n1 = n0 + kRsTile < n_out ? n0 + kRsTile : n_out;
              const int64_t lo = (n0 * P.M) / P.L + P.k_lo, hi = ((n1 - 1) * P.M) / P.L + P.k_lo + P.ntaps;
              CHECK(hi - lo <= ((int64_t)(kRsTile - 1) * P.M) / P.L + 1 + P.ntaps && hi - lo <= kRsMixSpanMax);
              std::vector<int32_t> sums;
              stage(x, n_in, C, lo, hi, &sums);
              for (int64_t n = n0; n < n1; n++) CHECK(resample_mix_sample(P, t.taps.data(), sums.data(), lo, hi, n, C) == y[(size_t)n]);
            }
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
      std::vector<int16_t> buf((size_t)(1 + n_in * C));
      for (auto& v : buf) v = rnd16();
      const int16_t* x = buf.data() + 1;
      for (int64_t n0 = 0; n0 < n_in; n0 += kRsTile) {
        const int64_t n1 = n0 + kRsTile < n_in ? n0 + kRsTile : n_in;
        const int64_t lo = (n0 * I.M) / I.L + I.k_lo, hi = ((n1 - 1) * I.M) / I.L + I.k_lo + I.ntaps;
        CHECK(lo == n0 && hi == n1);
        std::vector<int32_t> sums;
        stage(x, n_in, C, lo, hi, &sums);
        for (int64_t n = n0; n < n1; n++) {
          int32_t S = 0;
          for (int32_t c = 0; c < C; c++) S += x[n * C + c];
          CHECK(sums[(size_t)(n - lo)] == S);
          CHECK(resample_mix_mean(S, C) == (int16_t)floor_div((__int128)2 * S + C, 2 * C));
        }
      }
    }
  }
  std::printf("OK\n");
  return 0;
}
