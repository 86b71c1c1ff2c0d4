// tfp_resample.hpp — rate conversion in front of the int16 fingerprint path: the per-sample
// definition (one routine, host and device), the table builder (host) and the launch of
// tfp_resample.hip.
//
// A fingerprint is comparable only with fingerprints taken at the same sample rate (the window is 512
// samples, the filterbank is built per rate), and the reference takes every file at its native rate
// (/root/reference/src/fp_handler.c:37 DEF_AUBIO_SAMPLERATE 0). The converter is defined in integers
// alone, so host and device agree bit for bit and there is nothing to tolerate: int16 samples, int16
// Q15 taps, an exact 64-bit sum, one rounding, one clamp.
//
//   g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, D = max(L, M)
//   n_out = ceil(n_in L / M)                             (the output instants n M / L before n_in)
//   y[n]  = clamp((sum_k h[p][k] x[i0 + k] + 16384) >> 15), i0 = n M div L, p = n M mod L,
//           k = k_lo .. k_hi, x = 0 outside the clip's own [0, n_in)
//   k_lo = -(Z D div L), k_hi = ceil(Z D / L); tap k of phase p at u = (k L - p) / D:
//   h(u) = rho sinc(rho u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta) for |u| < Z, else 0
//   (a Kaiser-windowed sinc over Z zero crossings of the lower rate, cut off at rho of its Nyquist),
//   each phase scaled to sum 32768 exactly (the remainder goes to the phase's largest tap).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define TFP_RS_HD __host__ __device__ __forceinline__
#else
#define TFP_RS_HD static inline
#endif

#include <cmath>
#include <memory>
#include <vector>

namespace tfp {

constexpr int32_t kRsZ = 24;            // zero crossings each side, in periods of the lower rate
constexpr double kRsBeta = 8.0;         // Kaiser window
constexpr double kRsRho = 0.90;         // cutoff, as a fraction of the lower rate's Nyquist
constexpr int64_t kRsMaxEntries = (int64_t)1 << 20;  // L * ntaps
constexpr int32_t kRsTile = 1024;       // outputs per workgroup (tests/resample_util.py reads it here)
constexpr int32_t kRsSpanMax = 30720;   // int16 samples a workgroup of tfp_resample.hip stages per tile (60 KiB of LDS)

struct ResamplePlan {
  int32_t L, M, k_lo, ntaps;  // k_hi = k_lo + ntaps - 1
};

inline int64_t rs_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The plan of a rate pair; false for a rate < 1 (*bad_rate set) or a table past kRsMaxEntries.
inline bool resample_plan(int32_t rate_in, int32_t rate_out, ResamplePlan* P, bool* bad_rate) {
  *bad_rate = rate_in < 1 || rate_out < 1;
  if (*bad_rate) return false;
  const int64_t g = rs_gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, D = L > M ? L : M;
  const int64_t k_lo = -((kRsZ * D) / L), k_hi = (kRsZ * D + L - 1) / L, ntaps = k_hi - k_lo + 1;
  if (L * ntaps > kRsMaxEntries) return false;  // (ntaps > 2 Z D / L >= 48: L stays below 2^15)
  P->L = (int32_t)L;
  P->M = (int32_t)M;
  P->k_lo = (int32_t)k_lo;
  P->ntaps = (int32_t)ntaps;
  return true;
}

// ceil(n_in L / M), 0 for n_in <= 0; -1 when n_in L + M passes int64 (the index arithmetic's range).
inline int64_t resample_count(const ResamplePlan& P, int64_t n_in) {
  if (n_in <= 0) return 0;
  if (n_in > (INT64_MAX - P.M) / P.L) return -1;
  return (n_in * P.L + P.M - 1) / P.M;
}

TFP_RS_HD int16_t resample_round(int64_t acc) {
  const int64_t y = (acc + 16384) >> 15;  // arithmetic shift: floor
  return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}

// Output sample n of one clip. taps: the table, phase p at taps + p * ntaps. x holds the clip's samples
// [x_lo, x_hi) (sample i at x[i - x_lo]); every sample outside counts as 0. The host passes the whole
// clip (x_lo = 0, x_hi = n_in), the kernel its staged span (zeros staged past the clip's ends) or
// the whole clip in global memory. n M stays below 2^63 for every n < n_out (n M < n_in L + M, resample_count).
TFP_RS_HD int16_t resample_sample(const ResamplePlan& P, const int16_t* __restrict__ taps, const int16_t* __restrict__ x,
                                  int64_t x_lo, int64_t x_hi, int64_t n) {
  const int64_t t = n * P.M, i0 = t / P.L, p = t - i0 * P.L;
  int64_t ka = P.k_lo, kb = (int64_t)P.k_lo + P.ntaps - 1;
  if (ka < x_lo - i0) ka = x_lo - i0;
  if (kb > x_hi - 1 - i0) kb = x_hi - 1 - i0;
  if (kb < ka) return 0;  // no sample under the filter
  const int16_t* __restrict__ h = taps + p * P.ntaps + (ka - P.k_lo);
  const int16_t* __restrict__ s = x + (i0 + ka - x_lo);
  const int32_t cnt = (int32_t)(kb - ka + 1);  // <= ntaps
  int64_t acc = 0;
  for (int32_t j = 0; j < cnt; j++) acc += (int64_t)((int32_t)h[j] * (int32_t)s[j]);  // |product| <= 2^30
  return resample_round(acc);
}

// ---- the multichannel form: interleaved int16 frames of C channels, downmixed and converted -------
// (include/tiresias_fp.h, "rate-normalised ingest of multichannel int16"). The converter is linear and
// exact, so the exact sum over channels commutes with the exact sum over taps:
//   S[i] = sum_c x[i][c]                       (exact; 0 outside the clip's own frames)
//   acc  = sum_k h[p][k] S[i0 + k]             (exact, 64-bit: |h S| reaches 2^35 at C = 32, |acc| < 2^37)
//   y[n] = clamp(floor((acc + 16384 C) / (32768 C)), -32768, 32767)
// with L, M, k_lo, ntaps, h and n_out those of the pair's own table. C = 1 is resample_sample bit for
// bit. Equal rates run no filter (an identity tap of 32768 is no int16): y[i] = floor((2 S[i] + C) / (2 C)).
constexpr int32_t kRsMixChannelsMax = 32;  // TFP_MIX_CHANNELS_MAX
// Channel sums (int32) a workgroup of tfp_resample_mix.hip stages per tile; a pair whose span passes it
// takes the kernel's global-memory form (tests read it here, as they read kRsTile).
constexpr int32_t kRsMixSpanMax = 15360;

// floor((acc + 16384 C) / (32768 C)), clamped. floor(floor(a / 32768) / C) = floor(a / (32768 C)) for
// C >= 1, so the 64-bit part is one arithmetic shift and the division is a 32-bit one (|q| < 2^23).
TFP_RS_HD int16_t resample_mix_round(int64_t acc, int32_t C) {
  const int32_t q = (int32_t)((acc + (int64_t)16384 * C) >> 15);
  int32_t y = q / C;
  if (q - y * C < 0) y--;  // C++ truncates: floor
  return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}

// Equal rates: the integer mean of a frame's channel sum, rounded half up.
TFP_RS_HD int16_t resample_mix_mean(int32_t S, int32_t C) {
  const int32_t q = 2 * S + C, d = 2 * C;  // |q| <= 2^21 + 32
  int32_t y = q / d;
  if (q - y * d < 0) y--;
  return (int16_t)y;  // (a mean of int16 values rounded half up stays in int16)
}

// Output sample n of one clip over its channel sums: resample_sample with S in x's place. S holds the
// sums of the frames [x_lo, x_hi) (frame i at S[i - x_lo]); every frame outside counts as 0.
TFP_RS_HD int16_t resample_mix_sample(const ResamplePlan& P, const int16_t* __restrict__ taps, const int32_t* __restrict__ S,
                                      int64_t x_lo, int64_t x_hi, int64_t n, int32_t C) {
  const int64_t t = n * P.M, i0 = t / P.L, p = t - i0 * P.L;
  int64_t ka = P.k_lo, kb = (int64_t)P.k_lo + P.ntaps - 1;
  if (ka < x_lo - i0) ka = x_lo - i0;
  if (kb > x_hi - 1 - i0) kb = x_hi - 1 - i0;
  if (kb < ka) return 0;  // no frame under the filter
  const int16_t* __restrict__ h = taps + p * P.ntaps + (ka - P.k_lo);
  const int32_t* __restrict__ s = S + (i0 + ka - x_lo);
  const int32_t cnt = (int32_t)(kb - ka + 1);  // <= ntaps
  int64_t acc = 0;
  for (int32_t j = 0; j < cnt; j++) acc += (int64_t)h[j] * (int64_t)s[j];  // |product| <= 2^35
  return resample_mix_round(acc, C);
}

// The same over the clip's interleaved frames themselves (frame i, channel c at x[i * C + c], frames
// [0, n_in)): the channels are summed per tap. The kernel's form for a span past kRsMixSpanMax.
TFP_RS_HD int16_t resample_mix_sample_frames(const ResamplePlan& P, const int16_t* __restrict__ taps,
                                             const int16_t* __restrict__ x, int64_t n_in, int64_t n, int32_t C) {
  const int64_t t = n * P.M, i0 = t / P.L, p = t - i0 * P.L;
  int64_t ka = P.k_lo, kb = (int64_t)P.k_lo + P.ntaps - 1;
  if (ka < -i0) ka = -i0;
  if (kb > n_in - 1 - i0) kb = n_in - 1 - i0;
  if (kb < ka) return 0;
  const int16_t* __restrict__ h = taps + p * P.ntaps + (ka - P.k_lo);
  const int16_t* __restrict__ s = x + (i0 + ka) * C;
  const int32_t cnt = (int32_t)(kb - ka + 1);
  int64_t acc = 0;
  for (int32_t j = 0; j < cnt; j++) {
    int32_t sum = 0;
    for (int32_t c = 0; c < C; c++) sum += (int32_t)s[(int64_t)j * C + c];
    acc += (int64_t)h[j] * (int64_t)sum;
  }
  return resample_mix_round(acc, C);
}

// The channel sums of nframes interleaved frames.
inline void resample_mix_sums(const int16_t* x, int64_t nframes, int32_t C, int32_t* S) {
  for (int64_t i = 0; i < nframes; i++) {
    int32_t sum = 0;
    for (int32_t c = 0; c < C; c++) sum += (int32_t)x[i * C + c];
    S[i] = sum;
  }
}

// ---- the wide form: interleaved int32 Q31 frames of C channels, downmixed and converted ------------
// (include/tiresias_fp.h, "rate-normalised ingest of 24/32-bit and float audio"). Value v in [-1, 1) is
// stored as v 2^31. The converter is linear, so widening the samples changes no table and no rate
// arithmetic, only the accumulator's range, the final rounding and the staged width:
//   S[i] = sum_c q[i][c]                       (exact, |S| <= 2^36; 0 outside the clip's own frames)
//   acc  = sum_k h[p][k] S[i0 + k]             (exact, 64-bit: |acc| <= 2^31 C A, A = max_p sum_k |h[p][k]|)
//   y[n] = clamp(floor((acc + 2^30 C) / (2^31 C)), -32768, 32767)
// A wide call needs A C < 2^30 (ResampleTable::abs_sum, resample_wide_in_range): then |acc| < 2^61 and
// the quotient by 2^31 fits int32. On int16 frames x widened to x << 16, acc is 2^16 times the mix form's,
// so the output is resample_mix_sample's bit for bit. Equal rates run no filter:
// y[i] = clamp(floor((S[i] + 2^15 C) / (2^16 C))) (Q31 full scale rounds to 32768: the clamp is needed).
// Sums (int64) a workgroup of tfp_resample_wide.hip stages per tile for C >= 2: the bytes of
// kRsMixSpanMax int32. One channel stages its int32 samples themselves, up to kRsMixSpanMax of them.
constexpr int32_t kRsWideSpanMax = 7680;

// floor((acc + 2^30 C) / (2^31 C)), clamped: one arithmetic shift, then a 32-bit floor division, as
// resample_mix_round (|q| <= A C + C < 2^30 + 32).
TFP_RS_HD int16_t resample_wide_round(int64_t acc, int32_t C) {
  const int32_t q = (int32_t)((acc + ((int64_t)1 << 30) * C) >> 31);
  int32_t y = q / C;
  if (q - y * C < 0) y--;  // C++ truncates: floor
  return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}

// Equal rates: a frame's channel sum to int16, rounded half up and clamped (|q| <= 2^15 C + C).
TFP_RS_HD int16_t resample_wide_mean(int64_t S, int32_t C) {
  const int32_t q = (int32_t)((S + ((int64_t)1 << 15) * C) >> 16);
  int32_t y = q / C;
  if (q - y * C < 0) y--;
  return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}

// Output sample n of one clip over its staged elements: resample_mix_sample with T = int32_t samples
// (C = 1) or int64_t channel sums (C >= 2) in S's place. S holds the frames [x_lo, x_hi) (frame i at
// S[i - x_lo]); every frame outside counts as 0.
template <typename T>
TFP_RS_HD int16_t resample_wide_sample(const ResamplePlan& P, const int16_t* __restrict__ taps, const T* __restrict__ S,
                                       int64_t x_lo, int64_t x_hi, int64_t n, int32_t C) {
  const int64_t t = n * P.M, i0 = t / P.L, p = t - i0 * P.L;
  int64_t ka = P.k_lo, kb = (int64_t)P.k_lo + P.ntaps - 1;
  if (ka < x_lo - i0) ka = x_lo - i0;
  if (kb > x_hi - 1 - i0) kb = x_hi - 1 - i0;
  if (kb < ka) return 0;  // no frame under the filter
  const int16_t* __restrict__ h = taps + p * P.ntaps + (ka - P.k_lo);
  const T* __restrict__ s = S + (i0 + ka - x_lo);
  const int32_t cnt = (int32_t)(kb - ka + 1);  // <= ntaps
  int64_t acc = 0;
  for (int32_t j = 0; j < cnt; j++) acc += (int64_t)h[j] * (int64_t)s[j];  // |product| <= 2^51
  return resample_wide_round(acc, C);
}

// The same over the clip's interleaved frames themselves (frame i, channel c at x[i * C + c], frames
// [0, n_in)): the channels are summed per tap. The kernel's form for a span past its staging limit.
TFP_RS_HD int16_t resample_wide_sample_frames(const ResamplePlan& P, const int16_t* __restrict__ taps,
                                              const int32_t* __restrict__ x, int64_t n_in, int64_t n, int32_t C) {
  const int64_t t = n * P.M, i0 = t / P.L, p = t - i0 * P.L;
  int64_t ka = P.k_lo, kb = (int64_t)P.k_lo + P.ntaps - 1;
  if (ka < -i0) ka = -i0;
  if (kb > n_in - 1 - i0) kb = n_in - 1 - i0;
  if (kb < ka) return 0;
  const int16_t* __restrict__ h = taps + p * P.ntaps + (ka - P.k_lo);
  const int32_t* __restrict__ s = x + (i0 + ka) * C;
  const int32_t cnt = (int32_t)(kb - ka + 1);
  int64_t acc = 0;
  for (int32_t j = 0; j < cnt; j++) {
    int64_t sum = 0;
    for (int32_t c = 0; c < C; c++) sum += (int64_t)s[(int64_t)j * C + c];
    acc += (int64_t)h[j] * sum;
  }
  return resample_wide_round(acc, C);
}

// Sample to Q31, on the host only: clamp(nearbyint(x 2^31)) in the sample's own precision, ties to even
// (the product is exact: a power-of-two scale), +1.0 to 2^31 - 1, NaN to 0, +-inf clamped.
inline int32_t q31_from_f32(float x) {
  const float v = std::nearbyint(x * 2147483648.0f);
  if (!(v == v)) return 0;
  return v >= 2147483648.0f ? INT32_MAX : v <= -2147483648.0f ? INT32_MIN : (int32_t)v;
}
inline int32_t q31_from_f64(double x) {
  const double v = std::nearbyint(x * 2147483648.0);
  if (!(v == v)) return 0;
  return v >= 2147483648.0 ? INT32_MAX : v <= -2147483648.0 ? INT32_MIN : (int32_t)v;
}

struct ResampleTable {
  ResamplePlan plan;
  std::vector<int16_t> taps;  // [L][ntaps]
  int64_t abs_sum = 0;        // A = max_p sum_k |h[p][k]| (resample_abs_sum), set where the table is built
};

// A of a table: the largest absolute tap sum of a phase, the bound |acc| <= max|S| A of every form.
inline int64_t resample_abs_sum(const ResamplePlan& P, const std::vector<int16_t>& taps) {
  int64_t A = 0;
  for (int32_t p = 0; p < P.L; p++) {
    int64_t a = 0;
    for (int32_t j = 0; j < P.ntaps; j++) {
      const int32_t h = taps[(size_t)p * P.ntaps + j];
      a += h < 0 ? -h : h;
    }
    if (a > A) A = a;
  }
  return A;
}

// The wide form's range: A C < 2^30 keeps the accumulator below 2^61 and its quotient in int32.
inline bool resample_wide_in_range(const ResampleTable& T, int32_t C) { return T.abs_sum * C < ((int64_t)1 << 30); }

// I0 by its power series (every term positive; x <= beta here, 1e-17 relative after ~30 terms).
inline double rs_i0(double x) {
  const double q = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; k++) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-17) break;
  }
  return sum;
}

inline double rs_h(double u) {
  const double a = u / kRsZ;
  if (!(a > -1.0 && a < 1.0)) return 0.0;
  const double v = kRsRho * u, pi = 3.14159265358979323846;
  const double sinc = v == 0.0 ? 1.0 : std::sin(pi * v) / (pi * v);
  return kRsRho * sinc * rs_i0(kRsBeta * std::sqrt(1.0 - a * a)) / rs_i0(kRsBeta);
}

// The table of a plan, in double, each phase scaled to sum exactly 32768. false when a tap leaves
// int16 (no supported pair does: the largest tap is about rho * 32768).
inline bool resample_build(const ResamplePlan& P, std::vector<int16_t>* taps) {
  const int64_t D = P.L > P.M ? P.L : P.M;
  taps->assign((size_t)P.L * P.ntaps, 0);
  std::vector<double> h(P.ntaps);
  for (int32_t p = 0; p < P.L; p++) {
    double sum = 0.0;
    for (int32_t j = 0; j < P.ntaps; j++) {
      h[j] = rs_h((double)((int64_t)(P.k_lo + j) * P.L - p) / (double)D);
      sum += h[j];
    }
    int64_t isum = 0;
    int32_t big = 0;
    std::vector<int64_t> q(P.ntaps);
    for (int32_t j = 0; j < P.ntaps; j++) {
      q[j] = (int64_t)std::nearbyint(h[j] / sum * 32768.0);
      isum += q[j];
      if (q[j] > q[big]) big = j;
    }
    q[big] += 32768 - isum;
    for (int32_t j = 0; j < P.ntaps; j++) {
      if (q[j] < -32768 || q[j] > 32767) return false;
      (*taps)[(size_t)p * P.ntaps + j] = (int16_t)q[j];
    }
  }
  return true;
}

// One clip on the host: out[resample_count(n_in)].
inline void resample_clip(const ResampleTable& T, const int16_t* x, int64_t n_in, int16_t* out) {
  const int64_t n_out = resample_count(T.plan, n_in);
  for (int64_t n = 0; n < n_out; n++) out[n] = resample_sample(T.plan, T.taps.data(), x, 0, n_in, n);
}

// One multichannel clip on the host: out[resample_count(nframes)].
inline void resample_mix_clip(const ResampleTable& T, const int16_t* x, int64_t nframes, int32_t C, int16_t* out) {
  std::vector<int32_t> S((size_t)nframes);
  resample_mix_sums(x, nframes, C, S.data());
  const int64_t n_out = resample_count(T.plan, nframes);
  for (int64_t n = 0; n < n_out; n++) out[n] = resample_mix_sample(T.plan, T.taps.data(), S.data(), 0, nframes, n, C);
}

// One wide clip on the host: out[resample_count(nframes)]. One channel filters its samples as they are.
inline void resample_wide_clip(const ResampleTable& T, const int32_t* x, int64_t nframes, int32_t C, int16_t* out) {
  const int64_t n_out = resample_count(T.plan, nframes);
  if (C == 1) {
    for (int64_t n = 0; n < n_out; n++) out[n] = resample_wide_sample(T.plan, T.taps.data(), x, 0, nframes, n, 1);
    return;
  }
  std::vector<int64_t> S((size_t)nframes);
  for (int64_t i = 0; i < nframes; i++) {
    int64_t sum = 0;
    for (int32_t c = 0; c < C; c++) sum += (int64_t)x[i * C + c];
    S[i] = sum;
  }
  for (int64_t n = 0; n < n_out; n++) out[n] = resample_wide_sample(T.plan, T.taps.data(), S.data(), 0, nframes, n, C);
}

// The process's tables (tfp_resample.cpp): built once per rate pair, shared by the host routine and
// every engine. nullptr for a bad or unsupported pair, *bad_rate telling which.
std::shared_ptr<const ResampleTable> resample_table(int32_t rate_in, int32_t rate_out, bool* bad_rate);

// Tile t of the launch covers outputs [(t - toff[c]) * kRsTile, ...) of clip c = tclip[t].
inline void resample_tiles(const int64_t* out_off, int32_t nclips, std::vector<int32_t>* toff, std::vector<int32_t>* tclip) {
  toff->assign((size_t)nclips + 1, 0);
  tclip->clear();
  for (int32_t c = 0; c < nclips; c++) {
    const int64_t nt = (out_off[c + 1] - out_off[c] + kRsTile - 1) / kRsTile;
    (*toff)[c + 1] = (*toff)[c] + (int32_t)nt;
    tclip->insert(tclip->end(), (size_t)nt, c);
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
// A packed ragged batch: clip c is the input samples [in_off[c], in_off[c + 1]) of d_in and the output
// samples [out_off[c], out_off[c + 1]) of d_out, out_off[c + 1] - out_off[c] = resample_count of its
// input length; d_toff / d_tclip are resample_tiles of out_off, ntiles = toff[nclips]. All arrays on
// the device. One launch; ntiles = 0 launches nothing.
hipError_t launch_resample(const ResamplePlan& P, const int16_t* d_taps, const int16_t* d_in, const int64_t* d_in_off,
                           const int64_t* d_out_off, const int32_t* d_toff, const int32_t* d_tclip, int32_t ntiles,
                           int16_t* d_out, hipStream_t stream);

// The multichannel launch (tfp_resample_mix.hip): clip c is the frames [in_off[c], in_off[c + 1]) of d_in,
// C interleaved int16 each (its first sample at d_in[in_off[c] * C]; d_in itself 4-byte aligned), the
// outputs and tiles as launch_resample's. downmix: equal rates, out_off = in_off, no table is read (P
// and d_taps are ignored). *staged receives whether the LDS form ran (a plan's span within
// kRsMixSpanMax; the downmix always). One launch; ntiles = 0 launches nothing.
hipError_t launch_resample_mix(const ResamplePlan& P, const int16_t* d_taps, bool downmix, int32_t C, const int16_t* d_in,
                               const int64_t* d_in_off, const int64_t* d_out_off, const int32_t* d_toff,
                               const int32_t* d_tclip, int32_t ntiles, int16_t* d_out, hipStream_t stream, bool* staged);

// The wide launch (tfp_resample_wide.hip): clip c is the frames [in_off[c], in_off[c + 1]) of d_in, C
// interleaved int32 Q31 each, the outputs and tiles as launch_resample's. downmix: equal rates, out_off =
// in_off, no table is read (P and d_taps are ignored). *form receives the form that ran. The caller has
// checked resample_wide_in_range for the pair. One launch; ntiles = 0 launches nothing.
enum ResampleWideForm : int32_t { kRsWideNone = 0, kRsWideStagedMono, kRsWideStagedSums, kRsWideGlobal, kRsWideDownmix };
hipError_t launch_resample_wide(const ResamplePlan& P, const int16_t* d_taps, bool downmix, int32_t C, const int32_t* d_in,
                                const int64_t* d_in_off, const int64_t* d_out_off, const int32_t* d_toff,
                                const int32_t* d_tclip, int32_t ntiles, int16_t* d_out, hipStream_t stream,
                                ResampleWideForm* form);
#endif

}  // namespace tfp
