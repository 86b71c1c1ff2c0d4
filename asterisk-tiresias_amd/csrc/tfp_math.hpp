// tfp_math.hpp — exact scalar math shared by the host engine and the gfx950 kernels.
//
// Everything here is written with IEEE-754 basic operations only (+ - * / sqrt, fma where
// written explicitly, rint), so it evaluates bit-identically on x86-64 and on gfx950 when
// built with -ffp-contract=off (see Makefile). No libm/ocml calls.
//
// Functions and the reference behaviour they reproduce:
//   tfp_log10f()   == glibc 2.35 log10f, bit for bit, for every positive float.
//                     The reference applies it per mel band via aubio's fvec_log10
//                     (libaubio mathutils.c, called from aubio_mfcc_do; call site
//                     /root/reference/src/fp_handler.c:642). glibc 2.35 log10f is the fdlibm
//                     float wrapper around ARM-optimized-routines logf; both are restated
//                     below. Verified exhaustively on all 2^24 mantissas of [0.5,2) for logf
//                     and on 713 M sampled floats for log10f (tests/test_math_exact.py).
//   tfp_log10()    glibc 2.35 log10 wrapper (fdlibm e_log10.c) around an own near-CR log;
//                  used for `10*log10(fabs(c))` (/root/reference/src/fp_handler.c:651).
//                  Its callers only consume fmt6()/trunc of 10*log10(); agreement with glibc
//                  at that granularity is checked exhaustively over all floats c.
//   tfp_fmt6()     printf("%f") of a double = round-half-even of the EXACT binary value to
//                  6 decimals, returned as integer micro-units. The reference stores every
//                  fingerprint value through "%f" (/root/reference/src/db_ctx_handler.c:479-481)
//                  and prints search bounds through "%f" (/root/reference/src/fp_handler.c:308-314,
//                  339-347); SQLite then compares the parsed decimals, which orders exactly as
//                  these integers do.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define TFP_HD __host__ __device__ inline
#else
#define TFP_HD static inline
#endif

namespace tfp {

TFP_HD uint32_t f2u(float f) { return __builtin_bit_cast(uint32_t, f); }
TFP_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
TFP_HD uint64_t d2u(double d) { return __builtin_bit_cast(uint64_t, d); }
TFP_HD double u2d(uint64_t u) { return __builtin_bit_cast(double, u); }

// Micro-unit sentinel for a value the reference stores as SQL NULL (json_real(±inf) → NULL,
// /root/reference/src/fp_handler.c:651 + jansson). Valid fingerprints are within ±4.6e8.
constexpr int32_t kNullMicro = INT32_MIN;

// ---------------------------------------------------------------------------------------
// glibc 2.35 logf (ARM optimized-routines, LOGF_TABLE_BITS = 4), restated. The double-typed
// evaluation below is the non-FMA form; on [0.5,2) it equals the FMA form bit for bit
// (checked exhaustively), which is the only range tfp_log10f() feeds it.
struct LogfEntry { double invc, logc; };
#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__
#endif
inline const LogfEntry* logf_table() {
  static constexpr LogfEntry T[16] = {
      {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
      {0x1.49539f0f010bp+0, -0x1.01eae7f513a67p-2},  {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
      {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8eap+0, -0x1.1aa2bc79c81p-3},
      {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
      {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1p+0, 0x0p+0},
      {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5},  {0x1.ca4b31f026aap-1, 0x1.c5e53aa362eb4p-4},
      {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d22477p-3},
      {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2},  {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2},
  };
  return T;
}

// Valid for positive normal finite x (tfp_log10f only passes [0.5, 2)). T: the 16-entry table
// (device code passes a copy staged in LDS).
TFP_HD float logf_glibc(float x, const LogfEntry* T = logf_table()) {
  const double Ln2 = 0x1.62e42fefa39efp-1;
  const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
  const uint32_t ix = f2u(x);
  const uint32_t tmp = ix - 0x3f330000u;
  const int i = (int)((tmp >> 19) & 15u);
  const int k = (int32_t)tmp >> 23;
  const uint32_t iz = ix - (tmp & 0xff800000u);
  const LogfEntry e = T[i];
  const double z = (double)u2f(iz);
  const double r = z * e.invc - 1.0;
  const double y0 = e.logc + (double)k * Ln2;
  const double r2 = r * r;
  double y = A1 * r + A2;
  y = A0 * r2 + y;
  y = y * r2 + (y0 + r);
  return (float)y;
}

// glibc 2.35 log10f = fdlibm e_log10f.c float wrapper (all float arithmetic).
TFP_HD float log10f_glibc(float x, const LogfEntry* T = logf_table()) {
  const float two25 = 3.3554432000e+07f, ivln10 = 4.3429449201e-01f;
  const float log10_2hi = 3.0102920532e-01f, log10_2lo = 7.9034151668e-07f;
  int32_t hx = (int32_t)f2u(x);
  int32_t k = 0;
  if (hx < 0x00800000) {
    if ((hx & 0x7fffffff) == 0) return -u2f(0x7f800000u);  // -inf
    if (hx < 0) return u2f(0x7fc00000u);                    // NaN
    k -= 25;
    x *= two25;
    hx = (int32_t)f2u(x);
  }
  if (hx >= 0x7f800000) return x + x;
  k += (hx >> 23) - 127;
  const int32_t i = (int32_t)(((uint32_t)k & 0x80000000u) >> 31);
  hx = (hx & 0x007fffff) | ((0x7f - i) << 23);
  const float y = (float)(k + i);
  x = u2f((uint32_t)hx);
  const float z = y * log10_2lo + ivln10 * logf_glibc(x, T);
  return z + y * log10_2hi;
}

// aubio fvec_log10: LOG10(MAX(VERY_SMALL_NUMBER, x)), VERY_SMALL_NUMBER = 2.e-42 (a double
// literal, so the comparison is done in double and the clamp value is (float)2e-42).
TFP_HD float aubio_log10_clamped(float x, const LogfEntry* T = logf_table()) {
  const double v = 2.e-42;
  const double xd = (double)x;
  const float a = (float)((v > xd) ? v : xd);
  return log10f_glibc(a, T);
}

// aubio_log10_clamped for the filterbank sums (finite, >= -0), branch-free. For any non-NaN
// float x the double-precision clamp (2e-42 > (double)x ? (float)2e-42 : x) equals
// max(x, (float)2e-42), after which the only special case of log10f left is a subnormal
// argument (rescaled by 2^25 under a select). Bit-identical to aubio_log10_clamped on every
// non-negative float (tests/native/check_math.cpp #5, exhaustive log committed).
TFP_HD float aubio_log10_fast(float x, const LogfEntry* T = logf_table()) {
  const float two25 = 3.3554432000e+07f, ivln10 = 4.3429449201e-01f;
  const float log10_2hi = 3.0102920532e-01f, log10_2lo = 7.9034151668e-07f;
  const float c = (float)2.e-42;
  float a = x > c ? x : c;
  const bool den = f2u(a) < 0x00800000u;
  a = den ? a * two25 : a;
  int32_t hx = (int32_t)f2u(a);
  const int32_t k = (den ? -25 : 0) + (hx >> 23) - 127;
  const int32_t i = (int32_t)(((uint32_t)k & 0x80000000u) >> 31);
  hx = (hx & 0x007fffff) | ((0x7f - i) << 23);
  const float y = (float)(k + i);
  const float z = y * log10_2lo + ivln10 * logf_glibc(u2f((uint32_t)hx), T);
  return z + y * log10_2hi;
}

// ---------------------------------------------------------------------------------------
// Near-correctly-rounded natural log for x in [0.5, 2): reduce to [sqrt(1/2), sqrt(2)),
// log(m) = 2 atanh(s), s = (m-1)/(m+1) kept as a double-double, series tail in double.
// Relative error ~2^-59, so it rounds to the CR double except within ~2^-59 of a midpoint.
TFP_HD double log_acc(double x) {
  const double SQRT2 = 0x1.6a09e667f3bcdp+0, SQRT1_2 = 0x1.6a09e667f3bcdp-1;
  const double LN2_HI = 0x1.62e42fefa3800p-1;   // 43 significant bits: j*LN2_HI exact
  const double LN2_LO = 0x1.ef35793c7673p-45;
  double j = 0.0;
  if (x > SQRT2) { x = x * 0.5; j = 1.0; }
  else if (x < SQRT1_2) { x = x * 2.0; j = -1.0; }
  const double f = x - 1.0;                       // exact (Sterbenz)
  const double dh = 2.0 + f;
  const double dl = (2.0 - dh) + f;               // exact (Fast2Sum, |2| >= |f|)
  const double sh = f / dh;
  double r = __builtin_fma(-sh, dh, f);           // exact remainder f - sh*dh
  r = r - sh * dl;
  const double sl = r / dh;
  const double w = sh * sh;
  // p = sum_{n=1..11} 2/(2n+1) w^n
  double p = 2.0 / 23.0;
  p = p * w + 2.0 / 21.0;
  p = p * w + 2.0 / 19.0;
  p = p * w + 2.0 / 17.0;
  p = p * w + 2.0 / 15.0;
  p = p * w + 2.0 / 13.0;
  p = p * w + 2.0 / 11.0;
  p = p * w + 2.0 / 9.0;
  p = p * w + 2.0 / 7.0;
  p = p * w + 2.0 / 5.0;
  p = p * w + 2.0 / 3.0;
  p = p * w;
  const double tail = sh * p;
  const double hi = 2.0 * sh;                     // exact
  const double lo = 2.0 * sl + tail + j * LN2_LO;
  const double a = j * LN2_HI;                    // exact
  const double s = a + hi;                        // TwoSum(a, hi)
  const double bb = s - a;
  const double err = (a - (s - bb)) + (hi - bb);
  return s + (err + lo);
}

// glibc's inner log differs from log_acc on 58,054 of the 2^24 reduced arguments the wrapper
// below can see for a float input (the double of a float has 29 zero low mantissa bits; the
// reduced argument is its mantissa in [1, 2) or [0.5, 1)). LogFix lists them, keyed
// i << 23 | mantissa23 (i = 1 for [0.5, 1)), with glibc's value: built on the host from glibc
// itself (tfp_tables.cpp build_log_fix), ascending keys. n = 0: no table (log_acc everywhere).
// hashed: key/val are instead the 2^kLogFixHashBits slots of tfp_tables.cpp log_fix_hash (the
// device copy: at load 0.44 a lookup, hit or miss, reads one or two adjacent keys).
constexpr int kLogFixHashBits = 17;
constexpr uint32_t kLogFixEmpty = 0xffffffffu;
TFP_HD uint32_t log_fix_slot(uint32_t k) { return (k * 0x9E3779B1u) >> (32 - kLogFixHashBits); }
struct LogFix {
  const uint32_t* key;
  const double* val;
  int32_t n;
  int32_t hashed = 0;
  const uint32_t* bits = nullptr;  // (hashed) the keys present, one bit each over the 2^24 domain
};

TFP_HD double log_fixed(double x, int32_t i, const LogFix& fx) {
  if (fx.n > 0 && (d2u(x) & 0x1fffffffull) == 0) {  // (a float's double: the table's domain)
    const uint32_t k = ((uint32_t)i << 23) | (uint32_t)((d2u(x) >> 29) & 0x7fffffu);
    if (fx.hashed) {
      // one load decides for the 99.65 % of arguments without an entry (the probes of a miss are
      // dependent loads: they cost more than the log itself)
      if (fx.bits && !((fx.bits[k >> 5] >> (k & 31)) & 1u)) return log_acc(x);
      for (uint32_t h = log_fix_slot(k);; h = (h + 1) & ((1u << kLogFixHashBits) - 1)) {
        const uint32_t s = fx.key[h];
        if (s == k) return fx.val[h];
        if (s == kLogFixEmpty) break;
      }
      return log_acc(x);
    }
    int32_t lo = 0, hi = fx.n;
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (fx.key[mid] < k) lo = mid + 1; else hi = mid;
    }
    if (lo < fx.n && fx.key[lo] == k) return fx.val[lo];
  }
  return log_acc(x);
}

// glibc 2.35 log10 = fdlibm e_log10.c wrapper; the inner log is log_acc() above, or glibc's own
// value where the LogFix table lists it (then the result is glibc's, bit for bit, for every
// double of a float: tests/native/check_logfix.cpp).
TFP_HD double log10_glibc_wrapper(double x, const LogFix& fx = LogFix{nullptr, nullptr, 0}) {
  const double two54 = 1.80143985094819840000e+16;
  const double ivln10 = 4.34294481903251816668e-01;
  const double log10_2hi = 3.01029995663611771306e-01;
  const double log10_2lo = 3.69423907715893078616e-13;
  uint64_t bits = d2u(x);
  int32_t hx = (int32_t)(bits >> 32);
  const uint32_t lx = (uint32_t)bits;
  int32_t k = 0;
  if (hx < 0x00100000) {
    if (((hx & 0x7fffffff) | (int32_t)lx) == 0) return -u2d(0x7ff0000000000000ull);
    if (hx < 0) return u2d(0x7ff8000000000000ull);
    k -= 54;
    x *= two54;
    bits = d2u(x);
    hx = (int32_t)(bits >> 32);
  }
  if (hx >= 0x7ff00000) return x + x;
  k += (hx >> 20) - 1023;
  const int32_t i = (int32_t)(((uint32_t)k & 0x80000000u) >> 31);
  hx = (hx & 0x000fffff) | ((0x3ff - i) << 20);
  const double y = (double)(k + i);
  x = u2d(((uint64_t)(uint32_t)hx << 32) | (d2u(x) & 0xffffffffull));
  const double z = y * log10_2lo + ivln10 * log_fixed(x, i, fx);
  return z + y * log10_2hi;
}

// `10 * log10(fabs((double)c))` of /root/reference/src/fp_handler.c:651. Without a LogFix table
// the value may differ from glibc's in its last bit (152,867 floats), never in its "%f" micro-units
// or its truncation (what the stored rows and the max1 keys use); with the table it is glibc's.
TFP_HD double db_of_coef(float c, const LogFix& fx = LogFix{nullptr, nullptr, 0}) {
  const double a = (double)c;
  return 10.0 * log10_glibc_wrapper(a < 0.0 ? -a : a, fx);
}

// ---------------------------------------------------------------------------------------
// printf("%f") micro-units: round-half-even of the exact value x*1e6. Valid for |x| < 2^52/1e6
// (fingerprints are |x| < 460). two_prod(x, 1e6) = p + e exactly; only when p lands exactly on
// a half-integer does the sign of e decide.
TFP_HD int64_t fmt6(double x) {
  const double p = x * 1e6;
  const double e = __builtin_fma(x, 1e6, -p);
  double n = __builtin_rint(p);
  const double d = p - n;  // exact
  if (d == 0.5 || d == -0.5) {
    if (e > 0.0) n = p + 0.5;
    else if (e < 0.0) n = p - 0.5;
  }
  return (int64_t)n;
}

// fmt6 for a search bound that may be arbitrarily large (user tolerance): saturates far
// outside the range of any stored value, which preserves every comparison.
constexpr int64_t kBoundSat = (int64_t)1 << 60;
TFP_HD int64_t fmt6_bound(double x) {
  if (!(x < 1e12)) return kBoundSat;     // also +inf
  if (!(x > -1e12)) return -kBoundSat;   // also -inf
  return fmt6(x);
}

// Fingerprint value as stored: NULL when 10*log10|c| is ±inf/NaN (c == 0), else fmt6.
TFP_HD int32_t micro_of_db(double q) {
  const double inf = u2d(0x7ff0000000000000ull);
  if (!(q > -inf && q < inf)) return kNullMicro;
  return (int32_t)fmt6(q);
}

// ---------------------------------------------------------------------------------------
// Fast exact finish: micro_of_db(10 * log10|c|) of a float coefficient without the full log.
// The stored value is an integer of micro-units, so 10 log10|c| is needed to full precision only
// when it lies next to a rounding boundary of the 10^-6 grid. micro_of_coef_fast() computes
//   q~ = e K + l10c[i] + P(r),   |c| = 2^e m, m in [1, 2), i = the top 7 mantissa bits,
//   r = m invc[i] - 1,  l10c[i] = -10 log10(invc[i]),  P(r) ~ 10 log10(1 + r),
// then p = q~ 10^6, n = rint(p), and decides n when |p - n| < 1/2 - kFinMargin; otherwise it
// reports the value undecided and the caller runs micro_of_db(db_of_coef(c)).
//
// Error of q~ against the true 10 log10|c| (normal floats: |e| <= 127, |q| < 2^9):
//   r      exact: invc has 24 significant bits, so m invc (48 bits) and m invc - 1 are doubles;
//          |r| <= 2^-8 + 2^-23 (the bucket's half width over its centre, plus invc's rounding).
//   l10c   the correctly rounded double of -10 log10 of the rounded invc, < 3.02: <= 2^-53.
//   P      degree-6 Taylor of (10 / ln 10) log(1 + r): truncation <= 4.35 |r|^7 / (7 (1 - |r|))
//          < 2^-56.5; Horner's roundings (each <= 2^-53 of a partial sum < 4.4, then times
//          |r| <= 2^-8) and the last product's < 2^-57; coefficient rounding < 2^-58: < 2^-55.
//   e K    K = K_HI + K_LO with K_HI of 45 bits: e K_HI is exact; K_HI + K_LO is 10 log10(2) to
//          2^-97, times 127; t1 = fma(e, K_LO, l10c) and t2 = t1 + P round at < 4: 2 * 2^-52.
//   q~     = fma(e, K_HI, t2) rounds at < 2^9: <= 2^-45 (the dominant term).
//   total  < 2^-45 + 2^-51 + 2^-53 + 2^-55 < 1.02 * 2^-45 = 2.9e-14, i.e. 2.9e-8 micro-units.
// p = q~ 10^6 rounds at < 2^29: <= 2^-25 = 3.0e-8 micro-units. p - n is exact.
// glibc's own value q_g = 10.0 * log10(x) against the true one (e_log10.c: z = y log10_2lo +
// ivln10 log(m'); v = z + y log10_2hi, m' in [0.5, 2)): log(m') within 1 ulp <= 2^-53; ivln10
// log(m') (ivln10 to 2^-55, the product rounded at < 0.31) < 2^-53.3; z rounds at < 0.31:
// 2^-55; y log10_2hi is exact (40 x 8 bits); v rounds at < 2^6: 2^-48; so |v - log10 x| <
// 2^-47.95, and q_g = 10 v rounds at < 2^9: 2^-45; |q_g - q| < 10 * 2^-47.95 + 2^-45 < 6.6e-14,
// i.e. 6.6e-8 micro-units.
// So |p - 10^6 q_g| < 2.9e-8 + 3.0e-8 + 6.6e-8 = 1.25e-7 < kFinMargin = 2^-22 = 2.38e-7. When
// |p - n| < 1/2 - kFinMargin, the exact 10^6 q_g lies strictly inside (n - 1/2, n + 1/2), and
// fmt6(q_g) = n: no tie, no dependence on glibc's last bits. Checked against glibc over all 2^32
// bit patterns (tests/native/check_micro_fast.cpp; log under profiles/). A value is undecided
// with probability 2 kFinMargin = 4.8e-7.
// Zeros, infinities and NaNs give kNullMicro (log10 is -inf, +inf, NaN: micro_of_db's NULL) from
// the bit pattern alone; subnormals are reported undecided.
struct FinEntry { double invc, l10c; };
constexpr double kFinMargin = 0x1p-22;             // micro-units
constexpr double kFinThr = 0.5 - kFinMargin;       // decided iff |p - rint(p)| < thr (exact)
#if defined(__HIPCC__) || defined(__HIP__)
__host__ __device__
#endif
inline const FinEntry* fin_table() {
  // scripts/gen_fin_table.py
  static constexpr FinEntry T[128] = {
      {0x1.fe01fe0000000p-1, 0x1.156832e30da53p-6}, {0x1.fa11ca0000000p-1, 0x1.9e7fd7c55e623p-5},
      {0x1.f6310a0000000p-1, 0x1.58162d40b97dep-4}, {0x1.f25f640000000p-1, 0x1.dfe0ed39f1e47p-4},
      {0x1.ee9c800000000p-1, 0x1.335224efb067cp-3}, {0x1.eae8080000000p-1, 0x1.7632307771537p-3},
      {0x1.e741aa0000000p-1, 0x1.b892826586226p-3}, {0x1.e3a9180000000p-1, 0x1.fa74dbdcccda9p-3},
      {0x1.e01e020000000p-1, 0x1.1deda15a5edcbp-2}, {0x1.dca01e0000000p-1, 0x1.3e63b6ed6b043p-2},
      {0x1.d92f220000000p-1, 0x1.5e9d992a97c67p-2}, {0x1.d5cac80000000p-1, 0x1.7e9c1be8e9f4bp-2},
      {0x1.d272ca0000000p-1, 0x1.9e60213ea9aedp-2}, {0x1.cf26e60000000p-1, 0x1.bdea733b7a662p-2},
      {0x1.cbe6da0000000p-1, 0x1.dd3be95c238fcp-2}, {0x1.c8b2660000000p-1, 0x1.fc555531014b4p-2},
      {0x1.c5894e0000000p-1, 0x1.0d9bb71970a54p-1}, {0x1.c26b540000000p-1, 0x1.1cf185e18bf34p-1},
      {0x1.bf583e0000000p-1, 0x1.2c2c75282d466p-1}, {0x1.bc4fd60000000p-1, 0x1.3b4cd50ba1060p-1},
      {0x1.b951e20000000p-1, 0x1.4a530f3fc3f47p-1}, {0x1.b65e2e0000000p-1, 0x1.593f750f5f56fp-1},
      {0x1.b374840000000p-1, 0x1.6812673e01d0ep-1}, {0x1.b094b40000000p-1, 0x1.76cc2d4bc0c3fp-1},
      {0x1.adbe880000000p-1, 0x1.856d32939d748p-1}, {0x1.aaf1d20000000p-1, 0x1.93f5be7187247p-1},
      {0x1.a82e660000000p-1, 0x1.a2661265c70aep-1}, {0x1.a574100000000p-1, 0x1.b0be9e8b61fdep-1},
      {0x1.a2c2a80000000p-1, 0x1.beff98cb092f1p-1}, {0x1.a01a020000000p-1, 0x1.cd29505c669b8p-1},
      {0x1.9d79f20000000p-1, 0x1.db3c18faabaf5p-1}, {0x1.9ae24e0000000p-1, 0x1.e938401b283bcp-1},
      {0x1.9852f00000000p-1, 0x1.f71e01bb5b478p-1}, {0x1.95cbb00000000p-1, 0x1.0276d44e55ee6p+0},
      {0x1.934c680000000p-1, 0x1.0953bc4afda64p+0}, {0x1.90d4f20000000p-1, 0x1.1025dcaeacebfp+0},
      {0x1.8e65280000000p-1, 0x1.16ed5b4806afbp+0}, {0x1.8bfce80000000p-1, 0x1.1daa54a22568ep+0},
      {0x1.899c100000000p-1, 0x1.245ce6fdec20bp+0}, {0x1.87427c0000000p-1, 0x1.2b05380492b06p+0},
      {0x1.84f00c0000000p-1, 0x1.31a363cfe97f2p+0}, {0x1.82a4a00000000p-1, 0x1.38378817745afp+0},
      {0x1.8060180000000p-1, 0x1.3ec1c433c3033p+0}, {0x1.7e22560000000p-1, 0x1.454233500f5a0p+0},
      {0x1.7beb3a0000000p-1, 0x1.4bb8f7f69887bp+0}, {0x1.79baa60000000p-1, 0x1.522630791ff9fp+0},
      {0x1.7790820000000p-1, 0x1.5889eaf114c56p+0}, {0x1.756cac0000000p-1, 0x1.5ee454632ab89p+0},
      {0x1.734f0c0000000p-1, 0x1.65357db8b662fp+0}, {0x1.7137860000000p-1, 0x1.6b7d851179863p+0},
      {0x1.6f26020000000p-1, 0x1.71bc7de36c150p+0}, {0x1.6d1a620000000p-1, 0x1.77f28f1a0a259p+0},
      {0x1.6b14900000000p-1, 0x1.7e1fc8bc801a2p+0}, {0x1.6914740000000p-1, 0x1.8444420cd482dp+0},
      {0x1.6719f40000000p-1, 0x1.8a6019b5b4b00p+0}, {0x1.6524f80000000p-1, 0x1.9073698477f5ap+0},
      {0x1.63356c0000000p-1, 0x1.967e3ffd63d1dp+0}, {0x1.614b360000000p-1, 0x1.9c80bf7f282a9p+0},
      {0x1.5f66440000000p-1, 0x1.a27af27bdaceep+0}, {0x1.5d867c0000000p-1, 0x1.a86cfdb226461p+0},
      {0x1.5babcc0000000p-1, 0x1.ae56edb2b2247p+0}, {0x1.59d6200000000p-1, 0x1.b438d65a41ed1p+0},
      {0x1.5805600000000p-1, 0x1.ba12d975b48a8p+0}, {0x1.56397c0000000p-1, 0x1.bfe5001ea5306p+0},
      {0x1.54725e0000000p-1, 0x1.c5af67c7bef85p+0}, {0x1.52aff60000000p-1, 0x1.cb721b5c78451p+0},
      {0x1.50f22e0000000p-1, 0x1.d12d3a58ef232p+0}, {0x1.4f38f60000000p-1, 0x1.d6e0d18152b87p+0},
      {0x1.4d843c0000000p-1, 0x1.dc8cf50c5686ap+0}, {0x1.4bd3ee0000000p-1, 0x1.e231ba1cc050bp+0},
      {0x1.4a27fa0000000p-1, 0x1.e7cf36c2f45f2p+0}, {0x1.4880520000000p-1, 0x1.ed657474cc47bp+0},
      {0x1.46dce40000000p-1, 0x1.f2f48aee491c9p+0}, {0x1.453d9e0000000p-1, 0x1.f87c92dd74abdp+0},
      {0x1.43a2740000000p-1, 0x1.fdfd91471a2dfp+0}, {0x1.420b520000000p-1, 0x1.01bbd3ad73423p+1},
      {0x1.40782e0000000p-1, 0x1.04756a5809cc9p+1}, {0x1.3ee8f40000000p-1, 0x1.072b9e1387f5cp+1},
      {0x1.3d5d9a0000000p-1, 0x1.09de6f59c6068p+1}, {0x1.3bd60e0000000p-1, 0x1.0c8decf0bbc8dp+1},
      {0x1.3a52440000000p-1, 0x1.0f3a1b7f6fc4ep+1}, {0x1.38d22e0000000p-1, 0x1.11e30384cc624p+1},
      {0x1.3755be0000000p-1, 0x1.1488addbb9786p+1}, {0x1.35dce60000000p-1, 0x1.172b23bbac056p+1},
      {0x1.34679a0000000p-1, 0x1.19ca6b1e5250ep+1}, {0x1.32f5ce0000000p-1, 0x1.1c668a499df32p+1},
      {0x1.3187760000000p-1, 0x1.1eff87d049ae6p+1}, {0x1.301c820000000p-1, 0x1.219571e22b4dfp+1},
      {0x1.2eb4ea0000000p-1, 0x1.2428486ea5062p+1}, {0x1.2d50a00000000p-1, 0x1.26b816a268838p+1},
      {0x1.2bef980000000p-1, 0x1.2944e45559daep+1}, {0x1.2a91ca0000000p-1, 0x1.2bceb23c08e97p+1},
      {0x1.2937260000000p-1, 0x1.2e55902e6f18ap+1}, {0x1.27dfa40000000p-1, 0x1.30d97f6f8a42dp+1},
      {0x1.268b380000000p-1, 0x1.335a88fcc4d58p+1}, {0x1.2539d80000000p-1, 0x1.35d8b259deaf6p+1},
      {0x1.23eb7a0000000p-1, 0x1.3854014a9e27ep+1}, {0x1.22a0120000000p-1, 0x1.3acc7fa68d7e9p+1},
      {0x1.2157980000000p-1, 0x1.3d422fe80f84cp+1}, {0x1.2012020000000p-1, 0x1.3fb51895645e8p+1},
      {0x1.1ecf440000000p-1, 0x1.42254456c1ac6p+1}, {0x1.1d8f560000000p-1, 0x1.4492b65e4a89dp+1},
      {0x1.1c52300000000p-1, 0x1.46fd720f17927p+1}, {0x1.1b17c60000000p-1, 0x1.496582d85a773p+1},
      {0x1.19e0120000000p-1, 0x1.4bcae8a87894cp+1}, {0x1.18ab080000000p-1, 0x1.4e2daf70b4657p+1},
      {0x1.1778a20000000p-1, 0x1.508dd78821b1ep+1}, {0x1.1648d60000000p-1, 0x1.52eb6964a5658p+1},
      {0x1.151b9a0000000p-1, 0x1.55466dc07eab5p+1}, {0x1.13f0e80000000p-1, 0x1.579ee58bb0d35p+1},
      {0x1.12c8b80000000p-1, 0x1.59f4d5e44424dp+1}, {0x1.11a3020000000p-1, 0x1.5c48441c26e13p+1},
      {0x1.107fbc0000000p-1, 0x1.5e9939cdf2b90p+1}, {0x1.0f5ee00000000p-1, 0x1.60e7b8a87698ep+1},
      {0x1.0e40660000000p-1, 0x1.6333c69b0ebccp+1}, {0x1.0d24460000000p-1, 0x1.657d69ca2055dp+1},
      {0x1.0c0a780000000p-1, 0x1.67c4a88f5e97cp+1}, {0x1.0af2f80000000p-1, 0x1.6a098125ab909p+1},
      {0x1.09ddba0000000p-1, 0x1.6c4c0295239bap+1}, {0x1.08cabc0000000p-1, 0x1.6e8c2740515a0p+1},
      {0x1.07b9f20000000p-1, 0x1.70c9fea01234ep+1}, {0x1.06ab5a0000000p-1, 0x1.7305835cc1db7p+1},
      {0x1.059eea0000000p-1, 0x1.753ec1210fc73p+1}, {0x1.04949c0000000p-1, 0x1.7775bb5796076p+1},
      {0x1.038c6c0000000p-1, 0x1.79aa71483df15p+1}, {0x1.0286500000000p-1, 0x1.7bdcef3681af8p+1},
      {0x1.0182440000000p-1, 0x1.7e0d34bb1c4c5p+1}, {0x1.0080400000000p-1, 0x1.803b4a2f38bd8p+1},
  };
  return T;
}

// T: the 128-entry table (device code passes a copy staged in LDS). thr: kFinThr, or less (tests:
// thr <= 0 leaves every finite non-zero value undecided). *undecided is always written.
TFP_HD int32_t micro_of_coef_fast(float c, bool* undecided, const FinEntry* T = fin_table(), double thr = kFinThr) {
  const double K_HI = 0x1.8151824c75800p+1, K_LO = 0x1.fabf59b5d80b8p-45;  // 10 log10(2)
  const double A1 = 0x1.15f2ced384f29p+2, A2 = -0x1.15f2ced384f29p+1, A3 = 0x1.729913c4b1436p+0;
  const double A4 = -0x1.15f2ced384f29p+0, A5 = 0x1.bcb7b1526e50ep-1, A6 = -0x1.729913c4b1436p-1;
  const uint32_t ix = f2u(c) & 0x7fffffffu;
  const uint32_t be = ix >> 23;
  const bool null = ix == 0 || be == 255;  // +-0, +-inf, NaN
  const uint32_t mant = ix & 0x7fffffu;
  const FinEntry t = T[mant >> 16];
  const double m = u2d(0x3ff0000000000000ull | ((uint64_t)mant << 29));
  const double e = (double)((int32_t)be - 127);
  const double r = __builtin_fma(m, t.invc, -1.0);
  double P = __builtin_fma(A6, r, A5);
  P = __builtin_fma(P, r, A4);
  P = __builtin_fma(P, r, A3);
  P = __builtin_fma(P, r, A2);
  P = __builtin_fma(P, r, A1);
  P = P * r;
  const double t1 = __builtin_fma(e, K_LO, t.l10c);
  const double q = __builtin_fma(e, K_HI, t1 + P);
  const double p = q * 1e6;
  const double n = __builtin_rint(p);
  const double d = p - n;
  *undecided = !null && !(be != 0 && (d < 0.0 ? -d : d) < thr);
  return null ? kNullMicro : (int32_t)n;
}

}  // namespace tfp
