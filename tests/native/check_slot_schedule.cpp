// What the fingerprint kernels read of DspTables (tfp_tables.cpp build_tables), rebuilt into the
// dense filterbank (build_mel_dense) at every sample rate given: the sparse filters, the 3 x 16
// slot schedule indexed exactly as mel3 / mel3_fixed index it, the slot-2 deferral flags and,
// where there is one, the frame-pair schedule (fb_schedule_check.hpp).
//
//   check_slot_schedule RATE | FIRST:LAST:STEP ...
//
// A single rate prints one line of its table shape,
//   "rate R len A B C total T maxbin M defer D real R0 R1 empty E onebin O fb F nf N"
// or "rate R rejected" when build_tables refuses it. A range prints only its rejected rates (same
// line) and, as "fixedshape FIRST-LAST", the runs of rates whose tables have the shape of the 8 kHz
// ones (slots 36/16/8 in 960 floats, deferral on, a frame-pair schedule of 34 filters: the host
// side of DspTables_fixed8k). The last line is "OK: N rates, R rejected, ms_maxbin <= M" (M the
// greatest ms_maxbin met: build_tables refuses a rate whose M would pass 500); the first
// violation ends the program with "FAIL rate R: ..." and status 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fb_schedule_check.hpp"

using namespace tfp;

static DspTables T;
static float mel[kFilters][kBins];

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

#define FAIL(...) \
  do { printf("FAIL rate %d: ", sr); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

struct Shape {
  int empty, onebin;
  bool fixedshape;
};

// 0: every check holds (sh filled), 1: a violation (printed), 2: build_tables refused the rate
static int check_rate(int sr, Shape* sh) {
  memset(&T, 0xa5, sizeof T);  // build_tables must not depend on what the block held
  if (!build_tables(sr, &T)) return 2;
  build_mel_dense(sr, mel);

  // (a) the sparse form
  int total = 0, empty = 0, onebin = 0;
  for (int j = 0; j < kFilters; j++) {
    const int st = T.mel_start[j], len = T.mel_len[j];
    if (len < 0 || st < 0 || st + len > kBins) FAIL("filter %d: bins [%d, %d + %d)", j, st, st, len);
    if (T.mel_off[j] != total) FAIL("filter %d: mel_off %d, lengths so far %d", j, T.mel_off[j], total);
    float row[kBins];
    memset(row, 0, sizeof row);
    for (int i = 0; i < len; i++) row[st + i] = T.mel_w[T.mel_off[j] + i];
    if (memcmp(row, mel[j], sizeof row) != 0) FAIL("filter %d: sparse weights differ from the dense row", j);
    bool zero = true;
    for (int b = 0; b < kBins; b++) zero &= bits(mel[j][b]) == 0;
    if ((len == 0) != zero) FAIL("filter %d: mel_len %d, dense row %s", j, len, zero ? "all zero" : "not zero");
    if (len > 0 && (mel[j][st] == 0.f || mel[j][st + len - 1] == 0.f)) FAIL("filter %d: a zero end weight", j);
    total += len;
    empty += len == 0;
    onebin += len == 1;
  }
  if (T.mel_total != total || total > kFilters * kBins) FAIL("mel_total %d, lengths %d", T.mel_total, total);
  if (T.sample_rate != sr) FAIL("sample_rate %d", T.sample_rate);

  // (b) the slot schedule, as mel3 reads it: bin ms_start[sl][L] + q, weight
  // ms_w[ms_woff[sl] + (q >> 2) * 64 + L * 4 + (q & 3)]
  int woff = 0, seen[kFilters], unused = 0;
  memset(seen, 0, sizeof seen);
  if (T.ms_maxbin < kBins || T.ms_maxbin > 500) FAIL("ms_maxbin %d", T.ms_maxbin);
  for (int sl = 0; sl < 3; sl++) {
    const int len = T.ms_len[sl];
    if (len < 0 || len % 4 != 0) FAIL("slot %d: ms_len %d", sl, len);
    if (sl > 0 && len > T.ms_len[sl - 1]) FAIL("slot %d longer than slot %d", sl, sl - 1);  // mel3's phases
    if (T.ms_woff[sl] != woff) FAIL("slot %d: ms_woff %d, lens so far %d", sl, T.ms_woff[sl], woff);
    for (int L = 0; L < 16; L++) {
      const int j = T.ms_filter[sl][L], st = T.ms_start[sl][L];
      if (j < -1 || j >= kFilters) FAIL("slot %d lane %d: filter %d", sl, L, j);
      if (st < 0 || st % 4 != 0 || st + len > T.ms_maxbin) FAIL("slot %d lane %d: ms_start %d, len %d", sl, L, st, len);
      if (j >= 0) seen[j]++; else unused++;
      const int f0 = j >= 0 ? T.mel_start[j] : 0, f1 = j >= 0 ? f0 + T.mel_len[j] : 0;  // the filter's bins
      if (j >= 0 && f1 > f0 && (f0 < st || f1 > st + len)) FAIL("slot %d lane %d: filter %d not covered", sl, L, j);
      for (int q = 0; q < len; q++) {
        const int bin = st + q, wi = T.ms_woff[sl] + (q >> 2) * 64 + L * 4 + (q & 3);
        if (wi < 0 || wi >= 3 * (kBins + 8) * 16) FAIL("slot %d lane %d step %d: weight index %d", sl, L, q, wi);
        const uint32_t w = bits(T.ms_w[wi]);
        const uint32_t want = (bin >= f0 && bin < f1) ? bits(mel[j][bin]) : 0u;  // f1 <= 257: bins past 256 are +0
        if (w != want) FAIL("slot %d lane %d step %d (filter %d, bin %d): weight %08x, dense %08x", sl, L, q, j, bin, w, want);
      }
    }
    woff += 16 * len;
  }
  if (T.ms_total != woff || woff > 3 * (kBins + 8) * 16) FAIL("ms_total %d, lens %d", T.ms_total, woff);
  for (int j = 0; j < kFilters; j++)
    if (seen[j] != 1) FAIL("filter %d in %d lanes", j, seen[j]);
  if (unused != 48 - kFilters) FAIL("%d unused lanes", unused);

  // (c) the slot-2 deferral
  int real[16], nreal = 0;
  for (int L = 0; L < 16; L++) {
    const int j = T.ms_filter[2][L];
    if (j >= 0 && T.mel_len[j] > 0) real[nreal++] = j;
  }
  if (T.ms_c_defer != (nreal <= 2 ? 1 : 0)) FAIL("ms_c_defer %d with %d non-empty filters in slot 2", T.ms_c_defer, nreal);
  for (int i = 0; i < 2; i++) {
    const int r = T.ms_c_real[i];
    bool in = false;
    for (int k = 0; k < nreal; k++) in |= real[k] == r;
    if (r != -1 && !in) FAIL("ms_c_real[%d] = %d is no non-empty filter of slot 2", i, r);
  }
  if (T.ms_c_defer) {
    for (int k = 0; k < nreal; k++)
      if (T.ms_c_real[0] != real[k] && T.ms_c_real[1] != real[k]) FAIL("ms_c_real misses filter %d", real[k]);
    if ((T.ms_c_real[0] >= 0) + (T.ms_c_real[1] >= 0) != nreal) FAIL("ms_c_real %d %d for %d filters", T.ms_c_real[0], T.ms_c_real[1], nreal);
    if (nreal == 2 && T.ms_c_real[0] == T.ms_c_real[1]) FAIL("ms_c_real names filter %d twice", T.ms_c_real[0]);
  }

  // (d) the frame-pair schedule
  if (T.fb_ok != 0 && T.fb_ok != 1) FAIL("fb_ok %d", T.fb_ok);
  if (T.fb_ok) {
    if (T.fb_nfilters != kFilters - empty) FAIL("fb_nfilters %d, non-empty filters %d", T.fb_nfilters, kFilters - empty);
    for (int j = 0; j < kFilters; j++)
      if ((T.mel_len[j] > 0) != (j < T.fb_nfilters)) FAIL("filter %d: empty filters are not the last ones", j);
    if (check_fb_schedule(T, mel)) FAIL("the frame-pair schedule (line above)");
  }
  sh->empty = empty;
  sh->onebin = onebin;
  sh->fixedshape = T.ms_len[0] == 36 && T.ms_len[1] == 16 && T.ms_len[2] == 8 && T.ms_total == 960 && T.ms_c_defer == 1 &&
                   T.fb_ok == 1 && T.fb_nfilters == 34;
  return 0;
}

int main(int argc, char** argv) {
  long nrates = 0, nrejected = 0;
  int maxbin = 0;
  for (int a = 1; a < argc; a++) {
    long first = 0, last = 0, step = 1;
    const int n = sscanf(argv[a], "%ld:%ld:%ld", &first, &last, &step);
    if (n != 1 && n != 3) { printf("bad argument %s\n", argv[a]); return 2; }
    if (n == 1) last = first;
    if (first < 1 || last > 2147483647L || step < 1) { printf("bad argument %s\n", argv[a]); return 2; }
    long run0 = -1, run1 = -1;
    for (long r = first; r <= last; r += step) {
      Shape sh;
      const int rc = check_rate((int)r, &sh);
      if (rc == 1) return 1;
      nrates++;
      if (rc == 2) {
        nrejected++;
        printf("rate %ld rejected\n", r);
        continue;
      }
      if (T.ms_maxbin > maxbin) maxbin = T.ms_maxbin;
      if (n == 1)
        printf("rate %ld len %d %d %d total %d maxbin %d defer %d real %d %d empty %d onebin %d fb %d nf %d\n", r, T.ms_len[0],
               T.ms_len[1], T.ms_len[2], T.ms_total, T.ms_maxbin, T.ms_c_defer, T.ms_c_real[0], T.ms_c_real[1], sh.empty,
               sh.onebin, T.fb_ok, T.fb_ok ? T.fb_nfilters : -1);
      else if (sh.fixedshape) {
        if (run0 < 0) run0 = r;
        run1 = r;
      } else if (run0 >= 0) {
        printf("fixedshape %ld-%ld\n", run0, run1);
        run0 = -1;
      }
    }
    if (run0 >= 0) printf("fixedshape %ld-%ld\n", run0, run1);
  }
  printf("OK: %ld rates, %ld rejected, ms_maxbin <= %d\n", nrates, nrejected, maxbin);
  return 0;
}
