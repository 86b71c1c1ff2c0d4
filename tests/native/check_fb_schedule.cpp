// The throughput kernel's frame-pair filterbank schedule (tfp_tables.cpp build_fb_schedule) at the
// sample rate given as the first argument (8000 without one) against the dense filterbank: the
// reconstruction of fb_schedule_check.hpp. Prints "OK: N filters ..." with N the tables'
// fb_nfilters, or the first violation.
#include <stdio.h>
#include <stdlib.h>

#include "fb_schedule_check.hpp"

using namespace tfp;

static DspTables T;
static float mel[kFilters][kBins];

int main(int argc, char** argv) {
  const int sr = argc > 1 ? atoi(argv[1]) : 8000;
  if (!build_tables(sr, &T)) { printf("build_tables failed\n"); return 2; }
  if (!T.fb_ok) { printf("no frame-pair schedule at %d Hz\n", sr); return 3; }
  build_mel_dense(sr, mel);
  if (check_fb_schedule(T, mel)) return 1;
  printf("OK: %d filters in %d patterns x %d steps\n", T.fb_nfilters, kFbPatterns, kFbSteps);
  return 0;
}
