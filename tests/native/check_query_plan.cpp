// check_query_plan.cpp — a search batch's offset arithmetic (csrc/tfp_query_plan.hpp) against the public
// header's rules, stand-alone on the CPU (tests/test_query_plan_host.py builds it with ASan + UBSan). Each
// "frames n f" / "windows nframes window hop w" line it prints is a value of the header's that the test
// compares with the library's exported tfp_frame_count / tfp_sliding_windows.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/tiresias_fp.h"
#include "tfp_query_plan.hpp"

using namespace tfp;

static int fail(const char* what, long long a, long long b) {
  printf("FAIL %s: %lld vs %lld\n", what, a, b);
  return 1;
}

// tiresias_fp.h: tfp_frame_count = ceil(n / TFP_HOP); tfp_sliding_windows = the full windows, hop apart
static int64_t spec_frames(int64_t n) {
  int64_t f = 0;
  while (f * TFP_HOP < n) f++;
  return f;
}
static int64_t spec_windows(int64_t nframes, int64_t window, int64_t hop) {
  int64_t w = 0;
  while (window >= 1 && hop >= 1 && w * hop + window <= nframes) w++;
  return w;
}

int main() {
  // sample offsets to frame offsets, from a base other than 0
  const int64_t lens[] = {0, 1, TFP_HOP - 1, TFP_HOP, TFP_HOP + 1};
  std::vector<int64_t> off(1, 1000);
  for (int64_t n : lens) off.push_back(off.back() + n);
  const std::vector<int64_t> fo = sample_frame_offsets(off.data(), 5);
  if (fo.size() != 6 || fo[0] != 0) return fail("frame offsets size", (long long)fo.size(), fo[0]);
  for (int i = 0; i < 5; i++) {
    printf("frames %lld %lld\n", (long long)lens[i], (long long)plan_frames(lens[i]));
    if (plan_frames(lens[i]) != spec_frames(lens[i])) return fail("plan_frames", plan_frames(lens[i]), spec_frames(lens[i]));
    if (fo[i + 1] - fo[i] != spec_frames(lens[i])) return fail("frame offsets", fo[i + 1] - fo[i], spec_frames(lens[i]));
  }
  if (fo[5] != 0 + 1 + 1 + 1 + 2) return fail("frame total", fo[5], 5);
  const std::vector<int64_t> rel = relative_offsets(off.data(), 5);
  for (int i = 0; i <= 5; i++)
    if (rel[i] != off[i] - 1000) return fail("relative offsets", rel[i], off[i] - 1000);
  // a count below 1 reads no offset
  if (relative_offsets(nullptr, 0) != std::vector<int64_t>(1, 0) || relative_offsets(nullptr, -1) != std::vector<int64_t>(1, 0) ||
      sample_frame_offsets(nullptr, -1) != std::vector<int64_t>(1, 0) || !offsets_monotone(nullptr, 0) ||
      !offsets_monotone(nullptr, -1))
    return fail("empty batch", 0, 0);

  // monotone: equal neighbours pass, a fall anywhere does not
  const int64_t eq[] = {5, 5, 5, 9}, fall[] = {0, 4, 3, 9}, last[] = {0, 4, 9, 8};
  if (!offsets_monotone(eq, 3) || offsets_monotone(fall, 3) || offsets_monotone(last, 3) || !offsets_monotone(last, 2))
    return fail("monotone", 0, 0);

  // window offsets, window 8 and hop 4
  const int32_t W = 8, H = 4;
  const int64_t frames[] = {0, W - 1, W, W + H - 1, W + H};
  std::vector<int64_t> rfo(1, 0);
  for (int64_t n : frames) rfo.push_back(rfo.back() + n);
  const std::vector<int64_t> woff = window_offsets(rfo, 5, W, H);
  int64_t total = 0;
  for (int i = 0; i < 5; i++) {
    const int64_t want = spec_windows(frames[i], W, H);
    printf("windows %lld %d %d %lld\n", (long long)frames[i], W, H, (long long)(woff[i + 1] - woff[i]));
    if (woff[i + 1] - woff[i] != want) return fail("window offsets", woff[i + 1] - woff[i], want);
    total += want;
  }
  if (woff[0] != 0 || woff[5] != total || total != 0 + 0 + 1 + 1 + 2) return fail("window total", woff[5], total);
  if (window_offsets(rfo, 5, 0, H)[5] != 0 || window_offsets(rfo, 5, W, 0)[5] != 0) return fail("window or hop of 0", 0, 0);
  if (window_offsets(rfo, -1, W, H) != std::vector<int64_t>(1, 0)) return fail("no recording", 0, 0);

  // the capacity verdict: room for need - 1 and need, and a total past the 32-bit window index
  if (windows_fit(total, total - 1) || !windows_fit(total, total) || !windows_fit(0, 0)) return fail("capacity", total, total);
  const std::vector<int64_t> big = {0, (int64_t)INT32_MAX + 8};  // INT32_MAX + 1 windows of 8 frames, hop 1
  const int64_t nbig = window_offsets(big, 1, W, 1)[1];
  printf("windows %lld %d 1 %lld\n", (long long)big[1], W, (long long)nbig);
  if (nbig != (int64_t)INT32_MAX + 1) return fail("big total", nbig, (int64_t)INT32_MAX + 1);
  if (windows_fit(nbig, INT64_MAX) || !windows_fit(INT32_MAX, INT64_MAX)) return fail("capacity past 2^31", nbig, 0);

  // the census's bins: the longest query's frames + 1, 1 without a query
  if (census_need(fo.data(), 5) != 3 || census_need(rfo.data(), 5) != W + H + 1 || census_need(nullptr, 0) != 1)
    return fail("census bins", census_need(fo.data(), 5), 3);
  printf("OK\n");
  return 0;
}
