// check_live_trace.cpp — the carry argument of tfp_live_occurrences on the host, no GPU: a track's
// summary (csrc/tfp_occur.hpp's TraceSeg) kept over the final frames and extended by the frames that
// became final, in live_trace_kernel's shape (steps of 64 frames, one frame per lane, the 64 lane
// summaries joined by the shuffle tree in lane order, the step's summary appended to the carried one,
// the provisional tail frame's hit joined into a copy only), against the one-shot trace of the frames
// so far after every arrival, however the frames arrive. Prints OK.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "tfp_occur.hpp"

using namespace tfp;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                \
    }                                                         \
  } while (0)

// The definition: the hitting frames of [lo, hi) walked once (tiresias_fp.h's trace).
static TraceOut direct(const std::vector<char>& hit, int64_t lo, int64_t hi, int32_t max_gap) {
  TraceOut o{(int32_t)(hi > lo ? hi - lo : 0), 0, 0, 0, 0, 0};
  int64_t prev = -1, first = 0, n = 0;
  auto close = [&](int64_t last) {
    if (n > o.seg_hits) o.seg_hits = (int32_t)n, o.seg_first = (int32_t)first, o.seg_last = (int32_t)last;
  };
  for (int64_t x = lo; x < hi; x++) {
    if (!hit[(size_t)x]) continue;
    o.hits++;
    if (prev < 0 || x - prev - 1 > (int64_t)max_gap) {
      if (prev >= 0) close(prev);
      o.segments++;
      first = x;
      n = 0;
    }
    n++;
    prev = x;
  }
  if (prev >= 0) close(prev);
  return o;
}

// live_trace_kernel's fold of the final frames [beg, end) into the carried summary.
static void fold(TraceSeg& acc, const std::vector<char>& hit, int64_t beg, int64_t end, int32_t max_gap) {
  for (int64_t x0 = beg; x0 < end; x0 += 64) {
    TraceSeg t[64];
    for (int l = 0; l < 64; l++) {
      t[l] = trace_none();
      const int64_t x = x0 + l;
      if (x < end && hit[(size_t)x]) trace_push(t[l], (int32_t)x, max_gap);
    }
    for (int off = 1; off < 64; off <<= 1)
      for (int l = 0; l + off < 64; l += 2 * off) t[l] = trace_join(t[l], t[l + off], max_gap);
    acc = trace_join(acc, t[0], max_gap);
  }
}

static bool same(const TraceOut& a, const TraceOut& b) {
  return a.overlap == b.overlap && a.hits == b.hits && a.segments == b.segments && a.seg_hits == b.seg_hits &&
         a.seg_first == b.seg_first && a.seg_last == b.seg_last;
}

// A call of F final frames arriving `step` at a time (0: all at once), a track covering [lo, hi): after
// every arrival, with and without a provisional tail frame behind the final ones, the carried summary
// plus the tail equals the one-shot trace. tail_hit[x]: the hit of frame x while it is still the tail
// (its values change until it is final, so it may differ from hit[x]).
static int64_t run(const std::vector<char>& hit, const std::vector<char>& tail_hit, int64_t lo, int64_t hi, int64_t step,
                   int32_t max_gap) {
  const int64_t F = (int64_t)hit.size();
  TraceSeg acc = trace_none();
  int64_t done = lo, checks = 0;
  for (int64_t Ff = step ? step : F;; Ff += step) {
    if (Ff > F) Ff = F;
    const int64_t end = Ff < hi ? Ff : hi, beg = done;
    if (end > beg) fold(acc, hit, beg, end, max_gap), done = end;
    for (int with_tail = 0; with_tail < 2; with_tail++) {
      if (with_tail && Ff >= F) break;
      TraceSeg ans = acc;
      const int64_t Fall = Ff + with_tail;  // the frames so far, the tail included
      std::vector<char> now(hit.begin(), hit.begin() + Fall);
      if (with_tail) {
        now[(size_t)Ff] = tail_hit[(size_t)Ff];
        if (Ff >= lo && Ff < hi && tail_hit[(size_t)Ff]) trace_push(ans, (int32_t)Ff, max_gap);
      }
      const int64_t h = Fall < hi ? Fall : hi;
      CHECK(same(trace_result((int32_t)(h > lo ? h - lo : 0), ans), direct(now, lo, h, max_gap)));
      checks++;
    }
    if (Ff >= F) break;
  }
  // the stored summary never took a tail's hit: it is the final frames' alone
  CHECK(same(trace_result((int32_t)(hi - lo), acc), direct(hit, lo, hi, max_gap)));
  return checks;
}

int main() {
  std::mt19937 rng(0x11FE);
  const int32_t gaps[] = {0, 1, 5, INT32_MAX};
  const int64_t steps[] = {1, 63, 64, 65, 0};
  int64_t checks = 0;
  for (int round = 0; round < 120; round++) {
    const int64_t F = 1 + rng() % 300;
    const int density = 1 + rng() % 9;
    std::vector<char> hit((size_t)F), tail_hit((size_t)F);
    for (auto& h : hit) h = (int)(rng() % 10) < density;
    for (auto& h : tail_hit) h = rng() % 2;
    if (round % 9 == 0) std::fill(hit.begin(), hit.end(), round % 18 == 0);  // all-hit and no-hit
    const int64_t lo = round % 3 ? rng() % F : 0, hi = round % 5 ? lo + 1 + rng() % (F - lo) : F;
    for (const int32_t g : gaps)
      for (const int64_t st : steps) checks += run(hit, tail_hit, lo, hi, st, g);
  }
  CHECK(checks > 100000);
  printf("%lld checks\nOK\n", (long long)checks);
  return 0;
}
