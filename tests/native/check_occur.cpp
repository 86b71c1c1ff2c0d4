// check_occur.cpp — csrc/tfp_occur.hpp on the host, no GPU: the trace monoid folded and joined as
// tfp_trace.hip does it (64 contiguous chunks, a shuffle tree in lane order) against a direct walk of
// the hits, and occurrence search's grouping, suppression, order and count against a direct
// restatement of include/tiresias_fp.h's steps. Prints OK.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <string>
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

// The definition: the hitting frames of [lo, hi) walked once.
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

// The kernel's shape: lane l folds chunk l, then lane l joins lane l + off for off = 1, 2, .. 32.
static TraceOut as_kernel(const std::vector<char>& hit, int64_t lo, int64_t hi, int32_t max_gap) {
  const int64_t n = hi > lo ? hi - lo : 0, chunk = (n + 63) / 64;
  TraceSeg t[64];
  for (int l = 0; l < 64; l++) {
    t[l] = trace_none();
    const int64_t a = lo + l * chunk, b = a + chunk < hi ? a + chunk : hi;
    for (int64_t x = a; x < b; x++)
      if (hit[(size_t)x]) trace_push(t[l], (int32_t)x, max_gap);
  }
  for (int off = 1; off < 64; off <<= 1)
    for (int l = 0; l + off < 64; l += 2 * off) t[l] = trace_join(t[l], t[l + off], max_gap);
  return trace_result((int32_t)n, t[0]);
}

static bool same(const TraceOut& a, const TraceOut& b) {
  return a.overlap == b.overlap && a.hits == b.hits && a.segments == b.segments && a.seg_hits == b.seg_hits &&
         a.seg_first == b.seg_first && a.seg_last == b.seg_last;
}

static void check_trace() {
  std::mt19937 rng(0x0CC);
  const int32_t gaps[] = {0, 1, 3, 11, INT32_MAX};
  int64_t multi = 0, tied = 0;
  for (int round = 0; round < 1500; round++) {
    const int64_t F = 1 + rng() % 400;
    const int density = 1 + rng() % 9;
    std::vector<char> hit((size_t)F);
    for (auto& h : hit) h = (int)(rng() % 10) < density;
    if (round % 7 == 0) std::fill(hit.begin(), hit.end(), round % 14 == 0);  // all-hit and no-hit
    const int64_t lo = rng() % F, hi = lo + 1 + rng() % (F - lo);
    for (const int32_t g : gaps) {
      const TraceOut d = direct(hit, lo, hi, g), k = as_kernel(hit, lo, hi, g);
      CHECK(same(d, k));
      multi += d.segments >= 2;
      if (d.segments >= 2) {  // two segments tie for the best: the earlier one is named
        TraceOut later = direct(hit, d.seg_last + 1, hi, g);
        tied += later.seg_hits == d.seg_hits;
      }
    }
  }
  CHECK(multi > 1000 && tied > 50);
  // trace_span in 64 bits: any int32 start
  int64_t lo, hi;
  trace_span(700, 300, INT32_MIN, &lo, &hi);
  CHECK(hi <= lo);
  trace_span(700, 300, INT32_MAX, &lo, &hi);
  CHECK(hi <= lo);
  trace_span(700, 300, -10, &lo, &hi);
  CHECK(lo == 0 && hi == 290);
  trace_span(700, 300, 650, &lo, &hi);
  CHECK(lo == 650 && hi == 700);
  CHECK(trace_near(0, INT32_MAX, INT32_MAX) && !trace_near(0, 2, 0) && trace_near(0, 2, 1));
}

// include/tiresias_fp.h's steps 3-5 restated: quadratic, no sorting of index lists.
static std::vector<int64_t> select_direct(const std::vector<OccurCand>& c, const std::vector<TraceOut>& t, int32_t min_hits,
                                          const std::vector<std::string>& uuid) {
  const size_t n = c.size();
  std::vector<char> state(n, 0);  // 0 undecided, 1 kept, 2 gone
  for (size_t i = 0; i < n; i++)
    if (t[i].seg_hits < min_hits) state[i] = 2;
  for (;;) {
    // the undecided candidate that is visited first within its (rec, clip)
    int64_t pick = -1;
    for (size_t i = 0; i < n; i++) {
      if (state[i]) continue;
      bool firstOfGroup = true;
      for (size_t j = 0; j < n && firstOfGroup; j++) {
        if (j == i || state[j] || c[j].rec != c[i].rec || c[j].clip != c[i].clip) continue;
        const auto ki = std::make_tuple(-t[i].seg_hits, -c[i].windows, c[i].s);
        const auto kj = std::make_tuple(-t[j].seg_hits, -c[j].windows, c[j].s);
        if (kj < ki) firstOfGroup = false;
      }
      if (firstOfGroup) {
        pick = (int64_t)i;
        break;
      }
    }
    if (pick < 0) break;
    bool meets = false;
    for (size_t j = 0; j < n; j++)
      if (state[j] == 1 && c[j].rec == c[pick].rec && c[j].clip == c[pick].clip && t[pick].seg_first <= t[j].seg_last &&
          t[j].seg_first <= t[pick].seg_last)
        meets = true;
    state[(size_t)pick] = meets ? 2 : 1;
  }
  std::vector<int64_t> out;
  for (size_t i = 0; i < n; i++)
    if (state[i] == 1) out.push_back((int64_t)i);
  for (size_t a = 0; a < out.size(); a++)  // insertion sort by the output order
    for (size_t b = a; b > 0; b--) {
      const int64_t x = out[b - 1], y = out[b];
      const auto kx = std::make_tuple(c[x].rec, t[x].seg_first, -t[x].seg_hits), ky = std::make_tuple(c[y].rec, t[y].seg_first, -t[y].seg_hits);
      if (ky < kx || (ky == kx && uuid[c[y].clip] > uuid[c[x].clip])) std::swap(out[b - 1], out[b]);
      else break;
    }
  return out;
}

static void check_occurrences() {
  std::mt19937 rng(0x5E1);
  // clip numbers in an order unlike their uuids', with a byte above 0x7f: the order is memcmp's
  const std::vector<std::string> uuid = {"m-3", "a-0", "z-9", "\xc3\xa9-1", "b-7"};
  int64_t dups = 0, suppressed = 0, low = 0, ties = 0;
  for (int round = 0; round < 400; round++) {
    std::vector<OccurRow> rows;
    const int32_t hop = 1 + rng() % 7, nrows = rng() % 60;
    for (int i = 0; i < nrows; i++)
      rows.push_back(OccurRow{(int32_t)(rng() % 3), (int32_t)(rng() % 5), (int64_t)(rng() % 12), (int32_t)(rng() % 9) - 4});
    const std::vector<OccurCand> cand = occur_candidates(rows, hop);
    // every row is counted once, under its own (rec, clip, s), and the list is sorted and distinct
    std::map<std::tuple<int32_t, int32_t, int32_t>, int32_t> want;
    for (const OccurRow& r : rows) want[std::make_tuple(r.rec, r.clip, (int32_t)(r.w * hop - r.offset))]++;
    CHECK(cand.size() == want.size());
    size_t i = 0;
    for (const auto& kv : want) {
      CHECK(std::make_tuple(cand[i].rec, cand[i].clip, cand[i].s) == kv.first && cand[i].windows == kv.second);
      dups += kv.second > 1;
      i++;
    }
    std::vector<TraceOut> tr(cand.size());
    for (auto& t : tr) {
      const int32_t first = rng() % 40, len = rng() % 12, hits = 1 + rng() % 4;
      t = TraceOut{50, hits + (int32_t)(rng() % 3), 1 + (int32_t)(rng() % 2), hits, first, first + len};
    }
    const int32_t min_hits = 1 + rng() % 3;
    const std::vector<int64_t> got =
        occur_select(cand, tr.data(), min_hits, [&](int32_t c) { return uuid[(size_t)c].c_str(); });
    const std::vector<int64_t> exp = select_direct(cand, tr, min_hits, uuid);
    CHECK(got == exp);  // (its size is the count a call reports and checks against its capacity)
    int64_t ok = 0;
    for (const auto& t : tr) ok += t.seg_hits >= min_hits;
    low += (int64_t)tr.size() - ok;
    suppressed += ok - (int64_t)got.size();
    for (size_t a = 1; a < got.size(); a++) {
      const int64_t x = got[a - 1], y = got[a];
      if (cand[x].rec == cand[y].rec && tr[x].seg_first == tr[y].seg_first && tr[x].seg_hits == tr[y].seg_hits) {
        CHECK(uuid[cand[x].clip] > uuid[cand[y].clip]);
        ties++;
      }
    }
  }
  CHECK(dups > 100 && suppressed > 100 && low > 100 && ties > 5);
  CHECK(occur_candidates({}, 3).empty());
  CHECK(occur_select(std::vector<OccurCand>(), nullptr, 1, [](int32_t) { return ""; }).empty());
}

int main() {
  check_trace();
  check_occurrences();
  printf("OK\n");
  return 0;
}
