// check_live_window.cpp — the frame-range arithmetic of a live call's trailing window
// (csrc/tfp_live_window.hpp), host code with no GPU call, against sets of frames kept one flag per
// frame: what leaves a channel's count row, what enters it, when the row restarts, and that no call
// visits more frames than min(leaving + entering, target). Built with ASan + UBSan by
// tests/test_live_window_abi.py. Prints OK.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "tfp_live_window.hpp"

using namespace tfp;

static int fail(const char* what, int64_t S, int64_t tick, int64_t window, int64_t every) {
  printf("%s at S %lld tick %lld window %lld every %lld\n", what, (long long)S, (long long)tick, (long long)window,
         (long long)every);
  return 1;
}

static int64_t count(const std::vector<char>& v) { return std::count(v.begin(), v.end(), 1); }

int main() {
  if (live_window_frames_of_ms(2000, 8000) != 63 || live_window_frames_of_ms(32, 8000) != 1 ||
      live_window_frames_of_ms(33, 8000) != 2 || live_window_frames_of_ms(0, 8000) != 1 ||
      live_window_frames_of_ms(1, 8000) != 1 || live_window_frames_of_ms(64, 8000) != 2 ||
      live_window_frames_of_ms(2000, 16000) != 125 || live_window_frames_of_ms(-5, 8000) != 1)
    return fail("window_ms", 0, 0, 0, 0);
  const int64_t kMaxS = 2600, NF = kMaxS / 256 + 3;
  const int64_t ticks[] = {1, 160, 255, 256, 257, 1000}, windows[] = {1, 2, 3, 7, 100};
  // every: a window call after every `every`-th push (ingest-only pushes between: the row falls behind)
  const int64_t everys[] = {1, 2, 3, 5, 9};
  long cases = 0, restarts = 0, slides = 0, idle = 0;
  for (int64_t tick : ticks)
    for (int64_t window : windows)
      for (int64_t every : everys) {
        int64_t wbeg = 0, wend = 0, step = 0;
        for (int64_t S = 0; S <= kMaxS; S += tick, step++) {
          if (step % every) continue;
          const LiveWindowPlan p = live_window_plan(S, window, true, wbeg, wend);
          // the definition
          const int64_t F = (S + 255) / 256, Ff = S / 256, first = std::max<int64_t>(0, F - window);
          if (p.first != first || p.frames != F - first || p.a != first || p.b != Ff) return fail("definition", S, tick, window, every);
          if (S % 256 && (first > Ff || p.frames < 1)) return fail("tail outside the window", S, tick, window, every);
          std::vector<char> row(NF, 0), tgt(NF, 0), res(NF, 0);
          for (int64_t f = wbeg; f < wend; f++) row[f] = 1;
          for (int64_t f = first; f < Ff; f++) tgt[f] = 1;
          int64_t leaving = 0, entering = 0;
          for (int64_t f = 0; f < NF; f++) {
            leaving += row[f] && !tgt[f];
            entering += tgt[f] && !row[f];
          }
          // the plan applied to the row, frame by frame: nothing subtracted that is not there, nothing added twice
          if (!p.restart) res = row;
          if (p.restart && p.sub_end != p.sub_beg) return fail("restart subtracts", S, tick, window, every);
          if (p.sub_beg > p.sub_end || p.add_beg > p.add_end || p.sub_beg < 0 || p.add_beg < 0 || p.sub_end > NF || p.add_end > NF)
            return fail("range order", S, tick, window, every);
          for (int64_t f = p.sub_beg; f < p.sub_end; f++) {
            if (!res[f]) return fail("subtracts a frame the row does not hold", S, tick, window, every);
            res[f] = 0;
          }
          for (int64_t f = p.add_beg; f < p.add_end; f++) {
            if (res[f]) return fail("adds a frame twice", S, tick, window, every);
            if (f >= Ff) return fail("adds a frame that is not final", S, tick, window, every);
            res[f] = 1;
          }
          if (res != tgt) return fail("row != target", S, tick, window, every);
          // a sliding row's ranges are the set differences; a restart's add is the target
          const int64_t nsub = p.sub_end - p.sub_beg, nadd = p.add_end - p.add_beg;
          if (p.visited != nsub + nadd) return fail("visited", S, tick, window, every);
          if (!p.restart && (nsub != leaving || nadd != entering)) return fail("slide != set difference", S, tick, window, every);
          if (p.restart && (nadd != count(tgt) || p.dropped != count(row))) return fail("restart != target", S, tick, window, every);
          if (!p.restart && p.dropped) return fail("slide drops", S, tick, window, every);
          // restart exactly when it visits fewer frames (an empty row costs the same either way: it restarts)
          const bool fewer = count(tgt) < leaving + entering;
          if (count(row) ? (p.restart != 0) != fewer : !p.restart) return fail("restart choice", S, tick, window, every);
          if (p.visited > std::min(leaving + entering, count(tgt))) return fail("bound", S, tick, window, every);
          if ((p.owes != 0) != (row != tgt)) return fail("owes", S, tick, window, every);
          (p.owes ? (p.restart ? restarts : slides) : idle)++;
          wbeg = p.a, wend = p.b;
          cases++;
          // a stale row (any range) restarts into the target and drops nothing it can name
          const LiveWindowPlan st = live_window_plan(S, window, false, 3, 9);
          if (!st.restart || st.add_beg != first || st.add_end != Ff || st.dropped != 0 || st.sub_beg != st.sub_end ||
              st.owes != (Ff > first ? 1 : 0))
            return fail("stale", S, tick, window, every);
        }
      }
  if (!restarts || !slides || !idle) return fail("a path was never taken", restarts, slides, idle, 0);
  printf("%ld cases (%ld restarts, %ld slides, %ld idle)\nOK\n", cases, restarts, slides, idle);
  return 0;
}
