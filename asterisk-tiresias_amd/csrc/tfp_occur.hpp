// tfp_occur.hpp — the arithmetic of the diagonal trace and of occurrence search that needs no GPU
// (no HIP in this header: tests/native/check_occur.cpp compiles it with a host compiler).
//
// Trace. A clip with N rows laid on a recording of F frames with clip frame 0 at recording frame s
// covers the frames x in [lo, hi), lo = max(0, s), hi = min(F, s + N). hit(x, x - s) is aligned
// search's per-frame predicate (fp_handler.c:287-351). The hitting frames x_1 < ... < x_h fall into
// segments: maximal runs whose consecutive hits lie at most max_gap frames apart
// (x_{i+1} - x_i - 1 <= max_gap). The result names the hits, the segments and the best segment: the
// one with the most hits, the earliest of equals.
//
// TraceSeg is that summary for a stretch of frames, a monoid under trace_join: the summary of two
// adjacent stretches (the left one first) from their summaries. The kernel (tfp_trace.hip) folds a
// lane's frames with trace_push and joins the 64 lanes' summaries in lane order.
//
// Occurrences. The rows of a sliding aligned search name candidates (recording, clip,
// s = w * hop - offset); each is traced once, and within one (recording, clip) the traces are
// thinned by non-maximum suppression over the best segments' frame intervals (occur_select).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#ifdef __HIPCC__
#define TFP_OCCUR_HD __host__ __device__ __forceinline__
#else
#define TFP_OCCUR_HD inline
#endif

namespace tfp {

struct TraceOut {  // tfp_trace
  int32_t overlap, hits, segments, seg_hits, seg_first, seg_last;
};

// The frames [lo, hi) of a recording of F frames that a clip of N rows starting at frame s covers
// (hi <= lo: none), in 64 bits: s is any int32.
TFP_OCCUR_HD void trace_span(int64_t F, int64_t N, int64_t s, int64_t* lo, int64_t* hi) {
  *lo = s > 0 ? s : 0;
  *hi = s + N < F ? s + N : F;
}

struct TraceSeg {
  int32_t hits;         // 0: no hit, every other field unset
  int32_t first, last;  // the first and last hitting frame
  int32_t segs;
  int32_t lead_hits, lead_last;     // the first segment (it starts at first)
  int32_t trail_hits, trail_first;  // the last segment (it ends at last); segs == 1: the same one
  int32_t best_hits, best_first, best_last;
};

TFP_OCCUR_HD TraceSeg trace_none() { return TraceSeg{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// Frames a and b > a belong to one segment. b - a - 1 is in [0, 2^31 - 2]: no overflow at any max_gap.
TFP_OCCUR_HD bool trace_near(int32_t a, int32_t b, int32_t max_gap) { return b - a - 1 <= max_gap; }

// t with a hit at frame x appended, x greater than every frame of t.
TFP_OCCUR_HD void trace_push(TraceSeg& t, int32_t x, int32_t max_gap) {
  if (!t.hits) {
    t = TraceSeg{1, x, x, 1, 1, x, 1, x, 1, x, x};
    return;
  }
  if (trace_near(t.last, x, max_gap)) {
    t.trail_hits++;
    if (t.segs == 1) t.lead_hits++, t.lead_last = x;
  } else {
    t.segs++;
    t.trail_hits = 1;
    t.trail_first = x;
  }
  t.hits++;
  t.last = x;
  // (the trailing segment starts after every other: it is the best only with more hits)
  if (t.trail_hits > t.best_hits) t.best_hits = t.trail_hits, t.best_first = t.trail_first, t.best_last = x;
}

// The summary of a's frames followed by b's (every frame of a below every frame of b).
TFP_OCCUR_HD TraceSeg trace_join(const TraceSeg& a, const TraceSeg& b, int32_t max_gap) {
  if (!a.hits) return b;
  if (!b.hits) return a;
  TraceSeg r;
  r.hits = a.hits + b.hits;
  r.first = a.first;
  r.last = b.last;
  r.lead_hits = a.lead_hits, r.lead_last = a.lead_last;
  r.trail_hits = b.trail_hits, r.trail_first = b.trail_first;
  r.best_hits = a.best_hits, r.best_first = a.best_first, r.best_last = a.best_last;
  if (trace_near(a.last, b.first, max_gap)) {
    // a's trailing and b's leading segment are one
    const int32_t mh = a.trail_hits + b.lead_hits, mf = a.trail_first, ml = b.lead_last;
    r.segs = a.segs + b.segs - 1;
    if (a.segs == 1) r.lead_hits = mh, r.lead_last = ml;
    if (b.segs == 1) r.trail_hits = mh, r.trail_first = mf;
    // (it starts after a's best unless it holds it, and then has no fewer hits: strictly more, or a's stays)
    if (mh > r.best_hits || (mh == r.best_hits && mf < r.best_first)) r.best_hits = mh, r.best_first = mf, r.best_last = ml;
  } else {
    r.segs = a.segs + b.segs;
  }
  // (b's best starts after every segment so far)
  if (b.best_hits > r.best_hits) r.best_hits = b.best_hits, r.best_first = b.best_first, r.best_last = b.best_last;
  return r;
}

TFP_OCCUR_HD TraceOut trace_result(int32_t overlap, const TraceSeg& t) {
  if (!t.hits) return TraceOut{overlap, 0, 0, 0, 0, 0};
  return TraceOut{overlap, t.hits, t.segs, t.best_hits, t.best_first, t.best_last};
}

// ---- occurrence search: candidates, suppression, order (host) ----------------------------------

struct OccurRow {  // one row of a sliding aligned search
  int32_t rec;     // the recording
  int32_t clip;    // the caller's number for the clip (one per audio_uuid)
  int64_t w;       // the window's index inside the recording
  int32_t offset;  // the row's tfp_alignment.offset
};

struct OccurCand {
  int32_t rec, clip;
  int32_t s;        // the recording frame at which clip frame 0 lies: w * hop - offset
  int32_t windows;  // rows naming the candidate
};

// The distinct (rec, clip, s) of the rows, by (rec, clip, s) ascending, each with its row count.
inline std::vector<OccurCand> occur_candidates(const std::vector<OccurRow>& rows, int32_t hop) {
  std::vector<OccurCand> c;
  c.reserve(rows.size());
  for (const OccurRow& r : rows) c.push_back(OccurCand{r.rec, r.clip, (int32_t)(r.w * hop - r.offset), 1});
  std::sort(c.begin(), c.end(), [](const OccurCand& a, const OccurCand& b) {
    return std::tie(a.rec, a.clip, a.s) < std::tie(b.rec, b.clip, b.s);
  });
  size_t n = 0;
  for (size_t i = 0; i < c.size(); i++) {
    if (n && c[n - 1].rec == c[i].rec && c[n - 1].clip == c[i].clip && c[n - 1].s == c[i].s)
      c[n - 1].windows++;
    else
      c[n++] = c[i];
  }
  c.resize(n);
  return c;
}

// The candidates that are occurrences, as indices into cand (sorted as occur_candidates leaves it)
// in output order. trace[i] is candidate i's trace. Candidates whose best segment has fewer than
// min_hits hits are dropped; within one (rec, clip) the rest are visited by seg_hits descending,
// windows descending, s ascending, and one is kept unless its [seg_first, seg_last] meets the
// interval of one kept before it. Output: rec ascending, seg_first ascending, seg_hits descending,
// audio_uuid descending (fp_handler.c:367-374's tie order); uuid_of(clip) is the clip's audio_uuid.
template <class UuidOf>
std::vector<int64_t> occur_select(const std::vector<OccurCand>& cand, const TraceOut* trace, int32_t min_hits,
                                  UuidOf uuid_of) {
  std::vector<int64_t> kept, grp;
  for (size_t a = 0; a < cand.size();) {
    size_t b = a;
    grp.clear();
    for (; b < cand.size() && cand[b].rec == cand[a].rec && cand[b].clip == cand[a].clip; b++)
      if (trace[b].seg_hits >= min_hits) grp.push_back((int64_t)b);
    std::sort(grp.begin(), grp.end(), [&](int64_t x, int64_t y) {
      if (trace[x].seg_hits != trace[y].seg_hits) return trace[x].seg_hits > trace[y].seg_hits;
      if (cand[x].windows != cand[y].windows) return cand[x].windows > cand[y].windows;
      return cand[x].s < cand[y].s;
    });
    const size_t k0 = kept.size();
    for (const int64_t i : grp) {
      bool meets = false;
      for (size_t j = k0; j < kept.size() && !meets; j++)
        meets = trace[i].seg_first <= trace[kept[j]].seg_last && trace[kept[j]].seg_first <= trace[i].seg_last;
      if (!meets) kept.push_back(i);
    }
    a = b;
  }
  std::sort(kept.begin(), kept.end(), [&](int64_t x, int64_t y) {
    if (cand[x].rec != cand[y].rec) return cand[x].rec < cand[y].rec;
    if (trace[x].seg_first != trace[y].seg_first) return trace[x].seg_first < trace[y].seg_first;
    if (trace[x].seg_hits != trace[y].seg_hits) return trace[x].seg_hits > trace[y].seg_hits;
    if (cand[x].clip == cand[y].clip) return cand[x].s < cand[y].s;  // (never: one clip's kept intervals are disjoint)
    return std::string(uuid_of(cand[x].clip)) > std::string(uuid_of(cand[y].clip));
  });
  return kept;
}

}  // namespace tfp
