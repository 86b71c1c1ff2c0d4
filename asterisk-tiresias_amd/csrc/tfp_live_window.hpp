// tfp_live_window.hpp — the frame-range arithmetic of a live call's trailing window (tfp_live_window,
// tfp_live.hpp), as plain host functions with no GPU call (tests/native/check_live_window.cpp runs
// them under ASan/UBSan).
//
// A channel with S samples has F = ceil(S / 256) frames, of which [0, Ff), Ff = floor(S / 256), are
// final (tfp_live_plan.hpp). Its window of `window` frames is [first, F), first = max(0, F - window):
// the provisional tail, frame Ff, belongs to it when there is one. The window's count row holds the
// final frames of the window only, [first, Ff); the selection adds the tail's bit. Note that first
// advances by one when a tail appears (S = 256 n + 1) although no frame became final.
#pragma once
#include <stdint.h>

#include "tfp_live_plan.hpp"

namespace tfp {

// What a window call asks of one channel's count row, which holds the frames [wbeg, wend) (empty:
// wbeg == wend, the row is all zero) and is `valid` when it was built under the table's stamp.
struct LiveWindowPlan {
  int64_t frames;    // F - first: the window's frames, the tail included
  int64_t first;     // first frame of the window
  int64_t a, b;      // the row's target: the window's final frames [first, Ff)
  int64_t sub_beg, sub_end;  // frames to subtract from the row (empty when restart)
  int64_t add_beg, add_end;  // frames to add to it
  int32_t restart;   // 1: the row starts again from zero instead of being loaded
  int32_t owes;      // 1: the row changes (a descriptor for the slide kernel); 0: it already fits
  int64_t visited;   // frames the kernel reads for this channel: (sub_end - sub_beg) + (add_end - add_beg)
  int64_t dropped;   // frames a restart leaves behind without visiting them: wend - wbeg, 0 when sliding
};

// An empty, stale or disjoint row restarts and takes [a, b). Else the row slides: [wbeg, a) leaves and
// [wend, b) enters, unless restarting visits fewer frames (b - a < leaving + entering). A row that
// reaches past its target on either side (it cannot, while the stamp holds: first and Ff only grow
// between resets) restarts as well. So a call visits at most min(leaving + entering, b - a) frames of
// a channel, and none where the range already fits.
inline LiveWindowPlan live_window_plan(int64_t samples, int64_t window, bool valid, int64_t wbeg, int64_t wend) {
  LiveWindowPlan p{};
  const int64_t F = live_frames(samples);
  p.first = F > window ? F - window : 0;
  p.frames = F - p.first;
  p.a = p.first;
  p.b = live_final_frames(samples);  // (a <= b: window >= 1, and F - 1 <= Ff)
  const bool empty = !valid || wbeg >= wend;
  if (empty) {
    wbeg = wend = 0;
  }
  bool restart = empty || wend <= p.a || wbeg >= p.b || wbeg > p.a || wend > p.b;
  if (!restart) {
    const int64_t slide = (p.a - wbeg) + (p.b - wend);
    restart = p.b - p.a < slide;
  }
  if (restart) {
    p.restart = 1;
    p.sub_beg = p.sub_end = 0;
    p.add_beg = p.a;
    p.add_end = p.b;
    p.dropped = wend - wbeg;
    p.owes = (p.b > p.a || p.dropped > 0) ? 1 : 0;  // an empty row that stays empty is left alone
  } else {
    p.sub_beg = wbeg;
    p.sub_end = p.a;
    p.add_beg = wend;
    p.add_end = p.b;
    p.owes = (p.sub_end > p.sub_beg || p.add_end > p.add_beg) ? 1 : 0;
  }
  p.visited = (p.sub_end - p.sub_beg) + (p.add_end - p.add_beg);
  return p;
}

// window_ms of audio at `rate` samples per second in frames of 256 samples, rounded up, at least 1.
inline int64_t live_window_frames_of_ms(int64_t window_ms, int64_t rate) {
  if (window_ms <= 0 || rate <= 0) return 1;
  const int64_t num = window_ms * rate, den = 1000 * kLiveHop;
  const int64_t f = (num + den - 1) / den;
  return f < 1 ? 1 : f;
}

}  // namespace tfp
