// tfp_live_plan.hpp — the frame-range arithmetic of a live call's push (tfp_live.hpp), as plain host
// functions with no GPU call (tests/native/check_live_plan.cpp runs them under ASan/UBSan).
//
// A recording of S samples has ceil(S / 256) frames; frame f reads samples [256 (f - 1), 256 (f + 1)),
// zeros before the start and past the end (fp_handler.c:577-671). So frames [0, floor(S / 256)) are
// final, they never change as samples arrive, and at most one frame, floor(S / 256), is provisional:
// the zero-padded tail, present when S % 256 != 0.
#pragma once
#include <stdint.h>

namespace tfp {

constexpr int64_t kLiveHop = 256;                       // TFP_HOP
constexpr int64_t kLiveMaxSamples = 65535 * kLiveHop;   // a channel's final frames fit a 16-bit count

inline bool live_capacity_ok(int64_t max_samples) { return max_samples >= 1 && max_samples <= kLiveMaxSamples; }
inline int64_t live_frames(int64_t samples) { return samples <= 0 ? 0 : (samples + kLiveHop - 1) / kLiveHop; }
inline int64_t live_final_frames(int64_t samples) { return samples <= 0 ? 0 : samples / kLiveHop; }
// The provisional frame of a recording of `samples` samples, -1 when every frame is final.
inline int64_t live_tail_frame(int64_t samples) { return samples > 0 && samples % kLiveHop ? samples / kLiveHop : -1; }

// What a push of n_new > 0 samples onto s_old fingerprints: the frames [f0, f0 + keep) of the
// recording, f0 = floor(s_old / 256) (the old tail, if any, and everything after it), as one clip of
// samples [clip_beg, s_new): with f0 > 0 the clip starts one hop early, so its first frame (the
// lead-in, which reads zeros where the recording has samples) is dropped and its second frame reads
// exactly the recording's [256 (f0 - 1), 256 (f0 + 1)).
struct LivePlan {
  int64_t s_new;        // samples after the push
  int64_t f0;           // first frame fingerprinted
  int64_t clip_beg;     // first sample of the staged clip: 256 (f0 - 1), or 0 when f0 = 0
  int64_t clip_frames;  // frames launched: keep + drop
  int64_t keep;         // frames stored at f0 ...: ceil(s_new / 256) - f0 >= 1
  int32_t drop;         // 1: the clip's first frame is the lead-in
};
inline LivePlan live_plan(int64_t s_old, int64_t n_new) {
  LivePlan p;
  p.s_new = s_old + n_new;
  p.f0 = live_final_frames(s_old);
  p.drop = p.f0 > 0 ? 1 : 0;
  p.clip_beg = p.drop ? kLiveHop * (p.f0 - 1) : 0;
  p.clip_frames = live_frames(p.s_new - p.clip_beg);
  p.keep = p.clip_frames - p.drop;
  return p;
}

}  // namespace tfp
