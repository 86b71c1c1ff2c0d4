// tfp_live_plan.hpp — the frame-range arithmetic of a live call's push (tfp_live.hpp), as plain host
// functions with no GPU call (tests/native/check_live_plan.cpp runs them under ASan/UBSan).
//
// A recording of S samples has ceil(S / 256) frames; frame f reads samples [256 (f - 1), 256 (f + 1)),
// zeros before the start and past the end (fp_handler.c:577-671). So frames [0, floor(S / 256)) are
// final, they never change as samples arrive, and at most one frame, floor(S / 256), is provisional:
// the zero-padded tail, present when S % 256 != 0.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

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

// A verdict's argument rules (tiresias_fp.h), one statement for the engine and for a group (which
// checks before any shard is told, against its own per-channel sample counts): false with the reason
// in msg. coefs: params->coefs, or nullptr for NULL params; scopes may be nullptr (every clip).
inline bool live_verdict_args_ok(const int64_t* total, const int32_t* coefs, const int32_t* scopes, const int64_t* samples,
                                 int32_t nch, int64_t max_samples, char* msg, size_t cap) {
  if (!total || !coefs) {
    snprintf(msg, cap, "live verdict: NULL total_samples or params");
    return false;
  }
  if (*coefs != 1) {
    snprintf(msg, cap, "live verdict: coefs = %d (the counts a verdict reads are coefs = 1's)", *coefs);
    return false;
  }
  for (int32_t c = 0; c < nch; c++) {
    if (scopes && scopes[c] < -1) {  // below TFP_SCOPE_ANY
      snprintf(msg, cap, "live verdict: scope %d of channel %d", scopes[c], c);
      return false;
    }
    if (total[c] < samples[c] || total[c] > max_samples) {
      snprintf(msg, cap, "live verdict: total_samples[%d] = %lld outside [%lld, %lld]", c, (long long)total[c],
               (long long)samples[c], (long long)max_samples);
      return false;
    }
  }
  return true;
}

// The early verdict (tfp_live_verdict) of one channel with S samples of a planned `total`, from the two
// greatest candidate keys k0 >= k1 of launch_live_verdict: ((base count << 32) | tie key) + 1, 0 where
// there is no such candidate. leader / rival are the packed keys without the + 1.
// A clip gains at most one count per frame that is not final yet, so once the leader's
// (count, tie key) exceeds the rival's (count + remaining, tie key), and the rival bounds every other
// candidate, no continuation of the recording can put another clip first.
struct LiveVerdictRule {
  unsigned long long leader, rival;
  int32_t has_leader, has_rival, remaining, complete, decided;
};
inline LiveVerdictRule live_verdict_rule(unsigned long long k0, unsigned long long k1, int64_t S, int64_t total) {
  LiveVerdictRule r{0, 0, 0, 0, 0, 0, 0};
  r.complete = S == total ? 1 : 0;
  r.remaining = r.complete ? 0 : (int32_t)(live_frames(total) - live_final_frames(S));
  if (k0 && ((k0 - 1) >> 32) >= 1) {
    r.has_leader = 1;
    r.leader = k0 - 1;
    if (k1) {
      r.has_rival = 1;
      r.rival = k1 - 1;
    }
  }
  bool beats = r.has_leader && !r.has_rival;
  if (r.has_rival) {
    const unsigned long long lc = r.leader >> 32, lt = r.leader & 0xffffffffull;
    const unsigned long long rc = (r.rival >> 32) + (unsigned long long)r.remaining, rt = r.rival & 0xffffffffull;
    beats = lc > rc || (lc == rc && lt > rt);
  }
  r.decided = (r.complete || beats) ? 1 : 0;
  return r;
}

}  // namespace tfp
