// check_live_plan.cpp — the frame-range arithmetic of a live call's push (csrc/tfp_live_plan.hpp),
// host code with no GPU call, against a recording simulated sample by sample: which frames a push
// changes, which are final afterwards, and that the staged clip's kept frames read exactly the
// recording's samples. Built with ASan + UBSan by tests/test_live_abi.py. Prints OK.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "tfp_live_plan.hpp"

using namespace tfp;

// Frame f of a recording of S samples reads [256 (f - 1), 256 (f + 1)) clipped to [0, S): the range
// as (first, last + 1) of real samples (zeros elsewhere).
static void frame_reads(int64_t f, int64_t S, int64_t* lo, int64_t* hi) {
  *lo = 256 * (f - 1) < 0 ? 0 : 256 * (f - 1);
  *hi = 256 * (f + 1) > S ? S : 256 * (f + 1);
}

static int fail(const char* what, int64_t s_old, int64_t n) {
  printf("%s at s_old %lld n %lld\n", what, (long long)s_old, (long long)n);
  return 1;
}

int main() {
  if (live_capacity_ok(0) || !live_capacity_ok(1) || !live_capacity_ok(65535 * 256) || live_capacity_ok(65535 * 256 + 1) ||
      live_capacity_ok(-1))
    return fail("capacity", 0, 0);
  if (live_frames(0) != 0 || live_frames(1) != 1 || live_frames(256) != 1 || live_frames(257) != 2) return fail("frames", 0, 0);
  if (live_tail_frame(0) != -1 || live_tail_frame(255) != 0 || live_tail_frame(256) != -1 || live_tail_frame(257) != 1)
    return fail("tail", 0, 0);
  if (live_final_frames(kLiveMaxSamples) != 65535 || live_frames(kLiveMaxSamples) != 65535) return fail("max", 0, 0);
  long cases = 0;
  const int64_t olds[] = {0, 1, 2, 254, 255, 256, 257, 258, 511, 512, 513, 767, 768, 769, 1000, 4095, 4096, 4097};
  const int64_t news[] = {1, 2, 159, 160, 255, 256, 257, 511, 512, 513, 1000, 5000};
  for (int64_t s_old : olds)
    for (int64_t n : news) {
      const LivePlan p = live_plan(s_old, n);
      const int64_t S = s_old + n;
      if (p.s_new != S) return fail("s_new", s_old, n);
      // the frames whose reads differ between the old and the new recording, or that are new
      int64_t first_changed = -1;
      for (int64_t f = 0; f < live_frames(S); f++) {
        int64_t lo0, hi0, lo1, hi1;
        frame_reads(f, s_old, &lo0, &hi0);
        frame_reads(f, S, &lo1, &hi1);
        if (f >= live_frames(s_old) || lo0 != lo1 || hi0 != hi1) {
          first_changed = f;
          break;
        }
      }
      // every changed frame is fingerprinted: frames below f0 read only samples below s_old
      if (first_changed < p.f0) return fail("a final frame changed", s_old, n);
      if (p.f0 + p.keep != live_frames(S) || p.keep < 1) return fail("kept frames", s_old, n);
      if (p.clip_frames != p.keep + p.drop || p.drop != (p.f0 > 0)) return fail("lead-in", s_old, n);
      if (p.clip_beg < 0 || p.clip_beg > s_old || p.clip_beg % 256) return fail("clip start", s_old, n);
      if (live_frames(S - p.clip_beg) != p.clip_frames) return fail("clip frames", s_old, n);
      // kept clip frame j (clip frame j + drop) reads the recording's samples of frame f0 + j
      for (int64_t j = 0; j < p.keep; j++) {
        int64_t lo, hi, clo, chi;
        frame_reads(p.f0 + j, S, &lo, &hi);
        frame_reads(j + p.drop, S - p.clip_beg, &clo, &chi);
        if (clo + p.clip_beg != lo || chi + p.clip_beg != hi) return fail("clip frame reads", s_old, n);
        // and no zero-fill before the clip's start stands where the recording has samples
        if (256 * (j + p.drop - 1) < 0 && 256 * (p.f0 + j - 1) >= 0) return fail("lead-in zeros", s_old, n);
      }
      // final frames never include the tail; the tail is the only provisional frame
      const int64_t fin = live_final_frames(S), tail = live_tail_frame(S);
      if (tail >= 0 ? (tail != fin || fin + 1 != live_frames(S)) : fin != live_frames(S)) return fail("final / tail", s_old, n);
      if (live_final_frames(s_old) > fin) return fail("final frames shrink", s_old, n);
      cases++;
    }
  // a simulated call: pushes of varying sizes; the frames stored cover every frame exactly up to date
  std::vector<int64_t> stamp;  // per frame: the sample count it was last fingerprinted at
  int64_t S = 0;
  uint64_t r = 0x7153A1ull;
  for (int i = 0; i < 4000; i++) {
    r ^= r << 13, r ^= r >> 7, r ^= r << 17;
    const int64_t n = 1 + (int64_t)(r % 700);
    const LivePlan p = live_plan(S, n);
    S = p.s_new;
    stamp.resize((size_t)live_frames(S), -1);
    for (int64_t j = 0; j < p.keep; j++) stamp[(size_t)(p.f0 + j)] = S;
    for (int64_t f = 0; f < live_frames(S); f++) {
      // a frame is up to date if no sample it reads arrived after its last fingerprint
      const int64_t need = 256 * (f + 1) < S ? 256 * (f + 1) : S;
      if (stamp[(size_t)f] < need) return fail("stale frame", S, f);
    }
    cases++;
  }
  printf("%ld cases OK\n", cases);
  return 0;
}
