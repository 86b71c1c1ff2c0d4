// tfp_slide_align.hpp — sliding aligned search: the alignment (tfp_align.hpp) of every window of a
// recording (tfp_slide.hpp) with the clips of that window's rows. For window w of a recording (its
// frames [w * hop, w * hop + window)) and a clip, the result is the tfp_alignment of a query made of
// that window's frames alone: aligned_count, the smallest offset attaining it, first_frame and
// last_frame, all window-relative. The windows of one occurrence of a clip share offset - w * hop
// wherever the occurrence's diagonal alone attains the count (the smallest diagonal wins a tie).
//
// Consecutive windows share all but hop frames, so a clip's diagonal counts move from one window to
// the next by subtracting hit(x, x + D) for the hop frames that left and adding it for the hop that
// entered, D being the diagonal counted from the run's first frame (clip row minus frame): the
// window-relative diagonal of window s of the run is d = D + s * hop. Exact integers over the same
// FrameBox predicate align_band_kernel tests.
//
// The (window, row) entries of a call are grouped on the host by (recording, clip), windows
// ascending, and cut into runs wherever two successive needed windows share no frame. A run with one
// entry, and every run when 2 * hop >= window (a slid step tests 2 * hop * N boxes, a window from
// scratch window * N), is sent to launch_align as ordinary AlignPairs; the rest to
// launch_slide_align.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_align.hpp"

namespace tfp {

// Entries per run. A run's block walks its windows in turn, so a long run is a long serial chain
// and few blocks; a run of n > kSlideAlignRun entries is cut into ceil(n / kSlideAlignRun) runs of
// near-equal length (each of at least kSlideAlignRun / 2 entries, so never a single one).
constexpr int32_t kSlideAlignRun = 32;
constexpr int32_t kSlideAlignMaxRuns = 65535;  // runs per launch (the grid's second dimension)

// One run: the windows s = 0 .. nsteps - 1 of one recording against one clip, window s being the
// boxes [f0 + s * hop, f0 + s * hop + window). steps[e0 + s] = the entry (numbered within the call's
// slid entries) that wants window s, or -1 where no entry does (the window is stepped through).
struct SlideAlignRun {
  int64_t row0;  // the clip's rows [row0, row0 + N) of the staging arrays
  int64_t f0;    // the run's first box
  int32_t N;
  int32_t nsteps;
  int32_t e0;
  int32_t pad;
};

// The frames a run covers, and the bands of kAlignBand run-relative diagonals D in [-(L - 1), N - 1].
TFP_HD int64_t slide_align_frames(int64_t nsteps, int64_t window, int64_t hop) { return (nsteps - 1) * hop + window; }
TFP_HD int64_t slide_align_bands(int64_t nsteps, int64_t window, int64_t hop, int64_t N) {
  return align_bands(slide_align_frames(nsteps, window, hop), N);
}

// nruns <= kSlideAlignMaxRuns runs whose entries are the call's slid entries [ent0, ent0 + nent):
// d_out[i] = the alignment of entry ent0 + i. d_pairs[i] = that entry as an AlignPair (its window's
// first box, F = window), d_nb[i] = slide_align_bands of its run; max_bands >= every d_nb[i];
// d_part: nent * max_bands keys of scratch. hop < window.
hipError_t launch_slide_align(const SlideAlignRun* d_runs, int32_t nruns, const int32_t* d_steps, int32_t ent0,
                              int32_t nent, const AlignPair* d_pairs, const int32_t* d_nb, int64_t max_bands,
                              int32_t window, int32_t hop, const FrameBox* boxes, const int32_t* st_m1,
                              const int32_t* st_m2, bool coefs2, unsigned long long* d_part, AlignOut* d_out,
                              hipStream_t s);

}  // namespace tfp
