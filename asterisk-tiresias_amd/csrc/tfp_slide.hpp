// tfp_slide.hpp — sliding search: scoped ranked search (tfp_scope.hpp, tfp_rank.hpp) of every window
// of a long recording. The reference records a fixed duration and searches that one window
// (application_handler.c:152-185, fp_handler.c:275-374); a caller with a whole recording wants the
// first K rows of the result query (fp_handler.c:367-374) for the window frames
// [w * hop, w * hop + window) of the recording, for every w with a full window.
//
// Vote form (coefs = 1, keys inside the vote range): a keys pass turns each frame value into its key
// slot once for the whole recording (int16, -1 for a frame that runs no SQL); slide_vote_kernel
// gives one block a run of up to kSlideRun consecutive windows of one recording and one chunk of
// kRankVoteCols columns. The run's first window is scored as rank_vote_kernel scores a query (LDS
// histogram, one bitset word per used key); each later window subtracts the bitset words of the hop
// frames that left and adds those of the hop frames that entered, so a step costs O(hop) loads, not
// O(window). With hop >= window nothing is shared and every window is scored from its histogram
// (the frames in the gap between two windows are never read). Each window's K rounds write a
// partial list; ranked search's merge (launch_rank_merge) merges them, a window taking a query's place.
//
// General form (coefs = 2, a key outside the range, any other tolerance): slide_gather_kernel lays
// the windows' frame values end to end and the engine runs ranked search's general form on them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_kernels.hpp"
#include "tfp_rank.hpp"
#include "tfp_scope.hpp"

namespace tfp {

// Windows per run (TFP_SLIDE_RUN). A run starts with an O(window) scoring and then steps; a long run
// spreads that start over more windows, a short one gives more blocks. One 60 s recording (about
// 1,900 windows at hop 1) against 100k columns (98 chunks) gives 60 x 98 = 5,880 blocks at 32, nearly
// three times the 2,048 blocks 256 CUs hold, and the start (<= window loads) is then under a third
// of a run's loads for hop >= 2 at window 94.
constexpr int32_t kSlideRun = 32;
constexpr int32_t kSlideTile = 256;  // frames staged in LDS per step of a slide (one per thread)

// Windows w0 .. w0 + n - 1 (numbered within the launch) of one recording: window w0 + i is the
// frames [f0 + i * hop, f0 + i * hop + window) of the slots; 1 <= n <= kSlideRun.
struct SlideRun {
  int64_t f0;
  int32_t w0, n;
  int32_t scope;  // the recording's scope (>= kScopeAny)
  int32_t pad;
};

inline int64_t slide_windows(int64_t nframes, int64_t window, int64_t hop) {
  return (nframes <= 0 || window <= 0 || hop <= 0 || nframes < window) ? 0 : (nframes - window) / hop + 1;
}

// d_slots[i] = key slot (k + kKeyOffset) of frame i of d_q, -1 for a frame that runs no SQL or whose
// key lies outside the vote range; the latter sets *d_bad (zeroed by the caller).
hipError_t launch_slide_keys(const double* d_q, int64_t nf, SearchConsts sc, int16_t* d_slots, int32_t* d_bad,
                             hipStream_t s);

// d_keys[w * K + r] = row r of window w for the nwin windows the nruns runs cover (each window in
// one run), over the slots of launch_slide_keys, the key bitsets d_bits (launch_key_bits) and the
// scope table d_table (launch_scope_table) of C columns. d_part: nwin * rank_vote_blocks(C) * K keys
// of scratch. nruns <= 65535.
hipError_t launch_slide_vote(const int16_t* d_slots, const SlideRun* d_runs, int32_t nruns, int32_t nwin, int32_t window,
                             int32_t hop, const uint32_t* d_bits, int32_t C, const int32_t* d_tiekey, const int32_t* d_table,
                             int32_t K, unsigned long long* d_part, unsigned long long* d_keys, hipStream_t s);

// d_out (2 doubles per frame) = the frame values of nwin windows end to end: window w is the window
// frames of d_q from frame d_wsrc[w].
hipError_t launch_slide_gather(const double* d_q, const int64_t* d_wsrc, int32_t nwin, int32_t window, double* d_out,
                               hipStream_t s);

}  // namespace tfp
