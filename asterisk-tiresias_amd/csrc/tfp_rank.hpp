// tfp_rank.hpp — ranked search: the first K rows of the reference's result query
// ("select *, count(*) from temp group by audio_uuid order by count(*) DESC", fp_handler.c:367-374)
// instead of its first row alone. A row is the packed key count << 32 | tie key the other search
// forms maximise; SQLite orders the rows by (count descending, audio_uuid descending), which is
// the keys' descending order, so rank r is the r-th greatest key. Tie keys of live clips are
// distinct, so "the greatest key strictly below the previous round's" selects each row once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "tfp_kernels.hpp"

namespace tfp {

constexpr int32_t kRankMax = 32;         // TFP_RANK_MAX
// the launchers' own bound: catalog neighbours (tfp_neighbour.hpp) select k + 1 rows and delete one
constexpr int32_t kRankMaxInternal = kRankMax + 1;
constexpr int32_t kRankVoteCols = 1024;  // columns per rank_vote block (4 per thread)
inline int32_t rank_vote_blocks(int32_t C) { return (C + kRankVoteCols - 1) / kRankVoteCols; }

// coefs = 1, keys inside the vote range: d_keys[q * K + r] = row r of query q (0 past the last
// scoring clip) for the nq queries at relative frame offsets d_qoff[0..nq] of d_q, scored from the
// key bitsets d_bits (launch_key_bits) over C columns. d_part: nq * rank_vote_blocks(C) * K keys of
// scratch. *d_bad (zeroed by the caller) is set when a frame's key lies outside the range: the
// keys are then meaningless and the caller takes the general form.
hipError_t launch_rank_vote(const double* d_q, const int64_t* d_qoff, int32_t nq, SearchConsts sc, const uint32_t* d_bits,
                            int32_t C, const int32_t* d_tiekey, int32_t K, unsigned long long* d_part,
                            unsigned long long* d_keys, int32_t* d_bad, hipStream_t s);

// One wave per query: d_keys[q * K + r] = the r-th greatest of query q's nparts partial keys.
hipError_t launch_rank_merge(const unsigned long long* d_part, int32_t nq, int32_t nparts, int32_t K,
                             unsigned long long* d_keys, hipStream_t s);

}  // namespace tfp
