// tfp_census.hpp — match census: per query, how many clips of the query's scope the reference's
// result query (fp_handler.c:367-374) would list at each count(*):
//   select c, count(*) from (select count(*) c from temp group by audio_uuid) group by c
// over the table the scoped search sees (fp_handler.c:308-314 with "and context = ...",
// tfp_scope.hpp). The counts are scoped search's, for every clip instead of the first K: the vote
// form and the general form score every column as there and, where those select K rows, add 1 to
// the bin of each in-scope column's count. Integer adds only, so the result does not depend on
// the order of blocks, waves or lanes.
//
// d_hist is [nq][nbins] int32, zeroed by the caller on the same stream; bin c >= 1 of a query
// receives the number of in-scope columns with count c (count <= the query's frames < nbins); bin
// 0 is left to the host (the scope's live clips minus the other bins).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_kernels.hpp"
#include "tfp_rank.hpp"
#include "tfp_scope.hpp"

namespace tfp {

// Bins a block keeps in LDS (1 KiB); a count of kCensusLdsBins or more is added in global memory
// directly. A 3 s query at 8 kHz has 94 frames, so the LDS bins hold every count of one.
constexpr int32_t kCensusLdsBins = 256;

// coefs = 1, keys inside the vote range: launch_scope_vote's arguments and geometry (one block per
// query and chunk of kRankVoteCols columns) with d_hist / nbins in the selection's place. *d_bad as
// there: set, the bins are meaningless and the caller zeroes them and takes the general form.
hipError_t launch_census_vote(const double* d_q, const int64_t* d_qoff, const int32_t* d_qscope, int32_t nq, SearchConsts sc,
                              const uint32_t* d_bits, int32_t C, const int32_t* d_table, int32_t nbins, int32_t* d_hist,
                              int32_t* d_bad, hipStream_t s);

// The general form after launch_scan_touched (tfp_kernels.hpp) counted queries [q_begin, q_begin +
// nq): row q_begin + q of d_hist from the query's touched clips in scope d_qscope[q_begin + q]; the
// scratch of every touched clip, in scope or not, restored to zero (as launch_scope_final).
hipError_t launch_census_final(int32_t q_begin, int32_t nq, const int32_t* d_qscope, const int32_t* d_table, int32_t C,
                               int32_t* d_stamp, int32_t* d_score, const int32_t* d_touched, int32_t* d_tcnt,
                               int32_t nbins, int32_t* d_hist, hipStream_t s);

}  // namespace tfp
