// tfp_align.hpp — aligned search: where in a clip a query matches, and how many of its hits line up
// in time. For a query with frames i = 0..F-1 and a clip with stored rows j = 0..N-1 (frame order,
// NULL rows included, as they lie in the engine's staging buffers), hit(i, j) is the per-frame SQL
// predicate of fp_handler.c:287-351 (prep_boxes' FrameBox) applied to row j, and
//   hist[d] = #{(i, j) : hit(i, j), j - i = d},  d in [-(F-1), N-1].
// The alignment is aligned_count = max_d hist[d], offset = the smallest d attaining it, and
// first_frame / last_frame = the least / greatest i with hit(i, i + offset); all 0 when nothing hits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_kernels.hpp"

namespace tfp {

constexpr int32_t kAlignBand = 256;   // diagonals per block (one per thread)
constexpr int32_t kAlignTile = 256;   // query frames per LDS tile
constexpr int32_t kAlignMaxPairs = 65535;  // pairs per launch (the grid's second dimension)

// One (query, candidate clip) pair: the clip's rows [row0, row0 + N) of the staging arrays and the
// query's boxes [f0, f0 + F). N = 0 or F = 0: an empty pair (a zeroed result).
struct AlignPair {
  int64_t row0;
  int64_t f0;
  int32_t N;
  int32_t F;
};

struct AlignOut {  // tfp_alignment
  int32_t aligned_count, offset, first_frame, last_frame;
};

// Bands of kAlignBand diagonals covering d in [-(F-1), N-1].
TFP_HD int64_t align_bands(int64_t F, int64_t N) {
  return (F > 0 && N > 0) ? (F + N - 1 + kAlignBand - 1) / kAlignBand : 0;
}

// npairs <= kAlignMaxPairs pairs in one launch (plus the merge): out[p] = the alignment of pair p.
// max_bands >= align_bands of every pair; d_part: npairs * max_bands keys of scratch. coefs2: some
// box may carry a max2 condition (flags & 2), so the max2 rows are read.
hipError_t launch_align(const AlignPair* d_pairs, int32_t npairs, int64_t max_bands, const FrameBox* boxes,
                        const int32_t* st_m1, const int32_t* st_m2, bool coefs2, unsigned long long* d_part,
                        AlignOut* d_out, hipStream_t s);

}  // namespace tfp
