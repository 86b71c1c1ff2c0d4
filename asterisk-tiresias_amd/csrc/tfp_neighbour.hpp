// tfp_neighbour.hpp — catalog neighbours: which enrolled clips sound like a given enrolled clip.
// The neighbours of clip a under (params, scope, k) are the first k rows of the reference's result
// query (fp_handler.c:367-374) for the recording whose fingerprints are a's stored rows (NULL rows
// included as frames), restricted to the scope as scoped search restricts it (:308-314), with the
// row of a itself deleted. A stored row (m1, m2) used as a query frame has the frame values
// (double)m / 1e6 by IEEE division, -inf where m is the NULL marker: the double SQLite reads back
// from the "%f" text the reference stored (:559-571).
//
// Every operand lies on the device already: a clip's rows are contiguous in the staging arrays, in
// frame order, and the key bitsets, the scope table and the tie keys are those of the scoped vote. So
// the vote form reads the named clips' rows in place and writes no frame value; the rows' alignments
// (tfp_align.hpp) follow on the stream from boxes and pairs built in place, and one read-back brings
// the keys and the alignments. The general form (coefs = 2, a key outside the vote range, a tolerance
// the delta's bitsets do not hold) gathers the rows' frame values into a device buffer for the scoped
// search's general form at k + 1 and deletes the own row on the host (neighbour_drop_self).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "tfp_align.hpp"
#include "tfp_rank.hpp"
#include "tfp_scope.hpp"
#endif

namespace tfp {

constexpr int32_t kNeighbourNullMicro = INT32_MIN;  // TFP_NULL_MICRO: a stored NULL

// The frame value of a stored micro-unit value: both operands are exact and IEEE division rounds
// correctly, so the quotient is strtod of the "%d.%06d" decimal (tests/test_neighbours_host.py).
#ifdef __HIPCC__
__host__ __device__
#endif
inline double neighbour_frame_value(int32_t m) {
  return m == kNeighbourNullMicro ? -__builtin_inf() : (double)m / 1e6;
}

// "k + 1 rows minus self": ids[0, n) are the clips of the first n <= k + 1 rows, in row order. The
// kept rows' positions are written to keep[0, return value): self's row is dropped where it stands,
// and without it row k + 1 is (a clip need not match itself: its own row lies in a frame's box only
// when the frame value's fraction is within the tolerance). self < 0: no clip is dropped.
inline int32_t neighbour_drop_self(const int32_t* ids, int32_t n, int32_t self, int32_t k, int32_t* keep) {
  int32_t m = 0;
  for (int32_t r = 0; r < n && m < k; r++)
    if (self < 0 || ids[r] != self) keep[m++] = r;
  return m;
}

#ifdef __HIPCC__
// One named clip of a launch: its staged rows [row0, row0 + nrows), where its boxes go (box0, the
// running sum of the rows of the clips before it), the scope its rows are selected from and its own
// index column (-1: none on this engine), which scores nothing.
struct NeighbourClip {
  int64_t row0;
  int64_t box0;
  int32_t nrows;
  int32_t scope;
  int32_t self_col;
  int32_t pad;
};

// An index column's clip in the staging rows: [off, off + n), n = 0 without a clip.
struct NeighbourCol {
  int64_t off;
  int64_t n;
};

// launch_scope_vote with the queries' frames read from the named clips' staged max1 values:
// d_keys[i * K + r] = row r of clip i over the columns of its scope, its own column left out.
// d_part: nclips * rank_vote_blocks(C) * K keys of scratch. *d_bad (zeroed by the caller) is set when
// a row's key lies outside the vote range.
hipError_t launch_neighbour_vote(const int32_t* st_m1, const NeighbourClip* d_clips, int32_t nclips, SearchConsts sc,
                                 const uint32_t* d_bits, int32_t C, const int32_t* d_tiekey, const int32_t* d_table,
                                 int32_t K, unsigned long long* d_part, unsigned long long* d_keys, int32_t* d_bad,
                                 hipStream_t s);
// boxes[box0 + j] = frame_box of row j of each named clip (max_rows >= every clip's rows).
hipError_t launch_neighbour_boxes(const int32_t* st_m1, const int32_t* st_m2, const NeighbourClip* d_clips, int32_t nclips,
                                  int64_t max_rows, SearchConsts sc, FrameBox* d_boxes, hipStream_t s);
// d_cols[i * K + r] = the index column whose tie key is the low word of d_keys[i * K + r], among the
// columns of clip i's scope that hold a clip with rows. The caller has set d_cols to -1.
hipError_t launch_neighbour_key_cols(const unsigned long long* d_keys, const NeighbourClip* d_clips, int32_t nclips,
                                     int32_t K, const int32_t* d_tiekey, const int32_t* d_table, const NeighbourCol* d_cols_rows,
                                     int32_t C, int32_t* d_cols, hipStream_t s);
// pairs[i * K + r] = the rows of column d_cols[i * K + r] against clip i's boxes; an empty pair for a
// zeroed key, a column of -1 or a clip without rows.
hipError_t launch_neighbour_pairs(const unsigned long long* d_keys, const int32_t* d_cols, const NeighbourCol* d_cols_rows,
                                  int32_t C, const NeighbourClip* d_clips, int32_t nclips, int32_t K, AlignPair* d_pairs,
                                  hipStream_t s);
// q[2 * (box0 + j)], q[2 * (box0 + j) + 1] = the frame values of row j of each named clip.
hipError_t launch_neighbour_gather(const int32_t* st_m1, const int32_t* st_m2, const NeighbourClip* d_clips, int32_t nclips,
                                   int64_t max_rows, double* d_q, hipStream_t s);
#endif

}  // namespace tfp
