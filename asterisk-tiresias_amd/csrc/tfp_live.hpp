// tfp_live.hpp — live calls: the scoped rows (tfp_scope.hpp) of each call so far, after every push,
// with the per-clip counts carried from push to push.
//
// The dialplan application records a channel from the start of the call and searches the recording
// among its context's clips (application_handler.c:152-185, record_voice :248-312; fp_handler.c:287-374
// with the context predicate at :308-314, doc/dialplan_application.rst:11). A recording anchored at
// the call's start only grows: its frames [0, floor(S / 256)) are final (tfp_live_plan.hpp). For
// coefs = 1 a clip's count is the sum over the query frames of one bit of the key bitsets
// (launch_key_bits: bits[key][column]), so a channel keeps a row of 16-bit counts over the index
// columns, a push adds the bitset rows of its newly final frames to it, and the rows are selected
// from count + the provisional tail frame's bit. Everything else (coefs = 2, a key outside the vote
// range) runs the scoped search core over the kept frame values: exact, not incremental.
//
// Per live object, on the device: the int16 history [nchannels][max_samples]; the frame values
// [nchannels][Fmax] (2 doubles per frame, Fmax = ceil(max_samples / 256), the provisional tail
// included); the count table uint16 [nchannels][Cpad], Cpad = 32 key_bits_words(C) columns in the
// scope table's layout (main columns, then the delta's). The channels' sample counts and added-frame
// counts are kept by the host and travel with each push's descriptors.
//
// The trailing window (tfp_live_window, tfp_live_window.hpp) keeps a second count table in the same
// layout, allocated by the first window call: channel c's row holds the final frames of the last
// `window` frames of its call, moved from call to call by launch_live_slide (the rows of the frames
// that left subtracted, those of the newly final frames added) and read by launch_live_select as a
// push's row is. The rows' frame ranges are host state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_align.hpp"
#include "tfp_g711.hpp"
#include "tfp_kernels.hpp"
#include "tfp_live_plan.hpp"
#include "tfp_live_window.hpp"
#include "tfp_occur.hpp"
#include "tfp_rank.hpp"
#include "tfp_scope.hpp"

namespace tfp {

// Per channel and push (uploaded with the tick).
struct LiveChan {
  int64_t s_old;  // samples before the push
  int64_t tail;   // the provisional frame after the push, -1 when every frame is final (or none)
  int32_t n_new;  // samples of this push: tick[c][0, n_new)
  int32_t scope;  // the channel's scope of a searching push
};
// Frame values db[src, src + n) -> the frame history at frame dst (a flat index: channel * Fmax + frame).
struct LiveCopy {
  int64_t src, dst, n;
};
// Final frames [fbeg, fend) of channel ch to add to its count row.
struct LiveAdd {
  int32_t ch, fbeg, fend, pad;
};

// A window call's change to channel ch's row of the window count table (tfp_live_window.hpp): the
// final frames [sub_beg, sub_end) leave it, [add_beg, add_end) enter it; restart: the row starts from
// zero instead of from what it holds (and nothing is subtracted).
struct LiveSlide {
  int32_t ch, sub_beg, sub_end, add_beg, add_end, restart, pad0, pad1;
};

// Per channel and verdict (launch_live_verdict): a descriptor of its own, a push's LiveChan stays as it is.
struct LiveVerdictChan {
  int64_t tail;      // the provisional frame of the samples so far, -1 when every frame is final (or none)
  int32_t scope;     // the channel's scope
  int32_t complete;  // 1: the recording has its planned length, the tail's bit counts; 0: final frames only
};
// A column's clip in the staging rows (launch_live_candidates): rows [off, off + n), n = 0 without a clip.
struct LiveColRows {
  int64_t off;
  int64_t n;
};
constexpr int32_t kLiveNullM1 = INT32_MIN;  // a staged row with a NULL max1: it matches no frame

inline int64_t live_count_cols(int32_t C) { return (int64_t)key_bits_words(C) * 32; }  // Cpad: a multiple of 128

// tick[nch][T] -> hist[c][s_old, s_old + n_new) per channel (the host has checked s_old + n_new <= max_samples).
hipError_t launch_live_scatter(const int16_t* d_tick, int32_t T, const LiveChan* d_chan, int32_t nch, int64_t max_samples,
                               int16_t* d_hist, hipStream_t s);
// The same with G.711 codes tick[nch][T] (1 B per sample) of law kG711Ulaw / kG711Alaw, expanded by
// tfp_g711.hpp's map on their way into the int16 history.
hipError_t launch_live_scatter_g711(const uint8_t* d_tick, int32_t T, const LiveChan* d_chan, int32_t nch, int32_t law,
                                    int64_t max_samples, int16_t* d_hist, hipStream_t s);
// The verdict's candidate table over scope_table_cols(C) columns: d_cand[c] = d_table[c] (the scope
// table) where column c's clip has a staged row with a non-NULL max1 (d_m1[off, off + n) of d_rows[c]),
// else kScopeNone: a clip without such a row can never score, so it is no candidate.
hipError_t launch_live_candidates(const int32_t* d_m1, const LiveColRows* d_rows, const int32_t* d_table, int32_t C,
                                  int32_t* d_cand, hipStream_t s);
// d_keys[ch * 2 + r], r = 0, 1: the two greatest of ((count << 32 | tie key) + 1) over the columns of
// scope d_chan[ch].scope whose d_cand entry is not kScopeNone, a count of 0 included (0: no such
// column). count = the count row's entry, plus the tail frame's bit for a complete channel only.
// d_part: nch * rank_vote_blocks(C) * 2 keys of scratch. *d_bad as launch_live_select (the tail's key).
hipError_t launch_live_verdict(const double* d_q, int64_t Fmax, const LiveVerdictChan* d_chan, int32_t nch, SearchConsts sc,
                               const uint32_t* d_bits, int32_t C, const uint16_t* d_counts, const int32_t* d_tiekey,
                               const int32_t* d_cand, unsigned long long* d_part, unsigned long long* d_keys,
                               int32_t* d_bad, hipStream_t s);
// The ncopy copies of d_cp (each at most max_n frames).
hipError_t launch_live_store(const double* d_db, const LiveCopy* d_cp, int32_t ncopy, int64_t max_n, double* d_q,
                             hipStream_t s);
// counts[ch][col] += bits[key(frame)][col] for the frames of each of the nadd entries, in frame order
// (a frame whose SQL does not run adds nothing). One workgroup owns 2,048 columns of one channel:
// no atomics. *d_bad is set (never cleared) when a key lies outside [-512, 511].
hipError_t launch_live_add(const double* d_q, int64_t Fmax, const LiveAdd* d_add, int32_t nadd, SearchConsts sc,
                           const uint32_t* d_bits, int32_t C, uint16_t* d_counts, int32_t* d_bad, hipStream_t s);
// counts[ch][col] += bits[key(frame)][col] over each entry's entering frames and -= over its leaving
// frames (an entry with restart set starts its row from zero), live_add's shape: one workgroup owns
// 2,048 columns of one channel, one 16-byte load and store of the row per thread, no atomics. At most
// one entry per channel. *d_bad is set (never cleared) when an entering frame's key lies outside
// [-512, 511].
hipError_t launch_live_slide(const double* d_q, int64_t Fmax, const LiveSlide* d_slide, int32_t nslide, SearchConsts sc,
                             const uint32_t* d_bits, int32_t C, uint16_t* d_counts, int32_t* d_bad, hipStream_t s);
// d_keys[ch * K + r] = row r of channel ch: the r-th greatest (count + tail bit) << 32 | tie key over
// the columns of scope d_chan[ch].scope with a non-zero score. d_part: nch * rank_vote_blocks(C) * K
// keys of scratch. *d_bad as above (the tail's key).
hipError_t launch_live_select(const double* d_q, int64_t Fmax, const LiveChan* d_chan, int32_t nch, SearchConsts sc,
                              const uint32_t* d_bits, int32_t C, const uint16_t* d_counts, const int32_t* d_tiekey,
                              const int32_t* d_table, int32_t K, unsigned long long* d_part, unsigned long long* d_keys,
                              int32_t* d_bad, hipStream_t s);
// The channels' frame values laid end to end for the general form: channel c's frames
// [first, first + d_foff[c + 1] - d_foff[c]), first = d_first[c] (nullptr: 0), at d_out frame d_foff[c]
// (at most max_n frames per channel).
hipError_t launch_live_gather(const double* d_q, int64_t Fmax, const int64_t* d_foff, const int64_t* d_first, int32_t nch,
                              int64_t max_n, double* d_out, hipStream_t s);

// ---- the aligned trailing window (tfp_live_window_aligned): where each row's clip lies in the window.
// Every operand is on the device already: the kept frame values, the selected rows' keys and the
// clips' staged rows (LiveColRows), so the boxes and the pairs of launch_align (tfp_align.hpp) are
// built there and one read-back brings the keys and the alignments.

// Per channel and aligned window call: frames [first, first + F) of its call are its window.
struct LiveWinChan {
  int32_t first, F;
};

// d_cols[ch * K + r] = the index column of row r of channel ch (d_keys: launch_live_select's output),
// found by its tie key (the key's low word) among the columns of the channel's scope that have a
// clip with rows (d_rows[col].n > 0; tie keys are distinct among those). The caller has set d_cols to
// -1: a zeroed key's entry, and one whose column is not found, stay -1.
hipError_t launch_live_key_cols(const unsigned long long* d_keys, const LiveChan* d_chan, int32_t nch, int32_t K,
                                const int32_t* d_tiekey, const int32_t* d_table, const LiveColRows* d_rows, int32_t C,
                                int32_t* d_cols, hipStream_t s);
// boxes[ch * stride + x] = the box (prep_boxes_kernel's, the same device routine) of call frame
// d_wchan[ch].first + x of channel ch, read from the kept frame values in place; x in [F, stride): an
// empty box (L > U, no flag). stride >= every channel's F.
hipError_t launch_live_window_boxes(const double* d_q, int64_t Fmax, const LiveWinChan* d_wchan, int32_t nch, int64_t stride,
                                    SearchConsts sc, FrameBox* d_boxes, hipStream_t s);
// pairs[ch * K + r] = row r of channel ch against its window's boxes: the rows of column
// d_cols[ch * K + r] in staging (d_rows), f0 = ch * stride, F = d_wchan[ch].F; an empty pair for a
// zeroed key, a column of -1, a clip without rows or a window without frames. d_rows is read only for
// a non-zero key with a column in [0, ncols). *d_flag = *d_bad (the select's out-of-range flag, copied
// beside the results so that one read-back brings it).
hipError_t launch_live_pairs(const unsigned long long* d_keys, const int32_t* d_cols, const LiveColRows* d_rows, int32_t ncols,
                             const LiveWinChan* d_wchan, int32_t nch, int32_t K, int64_t stride, const int32_t* d_bad,
                             AlignPair* d_pairs, int32_t* d_flag, hipStream_t s);

// ---- the carried traces (tfp_live_occurrences, tfp_live_trace.hip): a channel keeps a list of tracks
// (clip, s), s the call frame at which clip frame 0 lies. A track's diagonal covers the call frames
// [lo, hi) = trace_span(F, N, s) (tfp_occur.hpp); the TraceSeg of its hits over the final frames
// [lo, min(Ff, s + N)) folded so far lives in one of nchannels x kLiveTracksMax device slots, allocated by
// the first occurrence call, and is extended in place by the frames that became final. The lists (clip,
// s, windows, frames folded so far) are host state, as the window table's ranges are.

constexpr int32_t kLiveTracksMax = 64;  // TFP_LIVE_TRACKS_MAX: tracks a channel's list can hold

// One track's step: fold the final call frames [beg, end) of channel ch (the host has clipped them to the
// track's span and to the channel's final frames) into the summary at d_segs[slot], then answer with the
// tail frame joined in.
struct LiveTrace {
  int64_t row0;     // the clip's staged rows [row0, row0 + N)
  int32_t N;
  int32_t s;        // the call frame at which clip frame 0 lies (any int32)
  int32_t ch;
  int32_t slot;     // the track's summary: d_segs[slot]
  int32_t beg, end; // final frames to fold (end <= beg: none)
  int32_t tail;     // the provisional tail frame when it lies in the span, else -1
  int32_t restart;  // 1: the stored summary is trace_none() (the slot is not read)
  int32_t overlap;  // tfp_trace.overlap, over all F frames
  int32_t pad;
};

// Per descriptor i < ndesc: d_segs[slot] = the stored summary (trace_none() on restart) extended by the
// hits of frames [beg, end), and d_out[i] = trace_result(overlap, that summary with the tail's hit
// joined in). A frame's box is built from d_q[ch * Fmax + x] (frame_box, prep_boxes_kernel's routine)
// and tested against staged row x - s with align_box; st_m2 is read only where the box carries the
// max2 flag (sc.coefs == 2). Descriptors name distinct slots. max_gap >= 0.
hipError_t launch_live_trace(const LiveTrace* d_desc, int32_t ndesc, int32_t max_gap, const double* d_q, int64_t Fmax,
                             SearchConsts sc, const int32_t* st_m1, const int32_t* st_m2, TraceSeg* d_segs, TraceOut* d_out,
                             hipStream_t s);

}  // namespace tfp
