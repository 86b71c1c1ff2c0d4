// tfp_live.hip — live calls (tfp_live.hpp): the kernels of a push around the existing fingerprint
// launch. live_scatter_kernel: the tick's samples to the end of each channel's history.
// live_store_kernel: the fingerprinted frames' values into the channels' frame histories (the
// lead-in frame dropped). live_add_kernel: the key bitset rows of the newly final frames added to the
// channels' count rows. live_select_kernel: scope_vote_kernel's selection (tfp_scope.hip) with the
// score read from the count row plus the provisional tail frame's bit, instead of summed over the
// query's keys; its partial lists go through ranked search's merge (launch_rank_merge).
// live_gather_kernel: the frame histories laid end to end for the general form.
// live_slide_kernel: a trailing window's count rows (tfp_live_window): the key bitset rows of the
// frames that left a channel's window subtracted from its row, those of the newly final frames added.
// live_scatter_g711_kernel: live_scatter_kernel over G.711 codes, expanded by tfp_g711.hpp's map.
// live_verdict_kernel: the two greatest candidates per channel for tfp_live_verdict, a count of 0
// included, over the candidate table live_candidates_kernel derives from the scope table.
// live_key_cols_kernel, live_window_boxes_kernel, live_pairs_kernel: the aligned window
// (tfp_live_window_aligned): the selected rows' columns, the window frames' boxes from the kept frame
// values in place, and one AlignPair per (channel, row) for launch_align, all without a host trip.
//
// The count row is what a push moves (2 bytes per column, read and written once per push however
// many frames it adds, against 1 bit per column and frame of bitset), so a thread owns 8 columns:
// one 16-byte load and store of counts, consecutive lanes on consecutive 16 bytes, and the 8 bits
// from the bitset word that 4 neighbouring lanes share. The 16-bit counts are added in pairs as
// 32-bit words: a count never exceeds the channel's final frames (<= 65535, kLiveMaxSamples), so no
// carry crosses.
#include <hip/hip_runtime.h>

#include "tfp_live.hpp"

namespace tfp {

namespace {

constexpr int kLiveAddCols = 8 * 256;  // columns per live_add / live_slide block (8 per thread)
constexpr int kLiveSlideAhead = 4;     // bitset loads live_slide_kernel issues ahead of their use

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long key) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o > key ? o : key;
  }
  return key;
}

__device__ __forceinline__ bool in_scope(int32_t qs, int32_t cs) { return qs == kScopeAny || cs == qs; }

__global__ __launch_bounds__(256) void live_scatter_kernel(const int16_t* __restrict__ tick, int32_t T,
                                                           const LiveChan* __restrict__ chan, int32_t nch,
                                                           int64_t max_samples, int16_t* __restrict__ hist) {
  const int64_t n = (int64_t)nch * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i / T, t = i % T;
    const int64_t at = chan[c].s_old + t;
    if (t < chan[c].n_new && at < max_samples) hist[c * max_samples + at] = tick[i];
  }
}

// live_scatter_kernel over codes: 1 B per sample in, the int16 of tfp_g711.hpp's map into the history.
template <int LAW>
__global__ __launch_bounds__(256) void live_scatter_g711_kernel(const uint8_t* __restrict__ tick, int32_t T,
                                                                const LiveChan* __restrict__ chan, int32_t nch,
                                                                int64_t max_samples, int16_t* __restrict__ hist) {
  const int64_t n = (int64_t)nch * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i / T, t = i % T;
    const int64_t at = chan[c].s_old + t;
    if (t < chan[c].n_new && at < max_samples) hist[c * max_samples + at] = (int16_t)g711_expand<LAW>(tick[i]);
  }
}

__global__ __launch_bounds__(256) void live_store_kernel(const double* __restrict__ db, const LiveCopy* __restrict__ cp,
                                                         double* __restrict__ q) {
  const LiveCopy c = cp[blockIdx.y];
  const double2* src = reinterpret_cast<const double2*>(db) + c.src;
  double2* dst = reinterpret_cast<double2*>(q) + c.dst;
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < c.n; f += (int64_t)gridDim.x * 256) dst[f] = src[f];
}

__global__ __launch_bounds__(256) void live_add_kernel(const double* __restrict__ q, int64_t Fmax,
                                                       const LiveAdd* __restrict__ adds, SearchConsts sc,
                                                       const uint32_t* __restrict__ bits, int32_t W, int64_t Cpad,
                                                       uint16_t* __restrict__ counts, int32_t* __restrict__ bad) {
  const LiveAdd a = adds[blockIdx.y];
  const int64_t c8 = 8 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (c8 >= Cpad) return;  // (Cpad is a multiple of 128: a thread's 8 columns lie inside the row or outside it)
  const double* qc = q + 2 * (int64_t)a.ch * Fmax;
  uint4* row = reinterpret_cast<uint4*>(counts + (int64_t)a.ch * Cpad + c8);
  uint4 v = *row;
  const uint32_t* col = bits + (c8 >> 5);
  const int sh = (int)(c8 & 31);
  bool out_of_range = false;
  for (int32_t f = a.fbeg; f < a.fend; f++) {  // the same frame and key in every lane
    int32_t k = 0;
    if (!frame_key(qc, f, sc, k)) continue;
    const int64_t idx = (int64_t)k + kKeyOffset;
    if (idx < 0 || idx >= kKeyRange) {
      out_of_range = true;
      continue;
    }
    const uint32_t b = col[idx * W] >> sh;  // bit j: column c8 + j
    v.x += (b & 1u) | ((b & 2u) << 15);
    v.y += ((b >> 2) & 1u) | ((b & 8u) << 13);
    v.z += ((b >> 4) & 1u) | ((b & 32u) << 11);
    v.w += ((b >> 6) & 1u) | ((b & 128u) << 9);
  }
  *row = v;
  if (out_of_range && blockIdx.x == 0 && threadIdx.x == 0) *bad = 1;
}

// live_add_kernel's row handling for a trailing window (tfp_live_window.hpp): the frames [sub_beg, sub_end)
// leave the row and [add_beg, add_end) enter it, with one 16-byte load and one 16-byte store of the
// counts however many frames move; a restarting row starts from zero instead of loading. The 16-bit
// counts are subtracted in pairs as 32-bit words: a row holds exactly the frames of its range under
// one stamp, so every bit a leaving frame subtracts was added by that frame and no borrow crosses
// (a leaving frame whose SQL does not run, or whose key is out of range, subtracts nothing, as it
// added nothing). The frame and its key are the same in every lane, and the bitset loads of
// successive frames depend on the frame values only, not on the accumulators: kLiveSlideAhead of
// them are issued, unconditionally (a frame past the range re-reads the last one and is masked, a
// key that does not count reads row 0), before the first is used.
template <bool ADD>
__device__ __forceinline__ void live_slide_side(const double* __restrict__ qc, int32_t fbeg, int32_t fend,
                                                const SearchConsts& sc, const uint32_t* __restrict__ col, int32_t W, int sh,
                                                uint4& v, bool& out_of_range) {
  for (int32_t f0 = fbeg; f0 < fend; f0 += kLiveSlideAhead) {
    uint32_t b[kLiveSlideAhead];
    bool use[kLiveSlideAhead];
#pragma unroll
    for (int j = 0; j < kLiveSlideAhead; j++) {
      const bool inside = f0 + j < fend;
      int32_t k = 0;
      const bool runs = frame_key(qc, inside ? f0 + j : fend - 1, sc, k);
      const int64_t idx = (int64_t)k + kKeyOffset;
      const bool in_range = idx >= 0 && idx < kKeyRange;
      if (ADD && inside && runs && !in_range) out_of_range = true;
      use[j] = inside && runs && in_range;
      b[j] = col[(use[j] ? idx : 0) * W];
    }
#pragma unroll
    for (int j = 0; j < kLiveSlideAhead; j++) {
      const uint32_t t = use[j] ? b[j] >> sh : 0u;  // bit i: column c8 + i
      const uint32_t x = (t & 1u) | ((t & 2u) << 15), y = ((t >> 2) & 1u) | ((t & 8u) << 13);
      const uint32_t z = ((t >> 4) & 1u) | ((t & 32u) << 11), w = ((t >> 6) & 1u) | ((t & 128u) << 9);
      if (ADD) {
        v.x += x, v.y += y, v.z += z, v.w += w;
      } else {
        v.x -= x, v.y -= y, v.z -= z, v.w -= w;
      }
    }
  }
}

__global__ __launch_bounds__(256) void live_slide_kernel(const double* __restrict__ q, int64_t Fmax,
                                                         const LiveSlide* __restrict__ slides, SearchConsts sc,
                                                         const uint32_t* __restrict__ bits, int32_t W, int64_t Cpad,
                                                         uint16_t* __restrict__ counts, int32_t* __restrict__ bad) {
  const LiveSlide d = slides[blockIdx.y];
  const int64_t c8 = 8 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
  if (c8 >= Cpad) return;  // (Cpad is a multiple of 128: a thread's 8 columns lie inside the row or outside it)
  const double* qc = q + 2 * (int64_t)d.ch * Fmax;
  uint4* row = reinterpret_cast<uint4*>(counts + (int64_t)d.ch * Cpad + c8);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (!d.restart) v = *row;  // (the same in every lane)
  const uint32_t* col = bits + (c8 >> 5);
  const int sh = (int)(c8 & 31);
  bool out_of_range = false;
  live_slide_side<false>(qc, d.sub_beg, d.sub_end, sc, col, W, sh, v, out_of_range);
  live_slide_side<true>(qc, d.add_beg, d.add_end, sc, col, W, sh, v, out_of_range);
  *row = v;
  if (out_of_range && blockIdx.x == 0 && threadIdx.x == 0) *bad = 1;
}

__global__ __launch_bounds__(256) void live_select_kernel(const double* __restrict__ q, int64_t Fmax,
                                                          const LiveChan* __restrict__ chan, SearchConsts sc,
                                                          const uint32_t* __restrict__ bits, int32_t C, int32_t W,
                                                          int64_t Cpad, const uint16_t* __restrict__ counts,
                                                          const int32_t* __restrict__ tiekey,
                                                          const int32_t* __restrict__ table, int32_t K,
                                                          unsigned long long* __restrict__ part, int32_t* __restrict__ bad) {
  static_assert(4 * 256 == kRankVoteCols, "4 columns per thread");
  __shared__ unsigned long long wmax[2][4];
  const int ch = blockIdx.y, blk = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const LiveChan lc = chan[ch];
  // this thread's columns in scope, as scope_vote_kernel reads them (one 16-byte load of the table)
  const int c4 = 4 * (blk * 256 + threadIdx.x);
  uint32_t in = 0;
  if (c4 < C) {
    const int4 s4 = *reinterpret_cast<const int4*>(table + c4);
    in = (in_scope(lc.scope, s4.x) ? 1u : 0u) | (in_scope(lc.scope, s4.y) ? 2u : 0u) | (in_scope(lc.scope, s4.z) ? 4u : 0u) |
         (in_scope(lc.scope, s4.w) ? 8u : 0u);
#pragma unroll
    for (int j = 1; j < 4; j++)
      if (c4 + j >= C) in &= ~(1u << j);
  }
  // the provisional tail frame's bitset row (-1: no tail, or its SQL does not run)
  int slot = -1;
  if (lc.tail >= 0) {
    int32_t k = 0;
    if (frame_key(q + 2 * (int64_t)ch * Fmax, lc.tail, sc, k)) {
      const int64_t idx = (int64_t)k + kKeyOffset;
      if (idx < 0 || idx >= kKeyRange) {
        if (threadIdx.x == 0) *bad = 1;  // (every writer stores 1)
      } else {
        slot = (int)idx;
      }
    }
  }
  uint32_t score[4] = {0, 0, 0, 0};
  if (in) {  // (in != 0 implies c4 < C <= Cpad; c4 is a multiple of 4: an aligned 8-byte load of 4 counts)
    const uint2 cv = *reinterpret_cast<const uint2*>(counts + (int64_t)ch * Cpad + c4);
    const uint32_t tb = slot >= 0 ? bits[(int64_t)slot * W + (c4 >> 5)] >> (c4 & 31) : 0u;
    score[0] = (cv.x & 0xffffu) + (tb & 1u);
    score[1] = (cv.x >> 16) + ((tb >> 1) & 1u);
    score[2] = (cv.y & 0xffffu) + ((tb >> 2) & 1u);
    score[3] = (cv.y >> 16) + ((tb >> 3) & 1u);
  }
  unsigned long long mine[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
    mine[j] = (((in >> j) & 1u) && score[j] > 0) ? ((unsigned long long)score[j] << 32) | (uint32_t)tiekey[c4 + j] : 0ull;
  unsigned long long* out = part + ((int64_t)ch * gridDim.x + blk) * K;
  unsigned long long prev = ~0ull;
  for (int r = 0; r < K; r++) {
    unsigned long long key = 0ull;
#pragma unroll
    for (int j = 0; j < 4; j++) key = (mine[j] < prev && mine[j] > key) ? mine[j] : key;
    key = wave_max_u64(key);
    if (lane == 0) wmax[r & 1][wv] = key;
    __syncthreads();  // (wmax[r & 1] is next written two rounds on, after the barrier of round r + 1)
    key = wmax[r & 1][0];
#pragma unroll
    for (int i = 1; i < 4; i++) key = wmax[r & 1][i] > key ? wmax[r & 1][i] : key;
    if (threadIdx.x == 0) out[r] = key;
    prev = key;  // (0: no key is below it, the remaining rounds give 0)
  }
}

// The verdict's selection: live_select_kernel's loads and reduction with three differences. A column
// is a candidate when it is in scope and its candidate-table entry is not kScopeNone (TFP_SCOPE_ANY
// does not admit a column without a clip, nor one whose clip has no row); a candidate with score 0
// keeps a key, ((score << 32) | tie key) + 1 (tie keys reach INT32_MAX and scores 65535: the + 1
// stays inside the low word, and 0 is left for "no column"); the tail frame's bit counts only for a
// channel flagged complete. The top 2 per block, then launch_rank_merge with K = 2.
__global__ __launch_bounds__(256) void live_verdict_kernel(const double* __restrict__ q, int64_t Fmax,
                                                           const LiveVerdictChan* __restrict__ chan, SearchConsts sc,
                                                           const uint32_t* __restrict__ bits, int32_t C, int32_t W,
                                                           int64_t Cpad, const uint16_t* __restrict__ counts,
                                                           const int32_t* __restrict__ tiekey,
                                                           const int32_t* __restrict__ cand,
                                                           unsigned long long* __restrict__ part, int32_t* __restrict__ bad) {
  static_assert(4 * 256 == kRankVoteCols, "4 columns per thread");
  __shared__ unsigned long long wmax[2][4];
  const int ch = blockIdx.y, blk = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const LiveVerdictChan lc = chan[ch];
  const int c4 = 4 * (blk * 256 + threadIdx.x);
  uint32_t in = 0;
  if (c4 < C) {  // (the table holds scope_table_cols(C) entries: the 16-byte load stays inside it)
    const int4 s4 = *reinterpret_cast<const int4*>(cand + c4);
    in = ((s4.x != kScopeNone && in_scope(lc.scope, s4.x)) ? 1u : 0u) | ((s4.y != kScopeNone && in_scope(lc.scope, s4.y)) ? 2u : 0u) |
         ((s4.z != kScopeNone && in_scope(lc.scope, s4.z)) ? 4u : 0u) | ((s4.w != kScopeNone && in_scope(lc.scope, s4.w)) ? 8u : 0u);
#pragma unroll
    for (int j = 1; j < 4; j++)
      if (c4 + j >= C) in &= ~(1u << j);
  }
  // a complete channel's provisional tail frame: its bitset row (-1: none, or its SQL does not run)
  int slot = -1;
  if (lc.complete && lc.tail >= 0) {
    int32_t k = 0;
    if (frame_key(q + 2 * (int64_t)ch * Fmax, lc.tail, sc, k)) {
      const int64_t idx = (int64_t)k + kKeyOffset;
      if (idx < 0 || idx >= kKeyRange) {
        if (threadIdx.x == 0) *bad = 1;  // (every writer stores 1)
      } else {
        slot = (int)idx;
      }
    }
  }
  uint32_t score[4] = {0, 0, 0, 0};
  if (in) {  // (in != 0 implies c4 < C <= Cpad; c4 is a multiple of 4: an aligned 8-byte load of 4 counts)
    const uint2 cv = *reinterpret_cast<const uint2*>(counts + (int64_t)ch * Cpad + c4);
    const uint32_t tb = slot >= 0 ? bits[(int64_t)slot * W + (c4 >> 5)] >> (c4 & 31) : 0u;
    score[0] = (cv.x & 0xffffu) + (tb & 1u);
    score[1] = (cv.x >> 16) + ((tb >> 1) & 1u);
    score[2] = (cv.y & 0xffffu) + ((tb >> 2) & 1u);
    score[3] = (cv.y >> 16) + ((tb >> 3) & 1u);
  }
  unsigned long long mine[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
    mine[j] = ((in >> j) & 1u) ? (((unsigned long long)score[j] << 32) | (uint32_t)tiekey[c4 + j]) + 1ull : 0ull;
  unsigned long long* out = part + ((int64_t)ch * gridDim.x + blk) * 2;
  unsigned long long prev = ~0ull;
  for (int r = 0; r < 2; r++) {
    unsigned long long key = 0ull;
#pragma unroll
    for (int j = 0; j < 4; j++) key = (mine[j] < prev && mine[j] > key) ? mine[j] : key;
    key = wave_max_u64(key);
    if (lane == 0) wmax[r][wv] = key;
    __syncthreads();
    key = wmax[r][0];
#pragma unroll
    for (int i = 1; i < 4; i++) key = wmax[r][i] > key ? wmax[r][i] : key;
    if (threadIdx.x == 0) out[r] = key;
    prev = key;  // (0: no key is below it, the second round gives 0)
  }
}

// One wave per column: any staged row of the column's clip with a non-NULL max1.
__global__ __launch_bounds__(256) void live_candidates_kernel(const int32_t* __restrict__ m1,
                                                              const LiveColRows* __restrict__ rows,
                                                              const int32_t* __restrict__ table, int32_t Cp,
                                                              int32_t* __restrict__ cand) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= Cp) return;  // (a whole wave leaves: c is the same in all its lanes)
  const LiveColRows r = rows[c];
  bool has = false;
  for (int64_t i = lane; i < r.n && !has; i += 64) has = m1[r.off + i] != kLiveNullM1;
  const bool any = __any(has);
  if (lane == 0) cand[c] = any ? table[c] : kScopeNone;
}

__global__ __launch_bounds__(256) void live_gather_kernel(const double* __restrict__ q, int64_t Fmax,
                                                          const int64_t* __restrict__ foff,
                                                          const int64_t* __restrict__ first, double* __restrict__ out) {
  const int ch = blockIdx.y;
  const int64_t f0 = foff[ch], n = foff[ch + 1] - f0;
  const double2* src = reinterpret_cast<const double2*>(q) + (int64_t)ch * Fmax + (first ? first[ch] : 0);
  double2* dst = reinterpret_cast<double2*>(out) + f0;
  for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < n; f += (int64_t)gridDim.x * 256) dst[f] = src[f];
}

// The aligned window's three kernels (tfp_live.hpp). live_key_cols_kernel: live_select_kernel's grid and
// column loads; a block whose channel has no row (its first key is 0: the keys descend) leaves at once.
// The channel's at most K tie keys sit in LDS, every lane reads the same one (a broadcast).
__global__ __launch_bounds__(256) void live_key_cols_kernel(const unsigned long long* __restrict__ keys,
                                                            const LiveChan* __restrict__ chan, int32_t K,
                                                            const int32_t* __restrict__ tiekey,
                                                            const int32_t* __restrict__ table,
                                                            const LiveColRows* __restrict__ rows, int32_t C,
                                                            int32_t* __restrict__ cols) {
  __shared__ uint32_t want[kRankMax];
  __shared__ int32_t nwant;
  const int ch = blockIdx.y;
  const unsigned long long* kc = keys + (int64_t)ch * K;
  if (!kc[0]) return;  // (the whole block)
  if (threadIdx.x < (unsigned)K) want[threadIdx.x] = (uint32_t)kc[threadIdx.x];
  if (threadIdx.x == 0) {
    int32_t n = 1;
    while (n < K && kc[n]) n++;
    nwant = n;
  }
  __syncthreads();
  const int c4 = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (c4 >= C) return;
  const int32_t qs = chan[ch].scope;
  const int4 s4 = *reinterpret_cast<const int4*>(table + c4);  // (scope_table_cols(C) entries: inside the table)
  const int32_t cs[4] = {s4.x, s4.y, s4.z, s4.w};
  const int32_t n = nwant;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (c4 + j >= C || !in_scope(qs, cs[j])) continue;
    const uint32_t tk = (uint32_t)tiekey[c4 + j];
    for (int32_t r = 0; r < n; r++)
      if (want[r] == tk && rows[c4 + j].n > 0) cols[(int64_t)ch * K + r] = c4 + j;
  }
}

__global__ __launch_bounds__(256) void live_window_boxes_kernel(const double* __restrict__ q, int64_t Fmax,
                                                                const LiveWinChan* __restrict__ wchan, int64_t stride,
                                                                SearchConsts sc, FrameBox* __restrict__ boxes) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= stride) return;
  const int64_t ch = blockIdx.y;
  const LiveWinChan w = wchan[ch];
  FrameBox bx;
  if (x < w.F) {
    const double* f = q + 2 * (ch * Fmax + w.first + x);  // (first + x < first + F <= Fmax)
    bx = frame_box(f[0], f[1], sc);
  } else {  // a slot past the channel's window: no row hits it
    bx.L1 = 1, bx.U1 = 0, bx.L2 = 1, bx.U2 = 0;
    bx.k = 0, bx.flags = 0;
  }
  boxes[ch * stride + x] = bx;
}

__global__ __launch_bounds__(256) void live_pairs_kernel(const unsigned long long* __restrict__ keys,
                                                         const int32_t* __restrict__ cols,
                                                         const LiveColRows* __restrict__ rows, int32_t ncols,
                                                         const LiveWinChan* __restrict__ wchan, int32_t npairs, int32_t K,
                                                         int64_t stride, const int32_t* __restrict__ bad,
                                                         AlignPair* __restrict__ pairs, int32_t* __restrict__ flag) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *flag = *bad;
  if (i >= npairs) return;
  AlignPair p{0, 0, 0, 0};
  if (keys[i]) {
    const int32_t col = cols[i], ch = i / K;
    if (col >= 0 && col < ncols) {
      const LiveColRows r = rows[col];
      const int32_t F = wchan[ch].F;
      if (r.n > 0 && r.n <= INT32_MAX && F > 0) p = AlignPair{r.off, (int64_t)ch * stride, (int32_t)r.n, F};
    }
  }
  pairs[i] = p;
}

inline unsigned copy_blocks(int64_t max_n) {
  const int64_t g = (max_n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 64 ? 64 : g));
}

}  // namespace

hipError_t launch_live_scatter(const int16_t* d_tick, int32_t T, const LiveChan* d_chan, int32_t nch, int64_t max_samples,
                               int16_t* d_hist, hipStream_t s) {
  const int64_t n = (int64_t)nch * T;
  if (n <= 0) return hipSuccess;
  const int64_t g = (n + 255) / 256;
  hipLaunchKernelGGL(live_scatter_kernel, dim3((unsigned)(g > 1024 ? 1024 : g)), dim3(256), 0, s, d_tick, T, d_chan, nch,
                     max_samples, d_hist);
  return hipGetLastError();
}

hipError_t launch_live_scatter_g711(const uint8_t* d_tick, int32_t T, const LiveChan* d_chan, int32_t nch, int32_t law,
                                    int64_t max_samples, int16_t* d_hist, hipStream_t s) {
  if (!g711_law_ok(law)) return hipErrorInvalidValue;
  const int64_t n = (int64_t)nch * T;
  if (n <= 0) return hipSuccess;
  const int64_t g = (n + 255) / 256;
  const dim3 grid((unsigned)(g > 1024 ? 1024 : g));
  if (law == kG711Alaw)
    hipLaunchKernelGGL(live_scatter_g711_kernel<kG711Alaw>, grid, dim3(256), 0, s, d_tick, T, d_chan, nch, max_samples, d_hist);
  else
    hipLaunchKernelGGL(live_scatter_g711_kernel<kG711Ulaw>, grid, dim3(256), 0, s, d_tick, T, d_chan, nch, max_samples, d_hist);
  return hipGetLastError();
}

hipError_t launch_live_candidates(const int32_t* d_m1, const LiveColRows* d_rows, const int32_t* d_table, int32_t C,
                                  int32_t* d_cand, hipStream_t s) {
  if (C <= 0) return hipSuccess;
  const int32_t Cp = scope_table_cols(C);
  hipLaunchKernelGGL(live_candidates_kernel, dim3((unsigned)((Cp + 3) / 4)), dim3(256), 0, s, d_m1, d_rows, d_table, Cp, d_cand);
  return hipGetLastError();
}

hipError_t launch_live_verdict(const double* d_q, int64_t Fmax, const LiveVerdictChan* d_chan, int32_t nch, SearchConsts sc,
                               const uint32_t* d_bits, int32_t C, const uint16_t* d_counts, const int32_t* d_tiekey,
                               const int32_t* d_cand, unsigned long long* d_part, unsigned long long* d_keys,
                               int32_t* d_bad, hipStream_t s) {
  if (nch <= 0) return hipSuccess;
  if (C <= 0 || nch > 65535) return hipErrorInvalidValue;
  const int32_t nb = rank_vote_blocks(C);
  hipLaunchKernelGGL(live_verdict_kernel, dim3(nb, nch), dim3(256), 0, s, d_q, Fmax, d_chan, sc, d_bits, C, key_bits_words(C),
                     live_count_cols(C), d_counts, d_tiekey, d_cand, d_part, d_bad);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? err : launch_rank_merge(d_part, nch, nb * 2, 2, d_keys, s);
}

hipError_t launch_live_store(const double* d_db, const LiveCopy* d_cp, int32_t ncopy, int64_t max_n, double* d_q,
                             hipStream_t s) {
  if (ncopy <= 0) return hipSuccess;
  if (ncopy > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(live_store_kernel, dim3(copy_blocks(max_n), ncopy), dim3(256), 0, s, d_db, d_cp, d_q);
  return hipGetLastError();
}

hipError_t launch_live_add(const double* d_q, int64_t Fmax, const LiveAdd* d_add, int32_t nadd, SearchConsts sc,
                           const uint32_t* d_bits, int32_t C, uint16_t* d_counts, int32_t* d_bad, hipStream_t s) {
  if (nadd <= 0) return hipSuccess;
  if (C <= 0 || nadd > 65535) return hipErrorInvalidValue;
  const int64_t Cpad = live_count_cols(C);
  hipLaunchKernelGGL(live_add_kernel, dim3((unsigned)((Cpad + kLiveAddCols - 1) / kLiveAddCols), nadd), dim3(256), 0, s, d_q,
                     Fmax, d_add, sc, d_bits, key_bits_words(C), Cpad, d_counts, d_bad);
  return hipGetLastError();
}

hipError_t launch_live_slide(const double* d_q, int64_t Fmax, const LiveSlide* d_slide, int32_t nslide, SearchConsts sc,
                             const uint32_t* d_bits, int32_t C, uint16_t* d_counts, int32_t* d_bad, hipStream_t s) {
  if (nslide <= 0) return hipSuccess;
  if (C <= 0 || nslide > 65535) return hipErrorInvalidValue;
  const int64_t Cpad = live_count_cols(C);
  hipLaunchKernelGGL(live_slide_kernel, dim3((unsigned)((Cpad + kLiveAddCols - 1) / kLiveAddCols), nslide), dim3(256), 0, s,
                     d_q, Fmax, d_slide, sc, d_bits, key_bits_words(C), Cpad, d_counts, d_bad);
  return hipGetLastError();
}

hipError_t launch_live_select(const double* d_q, int64_t Fmax, const LiveChan* d_chan, int32_t nch, SearchConsts sc,
                              const uint32_t* d_bits, int32_t C, const uint16_t* d_counts, const int32_t* d_tiekey,
                              const int32_t* d_table, int32_t K, unsigned long long* d_part, unsigned long long* d_keys,
                              int32_t* d_bad, hipStream_t s) {
  if (nch <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || C <= 0 || nch > 65535) return hipErrorInvalidValue;
  const int32_t nb = rank_vote_blocks(C);
  hipLaunchKernelGGL(live_select_kernel, dim3(nb, nch), dim3(256), 0, s, d_q, Fmax, d_chan, sc, d_bits, C, key_bits_words(C),
                     live_count_cols(C), d_counts, d_tiekey, d_table, K, d_part, d_bad);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? err : launch_rank_merge(d_part, nch, nb * K, K, d_keys, s);
}

hipError_t launch_live_key_cols(const unsigned long long* d_keys, const LiveChan* d_chan, int32_t nch, int32_t K,
                                const int32_t* d_tiekey, const int32_t* d_table, const LiveColRows* d_rows, int32_t C,
                                int32_t* d_cols, hipStream_t s) {
  if (nch <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || C <= 0 || nch > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(live_key_cols_kernel, dim3(rank_vote_blocks(C), nch), dim3(256), 0, s, d_keys, d_chan, K, d_tiekey,
                     d_table, d_rows, C, d_cols);
  return hipGetLastError();
}

hipError_t launch_live_window_boxes(const double* d_q, int64_t Fmax, const LiveWinChan* d_wchan, int32_t nch, int64_t stride,
                                    SearchConsts sc, FrameBox* d_boxes, hipStream_t s) {
  if (nch <= 0 || stride <= 0) return hipSuccess;
  if (nch > 65535 || stride > Fmax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(live_window_boxes_kernel, dim3((unsigned)((stride + 255) / 256), nch), dim3(256), 0, s, d_q, Fmax,
                     d_wchan, stride, sc, d_boxes);
  return hipGetLastError();
}

hipError_t launch_live_pairs(const unsigned long long* d_keys, const int32_t* d_cols, const LiveColRows* d_rows, int32_t ncols,
                             const LiveWinChan* d_wchan, int32_t nch, int32_t K, int64_t stride, const int32_t* d_bad,
                             AlignPair* d_pairs, int32_t* d_flag, hipStream_t s) {
  if (nch <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || nch > 65535) return hipErrorInvalidValue;
  const int32_t npairs = nch * K;
  hipLaunchKernelGGL(live_pairs_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, s, d_keys, d_cols, d_rows, ncols,
                     d_wchan, npairs, K, stride, d_bad, d_pairs, d_flag);
  return hipGetLastError();
}

hipError_t launch_live_gather(const double* d_q, int64_t Fmax, const int64_t* d_foff, const int64_t* d_first, int32_t nch,
                              int64_t max_n, double* d_out, hipStream_t s) {
  if (nch <= 0) return hipSuccess;
  if (nch > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(live_gather_kernel, dim3(copy_blocks(max_n), nch), dim3(256), 0, s, d_q, Fmax, d_foff, d_first, d_out);
  return hipGetLastError();
}

}  // namespace tfp
