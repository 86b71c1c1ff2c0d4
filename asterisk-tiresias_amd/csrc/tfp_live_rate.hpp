// tfp_live_rate.hpp — a live object with an input rate (tfp_live_create_rate): every push is converted to
// the index's rate on its way into the int16 history, with a carried input tail per channel. The host
// arithmetic is plain functions with no GPU call (tests/native/check_live_rate.cpp runs them under
// ASan/UBSan); the launch of tfp_live_rate.hip is declared at the end.
//
// The converter is tfp_resample.hpp's, as it is: output n reads the input samples i0 + k_lo .. i0 + k_hi,
// i0 = n M div L, k_hi = k_lo + ntaps - 1. With S_in input samples taken since the channel's last reset:
//   settled   output n is settled once i0 + k_hi <= S_in - 1: it reads no sample still to come, so it is
//             sample n of tfp_resample_pcm of the call so far and of every continuation of the call.
//             N(S_in) = resample_count(S_in - k_hi) outputs are settled, none while S_in <= k_hi
//             (i0 <= A = S_in - 1 - k_hi  <=>  n < (A + 1) L / M  <=>  n < ceil((A + 1) L / M)).
//   carry     output N(S_in), the first unsettled one, has i0 + k_hi >= S_in, so its first tap lies at
//             i0 + k_lo >= S_in - (ntaps - 1): the last ntaps - 1 input samples are all a later push needs.
//             Samples below index 0 are zeros (the batch definition's x = 0 before the clip).
//   flush     after k_hi zero samples N = resample_count(S_in) and the history is tfp_resample_pcm of the
//             call, its last outputs included (the batch form pads with the same zeros).
// The history of a rate object is therefore that of a plain live object that was pushed each tick's newly
// settled samples, and everything behind the history (frames, counts, verdict, windows, traces) is unchanged.
#pragma once

#include <stdint.h>

#include <vector>

#include "tfp_resample.hpp"

namespace tfp {

constexpr int64_t kLiveRateSpanMax = 30720;  // staged samples per tile: tfp_resample.hip's limit (60 KiB of LDS)

inline int64_t live_rate_lag(const ResamplePlan& P) { return (int64_t)P.k_lo + P.ntaps - 1; }  // k_hi >= 0

// The kernel always stages: a pair whose filter alone (two outputs' span) passes the limit is refused.
inline bool live_rate_supported(const ResamplePlan& P) {
  return (int64_t)P.ntaps + ((int64_t)P.M + P.L - 1) / P.L + 1 <= kLiveRateSpanMax;
}

// The staged span of t >= 1 consecutive outputs is at most this many samples.
inline int64_t live_rate_span(const ResamplePlan& P, int64_t t) { return ((t - 1) * P.M) / P.L + 1 + P.ntaps; }

// Outputs per tile: kRsTile, or the most whose span stays within the limit (>= 2 for a supported pair).
inline int32_t live_rate_tile(const ResamplePlan& P) {
  const int64_t room = kLiveRateSpanMax - P.ntaps - 1;  // (t - 1) M div L <= room  <=>  (t - 1) M < (room + 1) L
  if (room < 0) return 1;
  const int64_t t = 1 + ((room + 1) * P.L - 1) / P.M;
  return (int32_t)(t < kRsTile ? t : kRsTile);
}

// N(S_in); -1 when the index arithmetic's range is passed (resample_count).
inline int64_t live_rate_settled(const ResamplePlan& P, int64_t s_in) {
  const int64_t lag = live_rate_lag(P);
  return s_in <= lag ? 0 : resample_count(P, s_in - lag);
}

// One channel's push of n_in >= 0 samples onto s_in_old.
struct LiveRateStep {
  int64_t s_in_new;  // input samples after the push
  int64_t n_old;     // settled before it: the history's length
  int64_t n_new;     // newly settled: outputs [n_old, n_old + n_new)
  int64_t carry_lo;  // the carried span after the push: input samples [carry_lo, s_in_new), carry_lo may be < 0
};
// false when the settled count leaves the index arithmetic's range.
inline bool live_rate_step(const ResamplePlan& P, int64_t s_in_old, int64_t n_in, LiveRateStep* st) {
  st->s_in_new = s_in_old + n_in;
  st->n_old = live_rate_settled(P, s_in_old);
  const int64_t n = live_rate_settled(P, st->s_in_new);
  if (st->n_old < 0 || n < 0) return false;
  st->n_new = n - st->n_old;
  st->carry_lo = st->s_in_new - (P.ntaps - 1);
  return true;
}

// The device's descriptor of one channel's push.
struct LiveRateChan {
  int64_t s_in_old;  // input samples before the push
  int64_t n_old;     // settled before the push
  int32_t n_in;      // tick[c][0, n_in)
  int32_t n_new;     // newly settled
  int32_t parity;    // the carry side the push reads; it writes the other (only when n_in > 0)
  int32_t pad;
};

// The tile table of one push. Tile t < ntiles covers the new outputs [(t - toff[c]) * tile, ...) of channel
// c = tclip[t]; the entries tclip[ntiles ...] name the channels whose carry moves (n_in > 0), one each.
// Returns ntiles = toff[nch]; tclip->size() - ntiles workgroups move a carry.
inline int32_t live_rate_tiles(const LiveRateChan* chan, int32_t nch, int32_t tile, std::vector<int32_t>* toff,
                               std::vector<int32_t>* tclip) {
  toff->assign((size_t)nch + 1, 0);
  tclip->clear();
  for (int32_t c = 0; c < nch; c++) {
    const int32_t nt = (int32_t)(((int64_t)chan[c].n_new + tile - 1) / tile);
    (*toff)[c + 1] = (*toff)[c] + nt;
    tclip->insert(tclip->end(), (size_t)nt, c);
  }
  for (int32_t c = 0; c < nch; c++)
    if (chan[c].n_in > 0) tclip->push_back(c);
  return (*toff)[nch];
}

// Input sample s of a channel during a push, from the three sources the kernel stages from: zero below 0,
// the carry side below s_in_old (carry[i] is input sample s_in_old - (ntaps - 1) + i), else the tick.
inline int16_t live_rate_source(int64_t s, int64_t s_in_old, int32_t ntaps, const int16_t* carry, const int16_t* tick,
                                int64_t n_in) {
  if (s < 0) return 0;
  if (s < s_in_old) {
    const int64_t i = s - (s_in_old - (ntaps - 1));
    return i >= 0 && i < ntaps - 1 ? carry[i] : (int16_t)0;
  }
  const int64_t t = s - s_in_old;
  return t < n_in ? tick[t] : (int16_t)0;
}

// One channel on the host: the same carry-and-convert over resample_sample.
struct LiveRateHost {
  int64_t s_in = 0;               // input samples since the last reset
  int32_t parity = 0;             // the carry side the next push reads
  std::vector<int16_t> carry[2];  // ntaps - 1 samples each, sized by the first push
  void reset() { s_in = 0; }      // (the carry stays: samples below index 0 are never read from it)
};
// Pushes x[0, n_in) and appends the newly settled samples to *hist (hist->size() = the settled count
// before). 0: done. 1: the settled count would pass max_samples, nothing changed. -1: the index range.
inline int live_rate_push_host(const ResampleTable& T, LiveRateHost* st, const int16_t* x, int64_t n_in, int64_t max_samples,
                               std::vector<int16_t>* hist) {
  const ResamplePlan& P = T.plan;
  LiveRateStep step;
  if (!live_rate_step(P, st->s_in, n_in, &step)) return -1;
  if (step.n_old + step.n_new > max_samples) return 1;
  if (n_in <= 0) return 0;  // an idle channel keeps its parity
  const int32_t nc = P.ntaps - 1;
  for (auto& side : st->carry) side.resize((size_t)nc, 0);
  const int16_t* rd = st->carry[st->parity].data();
  std::vector<int16_t>& wr = st->carry[1 - st->parity];
  // the span [lo, hi) every new output and the new carry read, staged with zeros below index 0
  const int64_t lo = st->s_in - nc, hi = step.s_in_new;
  std::vector<int16_t> span((size_t)(hi - lo));
  for (int64_t s = lo; s < hi; s++) span[(size_t)(s - lo)] = live_rate_source(s, st->s_in, P.ntaps, rd, x, n_in);
  for (int64_t n = step.n_old; n < step.n_old + step.n_new; n++)
    hist->push_back(resample_sample(P, T.taps.data(), span.data(), lo, hi, n));
  for (int32_t i = 0; i < nc; i++) wr[(size_t)i] = span[(size_t)(step.carry_lo + i - lo)];
  st->parity = 1 - st->parity;
  st->s_in = step.s_in_new;
  return 0;
}

#if defined(__HIPCC__) || defined(__HIP__)
// One launch in place of launch_live_scatter / launch_live_scatter_g711 on a rate object. tick[nch][T]:
// int16 (law < 0) or G.711 codes of law kG711Ulaw / kG711Alaw, expanded by tfp_g711.hpp's map while
// staging. d_chan[nch], d_toff / d_tclip: live_rate_tiles with tile = live_rate_tile(P), ntiles and
// nmove = tclip.size() - ntiles; max_new: the greatest n_new (sizes the staged span). d_carry: int16
// [2][nch][ntaps - 1]; a push reads side parity and writes side 1 - parity, so no workgroup reads
// carry that another workgroup of the launch writes. Writes hist[c][n_old, n_old + n_new) (the host has
// checked n_old + n_new <= max_samples). ntiles + nmove = 0 launches nothing.
hipError_t launch_live_rate(const ResamplePlan& P, const int16_t* d_taps, const void* d_tick, int32_t law, int32_t T,
                            const LiveRateChan* d_chan, int32_t nch, const int32_t* d_toff, const int32_t* d_tclip,
                            int32_t ntiles, int32_t nmove, int32_t max_new, int16_t* d_carry, int64_t max_samples,
                            int16_t* d_hist, hipStream_t stream);
#endif

}  // namespace tfp
