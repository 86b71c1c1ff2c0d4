// tfp_live_rate.hip — a rate object's push (tfp_live_rate.hpp): the tick, taken at the object's input rate,
// converted into each channel's int16 history at the index's rate, and each channel's carried input tail
// moved on. One launch in place of the scatter; everything behind the history is the plain push.
//
// Tile workgroups (blockIdx.x < ntiles): one per tile of at most live_rate_tile(P) newly settled outputs
// of one channel, as resample_kernel<true>: the tile's input span is staged in LDS as int16 and every
// output is formed from it by resample_sample (the one definition), the taps read from the engine's
// device table of the pair. A staged sample comes from one of three sources: zero (index below 0), the
// channel's carry (below s_in_old) or the tick (at or above it; G.711 codes are expanded here, so the
// carry is int16 whatever a push held). A settled output reads no sample at or past s_in_old + n_in, and
// the first new one none before s_in_old - (ntaps - 1) (tfp_live_rate.hpp), so the three cover the span.
//
// Move workgroups (the rest): one per channel with n_in > 0, whether or not it settled an output: the last
// ntaps - 1 input samples, from the same three sources, into the other carry side. Every workgroup of
// the launch reads side `parity` and the tick alone, and only move workgroups write, to side 1 - parity
// of their own channel: no workgroup reads what another writes, however many tiles a channel spans. The
// host flips the parity of the channels that moved.
//
// 256 threads: four wave64s share one staged span; a 20 ms tick settles 160 outputs at 8 kHz (three
// waves busy, as many products per output as the filter has taps), and the span of a tick is a few KiB of
// LDS, sized per launch, so several workgroups share a CU. Every value leaves through plain 2-byte
// vector stores (the history offset n_old is of any parity); no atomics.
#include <hip/hip_runtime.h>

#include "tfp_g711.hpp"
#include "tfp_live_rate.hpp"

namespace tfp {
namespace {

constexpr int kBlock = 256;

// Input sample s of the channel (live_rate_source, with the tick's law): LAW < 0 is int16.
template <int LAW>
__device__ __forceinline__ int16_t rate_source(int64_t s, const LiveRateChan& lc, int32_t ntaps,
                                               const int16_t* __restrict__ carry, const void* __restrict__ tick) {
  if (s < 0) return 0;
  if (s < lc.s_in_old) {
    const int64_t i = s - (lc.s_in_old - (ntaps - 1));
    return i >= 0 && i < ntaps - 1 ? carry[i] : (int16_t)0;
  }
  const int64_t t = s - lc.s_in_old;
  if (t >= lc.n_in) return 0;
  if (LAW < 0) return static_cast<const int16_t*>(tick)[t];
  return (int16_t)g711_expand<(LAW < 0 ? kG711Ulaw : LAW)>(static_cast<const uint8_t*>(tick)[t]);
}

template <int LAW>
__global__ __launch_bounds__(kBlock) void live_rate_kernel(ResamplePlan P, const int16_t* __restrict__ taps,
                                                           const void* __restrict__ tick, int32_t T,
                                                           const LiveRateChan* __restrict__ chan,
                                                           const int32_t* __restrict__ toff,
                                                           const int32_t* __restrict__ tclip, int32_t ntiles, int32_t tile,
                                                           int32_t nch, int16_t* __restrict__ carry, int64_t max_samples,
                                                           int16_t* __restrict__ hist) {
  extern __shared__ int16_t span[];
  const int32_t b = (int32_t)blockIdx.x;
  const int32_t c = tclip[b];
  if (c < 0 || c >= nch) return;  // (uniform; live_rate_tiles names channels only)
  const LiveRateChan lc = chan[c];
  const int32_t nc = P.ntaps - 1;
  const int16_t* __restrict__ rd = carry + ((int64_t)(lc.parity & 1) * nch + c) * nc;
  const void* __restrict__ tk = LAW < 0 ? static_cast<const void*>(static_cast<const int16_t*>(tick) + (int64_t)c * T)
                                        : static_cast<const void*>(static_cast<const uint8_t*>(tick) + (int64_t)c * T);
  if (b >= ntiles) {  // this channel's carry: input samples [s_in_new - nc, s_in_new) to the other side
    int16_t* __restrict__ wr = carry + ((int64_t)(1 - (lc.parity & 1)) * nch + c) * nc;
    const int64_t lo = lc.s_in_old + lc.n_in - nc;
    for (int32_t i = threadIdx.x; i < nc; i += kBlock) wr[i] = rate_source<LAW>(lo + i, lc, P.ntaps, rd, tk);
    return;
  }
  const int64_t j0 = (int64_t)(b - toff[c]) * tile;
  const int64_t j1 = j0 + tile < lc.n_new ? j0 + tile : lc.n_new;
  if (j0 >= j1) return;  // (uniform; live_rate_tiles gives no such tile)
  const int64_t n0 = lc.n_old + j0, n1 = lc.n_old + j1;
  // samples [lo, hi) of the call: the first output's first tap to the last output's last tap
  const int64_t lo = (n0 * P.M) / P.L + P.k_lo, hi = ((n1 - 1) * P.M) / P.L + P.k_lo + P.ntaps;
  const int32_t len = (int32_t)(hi - lo);  // <= live_rate_span(P, j1 - j0): the launch's LDS
  for (int32_t i = threadIdx.x; i < len; i += kBlock) span[i] = rate_source<LAW>(lo + i, lc, P.ntaps, rd, tk);
  __syncthreads();
  int16_t* __restrict__ y = hist + (int64_t)c * max_samples;
  for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock)
    if (n < max_samples) y[n] = resample_sample(P, taps, span, lo, hi, n);
}

}  // namespace

hipError_t launch_live_rate(const ResamplePlan& P, const int16_t* d_taps, const void* d_tick, int32_t law, int32_t T,
                            const LiveRateChan* d_chan, int32_t nch, const int32_t* d_toff, const int32_t* d_tclip,
                            int32_t ntiles, int32_t nmove, int32_t max_new, int16_t* d_carry, int64_t max_samples,
                            int16_t* d_hist, hipStream_t stream) {
  if (ntiles < 0 || nmove < 0 || nch <= 0 || T <= 0 || max_new < 0 || P.L < 1 || P.M < 1 || P.ntaps < 1 ||
      (int64_t)P.L * P.ntaps > kRsMaxEntries || !live_rate_supported(P) || (law >= 0 && !g711_law_ok(law)))
    return hipErrorInvalidValue;
  if (ntiles + nmove == 0) return hipSuccess;
  if (!d_taps || !d_tick || !d_chan || !d_toff || !d_tclip || !d_carry || !d_hist) return hipErrorInvalidValue;
  const int32_t tile = live_rate_tile(P);
  const int64_t span = live_rate_span(P, max_new < tile ? (max_new > 1 ? max_new : 1) : tile);  // <= kLiveRateSpanMax
  const dim3 grid((unsigned)(ntiles + nmove));
  const size_t lds = sizeof(int16_t) * (size_t)span;
#define TFP_LIVE_RATE_LAUNCH(LAW)                                                                                        \
  hipLaunchKernelGGL(live_rate_kernel<LAW>, grid, dim3(kBlock), lds, stream, P, d_taps, d_tick, T, d_chan, d_toff, d_tclip, \
                     ntiles, tile, nch, d_carry, max_samples, d_hist)
  if (law < 0)
    TFP_LIVE_RATE_LAUNCH(-1);
  else if (law == kG711Alaw)
    TFP_LIVE_RATE_LAUNCH(kG711Alaw);
  else
    TFP_LIVE_RATE_LAUNCH(kG711Ulaw);
#undef TFP_LIVE_RATE_LAUNCH
  return hipGetLastError();
}

}  // namespace tfp
