// tfp_resample_mix.hip — interleaved int16 frames of C channels at one rate onto the int16 path at the
// index's rate: the multichannel form of tfp_resample.hip (tfp_resample.hpp, "the multichannel form").
//
// The converter is linear and exact, so the channels are summed first and the filter runs once over
// the sums: its cost does not depend on C. One workgroup per tile of kRsTile consecutive outputs of
// one clip, on the tile tables resample_tiles gives (the mono launch's own).
//
// Staging. The tile's span of frames [lo, hi), clipped to the clip's own [0, n_in), is one contiguous
// run of (fb - fa) C int16 in the interleaved input. The workgroup first zeroes the span's int32 sums
// in LDS (so frames past the clip's ends count as 0 and a neighbour's frames are never read), then
// walks the run word by word: lane j takes the 4-byte aligned word j of the run (consecutive lanes,
// consecutive words: full coalesced lines whatever C is), splits it into its two samples and adds each
// to its frame's sum with an LDS atomic add. A clip's first sample is only 2-byte aligned when C or its
// frame offset is odd: the walk starts at the aligned word that holds the first sample, and the two
// words that straddle the run's ends are read as single int16, so nothing outside the run is touched.
// Integer adds commute, so the sums are exact whatever order the adds land in.
//
// The filter loop is then the mono kernel's over int32 sums: one 64-bit multiply-add per tap, one floor
// division by the wave-uniform 32768 C (a shift and a 32-bit division, resample_mix_round) and one clamp
// per output. The taps are read from the pair's table in global memory, as both mono kernels read them;
// staging them in LDS is out of scope here and unmeasured.
//
// The LDS budget, kRsMixSpanMax = 15,360 sums = 60 KiB: the bytes the mono kernel stages (30,720
// int16), for the same reason. A CU has 160 KiB, so two workgroups (8 waves, 2 per SIMD) are resident
// with 40 KiB to spare, which lets one workgroup stage while the other filters; 80 KiB each would fill
// the CU exactly and leave no room for another kernel's workgroup beside them, and one workgroup per CU
// would leave every SIMD with a single wave and nothing to cover the tap reads' latency. At 4 bytes per
// frame the budget covers reductions up to about 14 (15,360 / (1,023 + 48) frames per output); the
// pairs the form exists for (44100 -> 8000: 5,906 frames, 48000 -> 8000: 6,428) use under half of it.
// A pair past it reads its clip in global memory, summing the channels per tap, bounds checked per
// output, as resample_kernel<false> does.
//
// Equal rates run no filter and touch no table: the same staging over the identity span (L = M = 1,
// one tap position), then y[i] = floor((2 S[i] + C) / (2 C)) (resample_mix_mean).
#include <hip/hip_runtime.h>

#include "tfp_resample.hpp"

namespace tfp {
namespace {

constexpr int kBlock = 256;
enum MixForm { kStaged = 0, kGlobal = 1, kDownmix = 2 };

// The staged span of a tile of a plan is at most this many frames (tfp_resample.hip's span_max).
inline int64_t span_max(const ResamplePlan& P) { return ((int64_t)(kRsTile - 1) * P.M) / P.L + 1 + P.ntaps; }

template <int FORM>
__global__ __launch_bounds__(kBlock) void resample_mix_kernel(ResamplePlan P, const int16_t* __restrict__ taps, int32_t C,
                                                              const int16_t* __restrict__ in,
                                                              const int64_t* __restrict__ in_off,
                                                              const int64_t* __restrict__ out_off,
                                                              const int32_t* __restrict__ toff,
                                                              const int32_t* __restrict__ tclip, int16_t* __restrict__ out) {
  extern __shared__ int32_t sums[];
  const int32_t c = tclip[blockIdx.x];
  const int64_t n_in = in_off[c + 1] - in_off[c], n_out = out_off[c + 1] - out_off[c];
  const int64_t n0 = (int64_t)((int32_t)blockIdx.x - toff[c]) * kRsTile;
  const int64_t n1 = n0 + kRsTile < n_out ? n0 + kRsTile : n_out;
  if (n0 >= n1) return;  // (uniform; resample_tiles gives no such tile)
  const int16_t* __restrict__ x = in + in_off[c] * C;  // the clip's first sample
  int16_t* __restrict__ y = out + out_off[c];
  if (FORM == kGlobal) {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_mix_sample_frames(P, taps, x, n_in, n, C);
    return;
  }
  // frames [lo, hi) of the clip: the first output's first tap to the last output's last tap
  const int64_t lo = (n0 * P.M) / P.L + P.k_lo, hi = ((n1 - 1) * P.M) / P.L + P.k_lo + P.ntaps;
  const int32_t len = (int32_t)(hi - lo);  // <= span_max(P) <= kRsMixSpanMax
  for (int32_t i = threadIdx.x; i < len; i += kBlock) sums[i] = 0;
  __syncthreads();
  // the clip's own frames [fa, fb) of the span: (fb - fa) C samples from xs, frame fa's sum at sums[fa - lo]
  const int64_t fa = lo > 0 ? lo : 0, fb = hi < n_in ? hi : n_in;
  if (fb > fa) {
    const int16_t* __restrict__ xs = x + fa * C;
    const int32_t total = (int32_t)(fb - fa) * C;  // <= kRsMixSpanMax * 32 < 2^19
    const int32_t head = (int32_t)((reinterpret_cast<uintptr_t>(xs) >> 1) & 1);  // xs sits in a word's upper half
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(xs - head);
    const int32_t nwords = (head + total + 1) / 2;
    int32_t* __restrict__ dst = sums + (int32_t)(fa - lo);
    for (int32_t j = threadIdx.x; j < nwords; j += kBlock) {
      const int32_t s0 = 2 * j - head, s1 = s0 + 1;  // the word's samples, counted from xs
      int32_t v0 = 0, v1 = 0;
      if (s0 >= 0 && s1 < total) {
        const uint32_t u = w[j];
        v0 = (int32_t)(int16_t)(u & 0xffffu);
        v1 = (int32_t)(int16_t)(u >> 16);
      } else {  // a word that straddles an end of the run: its samples inside the run, singly
        if (s0 >= 0) v0 = xs[s0];
        if (s1 < total) v1 = xs[s1];
      }
      const int32_t f0 = s0 >= 0 ? (int32_t)((uint32_t)s0 / (uint32_t)C) : 0;
      const int32_t f1 = s1 < total ? (int32_t)((uint32_t)s1 / (uint32_t)C) : f0;  // (f0, f1 < fb - fa)
      if (f0 == f1) {
        atomicAdd(dst + f0, v0 + v1);
      } else {
        atomicAdd(dst + f0, v0);
        atomicAdd(dst + f1, v1);
      }
    }
  }
  __syncthreads();
  if (FORM == kDownmix) {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_mix_mean(sums[n - lo], C);
  } else {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_mix_sample(P, taps, sums, lo, hi, n, C);
  }
}

}  // namespace

hipError_t launch_resample_mix(const ResamplePlan& P_in, const int16_t* d_taps, bool downmix, int32_t C, const int16_t* d_in,
                               const int64_t* d_in_off, const int64_t* d_out_off, const int32_t* d_toff,
                               const int32_t* d_tclip, int32_t ntiles, int16_t* d_out, hipStream_t stream, bool* staged) {
  const ResamplePlan P = downmix ? ResamplePlan{1, 1, 0, 1} : P_in;  // the identity span: frame n under output n
  if (staged) *staged = false;
  if (ntiles < 0 || C < 1 || C > kRsMixChannelsMax || P.L < 1 || P.M < 1 || P.ntaps < 1 ||
      (int64_t)P.L * P.ntaps > kRsMaxEntries)
    return hipErrorInvalidValue;
  if (ntiles == 0) return hipSuccess;
  if ((!downmix && !d_taps) || !d_in || !d_in_off || !d_out_off || !d_toff || !d_tclip || !d_out) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(d_in) & 3) return hipErrorInvalidValue;
  const int64_t span = span_max(P);
  const size_t lds = sizeof(int32_t) * (size_t)span;
  if (downmix) {
    hipLaunchKernelGGL(resample_mix_kernel<kDownmix>, dim3((unsigned)ntiles), dim3(kBlock), lds, stream, P, d_taps, C, d_in,
                       d_in_off, d_out_off, d_toff, d_tclip, d_out);
  } else if (span <= kRsMixSpanMax) {
    hipLaunchKernelGGL(resample_mix_kernel<kStaged>, dim3((unsigned)ntiles), dim3(kBlock), lds, stream, P, d_taps, C, d_in,
                       d_in_off, d_out_off, d_toff, d_tclip, d_out);
  } else {
    hipLaunchKernelGGL(resample_mix_kernel<kGlobal>, dim3((unsigned)ntiles), dim3(kBlock), 0, stream, P, d_taps, C, d_in,
                       d_in_off, d_out_off, d_toff, d_tclip, d_out);
  }
  if (staged) *staged = downmix || span <= kRsMixSpanMax;
  return hipGetLastError();
}

}  // namespace tfp
