// tfp_resample_wide.hip — interleaved int32 Q31 frames of C channels at one rate onto the int16 path at
// the index's rate: the wide form of tfp_resample_mix.hip (tfp_resample.hpp, "the wide form").
//
// One workgroup of 256 threads per tile of kRsTile consecutive outputs of one clip, on the tile tables
// resample_tiles gives (the mono launch's own). The filter runs once per output whatever C is; the taps
// are read from the pair's table in global memory, as the other three kernels read them (staging them in
// LDS is out of scope here and unmeasured). Four forms:
//
//  - C = 1, staged. The tile's span of samples [lo, hi) goes to LDS as int32 with plain coalesced
//    stores, zeros past the clip's ends. Up to kRsMixSpanMax = 15,360 samples = 60 KiB. The filter loop
//    is one (int64)h * (int64)s multiply-add per tap.
//  - C >= 2, staged. The workgroup zeroes the span's int64 sums in LDS, then walks the clip's own frames
//    of the span, one contiguous run of (fb - fa) C words: lane j takes word j (consecutive lanes,
//    consecutive words: full coalesced lines whatever C is) and adds it to sums[j / C] with a 64-bit LDS
//    atomic add. Every word is one whole sample and the input is 4-byte aligned, so there is no
//    alignment head and no straddling word, unlike the int16 kernel. Integer adds commute, so the sums
//    are exact whatever order the adds land in. Up to kRsWideSpanMax = 7,680 sums: the same 60 KiB, kept
//    for the residency reason written at the top of tfp_resample_mix.hip (two workgroups per CU with
//    room to spare). 44100 -> 8000 (5,906 frames) and 48000 -> 8000 (6,428) fit it.
//  - Global. A pair past its form's staging limit reads its clip in global memory, summing the channels
//    per tap, bounds checked per output (resample_wide_sample_frames).
//  - Downmix. Equal rates run no filter and read no table: C >= 2 stages over the identity span (L = M
//    = 1, one tap position) and applies resample_wide_mean; C = 1 rounds and clamps each sample as read.
//
// The 64-bit LDS atomic. atomicAdd on an unsigned long long in LDS whose result is not used compiles to
// one ds_add_u64 per lane for gfx950 (no compare-and-swap loop; seen in the compiler's assembly for this
// file), against one ds_add_u32 in the int16 kernel. C consecutive lanes add to the same sum, so a
// wave's 64 adds fall on 64 / C + 1 addresses at most and the LDS serialises the adds that share one.
// How long that takes, and how the staging time of this kernel compares with the int16 kernel's at the
// same frame count (twice the bytes read, 8-byte instead of 4-byte atomics), has not been measured: only
// whole calls were timed (scripts/resample_wide_latency.py).
#include <hip/hip_runtime.h>

#include "tfp_resample.hpp"

namespace tfp {
namespace {

constexpr int kBlock = 256;

// The staged span of a tile of a plan is at most this many frames (tfp_resample.hip's span_max).
inline int64_t span_max(const ResamplePlan& P) { return ((int64_t)(kRsTile - 1) * P.M) / P.L + 1 + P.ntaps; }

template <int FORM>
__global__ __launch_bounds__(kBlock) void resample_wide_kernel(ResamplePlan P, const int16_t* __restrict__ taps, int32_t C,
                                                               const int32_t* __restrict__ in,
                                                               const int64_t* __restrict__ in_off,
                                                               const int64_t* __restrict__ out_off,
                                                               const int32_t* __restrict__ toff,
                                                               const int32_t* __restrict__ tclip, int16_t* __restrict__ out) {
  extern __shared__ int64_t wide_lds[];  // int64 sums, or the mono form's int32 samples
  const int32_t c = tclip[blockIdx.x];
  const int64_t n_in = in_off[c + 1] - in_off[c], n_out = out_off[c + 1] - out_off[c];
  const int64_t n0 = (int64_t)((int32_t)blockIdx.x - toff[c]) * kRsTile;
  const int64_t n1 = n0 + kRsTile < n_out ? n0 + kRsTile : n_out;
  if (n0 >= n1) return;  // (uniform; resample_tiles gives no such tile)
  const int32_t* __restrict__ x = in + in_off[c] * C;  // the clip's first sample
  int16_t* __restrict__ y = out + out_off[c];
  if (FORM == kRsWideGlobal) {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_wide_sample_frames(P, taps, x, n_in, n, C);
    return;
  }
  if (FORM == kRsWideDownmix && C == 1) {  // (uniform) n_out = n_in: nothing to sum
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_wide_mean((int64_t)x[n], 1);
    return;
  }
  // frames [lo, hi) of the clip: the first output's first tap to the last output's last tap
  const int64_t lo = (n0 * P.M) / P.L + P.k_lo, hi = ((n1 - 1) * P.M) / P.L + P.k_lo + P.ntaps;
  const int32_t len = (int32_t)(hi - lo);  // <= span_max(P) <= the form's staging limit
  if (FORM == kRsWideStagedMono) {
    int32_t* __restrict__ s = reinterpret_cast<int32_t*>(wide_lds);
    for (int32_t i = threadIdx.x; i < len; i += kBlock) {
      const int64_t f = lo + i;
      s[i] = f >= 0 && f < n_in ? x[f] : 0;
    }
    __syncthreads();
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_wide_sample(P, taps, s, lo, hi, n, 1);
    return;
  }
  int64_t* __restrict__ sums = wide_lds;
  for (int32_t i = threadIdx.x; i < len; i += kBlock) sums[i] = 0;
  __syncthreads();
  // the clip's own frames [fa, fb) of the span: (fb - fa) C words from xs, frame fa's sum at sums[fa - lo]
  const int64_t fa = lo > 0 ? lo : 0, fb = hi < n_in ? hi : n_in;
  if (fb > fa) {
    const int32_t* __restrict__ xs = x + fa * C;
    const int32_t total = (int32_t)(fb - fa) * C;  // <= kRsWideSpanMax * 32 < 2^18
    unsigned long long* __restrict__ dst = reinterpret_cast<unsigned long long*>(sums + (int32_t)(fa - lo));
    for (int32_t j = threadIdx.x; j < total; j += kBlock)  // (j / C < fb - fa <= len - (fa - lo))
      atomicAdd(dst + (int32_t)((uint32_t)j / (uint32_t)C), (unsigned long long)(int64_t)xs[j]);
  }
  __syncthreads();
  if (FORM == kRsWideDownmix) {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_wide_mean(sums[n - lo], C);
  } else {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_wide_sample(P, taps, sums, lo, hi, n, C);
  }
}

}  // namespace

hipError_t launch_resample_wide(const ResamplePlan& P_in, const int16_t* d_taps, bool downmix, int32_t C, const int32_t* d_in,
                                const int64_t* d_in_off, const int64_t* d_out_off, const int32_t* d_toff,
                                const int32_t* d_tclip, int32_t ntiles, int16_t* d_out, hipStream_t stream,
                                ResampleWideForm* form) {
  const ResamplePlan P = downmix ? ResamplePlan{1, 1, 0, 1} : P_in;  // the identity span: frame n under output n
  if (form) *form = kRsWideNone;
  if (ntiles < 0 || C < 1 || C > kRsMixChannelsMax || P.L < 1 || P.M < 1 || P.ntaps < 1 ||
      (int64_t)P.L * P.ntaps > kRsMaxEntries)
    return hipErrorInvalidValue;
  if (ntiles == 0) return hipSuccess;
  if ((!downmix && !d_taps) || !d_in || !d_in_off || !d_out_off || !d_toff || !d_tclip || !d_out) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(d_in) & 3) return hipErrorInvalidValue;
  const int64_t span = span_max(P);
  ResampleWideForm f;
  if (downmix) {
    f = kRsWideDownmix;  // (span = kRsTile + 1 sums)
    hipLaunchKernelGGL(resample_wide_kernel<kRsWideDownmix>, dim3((unsigned)ntiles), dim3(kBlock),
                       C == 1 ? 0 : sizeof(int64_t) * (size_t)span, stream, P, d_taps, C, d_in, d_in_off, d_out_off, d_toff,
                       d_tclip, d_out);
  } else if (C == 1 && span <= kRsMixSpanMax) {
    f = kRsWideStagedMono;
    hipLaunchKernelGGL(resample_wide_kernel<kRsWideStagedMono>, dim3((unsigned)ntiles), dim3(kBlock),
                       sizeof(int32_t) * (size_t)span, stream, P, d_taps, C, d_in, d_in_off, d_out_off, d_toff, d_tclip, d_out);
  } else if (C >= 2 && span <= kRsWideSpanMax) {
    f = kRsWideStagedSums;
    hipLaunchKernelGGL(resample_wide_kernel<kRsWideStagedSums>, dim3((unsigned)ntiles), dim3(kBlock),
                       sizeof(int64_t) * (size_t)span, stream, P, d_taps, C, d_in, d_in_off, d_out_off, d_toff, d_tclip, d_out);
  } else {
    f = kRsWideGlobal;
    hipLaunchKernelGGL(resample_wide_kernel<kRsWideGlobal>, dim3((unsigned)ntiles), dim3(kBlock), 0, stream, P, d_taps, C, d_in,
                       d_in_off, d_out_off, d_toff, d_tclip, d_out);
  }
  if (form) *form = f;
  return hipGetLastError();
}

}  // namespace tfp
