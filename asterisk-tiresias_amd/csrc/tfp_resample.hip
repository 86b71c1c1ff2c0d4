// tfp_resample.hip — int16 PCM of one rate onto the int16 path at the index's rate (tfp_resample.hpp).
//
// The kernel sits in front of launch_fingerprint and changes nothing behind it: the host moves the
// samples to the card as they are, and the fingerprint kernels read the converted int16 where this
// launch wrote it. Integer arithmetic only (resample_sample, the host's routine), so the output equals
// tfp_resample_pcm bit for bit.
//
// One workgroup per tile of kRsTile consecutive outputs of one clip. The tile's input span, about
// kRsTile M / L + ntaps samples, is staged in LDS once with zeros past the clip's own ends (never a
// neighbour's samples), and every output is formed from it. A pair whose span passes kSpanMax samples
// (a reduction by more than about 29) reads its clip in global memory instead, bounds checked per
// output. The taps are read from the table in global memory: a table is up to 2 MiB, far past LDS for
// a pair of many phases, and one form for every pair keeps one definition; lanes of one wave walk
// their phases' rows in step, so the rows stay in L2 / the vector cache. Measured on an MI355X over
// 1,024 clips of 5 s (profiles/resample_latency.json): 1.23 ms at 16000 -> 8000 (one phase: the tap
// reads are uniform over a wave), 11.9 ms at 44100 -> 8000 (80 phases: every lane reads its own row),
// 3.2 against 0.9 G multiply-adds per ms. The choice of global taps is by these two timings only: that the
// per-lane tap reads make the difference is a supposition (no counter run stands behind it; the 64-bit
// add per product and the 2-byte LDS reads at stride M / L may weigh as much), and taps staged in LDS
// for the tables that fit have not been measured against it.
#include <hip/hip_runtime.h>

#include "tfp_resample.hpp"

namespace tfp {
namespace {

constexpr int kBlock = 256;
constexpr int64_t kSpanMax = kRsSpanMax;  // staged samples per tile (60 KiB of LDS)

// The staged span of a tile of a plan is at most this many samples.
inline int64_t span_max(const ResamplePlan& P) { return ((int64_t)(kRsTile - 1) * P.M) / P.L + 1 + P.ntaps; }

template <bool STAGED>
__global__ __launch_bounds__(kBlock) void resample_kernel(ResamplePlan P, const int16_t* __restrict__ taps,
                                                          const int16_t* __restrict__ in,
                                                          const int64_t* __restrict__ in_off,
                                                          const int64_t* __restrict__ out_off,
                                                          const int32_t* __restrict__ toff,
                                                          const int32_t* __restrict__ tclip, int16_t* __restrict__ out) {
  extern __shared__ int16_t span[];
  const int32_t c = tclip[blockIdx.x];
  const int64_t n_in = in_off[c + 1] - in_off[c], n_out = out_off[c + 1] - out_off[c];
  const int64_t n0 = (int64_t)((int32_t)blockIdx.x - toff[c]) * kRsTile;
  const int64_t n1 = n0 + kRsTile < n_out ? n0 + kRsTile : n_out;
  if (n0 >= n1) return;  // (uniform; resample_tiles gives no such tile)
  const int16_t* __restrict__ x = in + in_off[c];
  int16_t* __restrict__ y = out + out_off[c];
  if (STAGED) {
    // samples [lo, hi) of the clip: the first output's first tap to the last output's last tap
    const int64_t lo = (n0 * P.M) / P.L + P.k_lo, hi = ((n1 - 1) * P.M) / P.L + P.k_lo + P.ntaps;
    const int32_t len = (int32_t)(hi - lo);  // <= span_max(P) <= kSpanMax
    for (int32_t i = threadIdx.x; i < len; i += kBlock) {
      const int64_t s = lo + i;
      span[i] = s >= 0 && s < n_in ? x[s] : (int16_t)0;
    }
    __syncthreads();
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_sample(P, taps, span, lo, hi, n);
  } else {
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kBlock) y[n] = resample_sample(P, taps, x, 0, n_in, n);
  }
}

}  // namespace

hipError_t launch_resample(const ResamplePlan& P, const int16_t* d_taps, const int16_t* d_in, const int64_t* d_in_off,
                           const int64_t* d_out_off, const int32_t* d_toff, const int32_t* d_tclip, int32_t ntiles,
                           int16_t* d_out, hipStream_t stream) {
  if (ntiles < 0 || P.L < 1 || P.M < 1 || P.ntaps < 1 || (int64_t)P.L * P.ntaps > kRsMaxEntries) return hipErrorInvalidValue;
  if (ntiles == 0) return hipSuccess;
  if (!d_taps || !d_in || !d_in_off || !d_out_off || !d_toff || !d_tclip || !d_out) return hipErrorInvalidValue;
  const int64_t span = span_max(P);
  if (span <= kSpanMax)
    hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)ntiles), dim3(kBlock), sizeof(int16_t) * (size_t)span, stream, P,
                       d_taps, d_in, d_in_off, d_out_off, d_toff, d_tclip, d_out);
  else
    hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)ntiles), dim3(kBlock), 0, stream, P, d_taps, d_in, d_in_off,
                       d_out_off, d_toff, d_tclip, d_out);
  return hipGetLastError();
}

}  // namespace tfp
