// tfp_g711.hip — G.711 codes onto the int16 path the fingerprint kernels read (tfp_g711.hpp).
//
// Both kernels sit in front of launch_fingerprint and change nothing behind it: the host moves one
// byte per sample to the card, and the fingerprint kernels read the same int16 they read for an
// int16 call (aubio_source's table[code] / 32768, /root/reference/src/fp_handler.c:604, :633).
#include <hip/hip_runtime.h>

#include "tfp_g711.hpp"

namespace tfp {
namespace {

constexpr int kBlock = 256;
constexpr int kCodesPerLane = 16;  // one 16-byte load, two 16-byte stores

// Four codes (one loaded word) to four int16, as two packed words.
template <int LAW>
__device__ __forceinline__ void expand_word(uint32_t w, uint32_t* lo, uint32_t* hi) {
  const uint32_t s0 = (uint32_t)g711_expand<LAW>(w & 0xFFu) & 0xFFFFu;
  const uint32_t s1 = (uint32_t)g711_expand<LAW>((w >> 8) & 0xFFu) & 0xFFFFu;
  const uint32_t s2 = (uint32_t)g711_expand<LAW>((w >> 16) & 0xFFu) & 0xFFFFu;
  const uint32_t s3 = (uint32_t)g711_expand<LAW>(w >> 24) & 0xFFFFu;
  *lo = s0 | (s1 << 16);
  *hi = s2 | (s3 << 16);
}

// A bandwidth kernel over one flat array: the clip layout of the batch does not matter to it (clip
// c starts at sample offsets[c] - offsets[0], at any residue). Lane g of the grid takes the codes
// [16 g, 16 g + 16); the n % 16 codes after the last whole group are done one each by the grid's
// first lanes.
template <int LAW>
__global__ __launch_bounds__(kBlock) void g711_expand_kernel(const uint8_t* __restrict__ codes, int64_t n,
                                                             int16_t* __restrict__ pcm) {
  const int64_t ngroups = n / kCodesPerLane;
  const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(codes);
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(pcm);
  for (int64_t g = gid; g < ngroups; g += (int64_t)gridDim.x * kBlock) {
    const uint4 w = src[g];
    uint4 a, b;
    expand_word<LAW>(w.x, &a.x, &a.y);
    expand_word<LAW>(w.y, &a.z, &a.w);
    expand_word<LAW>(w.z, &b.x, &b.y);
    expand_word<LAW>(w.w, &b.z, &b.w);
    dst[2 * g] = a;
    dst[2 * g + 1] = b;
  }
  const int64_t tail = ngroups * kCodesPerLane + gid;  // gid < n % 16 only
  if (gid < kCodesPerLane && tail < n) pcm[tail] = (int16_t)g711_expand<LAW>(codes[tail]);
}

// stream_scatter_kernel (tfp_engine.cpp) with the expansion fused in: ring[c][2 W], every sample
// written at p and p + W, so a channel's last W samples are the run ring[c][wpos .. wpos + W).
template <int LAW>
__global__ __launch_bounds__(kBlock) void stream_scatter_g711_kernel(const uint8_t* __restrict__ tick, int32_t T,
                                                                     int64_t W, int64_t wpos, int32_t nch,
                                                                     int16_t* __restrict__ ring) {
  const int64_t n = (int64_t)nch * T;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int64_t c = i / T, t = i % T;
    int64_t p = wpos + t;
    if (p >= W) p -= W;
    const int16_t v = (int16_t)g711_expand<LAW>(tick[i]);
    ring[c * 2 * W + p] = v;
    ring[c * 2 * W + p + W] = v;
  }
}

}  // namespace

hipError_t launch_g711_expand(const uint8_t* d_codes, int64_t n, int32_t law, int16_t* d_pcm, hipStream_t stream) {
  if (n < 0 || !g711_law_ok(law)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  if (!d_codes || !d_pcm || (reinterpret_cast<uintptr_t>(d_codes) & 15) || (reinterpret_cast<uintptr_t>(d_pcm) & 15))
    return hipErrorInvalidValue;  // (the 16-byte loads and stores)
  const int64_t ngroups = n / kCodesPerLane;
  const int64_t blocks = (ngroups + kBlock - 1) / kBlock;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks)));
  if (law == kG711Alaw)
    hipLaunchKernelGGL(g711_expand_kernel<kG711Alaw>, grid, dim3(kBlock), 0, stream, d_codes, n, d_pcm);
  else
    hipLaunchKernelGGL(g711_expand_kernel<kG711Ulaw>, grid, dim3(kBlock), 0, stream, d_codes, n, d_pcm);
  return hipGetLastError();
}

hipError_t launch_stream_scatter_g711(const uint8_t* d_tick, int32_t T, int64_t W, int64_t wpos, int32_t nch, int32_t law,
                                      int16_t* d_ring, hipStream_t stream) {
  if (!d_tick || !d_ring || T <= 0 || T > W || wpos < 0 || wpos >= W || nch <= 0 || !g711_law_ok(law))
    return hipErrorInvalidValue;
  if (law == kG711Alaw)
    hipLaunchKernelGGL(stream_scatter_g711_kernel<kG711Alaw>, dim3(1024), dim3(kBlock), 0, stream, d_tick, T, W, wpos, nch,
                       d_ring);
  else
    hipLaunchKernelGGL(stream_scatter_g711_kernel<kG711Ulaw>, dim3(1024), dim3(kBlock), 0, stream, d_tick, T, W, wpos, nch,
                       d_ring);
  return hipGetLastError();
}

}  // namespace tfp
