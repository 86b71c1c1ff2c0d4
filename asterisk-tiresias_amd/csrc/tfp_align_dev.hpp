// tfp_align_dev.hpp — the device code aligned search (tfp_align.hip) and sliding aligned search
// (tfp_slide_align.hip) share: a frame's box as int32 bounds, the 64-lane key maximum, and the merge
// of one pair's per-band keys into its tfp_alignment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_align.hpp"

namespace tfp {

// The frame's box as four int32 bounds (L1, U1, L2, U2) a stored value is compared with directly.
template <bool M2>
__device__ __forceinline__ int4 align_box(const FrameBox& b) {
  int4 r = make_int4(1, 0, INT32_MIN, INT32_MAX);  // no row hits
  if (!(b.flags & 1)) return r;
  const int64_t L1 = b.L1 > (int64_t)INT32_MIN + 1 ? b.L1 : (int64_t)INT32_MIN + 1;
  const int64_t U1 = b.U1 < (int64_t)INT32_MAX ? b.U1 : (int64_t)INT32_MAX;
  if (L1 > U1) return r;
  if (M2 && (b.flags & 2)) {
    const int64_t L2 = b.L2 > (int64_t)INT32_MIN + 1 ? b.L2 : (int64_t)INT32_MIN + 1;
    const int64_t U2 = b.U2 < (int64_t)INT32_MAX ? b.U2 : (int64_t)INT32_MAX;
    if (L2 > U2) return r;
    r.z = (int32_t)L2;
    r.w = (int32_t)U2;
  }
  r.x = (int32_t)L1;
  r.y = (int32_t)U1;
  return r;
}

__device__ __forceinline__ unsigned long long align_wave_max(unsigned long long key) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o > key ? o : key;
  }
  return key;
}

// One 256-thread block and one pair: the greatest of the pair's nb per-band keys p[0 .. nb)
// (count << 32 | ~(d + F - 1)), then the winning diagonal walked once for its first and last hitting
// frame. *out = zeros for an empty pair or one with no hit. Every thread of the block calls it.
template <bool M2>
__device__ __forceinline__ void align_merge_pair(const AlignPair pr, int64_t nb, const unsigned long long* __restrict__ p,
                                                 const FrameBox* __restrict__ boxes, const int32_t* __restrict__ m1,
                                                 const int32_t* __restrict__ m2, AlignOut* __restrict__ out) {
  __shared__ unsigned long long wbest[4];
  __shared__ int32_t wmin[4], wmax[4];
  const int64_t F = pr.F, N = pr.N;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  unsigned long long key = 0ull;
  for (int64_t b = t; b < nb; b += 256) key = p[b] > key ? p[b] : key;
  key = align_wave_max(key);
  if (lane == 0) wbest[wv] = key;
  __syncthreads();
  key = wbest[0];
  for (int w = 1; w < 4; w++) key = wbest[w] > key ? wbest[w] : key;
  if (!key) {  // an empty pair, or no row hits (the whole block)
    if (t == 0) *out = AlignOut{0, 0, 0, 0};
    return;
  }
  const int64_t d = (int64_t)(0xffffffffu - (uint32_t)key) - (F - 1);
  const int64_t lo = d < 0 ? -d : 0, hi = N - d < F ? N - d : F;
  int32_t mn = INT32_MAX, mx = -1;
  for (int64_t i = lo + t; i < hi; i += 256) {
    const int4 bx = align_box<M2>(boxes[pr.f0 + i]);
    const int32_t a = m1[pr.row0 + i + d];
    bool hit = a >= bx.x && a <= bx.y;
    if (M2) {
      const int32_t b = m2[pr.row0 + i + d];
      hit = hit && b >= bx.z && b <= bx.w;
    }
    if (hit) {
      mn = (int32_t)i < mn ? (int32_t)i : mn;
      mx = (int32_t)i > mx ? (int32_t)i : mx;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int32_t a = __shfl_xor(mn, off, 64), b = __shfl_xor(mx, off, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if (lane == 0) wmin[wv] = mn, wmax[wv] = mx;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; w++) {
      mn = wmin[w] < mn ? wmin[w] : mn;
      mx = wmax[w] > mx ? wmax[w] : mx;
    }
    *out = AlignOut{(int32_t)(key >> 32), (int32_t)d, mn, mx};
  }
}

}  // namespace tfp
