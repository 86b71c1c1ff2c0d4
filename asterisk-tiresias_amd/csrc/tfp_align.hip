// tfp_align.hip — aligned search (tfp_align.hpp): per (query, candidate clip) pair the diagonal
// d = row - frame with the most hits of the per-frame SQL predicate (fp_handler.c:287-351), the
// smallest such d, and the first and last query frame that hit on it.
//
// align_band_kernel: one 256-thread block per (pair, band of 256 consecutive diagonals). Thread t owns
// diagonal d0 + t and walks the frames i that can meet a row of the clip on one of the band's
// diagonals, its count in a register: no histogram and no atomics. Frames are taken in tiles of
// 256: the tile's boxes go to LDS pre-clamped to int32 (L = max(L, INT32_MIN + 1), U = min(U,
// INT32_MAX), an empty box as L > U), so a NULL row (INT32_MIN) and a row outside [0, N) (staged as
// INT32_MIN) fail the compare on their own and a test is 2 (coefs = 1) or 4 int32 compares; the rows
// [i0 + d0, i0 + d0 + 255 + 256) go to LDS beside them, so lane t reads row[i + t], consecutive
// addresses. A frame's box is the same for the whole wave: each lane keeps one frame's box of the
// current 64 frames and the loop reads frame i's from lane i (v_readlane), which leaves the LDS the
// one row read per test. The block's best packed key (count << 32 | ~(d + F - 1): the greatest key
// is the greatest count and, among equal counts, the smallest d) goes to the pair's partial list.
//
// align_merge_kernel: one block per pair takes the greatest of the bands' keys and walks the winning
// diagonal once more for its first and last hitting frame (the band kernel's loop carries the count
// alone). It writes every pair's result, zeros for an empty pair or one with no hit.
#include <hip/hip_runtime.h>

#include "tfp_align.hpp"
#include "tfp_align_dev.hpp"

namespace tfp {

namespace {

constexpr int kRows = kAlignBand + kAlignTile;  // LDS rows per tile (the last one unused)
static_assert(kAlignBand == 256 && kAlignTile % 64 == 0, "one diagonal per thread, whole waves of boxes");

template <bool M2>
__global__ __launch_bounds__(256) void align_band_kernel(const AlignPair* __restrict__ pairs,
                                                         const FrameBox* __restrict__ boxes,
                                                         const int32_t* __restrict__ m1, const int32_t* __restrict__ m2,
                                                         int64_t max_bands, unsigned long long* __restrict__ part) {
  __shared__ int4 sbox[kAlignTile];
  __shared__ int32_t srow1[kRows];
  __shared__ int32_t srow2[M2 ? kRows : 1];
  __shared__ unsigned long long wbest[4];
  const AlignPair pr = pairs[blockIdx.y];
  const int64_t F = pr.F, N = pr.N, band = blockIdx.x;
  if (band >= align_bands(F, N)) return;  // (the whole block)
  const int t = threadIdx.x, lane = t & 63;
  const int64_t d0 = band * kAlignBand - (F - 1);  // this band's first diagonal
  // frames that meet a row in [0, N) on one of the diagonals d0 .. d0 + 255
  const int64_t i_lo = d0 + (kAlignBand - 1) < 0 ? -(d0 + (kAlignBand - 1)) : 0;
  const int64_t i_hi = N - d0 < F ? N - d0 : F;
  int32_t cnt = 0;
  for (int64_t i0 = i_lo; i0 < i_hi; i0 += kAlignTile) {
    const int tlen = (int)(i_hi - i0 < kAlignTile ? i_hi - i0 : kAlignTile);
    sbox[t] = t < tlen ? align_box<M2>(boxes[pr.f0 + i0 + t]) : make_int4(1, 0, INT32_MIN, INT32_MAX);
    for (int x = t; x < kRows - 1; x += 256) {
      const int64_t j = i0 + d0 + x;
      const bool in = j >= 0 && j < N;
      srow1[x] = in ? m1[pr.row0 + j] : INT32_MIN;
      if (M2) srow2[x] = in ? m2[pr.row0 + j] : INT32_MIN;
    }
    __syncthreads();
    for (int sub = 0; sub < tlen; sub += 64) {
      const int4 mine = sbox[sub + lane];  // frame i0 + sub + lane
      const int n = tlen - sub < 64 ? tlen - sub : 64;
      const int32_t* r1 = srow1 + sub + t;
      const int32_t* r2 = srow2 + (M2 ? sub + t : 0);
      // 8 frames at a time; the frames past tlen have empty boxes, their rows are staged
      for (int ii = 0; ii < n; ii += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int32_t L1 = __builtin_amdgcn_readlane(mine.x, ii + u), U1 = __builtin_amdgcn_readlane(mine.y, ii + u);
          const int32_t a = r1[ii + u];
          int hit = (a >= L1) & (a <= U1);
          if (M2) {
            const int32_t L2 = __builtin_amdgcn_readlane(mine.z, ii + u), U2 = __builtin_amdgcn_readlane(mine.w, ii + u);
            const int32_t b = r2[ii + u];
            hit &= (b >= L2) & (b <= U2);
          }
          cnt += hit;
        }
      }
    }
    __syncthreads();  // (the tile is read before the next one is staged)
  }
  // diagonals past N - 1 in the last band met no row: cnt = 0
  const uint32_t u = (uint32_t)(band * kAlignBand + t);  // d + F - 1 < 2^32
  unsigned long long key = cnt > 0 ? ((unsigned long long)(uint32_t)cnt << 32) | (0xffffffffu - u) : 0ull;
  key = align_wave_max(key);
  if (lane == 0) wbest[t >> 6] = key;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; w++) key = wbest[w] > key ? wbest[w] : key;
    part[(int64_t)blockIdx.y * max_bands + band] = key;
  }
}

template <bool M2>
__global__ __launch_bounds__(256) void align_merge_kernel(const AlignPair* __restrict__ pairs,
                                                          const FrameBox* __restrict__ boxes,
                                                          const int32_t* __restrict__ m1, const int32_t* __restrict__ m2,
                                                          int64_t max_bands, const unsigned long long* __restrict__ part,
                                                          AlignOut* __restrict__ out) {
  const AlignPair pr = pairs[blockIdx.x];
  align_merge_pair<M2>(pr, align_bands(pr.F, pr.N), part + (int64_t)blockIdx.x * max_bands, boxes, m1, m2,
                       out + blockIdx.x);
}

template <bool M2>
void launch(const AlignPair* d_pairs, int32_t npairs, int64_t max_bands, const FrameBox* boxes, const int32_t* st_m1,
            const int32_t* st_m2, unsigned long long* d_part, AlignOut* d_out, hipStream_t s) {
  if (max_bands > 0)
    hipLaunchKernelGGL(align_band_kernel<M2>, dim3((unsigned)max_bands, (unsigned)npairs), dim3(256), 0, s, d_pairs, boxes,
                       st_m1, st_m2, max_bands, d_part);
  hipLaunchKernelGGL(align_merge_kernel<M2>, dim3((unsigned)npairs), dim3(256), 0, s, d_pairs, boxes, st_m1, st_m2,
                     max_bands, d_part, d_out);
}

}  // namespace

hipError_t launch_align(const AlignPair* d_pairs, int32_t npairs, int64_t max_bands, const FrameBox* boxes,
                        const int32_t* st_m1, const int32_t* st_m2, bool coefs2, unsigned long long* d_part,
                        AlignOut* d_out, hipStream_t s) {
  if (npairs <= 0) return hipSuccess;
  // (bands * 256 threads must fit the grid's 32-bit x extent)
  if (npairs > kAlignMaxPairs || max_bands < 0 || max_bands >= (int64_t(1) << 24)) return hipErrorInvalidValue;
  if (coefs2) launch<true>(d_pairs, npairs, max_bands, boxes, st_m1, st_m2, d_part, d_out, s);
  else launch<false>(d_pairs, npairs, max_bands, boxes, st_m1, st_m2, d_part, d_out, s);
  return hipGetLastError();
}

}  // namespace tfp
