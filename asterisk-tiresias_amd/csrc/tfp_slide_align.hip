// tfp_slide_align.hip — sliding aligned search (tfp_slide_align.hpp): per (window, clip) entry of a
// run the diagonal with the most hits of the per-frame SQL predicate (fp_handler.c:287-351), the
// counts moved from one window of the run to the next instead of being rebuilt.
//
// slide_align_band_kernel: the cross of align_band_kernel and slide_vote_kernel. One 256-thread block
// per (run, band of 256 consecutive run-relative diagonals); thread t owns D = D0 + t (clip row minus
// frame counted from the run's first frame) and keeps that diagonal's count for the current window
// in a register: no histogram and no atomics. The run's first window is counted as align_band_kernel
// counts a query; each later window subtracts hit(x, x + D) for the hop frames that left and adds it
// for the hop that entered, the two sets staged side by side (boxes pre-clamped by align_box, rows
// outside [0, N) as INT32_MIN, so NULL rows and ignored frames need no branch) and read with the
// wave-uniform v_readlane box and consecutive row addresses of align_band_kernel. Frames that meet no
// row of the clip on the band's diagonals are not staged. At each window an entry needs, the block
// reduces the packed key count << 32 | ~(d + window - 1), d = D + s * hop being the window-relative
// diagonal, and writes it to that entry's per-band partial; windows no entry needs are stepped
// through without a reduction.
//
// slide_align_merge_kernel: align_merge_kernel's code (align_merge_pair) with the band count given
// per entry: an entry's partials are those of its run's bands.
#include <hip/hip_runtime.h>

#include "tfp_align_dev.hpp"
#include "tfp_slide_align.hpp"

namespace tfp {

namespace {

constexpr int kRows = kAlignBand + kAlignTile;  // LDS rows per tile (the last one unused)
static_assert(kAlignBand == 256 && kAlignTile == 256, "one diagonal and one staged frame per thread");

// The n <= kAlignTile frames from run frame x0 on: their boxes, and the rows the band's diagonals
// meet them on (row x of the tile is clip row x0 + D0 + x; lane t reads row[i + t] for frame i).
template <bool M2>
__device__ __forceinline__ void stage_tile(int4* sbox, int32_t* srow1, int32_t* srow2, const SlideAlignRun& run,
                                           const FrameBox* __restrict__ boxes, const int32_t* __restrict__ m1,
                                           const int32_t* __restrict__ m2, int64_t D0, int64_t x0, int n) {
  const int t = threadIdx.x;
  sbox[t] = t < n ? align_box<M2>(boxes[run.f0 + x0 + t]) : make_int4(1, 0, INT32_MIN, INT32_MAX);
  for (int x = t; x < n + kAlignBand - 1; x += 256) {
    const int64_t j = x0 + D0 + x;
    const bool in = j >= 0 && j < run.N;
    srow1[x] = in ? m1[run.row0 + j] : INT32_MIN;
    if (M2) srow2[x] = in ? m2[run.row0 + j] : INT32_MIN;
  }
}

// This thread's hits over the n staged frames. Frames past n have empty boxes, which no value
// passes, so the rows read for them (inside the tile's kRows, staged or not) do not count.
template <bool M2>
__device__ __forceinline__ int32_t count_tile(const int4* sbox, const int32_t* srow1, const int32_t* srow2, int n) {
  const int t = threadIdx.x, lane = t & 63;
  int32_t cnt = 0;
  for (int sub = 0; sub < n; sub += 64) {
    const int4 mine = sbox[sub + lane];  // frame sub + lane of the tile
    const int nn = n - sub < 64 ? n - sub : 64;
    const int32_t* r1 = srow1 + sub + t;
    const int32_t* r2 = srow2 + (M2 ? sub + t : 0);
    for (int ii = 0; ii < nn; ii += 8) {
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
  return cnt;
}

template <bool M2>
__global__ __launch_bounds__(256) void slide_align_band_kernel(const SlideAlignRun* __restrict__ runs,
                                                               const int32_t* __restrict__ steps, int32_t ent0,
                                                               int32_t window, int32_t hop,
                                                               const FrameBox* __restrict__ boxes,
                                                               const int32_t* __restrict__ m1,
                                                               const int32_t* __restrict__ m2, int64_t max_bands,
                                                               unsigned long long* __restrict__ part) {
  __shared__ int4 lbox[kAlignTile], ebox[kAlignTile];  // the frames leaving, entering (and the first window's)
  __shared__ int32_t lrow1[kRows], erow1[kRows];
  __shared__ int32_t lrow2[M2 ? kRows : 1], erow2[M2 ? kRows : 1];
  __shared__ unsigned long long wbest[2][4];
  const SlideAlignRun run = runs[blockIdx.y];
  const int64_t N = run.N, band = blockIdx.x;
  const int64_t L = slide_align_frames(run.nsteps, window, hop);
  if (band >= align_bands(L, N)) return;  // (the whole block)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t D0 = band * kAlignBand - (L - 1);  // this band's first diagonal
  // the run's frames that meet a row in [0, N) on one of the diagonals D0 .. D0 + 255
  const int64_t x_lo = D0 + (kAlignBand - 1) < 0 ? -(D0 + (kAlignBand - 1)) : 0;
  const int64_t x_hi = N - D0 < L ? N - D0 : L;
  int32_t cnt = 0;
  int rr = 0;  // reductions so far: wbest alternates over the whole run
  {
    // the first window, from nothing, as align_band_kernel counts a query
    const int64_t hi = x_hi < window ? x_hi : window;
    for (int64_t x0 = x_lo; x0 < hi; x0 += kAlignTile) {
      const int n = (int)(hi - x0 < kAlignTile ? hi - x0 : kAlignTile);
      stage_tile<M2>(ebox, erow1, erow2, run, boxes, m1, m2, D0, x0, n);
      __syncthreads();
      cnt += count_tile<M2>(ebox, erow1, erow2, n);
      __syncthreads();  // (the tile is read before the next one is staged)
    }
  }
  for (int s = 0; s < run.nsteps; s++) {
    if (s > 0) {
      // from window s - 1: the frames [lv0, lv0 + hop) left, [en0, en0 + hop) entered (hop < window:
      // the two do not meet), each cut to the frames this band can meet
      const int64_t lv0 = (int64_t)(s - 1) * hop, en0 = lv0 + window;
      for (int64_t t0 = 0; t0 < hop; t0 += kAlignTile) {
        const int64_t tl = hop - t0 < kAlignTile ? hop - t0 : kAlignTile;
        const int64_t la = lv0 + t0 > x_lo ? lv0 + t0 : x_lo, lb = lv0 + t0 + tl < x_hi ? lv0 + t0 + tl : x_hi;
        const int64_t ea = en0 + t0 > x_lo ? en0 + t0 : x_lo, eb = en0 + t0 + tl < x_hi ? en0 + t0 + tl : x_hi;
        const int nl = lb > la ? (int)(lb - la) : 0, ne = eb > ea ? (int)(eb - ea) : 0;
        if (!(nl | ne)) continue;  // (the whole block)
        if (nl) stage_tile<M2>(lbox, lrow1, lrow2, run, boxes, m1, m2, D0, la, nl);
        if (ne) stage_tile<M2>(ebox, erow1, erow2, run, boxes, m1, m2, D0, ea, ne);
        __syncthreads();
        if (ne) cnt += count_tile<M2>(ebox, erow1, erow2, ne);
        if (nl) cnt -= count_tile<M2>(lbox, lrow1, lrow2, nl);
        __syncthreads();
      }
    }
    const int32_t ent = steps[run.e0 + s];
    if (ent < 0) continue;  // no entry needs this window (the whole block)
    unsigned long long* dst = part + (int64_t)(ent - ent0) * max_bands + band;
    // the window's diagonals are d = D + s * hop in [-(window - 1), N - 1]: a band outside them holds no hit
    const int64_t d0 = D0 + (int64_t)s * hop;
    if (d0 + (kAlignBand - 1) < -(int64_t)(window - 1) || d0 > N - 1) {
      if (t == 0) *dst = 0ull;
      continue;
    }
    const uint32_t u = (uint32_t)(d0 + t + window - 1);  // d + window - 1 in [0, 2^31) wherever cnt > 0
    unsigned long long key = cnt > 0 ? ((unsigned long long)(uint32_t)cnt << 32) | (0xffffffffu - u) : 0ull;
    key = align_wave_max(key);
    if (lane == 0) wbest[rr & 1][wv] = key;
    __syncthreads();  // (wbest[rr & 1] is next written two reductions on, after the barrier of the one between)
    if (t == 0) {
      for (int w = 1; w < 4; w++) key = wbest[rr & 1][w] > key ? wbest[rr & 1][w] : key;
      *dst = key;
    }
    rr++;
  }
}

template <bool M2>
__global__ __launch_bounds__(256) void slide_align_merge_kernel(const AlignPair* __restrict__ pairs,
                                                                const int32_t* __restrict__ nb,
                                                                const FrameBox* __restrict__ boxes,
                                                                const int32_t* __restrict__ m1,
                                                                const int32_t* __restrict__ m2, int64_t max_bands,
                                                                const unsigned long long* __restrict__ part,
                                                                AlignOut* __restrict__ out) {
  align_merge_pair<M2>(pairs[blockIdx.x], nb[blockIdx.x], part + (int64_t)blockIdx.x * max_bands, boxes, m1, m2,
                       out + blockIdx.x);
}

template <bool M2>
void launch(const SlideAlignRun* d_runs, int32_t nruns, const int32_t* d_steps, int32_t ent0, int32_t nent,
            const AlignPair* d_pairs, const int32_t* d_nb, int64_t max_bands, int32_t window, int32_t hop,
            const FrameBox* boxes, const int32_t* st_m1, const int32_t* st_m2, unsigned long long* d_part, AlignOut* d_out,
            hipStream_t s) {
  hipLaunchKernelGGL(slide_align_band_kernel<M2>, dim3((unsigned)max_bands, (unsigned)nruns), dim3(256), 0, s, d_runs,
                     d_steps, ent0, window, hop, boxes, st_m1, st_m2, max_bands, d_part);
  hipLaunchKernelGGL(slide_align_merge_kernel<M2>, dim3((unsigned)nent), dim3(256), 0, s, d_pairs, d_nb, boxes, st_m1,
                     st_m2, max_bands, d_part, d_out);
}

}  // namespace

hipError_t launch_slide_align(const SlideAlignRun* d_runs, int32_t nruns, const int32_t* d_steps, int32_t ent0,
                              int32_t nent, const AlignPair* d_pairs, const int32_t* d_nb, int64_t max_bands,
                              int32_t window, int32_t hop, const FrameBox* boxes, const int32_t* st_m1,
                              const int32_t* st_m2, bool coefs2, unsigned long long* d_part, AlignOut* d_out,
                              hipStream_t s) {
  if (nruns <= 0 || nent <= 0) return hipSuccess;
  // (bands * 256 threads must fit the grid's 32-bit x extent)
  if (nruns > kSlideAlignMaxRuns || max_bands < 1 || max_bands >= (int64_t(1) << 24) || window < 2 || hop < 1 ||
      hop >= window)
    return hipErrorInvalidValue;
  if (coefs2)
    launch<true>(d_runs, nruns, d_steps, ent0, nent, d_pairs, d_nb, max_bands, window, hop, boxes, st_m1, st_m2, d_part,
                 d_out, s);
  else
    launch<false>(d_runs, nruns, d_steps, ent0, nent, d_pairs, d_nb, max_bands, window, hop, boxes, st_m1, st_m2, d_part,
                  d_out, s);
  return hipGetLastError();
}

}  // namespace tfp
