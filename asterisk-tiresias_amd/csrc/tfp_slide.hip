// tfp_slide.hip — sliding search (tfp_slide.hpp): the scoped ranked rows (fp_handler.c:367-374) of
// every window of a recording, the vote moved from one window to the next instead of being rebuilt.
//
// slide_keys_kernel: each frame's key slot, once per recording. slide_vote_kernel: the geometry of
// scope_vote_kernel with a run of windows in a query's place (one block per run and 1,024-column
// chunk, 4 columns per thread, their scores in registers across the run). The first window of a run
// is scored from an LDS histogram of its slots; a later window subtracts one bitset word per leaving
// frame and adds one per entering frame, the slots staged in LDS kSlideTile at a time. A slot of -1
// (an ignored frame) votes for nothing on either side. With hop >= window every window is scored
// from its histogram. Per window the K selection rounds write a partial list for launch_rank_merge.
// slide_gather_kernel: the windows' frame values end to end, for the general form.
#include <hip/hip_runtime.h>

#include "tfp_slide.hpp"

namespace tfp {

namespace {

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long key) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o > key ? o : key;
  }
  return key;
}

__device__ __forceinline__ bool in_scope(int32_t qs, int32_t cs) { return qs == kScopeAny || cs == qs; }

__global__ __launch_bounds__(256) void slide_keys_kernel(const double* __restrict__ q, int64_t nf, SearchConsts sc,
                                                         int16_t* __restrict__ slots, int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nf) return;
  int32_t k = 0;
  int slot = -1;
  if (frame_key(q, i, sc, k)) {
    const int64_t idx = (int64_t)k + kKeyOffset;
    if (idx < 0 || idx >= kKeyRange) *bad = 1;  // (every writer stores 1)
    else slot = (int)idx;
  }
  slots[i] = (int16_t)slot;
}

__global__ __launch_bounds__(256) void slide_vote_kernel(const int16_t* __restrict__ slots,
                                                         const SlideRun* __restrict__ runs, int32_t window, int32_t hop,
                                                         const uint32_t* __restrict__ bits, int32_t C,
                                                         const int32_t* __restrict__ tiekey,
                                                         const int32_t* __restrict__ table, int32_t K,
                                                         unsigned long long* __restrict__ part) {
  static_assert(4 * 256 == kRankVoteCols, "4 columns per thread");
  static_assert(kSlideTile == 256, "one staged frame per thread");
  __shared__ int32_t hist[kKeyRange];  // frames of the window per key
  __shared__ int32_t kcnt[kKeyRange];  // ... of used key kc
  __shared__ int16_t kkey[kKeyRange];  // kc -> key index (row of bits), ascending
  __shared__ int16_t lv[kSlideTile];   // slots of the frames leaving
  __shared__ int16_t en[kSlideTile];   // ... entering
  __shared__ int32_t s_ku;
  __shared__ unsigned long long wmax[2][4];
  const SlideRun run = runs[blockIdx.y];
  const int blk = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // this thread's columns in scope (bit j: column c4 + j), from one 16-byte load of the table
  // (scope_table_cols(C) entries, so the load of a thread with c4 < C stays inside it)
  const int c4 = 4 * (blk * 256 + threadIdx.x);
  uint32_t in = 0;
  int32_t tk[4] = {0, 0, 0, 0};
  if (c4 < C) {
    const int4 s4 = *reinterpret_cast<const int4*>(table + c4);
    in = (in_scope(run.scope, s4.x) ? 1u : 0u) | (in_scope(run.scope, s4.y) ? 2u : 0u) |
         (in_scope(run.scope, s4.z) ? 4u : 0u) | (in_scope(run.scope, s4.w) ? 8u : 0u);
#pragma unroll
    for (int j = 1; j < 4; j++)
      if (c4 + j >= C) in &= ~(1u << j);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if ((in >> j) & 1u) tk[j] = tiekey[c4 + j];
  }
  const int W = key_bits_words(C);
  const uint32_t* col = bits + (c4 >> 5);  // (read only with in != 0, which implies c4 < C)
  const int sh = c4 & 31;
  int32_t score[4] = {0, 0, 0, 0};
  int rr = 0;  // selection rounds so far: wmax alternates over the whole run
  for (int w = 0; w < run.n; w++) {
    const int64_t a = run.f0 + (int64_t)w * hop;  // the window is the frames [a, a + window)
    if (w == 0 || hop >= window) {
      // from nothing, as rank_vote_kernel scores a query
      for (int i = threadIdx.x; i < kKeyRange; i += 256) hist[i] = 0;
      __syncthreads();
      for (int64_t base = threadIdx.x & ~63; base < window; base += 256) {
        const int64_t i = base + lane;
        const int slot = i < window ? (int)slots[a + i] : -1;
        unsigned long long todo = __ballot(slot >= 0);
        while (todo) {  // one LDS add per distinct key among the wave's 64 frames
          const int lead = __builtin_ctzll(todo);
          const int ls = __shfl(slot, lead, 64);
          const unsigned long long same = __ballot(slot == ls);
          if (lane == lead) atomicAdd(&hist[ls], (int)__popcll(same));
          todo &= ~same;
        }
      }
      __syncthreads();
      if (wv == 0) {  // used keys compacted in ascending order by one wave: 16 ballots
        int ku = 0;
        for (int base = 0; base < kKeyRange; base += 64) {
          const int32_t n = hist[base + lane];
          const unsigned long long used = __ballot(n != 0);
          if (n != 0) {
            const int kc = ku + (int)__popcll(used & ((1ull << lane) - 1ull));
            kkey[kc] = (int16_t)(base + lane);
            kcnt[kc] = n;
          }
          ku += (int)__popcll(used);
        }
        if (lane == 0) s_ku = ku;
      }
      __syncthreads();
      const int ku = s_ku;
#pragma unroll
      for (int j = 0; j < 4; j++) score[j] = 0;
      if (in) {
        int kc = 0;
        for (; kc + 4 <= ku; kc += 4) {  // 4 independent bitset loads in flight
          uint32_t v[4];
#pragma unroll
          for (int u = 0; u < 4; u++) v[u] = col[(int64_t)kkey[kc + u] * W] >> sh;
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int32_t n = kcnt[kc + u];
#pragma unroll
            for (int j = 0; j < 4; j++) score[j] += ((v[u] >> j) & 1u) ? n : 0;
          }
        }
        for (; kc < ku; kc++) {
          const uint32_t x = col[(int64_t)kkey[kc] * W] >> sh;
          const int32_t n = kcnt[kc];
#pragma unroll
          for (int j = 0; j < 4; j++) score[j] += ((x >> j) & 1u) ? n : 0;
        }
      }
    } else {
      // from the previous window [a - hop, a - hop + window): the frames [a - hop, a) left, the
      // frames [a - hop + window, a + window) entered (hop < window: the two do not meet)
      const int64_t lv0 = a - hop, en0 = a - hop + window;
      for (int t0 = 0; t0 < hop; t0 += kSlideTile) {
        const int n = hop - t0 < kSlideTile ? hop - t0 : kSlideTile;
        __syncthreads();  // the previous tile is read
        if ((int)threadIdx.x < n) {
          lv[threadIdx.x] = slots[lv0 + t0 + threadIdx.x];
          en[threadIdx.x] = slots[en0 + t0 + threadIdx.x];
        }
        __syncthreads();
        if (in) {
          int i = 0;
          for (; i + 2 <= n; i += 2) {  // 4 independent bitset loads in flight (a slot is block-uniform)
            const int sl[4] = {lv[i], en[i], lv[i + 1], en[i + 1]};
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = sl[u] >= 0 ? col[(int64_t)sl[u] * W] >> sh : 0u;
#pragma unroll
            for (int j = 0; j < 4; j++)
              score[j] += (int32_t)((v[1] >> j) & 1u) + (int32_t)((v[3] >> j) & 1u) - (int32_t)((v[0] >> j) & 1u) -
                          (int32_t)((v[2] >> j) & 1u);
          }
          if (i < n) {
            const int sa = lv[i], sb = en[i];
            const uint32_t va = sa >= 0 ? col[(int64_t)sa * W] >> sh : 0u;
            const uint32_t vb = sb >= 0 ? col[(int64_t)sb * W] >> sh : 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) score[j] += (int32_t)((vb >> j) & 1u) - (int32_t)((va >> j) & 1u);
          }
        }
      }
    }
    unsigned long long mine[4];
#pragma unroll
    for (int j = 0; j < 4; j++)
      mine[j] = (((in >> j) & 1u) && score[j] > 0) ? ((unsigned long long)(uint32_t)score[j] << 32) | (uint32_t)tk[j] : 0ull;
    unsigned long long* out = part + ((int64_t)(run.w0 + w) * gridDim.x + blk) * K;
    unsigned long long prev = ~0ull;
    for (int r = 0; r < K; r++, rr++) {
      unsigned long long key = 0ull;
#pragma unroll
      for (int j = 0; j < 4; j++) key = (mine[j] < prev && mine[j] > key) ? mine[j] : key;
      key = wave_max_u64(key);
      if (lane == 0) wmax[rr & 1][wv] = key;
      __syncthreads();  // (wmax[rr & 1] is next written two rounds on, after the barrier of the round between)
      key = wmax[rr & 1][0];
#pragma unroll
      for (int i = 1; i < 4; i++) key = wmax[rr & 1][i] > key ? wmax[rr & 1][i] : key;
      if (threadIdx.x == 0) out[r] = key;
      prev = key;  // (0: no key is below it, the remaining rounds give 0)
    }
  }
}

__global__ __launch_bounds__(256) void slide_gather_kernel(const double* __restrict__ q, const int64_t* __restrict__ wsrc,
                                                           int64_t total, int32_t window, double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t w = i / window;
    const int64_t f = wsrc[w] + (i - w * window);
    out[2 * i] = q[2 * f];
    out[2 * i + 1] = q[2 * f + 1];
  }
}

}  // namespace

hipError_t launch_slide_keys(const double* d_q, int64_t nf, SearchConsts sc, int16_t* d_slots, int32_t* d_bad,
                             hipStream_t s) {
  if (nf <= 0) return hipSuccess;
  if (nf > (int64_t)INT32_MAX * 256) return hipErrorInvalidValue;
  hipLaunchKernelGGL(slide_keys_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, d_q, nf, sc, d_slots, d_bad);
  return hipGetLastError();
}

hipError_t launch_slide_vote(const int16_t* d_slots, const SlideRun* d_runs, int32_t nruns, int32_t nwin, int32_t window,
                             int32_t hop, const uint32_t* d_bits, int32_t C, const int32_t* d_tiekey, const int32_t* d_table,
                             int32_t K, unsigned long long* d_part, unsigned long long* d_keys, hipStream_t s) {
  if (nruns <= 0 || nwin <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || C <= 0 || nruns > 65535 || window < 1 || hop < 1) return hipErrorInvalidValue;
  const int32_t nb = rank_vote_blocks(C);
  hipLaunchKernelGGL(slide_vote_kernel, dim3(nb, nruns), dim3(256), 0, s, d_slots, d_runs, window, hop, d_bits, C, d_tiekey,
                     d_table, K, d_part);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? err : launch_rank_merge(d_part, nwin, nb * K, K, d_keys, s);
}

hipError_t launch_slide_gather(const double* d_q, const int64_t* d_wsrc, int32_t nwin, int32_t window, double* d_out,
                               hipStream_t s) {
  const int64_t total = (int64_t)nwin * window;
  if (total <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(slide_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_q, d_wsrc, total, window, d_out);
  return hipGetLastError();
}

}  // namespace tfp
