// tfp_rank.hip — ranked search, coefs = 1 with keys inside the vote range (tfp_rank.hpp): the
// first K rows of the reference's result query (fp_handler.c:367-374) per query, from the key
// bitsets the small vote reads.
//
// rank_vote_kernel: one block per (query, chunk of 1,024 columns). The block counts the query's
// frames per key into an LDS histogram (ballot-aggregated adds: keys concentrate on a few values),
// compacts the used keys, scores 4 columns per thread from one bitset word per used key, and
// selects its K greatest packed keys (count << 32 | tie key). rank_merge_kernel: one wave per
// query selects the K greatest of the blocks' partial lists.
//
// Selection is K rounds of "the greatest key strictly below the previous round's", from UINT64_MAX
// down; a round that finds none gives 0 and so do the rounds after it. Sound because live clips'
// tie keys are distinct (a key is taken once), and a column with no hit has key 0, never selected.
// Counts are int32: no bound on the frames per query.
#include <hip/hip_runtime.h>

#include "tfp_rank.hpp"

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

__global__ __launch_bounds__(256) void rank_vote_kernel(const double* __restrict__ q, const int64_t* __restrict__ qoff,
                                                        SearchConsts sc, const uint32_t* __restrict__ bits, int32_t C,
                                                        const int32_t* __restrict__ tiekey, int32_t K,
                                                        unsigned long long* __restrict__ part, int32_t* __restrict__ bad) {
  static_assert(4 * 256 == kRankVoteCols, "4 columns per thread");
  __shared__ int32_t hist[kKeyRange];  // frames of this query per key
  __shared__ int32_t kcnt[kKeyRange];  // ... of used key kc
  __shared__ int16_t kkey[kKeyRange];  // kc -> key index (row of bits), ascending
  __shared__ int32_t s_ku;
  __shared__ unsigned long long wmax[2][4];
  const int qi = blockIdx.y, blk = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t f0 = qoff[qi], f1 = qoff[qi + 1];
  for (int i = threadIdx.x; i < kKeyRange; i += 256) hist[i] = 0;
  __syncthreads();
  bool out_of_range = false;
  for (int64_t base = f0 + (threadIdx.x & ~63); base < f1; base += 256) {
    const int64_t i = base + lane;
    int32_t k = 0;
    int slot = -1;  // key index of this frame, -1 if ignored (or out of range)
    if (i < f1 && frame_key(q, i, sc, k)) {
      const int64_t idx = (int64_t)k + kKeyOffset;
      if (idx < 0 || idx >= kKeyRange) out_of_range = true;
      else slot = (int)idx;
    }
    unsigned long long todo = __ballot(slot >= 0);
    while (todo) {  // one LDS add per distinct key among the wave's 64 frames
      const int lead = __builtin_ctzll(todo);
      const int ls = __shfl(slot, lead, 64);
      const unsigned long long same = __ballot(slot == ls);
      if (lane == lead) atomicAdd(&hist[ls], (int)__popcll(same));
      todo &= ~same;
    }
  }
  if (out_of_range) *bad = 1;  // (every writer stores 1)
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
  const int c4 = 4 * (blk * 256 + threadIdx.x);  // first of this thread's 4 columns
  int32_t score[4] = {0, 0, 0, 0};
  if (c4 < C) {
    const int W = key_bits_words(C);
    const uint32_t* col = bits + (c4 >> 5);
    const int sh = c4 & 31;
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
  unsigned long long mine[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = c4 + j;
    mine[j] = (c < C && score[j] > 0) ? ((unsigned long long)(uint32_t)score[j] << 32) | (uint32_t)tiekey[c] : 0ull;
  }
  unsigned long long* out = part + ((int64_t)qi * gridDim.x + blk) * K;
  unsigned long long prev = ~0ull;
  for (int r = 0; r < K; r++) {
    unsigned long long key = 0ull;
#pragma unroll
    for (int j = 0; j < 4; j++) key = (mine[j] < prev && mine[j] > key) ? mine[j] : key;
    key = wave_max_u64(key);
    if (lane == 0) wmax[r & 1][wv] = key;
    __syncthreads();  // (wmax[r & 1] is next written two rounds on, after the barrier of round r + 1)
    key = wmax[r & 1][0];
#pragma unroll
    for (int i = 1; i < 4; i++) key = wmax[r & 1][i] > key ? wmax[r & 1][i] : key;
    if (threadIdx.x == 0) out[r] = key;
    prev = key;  // (0: no key is below it, the remaining rounds give 0)
  }
}

// One wave per query: the K greatest of its nblocks * K partial keys, descending.
__global__ __launch_bounds__(256) void rank_merge_kernel(const unsigned long long* __restrict__ part, int32_t nq,
                                                         int32_t nparts, int32_t K,
                                                         unsigned long long* __restrict__ out_keys) {
  const int wq = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wq >= nq) return;
  const unsigned long long* p = part + (int64_t)wq * nparts;
  unsigned long long prev = ~0ull;
  for (int r = 0; r < K; r++) {
    unsigned long long key = 0ull;
    if (prev)
      for (int32_t j = lane; j < nparts; j += 64) {
        const unsigned long long k = p[j];
        key = (k < prev && k > key) ? k : key;
      }
    key = wave_max_u64(key);
    if (lane == 0) out_keys[(int64_t)wq * K + r] = key;
    prev = key;
  }
}

}  // namespace

hipError_t launch_rank_vote(const double* d_q, const int64_t* d_qoff, int32_t nq, SearchConsts sc, const uint32_t* d_bits,
                            int32_t C, const int32_t* d_tiekey, int32_t K, unsigned long long* d_part,
                            unsigned long long* d_keys, int32_t* d_bad, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || C <= 0 || nq > 65535) return hipErrorInvalidValue;
  const int32_t nb = rank_vote_blocks(C);
  hipLaunchKernelGGL(rank_vote_kernel, dim3(nb, nq), dim3(256), 0, s, d_q, d_qoff, sc, d_bits, C, d_tiekey, K, d_part,
                     d_bad);
  hipLaunchKernelGGL(rank_merge_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, d_part, nq, nb * K, K, d_keys);
  return hipGetLastError();
}

// The merge alone, for partial lists of another vote form (tfp_scope.hip).
hipError_t launch_rank_merge(const unsigned long long* d_part, int32_t nq, int32_t nparts, int32_t K,
                             unsigned long long* d_keys, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(rank_merge_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, d_part, nq, nparts, K, d_keys);
  return hipGetLastError();
}

}  // namespace tfp
