// tfp_scope.hip — context-scoped search (tfp_scope.hpp): ranked search's two selections
// (tfp_rank.hip's vote form, tfp_scan.hip's rank_final_kernel) with a per-query scope filter at the
// point a column's key is formed, so the K rows are the first K of fp_handler.c:367-374 over a
// table holding the scope's clips only (:308-314 with "and context = ...").
//
// scope_table_kernel: the per-column scope table from the per-clip scopes. scope_vote_kernel: the
// geometry of rank_vote_kernel (one block per query and 1,024-column chunk, 4 columns per thread);
// a thread reads its four columns' scopes as one 16-byte load and, with none in scope, issues no
// bitset load; a column out of scope has key 0 and is never selected. scope_final_kernel: the
// general form's K rounds over the touched clips in scope, then the scratch of every touched clip
// restored. The partial lists go through ranked search's merge (launch_rank_merge).
#include <hip/hip_runtime.h>

#include "tfp_scope.hpp"

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

__global__ __launch_bounds__(256) void scope_table_kernel(const int32_t* __restrict__ col_clip,
                                                          const int32_t* __restrict__ clip_scope, int32_t n,
                                                          int32_t* __restrict__ table) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int32_t clip = col_clip[c];
  table[c] = clip >= 0 ? clip_scope[clip] : kScopeNone;
}

__global__ __launch_bounds__(256) void scope_vote_kernel(const double* __restrict__ q, const int64_t* __restrict__ qoff,
                                                         const int32_t* __restrict__ qscope, SearchConsts sc,
                                                         const uint32_t* __restrict__ bits, int32_t C,
                                                         const int32_t* __restrict__ tiekey,
                                                         const int32_t* __restrict__ table, int32_t K,
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
  const int32_t qs = qscope[qi];
  // this thread's columns in scope (bit j: column c4 + j), from one 16-byte load of the table
  // (scope_table_cols(C) entries, so the load of a thread with c4 < C stays inside it)
  const int c4 = 4 * (blk * 256 + threadIdx.x);
  uint32_t in = 0;
  if (c4 < C) {
    const int4 s4 = *reinterpret_cast<const int4*>(table + c4);
    in = (in_scope(qs, s4.x) ? 1u : 0u) | (in_scope(qs, s4.y) ? 2u : 0u) | (in_scope(qs, s4.z) ? 4u : 0u) |
         (in_scope(qs, s4.w) ? 8u : 0u);
#pragma unroll
    for (int j = 1; j < 4; j++)
      if (c4 + j >= C) in &= ~(1u << j);
  }
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
  int32_t score[4] = {0, 0, 0, 0};
  if (in) {  // (in != 0 implies c4 < C)
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
  for (int j = 0; j < 4; j++)
    mine[j] = (((in >> j) & 1u) && score[j] > 0) ? ((unsigned long long)(uint32_t)score[j] << 32) | (uint32_t)tiekey[c4 + j]
                                                 : 0ull;
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

// rank_final_kernel with the scope filter in the K rounds, one block per query; the scratch of every
// touched clip, in scope or not, is restored: the next search of any form finds it zero.
__global__ __launch_bounds__(256) void scope_final_kernel(int32_t q_begin, const int32_t* __restrict__ qscope,
                                                          const int32_t* __restrict__ tiekey,
                                                          const int32_t* __restrict__ table, int32_t C,
                                                          int32_t* __restrict__ stamp, int32_t* __restrict__ score,
                                                          const int32_t* __restrict__ touched, int32_t* __restrict__ tcnt,
                                                          int32_t K, unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long wmax[2][4];
  const int wq = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int32_t* st = stamp + (int64_t)wq * C;
  int32_t* sc = score + (int64_t)wq * C;
  const int32_t* tl = touched + (int64_t)wq * C;
  const int32_t n = tcnt[wq];
  const int32_t qs = qscope[q_begin + wq];
  unsigned long long* out = keys + (int64_t)(q_begin + wq) * K;
  unsigned long long prev = ~0ull;
  for (int32_t r = 0; r < K; r++) {
    unsigned long long key = 0;
    if (prev)  // (0: the rows ran out; the remaining ones are 0)
      for (int32_t j = threadIdx.x; j < n; j += 256) {
        const int32_t c = tl[j];
        const unsigned long long k =
            in_scope(qs, table[c]) ? ((unsigned long long)(uint32_t)sc[c] << 32) | (uint32_t)tiekey[c] : 0ull;
        key = (k < prev && k > key) ? k : key;
      }
    key = wave_max_u64(key);
    if (lane == 0) wmax[r & 1][wv] = key;
    __syncthreads();  // (wmax[r & 1] is next written two rounds on, after the barrier of round r + 1)
    key = wmax[r & 1][0];
#pragma unroll
    for (int i = 1; i < 4; i++) key = wmax[r & 1][i] > key ? wmax[r & 1][i] : key;
    if (threadIdx.x == 0) out[r] = key;
    prev = key;
  }
  for (int32_t j = threadIdx.x; j < n; j += 256) {
    const int32_t c = tl[j];
    sc[c] = 0;
    st[c] = 0;
  }
  __syncthreads();  // every thread has read tcnt[wq]
  if (threadIdx.x == 0) tcnt[wq] = 0;
}

}  // namespace

hipError_t launch_scope_table(const int32_t* d_col_clip, const int32_t* d_clip_scope, int32_t C, int32_t* d_table,
                              hipStream_t s) {
  const int32_t n = scope_table_cols(C);
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(scope_table_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_col_clip, d_clip_scope, n, d_table);
  return hipGetLastError();
}

hipError_t launch_scope_vote(const double* d_q, const int64_t* d_qoff, const int32_t* d_qscope, int32_t nq, SearchConsts sc,
                             const uint32_t* d_bits, int32_t C, const int32_t* d_tiekey, const int32_t* d_table, int32_t K,
                             unsigned long long* d_part, unsigned long long* d_keys, int32_t* d_bad, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (K < 1 || K > kRankMaxInternal || C <= 0 || nq > 65535) return hipErrorInvalidValue;
  const int32_t nb = rank_vote_blocks(C);
  hipLaunchKernelGGL(scope_vote_kernel, dim3(nb, nq), dim3(256), 0, s, d_q, d_qoff, d_qscope, sc, d_bits, C, d_tiekey,
                     d_table, K, d_part, d_bad);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? err : launch_rank_merge(d_part, nq, nb * K, K, d_keys, s);
}

hipError_t launch_scope_final(int32_t q_begin, int32_t nq, const int32_t* d_qscope, const int32_t* d_tiekey,
                              const int32_t* d_table, int32_t C, int32_t* d_stamp, int32_t* d_score,
                              const int32_t* d_touched, int32_t* d_tcnt, int32_t K, unsigned long long* d_keys,
                              hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (K < 1 || K > kRankMaxInternal) return hipErrorInvalidValue;
  hipLaunchKernelGGL(scope_final_kernel, dim3(nq), dim3(256), 0, s, q_begin, d_qscope, d_tiekey, d_table, C, d_stamp,
                     d_score, d_touched, d_tcnt, K, d_keys);
  return hipGetLastError();
}

}  // namespace tfp
