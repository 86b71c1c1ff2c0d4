// tfp_census.hip — match census (tfp_census.hpp): scoped search's two scoring passes
// (tfp_scope.hip's vote form, tfp_scan.hip's counts behind launch_scan_touched) with a histogram of
// the in-scope columns' counts in place of the K selection rounds.
//
// census_vote_kernel: the geometry of scope_vote_kernel (one block per query and 1,024-column
// chunk, 4 columns per thread, the four scopes as one 16-byte load). census_final_kernel: one block
// per query over the general form's touched clips, then their scratch restored. Both add into
// kCensusLdsBins LDS bins, one LDS add per distinct count among a wave's 64 lanes (counts
// concentrate, as keys do), and flush the non-zero bins with one global atomicAdd each; a count of
// kCensusLdsBins or more is added in global memory directly. Every add is an integer add, so the
// bins are exact whatever the order of lanes, waves and blocks.
#include <hip/hip_runtime.h>

#include "tfp_census.hpp"

namespace tfp {

namespace {

// (kScopeNone, a column without a clip, is in no scope: not in ANY either)
__device__ __forceinline__ bool in_scope(int32_t qs, int32_t cs) { return qs == kScopeAny ? cs != kScopeNone : cs == qs; }

// One column's count per lane (0: nothing to add) into the block's LDS bins, or into the query's
// row of nbins global bins where it is kCensusLdsBins or more. Called by all 64 lanes of a wave.
__device__ __forceinline__ void census_add(int32_t cnt, int lane, int32_t* bins, int32_t* __restrict__ row, int32_t nbins) {
  unsigned long long todo = __ballot(cnt > 0 && cnt < kCensusLdsBins);
  while (todo) {  // one LDS add per distinct count among the wave's 64 columns
    const int lead = __builtin_ctzll(todo);
    const int32_t lc = __shfl(cnt, lead, 64);
    const unsigned long long same = __ballot(cnt == lc);
    if (lane == lead) atomicAdd(&bins[lc], (int)__popcll(same));
    todo &= ~same;
  }
  if (cnt >= kCensusLdsBins && cnt < nbins) atomicAdd(&row[cnt], 1);  // (count <= frames < nbins)
}

// The block's non-zero LDS bins into the query's row, after a barrier behind the last census_add.
__device__ __forceinline__ void census_flush(const int32_t* bins, int32_t* __restrict__ row, int32_t nbins) {
  for (int i = threadIdx.x; i < kCensusLdsBins && i < nbins; i += 256) {
    const int32_t n = bins[i];
    if (n) atomicAdd(&row[i], n);
  }
}

__global__ __launch_bounds__(256) void census_vote_kernel(const double* __restrict__ q, const int64_t* __restrict__ qoff,
                                                          const int32_t* __restrict__ qscope, SearchConsts sc,
                                                          const uint32_t* __restrict__ bits, int32_t C,
                                                          const int32_t* __restrict__ table, int32_t nbins,
                                                          int32_t* __restrict__ out, int32_t* __restrict__ bad) {
  static_assert(4 * 256 == kRankVoteCols, "4 columns per thread");
  __shared__ int32_t hist[kKeyRange];  // frames of this query per key
  __shared__ int32_t kcnt[kKeyRange];  // ... of used key kc
  __shared__ int16_t kkey[kKeyRange];  // kc -> key index (row of bits), ascending
  __shared__ int32_t cbin[kCensusLdsBins];  // columns of this block per count
  __shared__ int32_t s_ku;
  const int qi = blockIdx.y, blk = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t f0 = qoff[qi], f1 = qoff[qi + 1];
  const int32_t qs = qscope[qi];
  // this thread's columns in scope (bit j: column c4 + j), from one 16-byte load of the table
  // (scope_table_cols(C) entries, so the load of a thread with c4 < C stays inside it); the
  // table's kScopeNone (padding, a column without a clip) is in no scope
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
  for (int i = threadIdx.x; i < kCensusLdsBins; i += 256) cbin[i] = 0;
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
  int32_t* row = out + (int64_t)qi * nbins;
#pragma unroll
  for (int j = 0; j < 4; j++) census_add(((in >> j) & 1u) ? score[j] : 0, lane, cbin, row, nbins);
  __syncthreads();
  census_flush(cbin, row, nbins);
}

// One block per query over the touched clips of launch_scan_touched; the scratch of every touched
// clip, in scope or not, is restored: the next search of any form finds it zero.
__global__ __launch_bounds__(256) void census_final_kernel(int32_t q_begin, const int32_t* __restrict__ qscope,
                                                           const int32_t* __restrict__ table, int32_t C,
                                                           int32_t* __restrict__ stamp, int32_t* __restrict__ score,
                                                           const int32_t* __restrict__ touched, int32_t* __restrict__ tcnt,
                                                           int32_t nbins, int32_t* __restrict__ out) {
  __shared__ int32_t cbin[kCensusLdsBins];
  const int wq = blockIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t* st = stamp + (int64_t)wq * C;
  int32_t* sc = score + (int64_t)wq * C;
  const int32_t* tl = touched + (int64_t)wq * C;
  const int32_t n = tcnt[wq];
  const int32_t qs = qscope[q_begin + wq];
  int32_t* row = out + (int64_t)(q_begin + wq) * nbins;
  for (int i = threadIdx.x; i < kCensusLdsBins; i += 256) cbin[i] = 0;
  __syncthreads();
  for (int32_t base = 0; base < n; base += 256) {  // (every lane of a wave makes the same trips)
    const int32_t j = base + threadIdx.x;
    int32_t cnt = 0;
    if (j < n) {
      const int32_t c = tl[j];
      cnt = in_scope(qs, table[c]) ? sc[c] : 0;
      sc[c] = 0;
      st[c] = 0;
    }
    census_add(cnt, lane, cbin, row, nbins);
  }
  __syncthreads();  // the bins are complete, and every thread has read tcnt[wq]
  census_flush(cbin, row, nbins);
  if (threadIdx.x == 0) tcnt[wq] = 0;
}

}  // namespace

hipError_t launch_census_vote(const double* d_q, const int64_t* d_qoff, const int32_t* d_qscope, int32_t nq, SearchConsts sc,
                              const uint32_t* d_bits, int32_t C, const int32_t* d_table, int32_t nbins, int32_t* d_hist,
                              int32_t* d_bad, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (nbins < 1 || C <= 0 || nq > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(census_vote_kernel, dim3(rank_vote_blocks(C), nq), dim3(256), 0, s, d_q, d_qoff, d_qscope, sc, d_bits, C,
                     d_table, nbins, d_hist, d_bad);
  return hipGetLastError();
}

hipError_t launch_census_final(int32_t q_begin, int32_t nq, const int32_t* d_qscope, const int32_t* d_table, int32_t C,
                               int32_t* d_stamp, int32_t* d_score, const int32_t* d_touched, int32_t* d_tcnt,
                               int32_t nbins, int32_t* d_hist, hipStream_t s) {
  if (nq <= 0) return hipSuccess;
  if (nbins < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(census_final_kernel, dim3(nq), dim3(256), 0, s, q_begin, d_qscope, d_table, C, d_stamp, d_score,
                     d_touched, d_tcnt, nbins, d_hist);
  return hipGetLastError();
}

}  // namespace tfp
