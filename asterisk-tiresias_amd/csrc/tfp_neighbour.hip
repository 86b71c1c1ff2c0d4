// tfp_neighbour.hip — catalog neighbours (tfp_neighbour.hpp): scoped search's vote form with the
// query frames read from the named clips' staged rows in place.
//
// neighbour_vote_kernel: scope_vote_kernel's geometry (one block per named clip and 1,024-column
// chunk, 4 columns per thread). The key histogram is counted from the clip's st_m1 range: a row's key
// and ignore test are frame_key's on the converted value, so nothing else decides a frame. The named
// clip's own column has key 0 like a column out of scope, in the main columns and the delta's alike.
// neighbour_boxes_kernel / neighbour_key_cols_kernel / neighbour_pairs_kernel: the boxes and pairs of
// launch_align from the rows and the selected keys, all on the device. neighbour_gather_kernel: the
// rows' frame values for the general form.
#include <hip/hip_runtime.h>

#include "tfp_neighbour.hpp"

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

__global__ __launch_bounds__(256) void neighbour_vote_kernel(const int32_t* __restrict__ m1,
                                                             const NeighbourClip* __restrict__ clips, SearchConsts sc,
                                                             const uint32_t* __restrict__ bits, int32_t C,
                                                             const int32_t* __restrict__ tiekey,
                                                             const int32_t* __restrict__ table, int32_t K,
                                                             unsigned long long* __restrict__ part, int32_t* __restrict__ bad) {
  static_assert(4 * 256 == kRankVoteCols, "4 columns per thread");
  __shared__ int32_t hist[kKeyRange];  // rows of this clip per key
  __shared__ int32_t kcnt[kKeyRange];  // ... of used key kc
  __shared__ int16_t kkey[kKeyRange];  // kc -> key index (row of bits), ascending
  __shared__ int32_t s_ku;
  __shared__ unsigned long long wmax[2][4];
  const int qi = blockIdx.y, blk = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const NeighbourClip nc = clips[qi];
  const int64_t f0 = nc.row0, f1 = nc.row0 + nc.nrows;
  // this thread's columns in scope (bit j: column c4 + j), from one 16-byte load of the table
  // (scope_table_cols(C) entries, so the load of a thread with c4 < C stays inside it); the clip's own
  // column is never among them
  const int c4 = 4 * (blk * 256 + threadIdx.x);
  uint32_t in = 0;
  if (c4 < C) {
    const int4 s4 = *reinterpret_cast<const int4*>(table + c4);
    in = (in_scope(nc.scope, s4.x) ? 1u : 0u) | (in_scope(nc.scope, s4.y) ? 2u : 0u) | (in_scope(nc.scope, s4.z) ? 4u : 0u) |
         (in_scope(nc.scope, s4.w) ? 8u : 0u);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (c4 + j >= C || c4 + j == nc.self_col) in &= ~(1u << j);
  }
  for (int i = threadIdx.x; i < kKeyRange; i += 256) hist[i] = 0;
  __syncthreads();
  bool out_of_range = false;
  for (int64_t base = f0 + (threadIdx.x & ~63); base < f1; base += 256) {
    const int64_t i = base + lane;
    int32_t k = 0;
    int slot = -1;  // key index of this row, -1 if ignored (or out of range)
    if (i < f1) {
      const double q[2] = {neighbour_frame_value(m1[i]), 0.0};
      if (frame_key(q, 0, sc, k)) {
        const int64_t idx = (int64_t)k + kKeyOffset;
        if (idx < 0 || idx >= kKeyRange) out_of_range = true;
        else slot = (int)idx;
      }
    }
    unsigned long long todo = __ballot(slot >= 0);
    while (todo) {  // one LDS add per distinct key among the wave's 64 rows
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

__global__ __launch_bounds__(256) void neighbour_boxes_kernel(const int32_t* __restrict__ m1, const int32_t* __restrict__ m2,
                                                              const NeighbourClip* __restrict__ clips, SearchConsts sc,
                                                              FrameBox* __restrict__ boxes) {
  const NeighbourClip nc = clips[blockIdx.y];
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nc.nrows; j += (int64_t)gridDim.x * 256)
    boxes[nc.box0 + j] = frame_box(neighbour_frame_value(m1[nc.row0 + j]), neighbour_frame_value(m2[nc.row0 + j]), sc);
}

__global__ __launch_bounds__(256) void neighbour_gather_kernel(const int32_t* __restrict__ m1, const int32_t* __restrict__ m2,
                                                               const NeighbourClip* __restrict__ clips,
                                                               double* __restrict__ q) {
  const NeighbourClip nc = clips[blockIdx.y];
  double2* dst = reinterpret_cast<double2*>(q) + nc.box0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nc.nrows; j += (int64_t)gridDim.x * 256)
    dst[j] = double2{neighbour_frame_value(m1[nc.row0 + j]), neighbour_frame_value(m2[nc.row0 + j])};
}

// live_key_cols_kernel's shape: a block whose clip has no row (its first key is 0: the keys descend)
// leaves at once; the clip's at most K tie keys sit in LDS, every lane reads the same one.
__global__ __launch_bounds__(256) void neighbour_key_cols_kernel(const unsigned long long* __restrict__ keys,
                                                                 const NeighbourClip* __restrict__ clips, int32_t K,
                                                                 const int32_t* __restrict__ tiekey,
                                                                 const int32_t* __restrict__ table,
                                                                 const NeighbourCol* __restrict__ rows, int32_t C,
                                                                 int32_t* __restrict__ cols) {
  __shared__ uint32_t want[kRankMax];
  __shared__ int32_t nwant;
  const int qi = blockIdx.y;
  const unsigned long long* kc = keys + (int64_t)qi * K;
  if (!kc[0]) return;  // (the whole block)
  if (threadIdx.x < (unsigned)K) want[threadIdx.x] = (uint32_t)kc[threadIdx.x];
  if (threadIdx.x == 0) {
    int32_t n = 1;
    while (n < K && kc[n]) n++;
    nwant = n;
  }
  __syncthreads();
  const int c4 = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (c4 >= C) return;
  const NeighbourClip nc = clips[qi];
  const int4 s4 = *reinterpret_cast<const int4*>(table + c4);  // (scope_table_cols(C) entries: inside the table)
  const int32_t cs[4] = {s4.x, s4.y, s4.z, s4.w};
  const int32_t n = nwant;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (c4 + j >= C || c4 + j == nc.self_col || !in_scope(nc.scope, cs[j])) continue;
    const uint32_t tk = (uint32_t)tiekey[c4 + j];
    for (int32_t r = 0; r < n; r++)
      if (want[r] == tk && rows[c4 + j].n > 0) cols[(int64_t)qi * K + r] = c4 + j;
  }
}

__global__ __launch_bounds__(256) void neighbour_pairs_kernel(const unsigned long long* __restrict__ keys,
                                                              const int32_t* __restrict__ cols,
                                                              const NeighbourCol* __restrict__ rows, int32_t ncols,
                                                              const NeighbourClip* __restrict__ clips, int32_t npairs,
                                                              int32_t K, AlignPair* __restrict__ pairs) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npairs) return;
  AlignPair p{0, 0, 0, 0};
  if (keys[i]) {
    const int32_t col = cols[i];
    if (col >= 0 && col < ncols) {
      const NeighbourCol r = rows[col];
      const NeighbourClip nc = clips[i / K];
      if (r.n > 0 && r.n <= INT32_MAX && nc.nrows > 0) p = AlignPair{r.off, nc.box0, (int32_t)r.n, nc.nrows};
    }
  }
  pairs[i] = p;
}

inline unsigned row_blocks(int64_t max_rows) {
  const int64_t g = (max_rows + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

}  // namespace

hipError_t launch_neighbour_vote(const int32_t* st_m1, const NeighbourClip* d_clips, int32_t nclips, SearchConsts sc,
                                 const uint32_t* d_bits, int32_t C, const int32_t* d_tiekey, const int32_t* d_table,
                                 int32_t K, unsigned long long* d_part, unsigned long long* d_keys, int32_t* d_bad,
                                 hipStream_t s) {
  if (nclips <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || C <= 0 || nclips > 65535) return hipErrorInvalidValue;
  const int32_t nb = rank_vote_blocks(C);
  hipLaunchKernelGGL(neighbour_vote_kernel, dim3(nb, nclips), dim3(256), 0, s, st_m1, d_clips, sc, d_bits, C, d_tiekey,
                     d_table, K, d_part, d_bad);
  const hipError_t err = hipGetLastError();
  return err != hipSuccess ? err : launch_rank_merge(d_part, nclips, nb * K, K, d_keys, s);
}

hipError_t launch_neighbour_boxes(const int32_t* st_m1, const int32_t* st_m2, const NeighbourClip* d_clips, int32_t nclips,
                                  int64_t max_rows, SearchConsts sc, FrameBox* d_boxes, hipStream_t s) {
  if (nclips <= 0 || max_rows <= 0) return hipSuccess;
  if (nclips > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(neighbour_boxes_kernel, dim3(row_blocks(max_rows), nclips), dim3(256), 0, s, st_m1, st_m2, d_clips, sc,
                     d_boxes);
  return hipGetLastError();
}

hipError_t launch_neighbour_key_cols(const unsigned long long* d_keys, const NeighbourClip* d_clips, int32_t nclips,
                                     int32_t K, const int32_t* d_tiekey, const int32_t* d_table, const NeighbourCol* d_cols_rows,
                                     int32_t C, int32_t* d_cols, hipStream_t s) {
  if (nclips <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || C <= 0 || nclips > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(neighbour_key_cols_kernel, dim3(rank_vote_blocks(C), nclips), dim3(256), 0, s, d_keys, d_clips, K,
                     d_tiekey, d_table, d_cols_rows, C, d_cols);
  return hipGetLastError();
}

hipError_t launch_neighbour_pairs(const unsigned long long* d_keys, const int32_t* d_cols, const NeighbourCol* d_cols_rows,
                                  int32_t C, const NeighbourClip* d_clips, int32_t nclips, int32_t K, AlignPair* d_pairs,
                                  hipStream_t s) {
  if (nclips <= 0) return hipSuccess;
  if (K < 1 || K > kRankMax || nclips > 65535) return hipErrorInvalidValue;
  const int32_t npairs = nclips * K;
  hipLaunchKernelGGL(neighbour_pairs_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, s, d_keys, d_cols,
                     d_cols_rows, C, d_clips, npairs, K, d_pairs);
  return hipGetLastError();
}

hipError_t launch_neighbour_gather(const int32_t* st_m1, const int32_t* st_m2, const NeighbourClip* d_clips, int32_t nclips,
                                   int64_t max_rows, double* d_q, hipStream_t s) {
  if (nclips <= 0 || max_rows <= 0) return hipSuccess;
  if (nclips > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(neighbour_gather_kernel, dim3(row_blocks(max_rows), nclips), dim3(256), 0, s, st_m1, st_m2, d_clips,
                     d_q);
  return hipGetLastError();
}

}  // namespace tfp
