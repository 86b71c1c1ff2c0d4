// tfp_trace_dev.hpp — the device code the diagonal trace (tfp_trace.hip) and the live trace
// (tfp_live_trace.hip) share: the join of a wave's 64 lane summaries in lane order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_occur.hpp"

namespace tfp {

__device__ __forceinline__ TraceSeg shfl_down_seg(const TraceSeg& t, int off) {
  TraceSeg r;
  r.hits = __shfl_down(t.hits, off, 64);
  r.first = __shfl_down(t.first, off, 64);
  r.last = __shfl_down(t.last, off, 64);
  r.segs = __shfl_down(t.segs, off, 64);
  r.lead_hits = __shfl_down(t.lead_hits, off, 64);
  r.lead_last = __shfl_down(t.lead_last, off, 64);
  r.trail_hits = __shfl_down(t.trail_hits, off, 64);
  r.trail_first = __shfl_down(t.trail_first, off, 64);
  r.best_hits = __shfl_down(t.best_hits, off, 64);
  r.best_first = __shfl_down(t.best_first, off, 64);
  r.best_last = __shfl_down(t.best_last, off, 64);
  return r;
}

// The summary of the wave's frames, lane l's frames before lane l + 1's, from the 64 lane summaries:
// a shuffle tree in which lane l takes lane l + off's summary as its right neighbour, off = 1, 2, .. 32.
// Every lane of the wave calls it; the result is lane 0's (the other lanes hold partial joins).
__device__ __forceinline__ TraceSeg trace_wave_join(TraceSeg t, int lane, int32_t max_gap) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const TraceSeg right = shfl_down_seg(t, off);  // lanes [lane + off, lane + 2 * off), where lane is a multiple of 2 * off
    if (!(lane & (2 * off - 1))) t = trace_join(t, right, max_gap);
  }
  return t;
}

}  // namespace tfp
