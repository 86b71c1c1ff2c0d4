// tfp_trace.hip — diagonal trace (tfp_trace.hpp): per request the hits of the per-frame SQL predicate
// (fp_handler.c:287-351) along one diagonal of a recording against a clip, their segments at max_gap
// and the best segment.
//
// trace_kernel: one 64-lane wave per request, four requests per 256-thread block. The diagonal's
// frames [lo, hi) are cut into 64 contiguous chunks of ceil((hi - lo) / 64) frames, lane l taking
// chunk l: it tests its frames in order (align_box, the row at x - s) and folds the hits into a
// TraceSeg with trace_push. The 64 summaries are then joined in lane order by a shuffle tree
// (trace_wave_join of tfp_trace_dev.hpp, shared with the live trace), trace_join
// fusing the left one's trailing segment with the right one's leading segment where the gap between
// them is at most max_gap, and lane 0 writes the result. No LDS, no atomics, no scratch: a request
// is one wave's registers, so requests of any length mix in one launch.
#include <hip/hip_runtime.h>

#include "tfp_align_dev.hpp"
#include "tfp_trace.hpp"
#include "tfp_trace_dev.hpp"

namespace tfp {

namespace {

template <bool M2>
__global__ __launch_bounds__(64 * kTraceWaves) void trace_kernel(const TraceReq* __restrict__ reqs, int32_t nreq,
                                                                 int32_t max_gap, const FrameBox* __restrict__ boxes,
                                                                 const int32_t* __restrict__ m1,
                                                                 const int32_t* __restrict__ m2,
                                                                 TraceOut* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kTraceWaves + (threadIdx.x >> 6);
  if (r >= nreq) return;  // (the whole wave)
  const TraceReq q = reqs[r];
  const int64_t s = q.s;
  int64_t lo, hi;
  trace_span(q.F, q.N, s, &lo, &hi);
  const int64_t n = hi > lo ? hi - lo : 0;
  const int64_t chunk = (n + 63) / 64;
  const int64_t a = lo + lane * chunk;
  const int64_t b = a + chunk < hi ? a + chunk : hi;
  TraceSeg t = trace_none();
  for (int64_t x = a; x < b; x++) {  // x in [lo, hi): box f0 + x of the recording's F, row x - s in [0, N)
    const int4 bx = align_box<M2>(boxes[q.f0 + x]);
    const int32_t v1 = m1[q.row0 + (x - s)];
    bool hit = v1 >= bx.x && v1 <= bx.y;
    if (M2) {
      const int32_t v2 = m2[q.row0 + (x - s)];
      hit = hit && v2 >= bx.z && v2 <= bx.w;
    }
    if (hit) trace_push(t, (int32_t)x, max_gap);
  }
  t = trace_wave_join(t, lane, max_gap);
  if (lane == 0) out[r] = trace_result((int32_t)n, t);
}

}  // namespace

hipError_t launch_trace(const TraceReq* d_reqs, int32_t nreq, int32_t max_gap, const FrameBox* boxes,
                        const int32_t* st_m1, const int32_t* st_m2, bool coefs2, TraceOut* d_out, hipStream_t s) {
  if (nreq <= 0) return hipSuccess;
  if (max_gap < 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((int64_t)nreq + kTraceWaves - 1) / kTraceWaves)), block(64 * kTraceWaves);
  if (coefs2)
    hipLaunchKernelGGL(trace_kernel<true>, grid, block, 0, s, d_reqs, nreq, max_gap, boxes, st_m1, st_m2, d_out);
  else
    hipLaunchKernelGGL(trace_kernel<false>, grid, block, 0, s, d_reqs, nreq, max_gap, boxes, st_m1, st_m2, d_out);
  return hipGetLastError();
}

}  // namespace tfp
