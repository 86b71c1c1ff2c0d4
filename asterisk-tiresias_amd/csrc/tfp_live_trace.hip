// tfp_live_trace.hip — the carried traces of live calls (tfp_live_occurrences, tfp_live.hpp): per track
// (channel, clip, s) the summary of the per-frame predicate's hits (fp_handler.c:287-351) along the
// track's diagonal over the call's final frames is kept on the device and extended in place by the
// frames that became final since the last call.
//
// live_trace_kernel: one 64-lane wave per descriptor, kTraceWaves descriptors per 256-thread block, as
// trace_kernel. The wave folds the final frames [beg, end) in steps of 64: lane l takes frame
// beg + 64 i + l, builds its box from the kept frame values in place (frame_box, the routine
// prep_boxes_kernel and live_window_boxes_kernel share: no box buffer for the call), tests clip row
// x - s of the staging arrays (align_box) and holds a summary of at most one hit; the 64 summaries are
// joined in lane order (trace_wave_join, tfp_trace.hip's) and lane 0 appends the step's summary to the
// carried one. Consecutive lanes read consecutive frame values (16 B each) and consecutive rows. The
// carried summary is stored back, and the provisional tail frame's hit, if any, is joined into a copy
// for the output row only: a tail frame's values still change with the samples to come. Integer
// arithmetic after the box, no atomics, no LDS.
#include <hip/hip_runtime.h>

#include "tfp_align_dev.hpp"
#include "tfp_live.hpp"
#include "tfp_trace.hpp"
#include "tfp_trace_dev.hpp"

namespace tfp {

namespace {

// hit(x, x - s) for call frame x of channel d.ch; false outside the channel's frames or the clip's rows.
template <bool M2>
__device__ __forceinline__ bool live_trace_hit(const LiveTrace& d, int64_t x, const double* __restrict__ q, int64_t Fmax,
                                               const SearchConsts& sc, const int32_t* __restrict__ m1,
                                               const int32_t* __restrict__ m2) {
  const int64_t j = x - d.s;
  if (x < 0 || x >= Fmax || j < 0 || j >= d.N) return false;
  const double2 f = reinterpret_cast<const double2*>(q)[(int64_t)d.ch * Fmax + x];
  const FrameBox box = frame_box(f.x, f.y, sc);
  const int4 bx = align_box<M2>(box);
  const int32_t v1 = m1[d.row0 + j];
  bool hit = v1 >= bx.x && v1 <= bx.y;
  if (M2 && (box.flags & 2)) {  // (without the flag align_box leaves the max2 bounds open: no read)
    const int32_t v2 = m2[d.row0 + j];
    hit = hit && v2 >= bx.z && v2 <= bx.w;
  }
  return hit;
}

template <bool M2>
__global__ __launch_bounds__(64 * kTraceWaves) void live_trace_kernel(const LiveTrace* __restrict__ desc, int32_t ndesc,
                                                                      int32_t max_gap, const double* __restrict__ q,
                                                                      int64_t Fmax, SearchConsts sc,
                                                                      const int32_t* __restrict__ m1,
                                                                      const int32_t* __restrict__ m2,
                                                                      TraceSeg* __restrict__ segs,
                                                                      TraceOut* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kTraceWaves + (threadIdx.x >> 6);
  if (r >= ndesc) return;  // (the whole wave)
  const LiveTrace d = desc[r];
  TraceSeg acc = trace_none();
  if (!d.restart) acc = segs[d.slot];  // (the same address in every lane; lane 0's copy is the one carried)
  for (int64_t x0 = d.beg; x0 < d.end; x0 += 64) {
    const int64_t x = x0 + lane;
    TraceSeg t = trace_none();
    if (x < d.end && live_trace_hit<M2>(d, x, q, Fmax, sc, m1, m2)) trace_push(t, (int32_t)x, max_gap);
    t = trace_wave_join(t, lane, max_gap);
    if (lane == 0) acc = trace_join(acc, t, max_gap);
  }
  if (lane != 0) return;
  segs[d.slot] = acc;
  if (d.tail >= 0 && live_trace_hit<M2>(d, d.tail, q, Fmax, sc, m1, m2)) trace_push(acc, d.tail, max_gap);
  out[r] = trace_result(d.overlap, acc);
}

}  // namespace

hipError_t launch_live_trace(const LiveTrace* d_desc, int32_t ndesc, int32_t max_gap, const double* d_q, int64_t Fmax,
                             SearchConsts sc, const int32_t* st_m1, const int32_t* st_m2, TraceSeg* d_segs, TraceOut* d_out,
                             hipStream_t s) {
  if (ndesc <= 0) return hipSuccess;
  if (max_gap < 0 || Fmax <= 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((int64_t)ndesc + kTraceWaves - 1) / kTraceWaves)), block(64 * kTraceWaves);
  if (sc.coefs == 2)
    hipLaunchKernelGGL(live_trace_kernel<true>, grid, block, 0, s, d_desc, ndesc, max_gap, d_q, Fmax, sc, st_m1, st_m2, d_segs,
                       d_out);
  else
    hipLaunchKernelGGL(live_trace_kernel<false>, grid, block, 0, s, d_desc, ndesc, max_gap, d_q, Fmax, sc, st_m1, st_m2,
                       d_segs, d_out);
  return hipGetLastError();
}

}  // namespace tfp
