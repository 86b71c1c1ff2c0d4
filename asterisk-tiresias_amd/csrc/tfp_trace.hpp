// tfp_trace.hpp — diagonal trace: a clip laid on a recording at a given start frame, verified along
// that one diagonal over the whole recording with aligned search's per-frame predicate
// (fp_handler.c:287-351, align_box of tfp_align_dev.hpp): the hits, the segments they fall into at
// a given max_gap, and the best segment (tfp_occur.hpp has the definitions and the monoid).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tfp_align.hpp"
#include "tfp_occur.hpp"

namespace tfp {

constexpr int32_t kTraceWaves = 4;  // requests per 256-thread block, one 64-lane wave each

// One request: an AlignPair (the clip's rows [row0, row0 + N) of the staging arrays, the
// recording's boxes [f0, f0 + F)) plus the recording frame s at which clip frame 0 lies (any int32).
struct TraceReq {
  int64_t row0;
  int64_t f0;
  int32_t N;
  int32_t F;
  int32_t s;
  int32_t pad;
};

// out[i] = the trace of request i, i < nreq, at max_gap >= 0. coefs2: some box may carry a max2
// condition (flags & 2), so the max2 rows are read.
hipError_t launch_trace(const TraceReq* d_reqs, int32_t nreq, int32_t max_gap, const FrameBox* boxes,
                        const int32_t* st_m1, const int32_t* st_m2, bool coefs2, TraceOut* d_out, hipStream_t s);

}  // namespace tfp
