// tfp_resample_any.hip — a mixed batch onto the int16 path at the index's rate in one launch: clips of any
// rate, channel count (1 to 32) and sample kind (int16, int32 Q31, mu-law, A-law), each converted by the
// existing routines of its own class (tfp_resample_any.hpp).
//
// One workgroup of 256 threads per tile of kRsTile consecutive outputs of one clip, on the tile tables
// resample_tiles gives over the call's output offsets, as the four single-class kernels. The workgroup
// reads its clip's descriptor (48 bytes, one address for the whole workgroup: scalar loads), from it the
// clip's plan and the start of the plan's table in the call's concatenated taps, and runs any_tile: a
// switch on the clip's form, which is the same for every thread of the workgroup, so no wave diverges on
// it. The work behind each case is the statement list of the single-class kernel of that form.
//
// LDS. One untyped dynamic buffer, declared int64 for the widest element's alignment and read as int16
// samples, int32 samples or sums, or int64 sums by the clip's form. A launch has one size: the largest span
// any clip of the call with output may stage, 60 KiB at most (the single-class kernels' budget: two
// workgroups per CU with 40 KiB to spare, the reasoning at the top of tfp_resample_mix.hip). A call of
// telephone-rate clips alone asks for a few KiB. A workgroup of a clip with a small span beside a clip
// with a large one holds the large size without using it: the price of one launch, and the reason a call
// that mixes a 192 kHz master into thousands of 8 kHz clips is better split by the caller. Unmeasured.
//
// Registers: the kernel's allocation is the largest of its cases', which every workgroup pays. The compiler
// reports 30 VGPRs and no scratch for gfx950, so the switch costs no residency: LDS limits a CU to two
// workgroups of a 60 KiB call long before registers do. The taps are read from global memory, as the other
// kernels read them; taps in LDS stay out of scope.
#include <hip/hip_runtime.h>

#include "tfp_resample_any.hpp"

namespace tfp {
namespace {

constexpr int kBlock = 256;
constexpr int64_t kLdsMax = 61440;  // 60 KiB: sizeof(int16_t) * kRsSpanMax = 4 * kRsMixSpanMax = 8 * kRsWideSpanMax
static_assert(2 * (int64_t)kRsSpanMax == kLdsMax && 4 * (int64_t)kRsMixSpanMax == kLdsMax && 8 * (int64_t)kRsWideSpanMax == kLdsMax,
              "every class stages within the same 60 KiB");

__global__ __launch_bounds__(kBlock) void resample_any_kernel(const uint8_t* __restrict__ data,
                                                              const AnyClipDev* __restrict__ clips,
                                                              const AnyPlanDev* __restrict__ plans,
                                                              const int16_t* __restrict__ taps_all,
                                                              const int32_t* __restrict__ toff,
                                                              const int32_t* __restrict__ tclip, int64_t lds_bytes,
                                                              int16_t* __restrict__ out) {
  extern __shared__ int64_t any_lds[];
  const int32_t c = tclip[blockIdx.x];
  const AnyClipDev d = clips[c];
  ResamplePlan P{1, 1, 0, 1};
  const int16_t* __restrict__ taps = taps_all;
  if (d.plan >= 0) {  // (uniform)
    const AnyPlanDev pd = plans[d.plan];
    P = pd.P;
    taps = taps_all + pd.taps_off;
  }
  any_tile(data, d, P, taps, (int64_t)((int32_t)blockIdx.x - toff[c]), any_lds, lds_bytes, out, (int32_t)threadIdx.x, kBlock);
}

}  // namespace

hipError_t launch_resample_any(const uint8_t* d_data, const AnyClipDev* d_clips, const AnyPlanDev* d_plans, const int16_t* d_taps,
                               const int32_t* d_toff, const int32_t* d_tclip, int32_t ntiles, int64_t lds_bytes, int16_t* d_out,
                               hipStream_t stream) {
  if (ntiles < 0 || lds_bytes < 0 || lds_bytes > kLdsMax) return hipErrorInvalidValue;
  if (ntiles == 0) return hipSuccess;
  if (!d_data || !d_clips || !d_plans || !d_toff || !d_tclip || !d_out) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(d_data) & 3) return hipErrorInvalidValue;
  hipLaunchKernelGGL(resample_any_kernel, dim3((unsigned)ntiles), dim3(kBlock), (size_t)lds_bytes, stream, d_data, d_clips,
                     d_plans, d_taps, d_toff, d_tclip, lds_bytes, d_out);
  return hipGetLastError();
}

}  // namespace tfp
