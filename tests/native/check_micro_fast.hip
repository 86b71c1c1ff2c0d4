// check_micro_fast.hip — the fast exact finish (asterisk-tiresias_amd/csrc/tfp_math.hpp
// micro_of_coef_fast) evaluated on gfx950 against the same function evaluated on the host, value and
// undecided flag, and (the slow path substituted where undecided) against the host's glibc
// micro_of_db(10.0 * log10(fabs((double)c))), over the bit patterns of the host check's sampled run:
// a strided walk of all 2^32 patterns plus micro_fast_subset.hpp's list. The table is staged in LDS
// as the throughput kernel stages it. Exit status 0 iff there are no mismatches.
// usage: check_micro_fast <stride> [list-file]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../asterisk-tiresias_amd/csrc/tfp_math.hpp"
#include "micro_fast_subset.hpp"

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return 2;                                                                \
    }                                                                          \
  } while (0)

// out[i] = the helper's micro-units, und[i] = its undecided flag, slow[i] = the slow path's value
__global__ void check_kernel(const uint32_t* __restrict__ bits, int64_t n, int32_t* __restrict__ out,
                             uint8_t* __restrict__ und, int32_t* __restrict__ slow) {
  __shared__ tfp::FinEntry FT[128];
  if (threadIdx.x < 128) FT[threadIdx.x] = tfp::fin_table()[threadIdx.x];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float c = tfp::u2f(bits[i]);
    bool u;
    out[i] = tfp::micro_of_coef_fast(c, &u, FT, tfp::kFinThr);
    und[i] = u;
    slow[i] = tfp::micro_of_db(tfp::db_of_coef(c));
  }
}

int main(int argc, char** argv) {
  const uint64_t stride = argc > 1 ? strtoull(argv[1], 0, 10) : 9973;
  const char* list = argc > 2 ? argv[2] : nullptr;
  if (stride < 64) return 2;  // (a sampled run: at most 2^26 patterns)
  std::vector<uint32_t> bits;
  for (uint64_t u = 0; u <= 0xffffffffull; u += stride) bits.push_back((uint32_t)u);
  const std::vector<uint32_t> extra = micro_fast_extras(list);
  if (extra.empty()) return 2;
  bits.insert(bits.end(), extra.begin(), extra.end());
  const int64_t n = (int64_t)bits.size();

  uint32_t* d_bits;
  int32_t *d_out, *d_slow;
  uint8_t* d_und;
  CK(hipMalloc(&d_bits, n * sizeof(uint32_t)));
  CK(hipMalloc(&d_out, n * sizeof(int32_t)));
  CK(hipMalloc(&d_slow, n * sizeof(int32_t)));
  CK(hipMalloc(&d_und, n));
  CK(hipMemcpy(d_bits, bits.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(check_kernel, dim3(grid), dim3(256), 0, 0, d_bits, n, d_out, d_und, d_slow);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<int32_t> out(n), slow(n);
  std::vector<uint8_t> und(n);
  CK(hipMemcpy(out.data(), d_out, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(slow.data(), d_slow, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(und.data(), d_und, n, hipMemcpyDeviceToHost));

  uint64_t bad_host = 0, bad_glibc = 0, nund = 0;
  for (int64_t i = 0; i < n; i++) {
    const float c = tfp::u2f(bits[i]);
    bool hu;
    const int32_t hv = tfp::micro_of_coef_fast(c, &hu);
    const int32_t want = tfp::micro_of_db(10.0 * log10(fabs((double)c)));
    const bool b0 = hu != (und[i] != 0) || (!hu && hv != out[i]);
    const bool b1 = (und[i] ? slow[i] : out[i]) != want;
    if ((b0 || b1) && bad_host + bad_glibc < 8)
      printf("  c bits 0x%08x: gpu %d und %d slow %d | host %d und %d | glibc %d\n", bits[i], out[i], und[i], slow[i], hv,
             (int)hu, want);
    bad_host += b0;
    bad_glibc += b1;
    nund += und[i];
  }
  printf("checked %ld patterns (stride %lu + %zu listed): gpu != host on %lu, gpu != glibc on %lu, undecided %lu\n", (long)n,
         (unsigned long)stride, extra.size(), (unsigned long)bad_host, (unsigned long)bad_glibc, (unsigned long)nund);
  (void)hipFree(d_bits);
  (void)hipFree(d_out);
  (void)hipFree(d_slow);
  (void)hipFree(d_und);
  const bool ok = bad_host == 0 && bad_glibc == 0;
  printf("%s\n", ok ? "OK" : "FAIL");
  return ok ? 0 : 1;
}
