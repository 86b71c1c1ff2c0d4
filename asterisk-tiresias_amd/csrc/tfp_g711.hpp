// tfp_g711.hpp — G.711 codes in front of the int16 fingerprint path: the exact 16-bit expansion
// (one definition, host and device) and the launches of tfp_g711.hip.
//
// libsndfile, the backend of the reference's new_aubio_source (/root/reference/src/fp_handler.c:604,
// :633), hands aubio table[code] / 32768 for a mu-law or A-law WAV, and table[code] is the int16
// below (the expansion libsndfile, Asterisk and Python's audioop share). The int16 kernels compute
// s / 32768 from an int16 s, so fingerprints from codes equal fingerprints from the expanded int16
// bit for bit: there is nothing to tolerate, only an integer map to get right.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define TFP_G711_HD __host__ __device__ __forceinline__
#else
#define TFP_G711_HD static inline
#endif

namespace tfp {

constexpr int32_t kG711Ulaw = 0, kG711Alaw = 1;  // TFP_G711_ULAW, TFP_G711_ALAW

// mu-law: range +-32124; codes 0x7F and 0xFF both give 0.
TFP_G711_HD int32_t g711_ulaw(uint32_t code) {
  const uint32_t c = ~code & 0xFFu;
  const int32_t t = (int32_t)((((c & 0x0Fu) << 3) + 0x84u) << ((c & 0x70u) >> 4));
  return (c & 0x80u) ? 0x84 - t : t - 0x84;
}

// A-law: range +-32256, 256 distinct values. The three segment cases are selects.
TFP_G711_HD int32_t g711_alaw(uint32_t code) {
  const uint32_t c = (code ^ 0x55u) & 0xFFu;
  const uint32_t seg = (c & 0x70u) >> 4;
  const uint32_t base = ((c & 0x0Fu) << 4) + (seg == 0u ? 8u : 0x108u);
  const int32_t t = (int32_t)(base << (seg > 1u ? seg - 1u : 0u));
  return (c & 0x80u) ? t : -t;
}

template <int LAW>
TFP_G711_HD int32_t g711_expand(uint32_t code) {
  return LAW == kG711Alaw ? g711_alaw(code) : g711_ulaw(code);
}

inline bool g711_law_ok(int32_t law) { return law == kG711Ulaw || law == kG711Alaw; }

#if defined(__HIPCC__) || defined(__HIP__)
// codes[n] -> pcm[n] on the device (both 16-byte aligned: the engine's own buffers). One launch; a
// call with n = 0 launches nothing.
hipError_t launch_g711_expand(const uint8_t* d_codes, int64_t n, int32_t law, int16_t* d_pcm, hipStream_t stream);
// A stream tick of codes tick[nch][T] into ring[nch][2 W]: each sample expanded and written at p and
// p + W, p = (wpos + t) mod W (stream_scatter_kernel with the expansion fused in).
hipError_t launch_stream_scatter_g711(const uint8_t* d_tick, int32_t T, int64_t W, int64_t wpos, int32_t nch, int32_t law,
                                      int16_t* d_ring, hipStream_t stream);
#endif

}  // namespace tfp
