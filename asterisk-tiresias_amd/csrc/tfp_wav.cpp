// Audio ingest in front of create_audio_fingerprints: RIFF/WAVE -> the int16 samples the
// fingerprint path reads, with aubio_source semantics at the file's native rate
// (/root/reference/src/fp_handler.c:37 DEF_AUBIO_SAMPLERATE 0, :604 new_aubio_source, :633
// aubio_source_do). Host code only: the decoded PCM is what tfp_fingerprint_pcm /
// tfp_search_pcm_batch take.
//
// aubio turns a w-bit integer sample x into the fp32 value x / 2^(w-1) (8-bit data is unsigned
// and is offset by -128 first), and averages channels to mono. The engine reads int16 and
// computes x / 32768 exactly, so it accepts exactly the inputs whose aubio value is an int16
// over 32768:
//   * 16-bit mono: the stored samples;
//   * 8-bit mono: (u - 128) << 8, since (u - 128) / 128 == ((u - 128) << 8) / 32768.
// Multichannel (the mean of C channels), 24/32-bit and float data have aubio values between
// int16 steps, so tfp_wav_decode refuses them with TFP_E_FORMAT rather than silently rounding;
// tfp_wav_decode_f32 decodes them (and everything else) to the fp32 values aubio computes, for
// the fp32-sample entry points. Asterisk's own recordings (format_wav: PCM, mono, 16-bit, 8 kHz;
// application_handler.c:155) and the SLIN stream take the int16 path.
//
// G.711 (format tags 6 and 7, mono, 8-bit): aubio's value is table[code] / 32768 with table the
// 16-bit expansion of tfp_g711.hpp, an int16 over 32768 too. tfp_wav_decode_g711 hands out the
// codes as stored (one byte per sample, for the code entry points, which expand on the GPU) and
// tfp_g711_decode is the expansion on the host. tfp_wav_decode / _f32 keep refusing those tags.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tfp_g711.hpp"
#include "tfp_resample.hpp"
#include "tiresias_fp.h"

namespace {

thread_local std::string g_err;  // engine-less calls report through tfp_engine_last_error(NULL)

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

constexpr uint16_t kFormatPcm = 1;
constexpr uint16_t kFormatFloat = 3;
constexpr uint16_t kFormatAlaw = 6;
constexpr uint16_t kFormatUlaw = 7;
constexpr uint16_t kFormatExtensible = 0xFFFE;

int read_file(const char* path, std::vector<uint8_t>& buf) {
  if (!path) return fail(TFP_E_ARG, "bad argument");
  FILE* fp = std::fopen(path, "rb");
  if (!fp) return fail(TFP_E_NOENT, std::string("cannot open ") + path);
  uint8_t chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof chunk, fp)) > 0) buf.insert(buf.end(), chunk, chunk + got);
  const bool err = std::ferror(fp) != 0;
  std::fclose(fp);
  if (err) return fail(TFP_E_NOENT, std::string("read error on ") + path);
  if (buf.empty()) return fail(TFP_E_FORMAT, std::string("empty file ") + path);
  return TFP_OK;
}

struct WavFormat {
  uint16_t tag = 0, channels = 0, block_align = 0, bits = 0;
  uint32_t rate = 0;
};

// The fmt chunk in force at the data chunk, and the data bytes that are present.
struct WavData {
  WavFormat f;
  const uint8_t* data = nullptr;
  uint64_t size = 0;
};

// The chunk walk every decoder shares: RIFF/WAVE, the fmt chunk (EXTENSIBLE resolved to its
// sub-format's tag), then the first data chunk. What the format may be is the caller's business.
int find_data(const uint8_t* b, uint64_t n, WavData* out) {
  if (n < 12 || std::memcmp(b, "RIFF", 4) != 0 || std::memcmp(b + 8, "WAVE", 4) != 0)
    return fail(TFP_E_FORMAT, "not a RIFF/WAVE file");
  WavFormat& f = out->f;
  bool have_fmt = false;
  uint64_t pos = 12;
  while (pos + 8 <= n) {
    const uint8_t* id = b + pos;
    uint64_t size = le32(b + pos + 4);
    const uint64_t body = pos + 8;
    if (std::memcmp(id, "fmt ", 4) == 0) {
      if (size < 16 || body + 16 > n) return fail(TFP_E_FORMAT, "short fmt chunk");
      f.tag = le16(b + body);
      f.channels = le16(b + body + 2);
      f.rate = le32(b + body + 4);
      f.block_align = le16(b + body + 12);
      f.bits = le16(b + body + 14);
      if (f.tag == kFormatExtensible) {
        // WAVEFORMATEXTENSIBLE: cbSize(2) validBits(2) channelMask(4) SubFormat GUID(16); the
        // GUID's first two bytes are the plain format tag.
        if (size < 40 || body + 40 > n) return fail(TFP_E_FORMAT, "short WAVE_FORMAT_EXTENSIBLE chunk");
        f.tag = le16(b + body + 24);
      }
      have_fmt = true;
    } else if (std::memcmp(id, "data", 4) == 0) {
      if (!have_fmt) return fail(TFP_E_FORMAT, "data chunk before fmt chunk");
      // A writer that never patched the header (0 or 0xFFFFFFFF) or a truncated file: take the
      // whole samples that are present, as a streaming reader does.
      const uint64_t avail = n - body;
      if (size == 0 || size > avail) size = avail;
      out->data = b + body;
      out->size = size;
      return TFP_OK;
    }
    pos = body + size + (size & 1);  // RIFF chunks are padded to even sizes
  }
  return fail(TFP_E_FORMAT, have_fmt ? "no data chunk" : "no fmt chunk");
}

}  // namespace

// tfp_engine_last_error(NULL) (tfp_engine.cpp) reads this; not part of the C-ABI.
extern "C" __attribute__((visibility("hidden"))) const char* tfp_ingest_last_error() { return g_err.c_str(); }
// ... and the other engine-less ingest calls (tfp_resample.cpp) write it.
extern "C" __attribute__((visibility("hidden"))) void tfp_ingest_set_error(const char* msg) { g_err = msg; }

extern "C" int tfp_wav_decode(const void* bytes, int64_t nbytes, int16_t* pcm, int64_t cap, int64_t* nsamples,
                              int32_t* sample_rate) {
  if (!bytes || nbytes < 0 || !nsamples || cap < 0 || (cap > 0 && !pcm)) return fail(TFP_E_ARG, "bad argument");
  WavData w;
  if (const int rc = find_data(static_cast<const uint8_t*>(bytes), (uint64_t)nbytes, &w)) return rc;
  const WavFormat& f = w.f;
  if (f.tag != kFormatPcm) return fail(TFP_E_FORMAT, "format tag " + std::to_string(f.tag) + " is not integer PCM");
  if (f.channels != 1)
    return fail(TFP_E_FORMAT, std::to_string(f.channels) +
                                  " channels: aubio's channel mean is not an int16 sample (mono only)");
  if (f.bits != 16 && f.bits != 8)
    return fail(TFP_E_FORMAT, std::to_string(f.bits) + "-bit samples: only 8- and 16-bit PCM map exactly to int16");
  if (f.rate == 0 || f.rate > (uint32_t)INT32_MAX) return fail(TFP_E_FORMAT, "bad sample rate");
  const uint32_t width = f.bits / 8;
  if (f.block_align != width) return fail(TFP_E_FORMAT, "block align does not match mono " + std::to_string(f.bits) + "-bit");
  const int64_t ns = (int64_t)(w.size / width);
  *nsamples = ns;
  if (sample_rate) *sample_rate = (int32_t)f.rate;
  if (!pcm) return TFP_OK;  // size query
  if (cap < ns) return fail(TFP_E_CAPACITY, "pcm buffer holds " + std::to_string(cap) + " of " + std::to_string(ns) + " samples");
  const uint8_t* d = w.data;
  if (width == 2) {
    for (int64_t i = 0; i < ns; ++i) pcm[i] = (int16_t)le16(d + 2 * i);
  } else {
    for (int64_t i = 0; i < ns; ++i) pcm[i] = (int16_t)(((int)d[i] - 128) * 256);
  }
  return TFP_OK;
}

// Interleaved form: 8/16-bit integer PCM of 1 to 32 channels, the samples as stored (frame i, channel c
// at pcm[i * channels + c]), for the multichannel rate forms (tfp_resample_mix_pcm,
// tfp_fingerprint_mix_rate_batch), which downmix and convert in integers. No downmix happens here.
extern "C" int tfp_wav_decode_interleaved(const void* bytes, int64_t nbytes, int16_t* pcm, int64_t cap, int64_t* nframes,
                                          int32_t* channels, int32_t* sample_rate) {
  if (!bytes || nbytes < 0 || !nframes || cap < 0 || (cap > 0 && !pcm)) return fail(TFP_E_ARG, "bad argument");
  WavData w;
  if (const int rc = find_data(static_cast<const uint8_t*>(bytes), (uint64_t)nbytes, &w)) return rc;
  const WavFormat& f = w.f;
  if (f.tag != kFormatPcm)
    return fail(TFP_E_FORMAT, "format tag " + std::to_string(f.tag) + " is not integer PCM (float and G.711 are not taken)");
  if (f.bits != 16 && f.bits != 8)
    return fail(TFP_E_FORMAT, std::to_string(f.bits) + "-bit samples: only 8- and 16-bit PCM map exactly to int16");
  if (f.channels < 1 || f.channels > TFP_MIX_CHANNELS_MAX)
    return fail(TFP_E_FORMAT, std::to_string(f.channels) + " channels: 1 to " + std::to_string(TFP_MIX_CHANNELS_MAX) + " are taken");
  if (f.rate == 0 || f.rate > (uint32_t)INT32_MAX) return fail(TFP_E_FORMAT, "bad sample rate");
  const uint32_t width = f.bits / 8;
  if (f.block_align != width * f.channels) return fail(TFP_E_FORMAT, "block align does not match the format");
  const int64_t nf = (int64_t)(w.size / f.block_align), ns = nf * f.channels;  // a trailing partial frame is dropped
  *nframes = nf;
  if (channels) *channels = (int32_t)f.channels;
  if (sample_rate) *sample_rate = (int32_t)f.rate;
  if (!pcm) return TFP_OK;  // size query
  if (cap < ns) return fail(TFP_E_CAPACITY, "pcm buffer holds " + std::to_string(cap) + " of " + std::to_string(ns) + " samples");
  const uint8_t* d = w.data;
  if (width == 2) {
    for (int64_t i = 0; i < ns; ++i) pcm[i] = (int16_t)le16(d + 2 * i);
  } else {
    for (int64_t i = 0; i < ns; ++i) pcm[i] = (int16_t)(((int)d[i] - 128) * 256);
  }
  return TFP_OK;
}

extern "C" int tfp_wav_read_interleaved(const char* path, int16_t* pcm, int64_t cap, int64_t* nframes, int32_t* channels,
                                        int32_t* sample_rate) {
  std::vector<uint8_t> buf;
  const int rc = read_file(path, buf);
  if (rc) return rc;
  return tfp_wav_decode_interleaved(buf.data(), (int64_t)buf.size(), pcm, cap, nframes, channels, sample_rate);
}

// Q31 form: integer PCM of 8, 16, 24 or 32 bits and float data of 32 or 64 bits, 1 to 32 channels, each
// sample as int32 Q31 (frame i, channel c at q31[i * channels + c]) for the wide rate forms
// (tfp_resample_wide_pcm, tfp_fingerprint_wide_rate_batch). Integer samples are shifted to the top of the
// word, float samples go through q31_from_f32 / q31_from_f64. No downmix happens here.
extern "C" int tfp_wav_decode_interleaved_q31(const void* bytes, int64_t nbytes, int32_t* q31, int64_t cap, int64_t* nframes,
                                              int32_t* channels, int32_t* sample_rate) {
  if (!bytes || nbytes < 0 || !nframes || cap < 0 || (cap > 0 && !q31)) return fail(TFP_E_ARG, "bad argument");
  WavData w;
  if (const int rc = find_data(static_cast<const uint8_t*>(bytes), (uint64_t)nbytes, &w)) return rc;
  const WavFormat& f = w.f;
  const bool pcm = f.tag == kFormatPcm && (f.bits == 8 || f.bits == 16 || f.bits == 24 || f.bits == 32);
  const bool flt = f.tag == kFormatFloat && (f.bits == 32 || f.bits == 64);
  if (!pcm && !flt)
    return fail(TFP_E_FORMAT, "format tag " + std::to_string(f.tag) + " with " + std::to_string(f.bits) +
                                  "-bit samples is neither 8/16/24/32-bit PCM nor 32/64-bit float (G.711 is not taken)");
  if (f.channels < 1 || f.channels > TFP_MIX_CHANNELS_MAX)
    return fail(TFP_E_FORMAT, std::to_string(f.channels) + " channels: 1 to " + std::to_string(TFP_MIX_CHANNELS_MAX) + " are taken");
  if (f.rate == 0 || f.rate > (uint32_t)INT32_MAX) return fail(TFP_E_FORMAT, "bad sample rate");
  const uint32_t width = f.bits / 8;
  if (f.block_align != width * f.channels) return fail(TFP_E_FORMAT, "block align does not match the format");
  const int64_t nf = (int64_t)(w.size / f.block_align), ns = nf * f.channels;  // a trailing partial frame is dropped
  *nframes = nf;
  if (channels) *channels = (int32_t)f.channels;
  if (sample_rate) *sample_rate = (int32_t)f.rate;
  if (!q31) return TFP_OK;  // size query
  if (cap < ns) return fail(TFP_E_CAPACITY, "sample buffer holds " + std::to_string(cap) + " of " + std::to_string(ns) + " samples");
  const uint8_t* d = w.data;
  for (int64_t i = 0; i < ns; ++i) {
    const uint8_t* p = d + (uint64_t)i * width;
    if (flt && width == 4) {
      q31[i] = tfp::q31_from_f32(__builtin_bit_cast(float, le32(p)));
    } else if (flt) {
      q31[i] = tfp::q31_from_f64(__builtin_bit_cast(double, (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32)));
    } else if (width == 1) {
      q31[i] = (int32_t)((uint32_t)((int)p[0] - 128) << 24);
    } else if (width == 2) {
      q31[i] = (int32_t)((uint32_t)le16(p) << 16);
    } else if (width == 3) {
      q31[i] = (int32_t)(((uint32_t)p[0] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 24));
    } else {
      q31[i] = (int32_t)le32(p);
    }
  }
  return TFP_OK;
}

extern "C" int tfp_wav_read_interleaved_q31(const char* path, int32_t* q31, int64_t cap, int64_t* nframes, int32_t* channels,
                                            int32_t* sample_rate) {
  std::vector<uint8_t> buf;
  const int rc = read_file(path, buf);
  if (rc) return rc;
  return tfp_wav_decode_interleaved_q31(buf.data(), (int64_t)buf.size(), q31, cap, nframes, channels, sample_rate);
}

// fp32 form: every PCM width and float data, any channel count, as aubio 0.4.5's sndfile and
// wavread sources compute the mono hop (aubio_source_do with its default downmix): each sample
// to fp32 (unsigned 8-bit (u - 128) / 128, w-bit signed x / 2^(w-1) with 32-bit x first rounded
// to float as libsndfile's normalised read does, float data as stored, double data rounded to
// float), then per frame the channels summed in fp32 in channel order and divided by the
// channel count in fp32.
extern "C" int tfp_wav_decode_f32(const void* bytes, int64_t nbytes, float* x, int64_t cap, int64_t* nsamples,
                                  int32_t* sample_rate) {
  if (!bytes || nbytes < 0 || !nsamples || cap < 0 || (cap > 0 && !x)) return fail(TFP_E_ARG, "bad argument");
  WavData w;
  if (const int rc = find_data(static_cast<const uint8_t*>(bytes), (uint64_t)nbytes, &w)) return rc;
  const WavFormat& f = w.f;
  const bool pcm = f.tag == kFormatPcm && (f.bits == 8 || f.bits == 16 || f.bits == 24 || f.bits == 32);
  const bool flt = f.tag == kFormatFloat && (f.bits == 32 || f.bits == 64);
  if (!pcm && !flt)
    return fail(TFP_E_FORMAT, "format tag " + std::to_string(f.tag) + " with " + std::to_string(f.bits) +
                                  "-bit samples is neither 8/16/24/32-bit PCM nor 32/64-bit float");
  if (f.channels == 0) return fail(TFP_E_FORMAT, "zero channels");
  if (f.rate == 0 || f.rate > (uint32_t)INT32_MAX) return fail(TFP_E_FORMAT, "bad sample rate");
  const uint32_t width = f.bits / 8;
  if (f.block_align != width * f.channels) return fail(TFP_E_FORMAT, "block align does not match the format");
  const int64_t ns = (int64_t)(w.size / f.block_align);
  *nsamples = ns;
  if (sample_rate) *sample_rate = (int32_t)f.rate;
  if (!x) return TFP_OK;  // size query
  if (cap < ns) return fail(TFP_E_CAPACITY, "sample buffer holds " + std::to_string(cap) + " of " + std::to_string(ns) + " samples");
  const uint8_t* d = w.data;
  const float nch = (float)f.channels;
  for (int64_t i = 0; i < ns; ++i) {
    float acc = 0.f;
    for (uint32_t c = 0; c < f.channels; ++c) {
      const uint8_t* p = d + (uint64_t)i * f.block_align + (uint64_t)c * width;
      float v;
      if (flt && width == 4) {
        v = __builtin_bit_cast(float, le32(p));
      } else if (flt) {
        v = (float)__builtin_bit_cast(double, (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32));
      } else if (width == 1) {
        v = (float)((int)p[0] - 128) / 128.f;
      } else if (width == 2) {
        v = (float)(int16_t)le16(p) / 32768.f;
      } else if (width == 3) {
        const int32_t s = (int32_t)(((uint32_t)p[0] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 24)) >> 8;
        v = (float)s / 8388608.f;
      } else {
        v = (float)(int32_t)le32(p) * (1.f / 2147483648.f);
      }
      acc = acc + v;
    }
    x[i] = acc / nch;
  }
  return TFP_OK;
}

// G.711 codes -> int16: libsndfile's table[code], the numerator of the table[code] / 32768 that
// aubio_source_do hands out for these files (fp_handler.c:604, :633).
extern "C" int tfp_g711_decode(const uint8_t* codes, int64_t n, int32_t law, int16_t* pcm) {
  if (n < 0 || !tfp::g711_law_ok(law) || (n > 0 && (!codes || !pcm))) return fail(TFP_E_ARG, "bad argument");
  if (law == tfp::kG711Alaw) {
    for (int64_t i = 0; i < n; ++i) pcm[i] = (int16_t)tfp::g711_alaw(codes[i]);
  } else {
    for (int64_t i = 0; i < n; ++i) pcm[i] = (int16_t)tfp::g711_ulaw(codes[i]);
  }
  return TFP_OK;
}

// The codes of a mono 8-bit mu-law / A-law WAV as stored (one byte per sample).
extern "C" int tfp_wav_decode_g711(const void* bytes, int64_t nbytes, uint8_t* codes, int64_t cap, int64_t* nsamples,
                                   int32_t* sample_rate, int32_t* law) {
  if (!bytes || nbytes < 0 || !nsamples || cap < 0 || (cap > 0 && !codes)) return fail(TFP_E_ARG, "bad argument");
  WavData w;
  if (const int rc = find_data(static_cast<const uint8_t*>(bytes), (uint64_t)nbytes, &w)) return rc;
  const WavFormat& f = w.f;
  if (f.tag != kFormatAlaw && f.tag != kFormatUlaw)
    return fail(TFP_E_FORMAT, "format tag " + std::to_string(f.tag) + " is neither A-law (6) nor mu-law (7)");
  if (f.channels != 1)
    return fail(TFP_E_FORMAT, std::to_string(f.channels) +
                                  " channels: aubio's channel mean is not a G.711 code's value (mono only)");
  if (f.bits != 8) return fail(TFP_E_FORMAT, std::to_string(f.bits) + "-bit samples: G.711 codes are 8-bit");
  if (f.rate == 0 || f.rate > (uint32_t)INT32_MAX) return fail(TFP_E_FORMAT, "bad sample rate");
  if (f.block_align != 1) return fail(TFP_E_FORMAT, "block align does not match mono 8-bit codes");
  const int64_t ns = (int64_t)w.size;
  *nsamples = ns;
  if (sample_rate) *sample_rate = (int32_t)f.rate;
  if (law) *law = f.tag == kFormatAlaw ? TFP_G711_ALAW : TFP_G711_ULAW;
  if (!codes) return TFP_OK;  // size query
  if (cap < ns) return fail(TFP_E_CAPACITY, "code buffer holds " + std::to_string(cap) + " of " + std::to_string(ns) + " samples");
  if (ns) std::memcpy(codes, w.data, (size_t)ns);
  return TFP_OK;
}

extern "C" int tfp_wav_read_g711(const char* path, uint8_t* codes, int64_t cap, int64_t* nsamples, int32_t* sample_rate,
                                 int32_t* law) {
  std::vector<uint8_t> buf;
  const int rc = read_file(path, buf);
  if (rc) return rc;
  return tfp_wav_decode_g711(buf.data(), (int64_t)buf.size(), codes, cap, nsamples, sample_rate, law);
}

extern "C" int tfp_wav_read_f32(const char* path, float* x, int64_t cap, int64_t* nsamples, int32_t* sample_rate) {
  std::vector<uint8_t> buf;
  const int rc = read_file(path, buf);
  if (rc) return rc;
  return tfp_wav_decode_f32(buf.data(), (int64_t)buf.size(), x, cap, nsamples, sample_rate);
}

extern "C" int tfp_wav_read(const char* path, int16_t* pcm, int64_t cap, int64_t* nsamples, int32_t* sample_rate) {
  std::vector<uint8_t> buf;
  const int rc = read_file(path, buf);
  if (rc) return rc;
  return tfp_wav_decode(buf.data(), (int64_t)buf.size(), pcm, cap, nsamples, sample_rate);
}
