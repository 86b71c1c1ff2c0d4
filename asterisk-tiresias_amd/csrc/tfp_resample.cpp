// tfp_resample.cpp — the host side of rate conversion (tfp_resample.hpp): the process's tables and the
// host-only entry points tfp_resample_count / _taps / _pcm / _mix_pcm / _wide_pcm / _any_pcm, tfp_q31_from_*
// and tfp_audio_clips_check.
// tfp_resample_pcm is the map the kernel of
// tfp_resample.hip computes (one routine, resample_sample), for the search forms without a rate twin.
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "tfp_resample_any.hpp"
#include "tiresias_fp.h"

// engine-less calls report through tfp_engine_last_error(NULL) (tfp_wav.cpp)
extern "C" __attribute__((visibility("hidden"))) void tfp_ingest_set_error(const char* msg);

namespace tfp {

std::shared_ptr<const ResampleTable> resample_table(int32_t rate_in, int32_t rate_out, bool* bad_rate) {
  static std::mutex mu;
  static std::map<std::pair<int32_t, int32_t>, std::shared_ptr<const ResampleTable>> tables;
  ResamplePlan P;
  if (!resample_plan(rate_in, rate_out, &P, bad_rate)) return nullptr;
  const int64_t g = rs_gcd(rate_in, rate_out);  // the table depends on the ratio alone
  const std::pair<int32_t, int32_t> key((int32_t)(rate_in / g), (int32_t)(rate_out / g));
  std::lock_guard<std::mutex> lk(mu);
  auto it = tables.find(key);
  if (it != tables.end()) return it->second;
  auto t = std::make_shared<ResampleTable>();
  t->plan = P;
  if (!resample_build(P, &t->taps)) return nullptr;
  t->abs_sum = resample_abs_sum(P, t->taps);
  if (tables.size() >= 64) tables.clear();  // (holders keep theirs)
  tables[key] = t;
  return t;
}

}  // namespace tfp

namespace {

int fail(int code, const std::string& msg) {
  tfp_ingest_set_error(msg.c_str());
  return code;
}

// The pair's table, or the error the engine forms give for it.
int table_of(int32_t rate_in, int32_t rate_out, std::shared_ptr<const tfp::ResampleTable>* t) {
  bool bad = false;
  *t = tfp::resample_table(rate_in, rate_out, &bad);
  if (*t) return TFP_OK;
  if (bad) return fail(TFP_E_ARG, "bad sample rate " + std::to_string(rate_in < 1 ? rate_in : rate_out));
  return fail(TFP_E_ARG, "unsupported rate ratio " + std::to_string(rate_in) + " -> " + std::to_string(rate_out));
}

}  // namespace

extern "C" int64_t tfp_resample_count(int64_t nsamples, int32_t rate_in, int32_t rate_out) {
  tfp::ResamplePlan P;
  bool bad = false;
  if (!tfp::resample_plan(rate_in, rate_out, &P, &bad)) return -1;
  return tfp::resample_count(P, nsamples);
}

extern "C" int tfp_resample_taps(int32_t rate_in, int32_t rate_out, int32_t* L, int32_t* M, int32_t* k_lo, int32_t* ntaps,
                                 int16_t* taps, int64_t cap) {
  std::shared_ptr<const tfp::ResampleTable> t;
  if (int rc = table_of(rate_in, rate_out, &t)) return rc;
  if (L) *L = t->plan.L;
  if (M) *M = t->plan.M;
  if (k_lo) *k_lo = t->plan.k_lo;
  if (ntaps) *ntaps = t->plan.ntaps;
  const int64_t n = (int64_t)t->taps.size();
  if (!taps && cap == 0) return TFP_OK;  // size query
  if (!taps || cap < n) return fail(TFP_E_CAPACITY, "tap buffer holds " + std::to_string(cap) + " of " + std::to_string(n) + " entries");
  std::memcpy(taps, t->taps.data(), sizeof(int16_t) * (size_t)n);
  return TFP_OK;
}

extern "C" int tfp_resample_pcm(const int16_t* pcm, int64_t n, int32_t rate_in, int32_t rate_out, int16_t* out, int64_t cap,
                                int64_t* nout) {
  if (n < 0 || !nout || (n > 0 && !pcm)) return fail(TFP_E_ARG, "bad argument");
  std::shared_ptr<const tfp::ResampleTable> t;
  if (int rc = table_of(rate_in, rate_out, &t)) return rc;
  const int64_t no = rate_in == rate_out ? n : tfp::resample_count(t->plan, n);
  if (no < 0) return fail(TFP_E_ARG, "sample count " + std::to_string(n) + " past the index range");
  *nout = no;
  if (!out && cap == 0) return TFP_OK;  // size query
  if (!out || cap < no) return fail(TFP_E_CAPACITY, "pcm buffer holds " + std::to_string(cap) + " of " + std::to_string(no) + " samples");
  if (rate_in == rate_out) {
    if (n) std::memmove(out, pcm, sizeof(int16_t) * (size_t)n);  // equal rates: the filter is not run
    return TFP_OK;
  }
  tfp::resample_clip(*t, pcm, n, out);
  return TFP_OK;
}

static_assert(tfp::kRsMixChannelsMax == TFP_MIX_CHANNELS_MAX, "tfp_resample.hpp and the public header agree");

// The multichannel form on the host: the map the kernel of tfp_resample_mix.hip computes (one routine,
// resample_mix_sample). One channel is tfp_resample_pcm.
extern "C" int tfp_resample_mix_pcm(const int16_t* pcm, int64_t nframes, int32_t channels, int32_t rate_in, int32_t rate_out,
                                    int16_t* out, int64_t cap, int64_t* nout) {
  if (channels < 1 || channels > TFP_MIX_CHANNELS_MAX)
    return fail(TFP_E_ARG, "unsupported channel count " + std::to_string(channels));
  if (channels == 1) return tfp_resample_pcm(pcm, nframes, rate_in, rate_out, out, cap, nout);
  if (nframes < 0 || !nout || (nframes > 0 && !pcm)) return fail(TFP_E_ARG, "bad argument");
  std::shared_ptr<const tfp::ResampleTable> t;
  if (int rc = table_of(rate_in, rate_out, &t)) return rc;
  const int64_t no = rate_in == rate_out ? nframes : tfp::resample_count(t->plan, nframes);
  if (no < 0 || nframes > INT64_MAX / channels)
    return fail(TFP_E_ARG, "frame count " + std::to_string(nframes) + " past the index range");
  *nout = no;
  if (!out && cap == 0) return TFP_OK;  // size query
  if (!out || cap < no) return fail(TFP_E_CAPACITY, "pcm buffer holds " + std::to_string(cap) + " of " + std::to_string(no) + " samples");
  if (rate_in == rate_out) {  // equal rates: the integer mean, the filter is not run
    for (int64_t i = 0; i < nframes; i++) {
      int32_t S = 0;
      for (int32_t c = 0; c < channels; c++) S += pcm[i * channels + c];
      out[i] = tfp::resample_mix_mean(S, channels);
    }
    return TFP_OK;
  }
  tfp::resample_mix_clip(*t, pcm, nframes, channels, out);
  return TFP_OK;
}

// The wide form on the host: the map the kernel of tfp_resample_wide.hip computes (one routine,
// resample_wide_sample). The frames are int32 Q31; one channel runs the same routine over the samples
// themselves, and equal rates round and clamp (resample_wide_mean) without a filter.
extern "C" int tfp_resample_wide_pcm(const int32_t* q31, int64_t nframes, int32_t channels, int32_t rate_in, int32_t rate_out,
                                     int16_t* out, int64_t cap, int64_t* nout) {
  if (channels < 1 || channels > TFP_MIX_CHANNELS_MAX)
    return fail(TFP_E_ARG, "unsupported channel count " + std::to_string(channels));
  if (nframes < 0 || !nout || (nframes > 0 && !q31)) return fail(TFP_E_ARG, "bad argument");
  std::shared_ptr<const tfp::ResampleTable> t;
  if (int rc = table_of(rate_in, rate_out, &t)) return rc;
  if (rate_in != rate_out && !tfp::resample_wide_in_range(*t, channels))
    return fail(TFP_E_ARG, "unsupported rate ratio " + std::to_string(rate_in) + " -> " + std::to_string(rate_out) +
                               " for " + std::to_string(channels) + " wide channels");
  const int64_t no = rate_in == rate_out ? nframes : tfp::resample_count(t->plan, nframes);
  if (no < 0 || nframes > INT64_MAX / channels)
    return fail(TFP_E_ARG, "frame count " + std::to_string(nframes) + " past the index range");
  *nout = no;
  if (!out && cap == 0) return TFP_OK;  // size query
  if (!out || cap < no) return fail(TFP_E_CAPACITY, "pcm buffer holds " + std::to_string(cap) + " of " + std::to_string(no) + " samples");
  if (rate_in == rate_out) {  // equal rates: the filter is not run
    for (int64_t i = 0; i < nframes; i++) {
      int64_t S = 0;
      for (int32_t c = 0; c < channels; c++) S += (int64_t)q31[i * channels + c];
      out[i] = tfp::resample_wide_mean(S, channels);
    }
    return TFP_OK;
  }
  tfp::resample_wide_clip(*t, q31, nframes, channels, out);
  return TFP_OK;
}

// Sample to Q31 (tfp_resample.hpp, q31_from_f32 / q31_from_f64): the map tfp_wav_decode_interleaved_q31
// applies to float data. dst may not overlap src.
extern "C" int tfp_q31_from_f32(const float* src, int64_t n, int32_t* dst) {
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(TFP_E_ARG, "bad argument");
  for (int64_t i = 0; i < n; i++) dst[i] = tfp::q31_from_f32(src[i]);
  return TFP_OK;
}

extern "C" int tfp_q31_from_f64(const double* src, int64_t n, int32_t* dst) {
  if (n < 0 || (n > 0 && (!src || !dst))) return fail(TFP_E_ARG, "bad argument");
  for (int64_t i = 0; i < n; i++) dst[i] = tfp::q31_from_f64(src[i]);
  return TFP_OK;
}

// ---- mixed batches (tfp_resample_any.hpp): the dispatch to the four host maps above ----------------
// One clip on the host. The clip's own rules are any_prepare's (a batch of one clip that reaches exactly
// its own end), so the messages are the engine forms'; the arithmetic is the class's existing entry point.
extern "C" int tfp_resample_any_pcm(const void* data, const tfp_audio_clip* clip, int32_t rate_out, int16_t* out, int64_t cap,
                                    int64_t* nout) {
  if (!clip || !nout) return fail(TFP_E_ARG, "bad argument");
  tfp::AnyBatch B;
  std::string err;
  tfp_audio_clip k = *clip;
  k.offset = clip->offset < 0 ? clip->offset : clip->offset % tfp::any_sample_size(clip->kind);  // (alignment alone)
  if (!tfp::any_prepare(&k, 1, INT64_MAX, rate_out, tfp::resample_table, &B, &err)) return fail(TFP_E_ARG, err);
  if (clip->nframes > 0 && !data) return fail(TFP_E_ARG, "clip 0: samples are NULL");
  const uint8_t* src = static_cast<const uint8_t*>(data) + (data ? clip->offset : 0);
  switch (clip->kind) {
    case TFP_AUDIO_S16:
      return tfp_resample_mix_pcm(reinterpret_cast<const int16_t*>(src), clip->nframes, clip->channels, clip->rate_in, rate_out,
                                  out, cap, nout);
    case TFP_AUDIO_Q31:
      return tfp_resample_wide_pcm(reinterpret_cast<const int32_t*>(src), clip->nframes, clip->channels, clip->rate_in,
                                   rate_out, out, cap, nout);
    default: {
      std::vector<int16_t> pcm((size_t)clip->nframes);
      if (int rc = tfp_g711_decode(src, clip->nframes, clip->kind - TFP_AUDIO_ULAW, pcm.data())) return rc;
      return tfp_resample_pcm(pcm.data(), clip->nframes, clip->rate_in, rate_out, out, cap, nout);
    }
  }
}

extern "C" int tfp_audio_clips_check(const tfp_audio_clip* clips, int32_t nclips, int64_t nbytes, int32_t rate_out,
                                     int64_t* nout) {
  tfp::AnyBatch B;
  std::string err;
  if (!tfp::any_prepare(clips, nclips, nbytes, rate_out, tfp::resample_table, &B, &err)) return fail(TFP_E_ARG, err);
  for (int32_t c = 0; nout && c < nclips; c++) nout[c] = B.clips[(size_t)c].n_out;
  return TFP_OK;
}
