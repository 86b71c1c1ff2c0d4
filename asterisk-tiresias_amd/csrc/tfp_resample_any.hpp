// tfp_resample_any.hpp — mixed batches: clips that each carry their own rate, channel count and sample
// kind, converted to the index's rate by one launch (include/tiresias_fp.h, "mixed batches").
//
// Nothing is defined here that was not defined before. A clip's output is the existing host map of its own
// class (tfp_resample_pcm, tfp_resample_mix_pcm, tfp_resample_wide_pcm, or tfp_g711_decode followed by
// tfp_resample_pcm), and the per-sample arithmetic is tfp_resample.hpp's routines and tfp_g711.hpp's map,
// called as the four single-class kernels call them. What this header adds:
//   - the host arithmetic of a call (any_prepare): descriptor validation, the call's distinct plans, each
//     clip's form, the output offsets and the tile counts;
//   - one tile of one clip (any_tile): the staging of the tile's span in one untyped LDS buffer by the rule
//     of the clip's class, then the class's sample routine. It is written once for host and device: the
//     kernel runs it with a workgroup's threads, tests/native/check_resample_any.cpp with one "thread";
//   - the launch (tfp_resample_any.hip).
//
// A clip's form depends on the clip alone (kind, channels, pair), so it is uniform over every workgroup of
// the clip and the kernel branches on workgroup-uniform values only. Each class keeps its own staging limit:
//   int16 mono and G.711   int16 samples     kRsSpanMax      (G.711 codes are expanded while staging)
//   int16, C >= 2          int32 channel sums kRsMixSpanMax
//   Q31 mono               int32 samples     kRsMixSpanMax
//   Q31, C >= 2            int64 channel sums kRsWideSpanMax
// all of them 60 KiB. A span past the limit takes the class's per-tap global-memory routine; G.711 has no
// such routine (no int16 array exists to read), so a G.711 clip at a reduction past the int16 limit
// (about 29 to 1: no telephone rate) is refused with "unsupported rate ratio", as the live forms refuse it.
#pragma once

#include <map>
#include <string>

#include "tfp_g711.hpp"
#include "tfp_resample.hpp"
#include "tiresias_fp.h"

namespace tfp {

static_assert(TFP_AUDIO_ULAW - 2 == kG711Ulaw && TFP_AUDIO_ALAW - 2 == kG711Alaw, "a G.711 kind is its law + 2");

// The form of a clip. Plain: equal rates, no filter and no table. Staged: the tile's span in LDS. Global:
// the clip read per tap in global memory.
enum AnyForm : int32_t {
  kAnyCopy = 0,     // int16 mono, equal rates: the samples as they are
  kAnyExpand,       // G.711, equal rates: the expansion
  kAnyMixMean,      // int16 C >= 2, equal rates: int32 sums over the identity span, resample_mix_mean
  kAnyWideRound,    // Q31 mono, equal rates: resample_wide_mean of each sample
  kAnyWideMean,     // Q31 C >= 2, equal rates: int64 sums over the identity span, resample_wide_mean
  kAnyMono,         // int16 mono, staged: resample_sample
  kAnyG711,         // G.711, staged as int16: resample_sample
  kAnyMix,          // int16 C >= 2, staged int32 sums: resample_mix_sample
  kAnyWideMono,     // Q31 mono, staged int32: resample_wide_sample<int32_t>
  kAnyWideSums,     // Q31 C >= 2, staged int64 sums: resample_wide_sample<int64_t>
  kAnyMonoGlobal,   // resample_sample over the whole clip
  kAnyMixGlobal,    // resample_mix_sample_frames
  kAnyWideGlobal,   // resample_wide_sample_frames
  kAnyForms
};
TFP_RS_HD bool any_form_plain(int32_t f) { return f >= kAnyCopy && f <= kAnyWideMean; }
TFP_RS_HD bool any_form_staged(int32_t f) { return f >= kAnyMono && f <= kAnyWideSums; }
TFP_RS_HD bool any_form_global(int32_t f) { return f >= kAnyMonoGlobal && f < kAnyForms; }

// A clip as the kernel reads it.
struct AnyClipDev {
  int64_t byte_off;  // of the clip's first sample in the call's bytes
  int64_t nframes;
  int64_t out_off;   // of the clip's first output in the call's output
  int64_t n_out;
  int32_t channels;
  int32_t form;      // AnyForm
  int32_t plan;      // index into the call's plans, -1 at equal rates
  int32_t law;       // kG711Ulaw / kG711Alaw for the G.711 forms, else -1
};
// One of the call's distinct plans and where its table starts in the call's concatenated taps.
struct AnyPlanDev {
  ResamplePlan P;
  int64_t taps_off;  // in int16 entries
};

inline int32_t any_sample_size(int32_t kind) { return kind == TFP_AUDIO_S16 ? 2 : kind == TFP_AUDIO_Q31 ? 4 : 1; }

// The staged span of a tile of a plan is at most this many frames (tfp_resample.hip's span_max).
inline int64_t any_span_max(const ResamplePlan& P) { return ((int64_t)(kRsTile - 1) * P.M) / P.L + 1 + P.ntaps; }

// The form of a clip of `kind` and C channels whose pair's span is `span` (equal: rate_in == rate_out), and
// the LDS bytes a tile of it may stage. kAnyForms: G.711 past the int16 limit (refused).
inline int32_t any_form(int32_t kind, int32_t C, bool equal, int64_t span, int64_t* lds_bytes) {
  *lds_bytes = 0;
  const bool g711 = kind == TFP_AUDIO_ULAW || kind == TFP_AUDIO_ALAW;
  if (equal) {
    if (g711) return kAnyExpand;
    if (C == 1) return kind == TFP_AUDIO_S16 ? kAnyCopy : kAnyWideRound;
    *lds_bytes = (kind == TFP_AUDIO_S16 ? 4 : 8) * (int64_t)(kRsTile + 1);  // the identity span's sums
    return kind == TFP_AUDIO_S16 ? kAnyMixMean : kAnyWideMean;
  }
  if (g711 || (kind == TFP_AUDIO_S16 && C == 1)) {
    if (span > kRsSpanMax) return g711 ? kAnyForms : kAnyMonoGlobal;
    *lds_bytes = 2 * span;
    return g711 ? kAnyG711 : kAnyMono;
  }
  if (kind == TFP_AUDIO_S16) {
    if (span > kRsMixSpanMax) return kAnyMixGlobal;
    *lds_bytes = 4 * span;
    return kAnyMix;
  }
  if (C == 1) {
    if (span > kRsMixSpanMax) return kAnyWideGlobal;
    *lds_bytes = 4 * span;
    return kAnyWideMono;
  }
  if (span > kRsWideSpanMax) return kAnyWideGlobal;
  *lds_bytes = 8 * span;
  return kAnyWideSums;
}

// A validated call.
struct AnyBatch {
  std::vector<AnyClipDev> clips;
  std::vector<AnyPlanDev> plans;
  std::vector<std::shared_ptr<const ResampleTable>> tables;  // plans[i]'s table
  std::vector<int64_t> in_off, out_off;  // running frames in / samples out, nclips + 1 each
  int64_t taps_total = 0;                // entries of the concatenated taps
  int64_t lds_bytes = 0;                 // the largest span any clip with output stages
  int64_t tiles_staged = 0, tiles_global = 0, tiles_plain = 0;
};

// Validates clips[0..n) against nbytes and rate_out and fills *B; false with *err set ("clip i: ..." for a
// rule a clip breaks, the first such clip). table(rate_in, rate_out, &bad) is resample_table or a stand-in.
template <typename TableFn>
inline bool any_prepare(const tfp_audio_clip* clips, int32_t n, int64_t nbytes, int32_t rate_out, TableFn table, AnyBatch* B,
                        std::string* err) {
  auto bad = [&](int32_t c, const std::string& m) {
    *err = "clip " + std::to_string(c) + ": " + m;
    return false;
  };
  *B = AnyBatch();
  if (rate_out < 1) {
    *err = "bad sample rate " + std::to_string(rate_out);
    return false;
  }
  if (n < 0 || nbytes < 0 || (n > 0 && !clips)) {
    *err = "bad arguments";
    return false;
  }
  B->clips.resize((size_t)n);
  B->in_off.assign((size_t)n + 1, 0);
  B->out_off.assign((size_t)n + 1, 0);
  std::map<int32_t, int32_t> plan_of;  // rate_in -> plan index (-1: rate_out itself)
  for (int32_t c = 0; c < n; c++) {
    const tfp_audio_clip& k = clips[c];
    if (k.reserved != 0) return bad(c, "reserved is " + std::to_string(k.reserved) + ", not 0");
    if (k.kind < TFP_AUDIO_S16 || k.kind > TFP_AUDIO_ALAW) return bad(c, "unknown sample kind " + std::to_string(k.kind));
    const bool g711 = k.kind >= TFP_AUDIO_ULAW;
    if (k.channels < 1 || k.channels > kRsMixChannelsMax) return bad(c, "unsupported channel count " + std::to_string(k.channels));
    if (g711 && k.channels != 1) return bad(c, "G.711 of " + std::to_string(k.channels) + " channels");
    if (k.rate_in < 1) return bad(c, "bad sample rate " + std::to_string(k.rate_in));
    if (k.nframes < 0) return bad(c, "negative frame count " + std::to_string(k.nframes));
    const int64_t fb = (int64_t)any_sample_size(k.kind) * k.channels;  // bytes per frame
    if (k.offset < 0 || k.offset % any_sample_size(k.kind))
      return bad(c, "offset " + std::to_string(k.offset) + " is no multiple of the sample size " + std::to_string(any_sample_size(k.kind)));
    if (k.offset > nbytes || k.nframes > (nbytes - k.offset) / fb)
      return bad(c, "reaches past the " + std::to_string(nbytes) + " bytes given");
    auto it = plan_of.find(k.rate_in);
    if (it == plan_of.end()) {
      if ((int32_t)plan_of.size() >= TFP_ANY_RATES_MAX)
        return bad(c, "more than " + std::to_string(TFP_ANY_RATES_MAX) + " distinct input rates in one call");
      int32_t idx = -1;
      if (k.rate_in != rate_out) {
        bool bad_rate = false;
        std::shared_ptr<const ResampleTable> t = table(k.rate_in, rate_out, &bad_rate);
        if (!t) return bad(c, "unsupported rate ratio " + std::to_string(k.rate_in) + " -> " + std::to_string(rate_out));
        idx = (int32_t)B->plans.size();
        B->plans.push_back(AnyPlanDev{t->plan, B->taps_total});
        B->taps_total += (int64_t)t->taps.size();
        B->tables.push_back(t);
      }
      it = plan_of.emplace(k.rate_in, idx).first;
    }
    const int32_t pi = it->second;
    const std::string ratio = "unsupported rate ratio " + std::to_string(k.rate_in) + " -> " + std::to_string(rate_out);
    if (pi >= 0 && k.kind == TFP_AUDIO_Q31 && !resample_wide_in_range(*B->tables[(size_t)pi], k.channels))
      return bad(c, ratio + " for " + std::to_string(k.channels) + " wide channels");
    int64_t lds = 0;
    const int32_t form = any_form(k.kind, k.channels, pi < 0, pi < 0 ? 0 : any_span_max(B->plans[(size_t)pi].P), &lds);
    if (form == kAnyForms) return bad(c, ratio + " for G.711 codes");
    const int64_t no = pi < 0 ? k.nframes : resample_count(B->plans[(size_t)pi].P, k.nframes);
    if (no < 0 || no > INT64_MAX / 4 - B->out_off[c] || k.nframes > INT64_MAX / 4 - B->in_off[c])
      return bad(c, std::to_string(k.nframes) + " frames past the index range");
    AnyClipDev& d = B->clips[(size_t)c];
    d.byte_off = k.offset;
    d.nframes = k.nframes;
    d.out_off = B->out_off[c];
    d.n_out = no;
    d.channels = k.channels;
    d.form = form;
    d.plan = pi;
    d.law = g711 ? k.kind - TFP_AUDIO_ULAW : -1;
    B->in_off[c + 1] = B->in_off[c] + k.nframes;
    B->out_off[c + 1] = B->out_off[c] + no;
    const int64_t nt = (no + kRsTile - 1) / kRsTile;
    if (nt && lds > B->lds_bytes) B->lds_bytes = lds;
    (any_form_plain(form) ? B->tiles_plain : any_form_staged(form) ? B->tiles_staged : B->tiles_global) += nt;
  }
  return true;
}

// ---- one tile, host and device ---------------------------------------------------------------------
// The device runs the loops below with a workgroup's threads (tid, nthr), LDS atomics and barriers; the
// host runs them with one thread (tid 0 of 1), plain adds and no barrier: the same statements either way.
#if defined(__HIP_DEVICE_COMPILE__)
#define TFP_ANY_SYNC() __syncthreads()
#define TFP_ANY_ADD32(p, v) atomicAdd((p), (v))
#define TFP_ANY_ADD64(p, v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)(v))
#else
#define TFP_ANY_SYNC() ((void)0)
#define TFP_ANY_ADD32(p, v) (*(p) += (v))
#define TFP_ANY_ADD64(p, v) (*(p) += (v))
#endif

// int32 sums of the frames [lo, lo + len) of an interleaved int16 clip into sums (tfp_resample_mix.hip's
// staging: zeros, then the clip's own run word by word, its straddling ends read singly).
TFP_RS_HD void any_stage_mix(const int16_t* __restrict__ x, int64_t n_in, int32_t C, int64_t lo, int32_t len,
                             int32_t* __restrict__ sums, int32_t tid, int32_t nthr) {
  for (int32_t i = tid; i < len; i += nthr) sums[i] = 0;
  TFP_ANY_SYNC();
  const int64_t hi = lo + len, fa = lo > 0 ? lo : 0, fb = hi < n_in ? hi : n_in;
  if (fb > fa) {
    const int16_t* __restrict__ xs = x + fa * C;
    const int32_t total = (int32_t)(fb - fa) * C;  // <= kRsMixSpanMax * 32 < 2^19
    const int32_t head = (int32_t)((reinterpret_cast<uintptr_t>(xs) >> 1) & 1);  // xs sits in a word's upper half
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(xs - head);
    const int32_t nwords = (head + total + 1) / 2;
    int32_t* __restrict__ dst = sums + (int32_t)(fa - lo);
    for (int32_t j = tid; j < nwords; j += nthr) {
      const int32_t s0 = 2 * j - head, s1 = s0 + 1;  // the word's samples, counted from xs
      int32_t v0 = 0, v1 = 0;
      if (s0 >= 0 && s1 < total) {
        const uint32_t u = w[j];
        v0 = (int32_t)(int16_t)(u & 0xffffu);
        v1 = (int32_t)(int16_t)(u >> 16);
      } else {  // a word that straddles an end of the run: its samples inside the run, singly
        if (s0 >= 0) v0 = xs[s0];
        if (s1 < total) v1 = xs[s1];
      }
      const int32_t f0 = s0 >= 0 ? (int32_t)((uint32_t)s0 / (uint32_t)C) : 0;
      const int32_t f1 = s1 < total ? (int32_t)((uint32_t)s1 / (uint32_t)C) : f0;  // (f0, f1 < fb - fa)
      if (f0 == f1) {
        TFP_ANY_ADD32(dst + f0, v0 + v1);
      } else {
        TFP_ANY_ADD32(dst + f0, v0);
        TFP_ANY_ADD32(dst + f1, v1);
      }
    }
  }
  TFP_ANY_SYNC();
}

// int64 sums of the frames [lo, lo + len) of an interleaved Q31 clip (tfp_resample_wide.hip's staging).
TFP_RS_HD void any_stage_wide(const int32_t* __restrict__ x, int64_t n_in, int32_t C, int64_t lo, int32_t len,
                              int64_t* __restrict__ sums, int32_t tid, int32_t nthr) {
  for (int32_t i = tid; i < len; i += nthr) sums[i] = 0;
  TFP_ANY_SYNC();
  const int64_t hi = lo + len, fa = lo > 0 ? lo : 0, fb = hi < n_in ? hi : n_in;
  if (fb > fa) {
    const int32_t* __restrict__ xs = x + fa * C;
    const int32_t total = (int32_t)(fb - fa) * C;  // <= kRsWideSpanMax * 32 < 2^18
    int64_t* __restrict__ dst = sums + (int32_t)(fa - lo);
    for (int32_t j = tid; j < total; j += nthr)  // (j / C < fb - fa <= len - (fa - lo))
      TFP_ANY_ADD64(dst + (int32_t)((uint32_t)j / (uint32_t)C), (int64_t)xs[j]);
  }
  TFP_ANY_SYNC();
}

// Tile `tile` of clip d: outputs [tile kRsTile, ...) of the clip into out + d.out_off. data: the call's
// bytes (4-byte aligned); P and taps: the clip's plan and table (not read by a plain form); lds: lds_bytes
// of scratch, 8-byte aligned, shared by the nthr threads that make this call together. A tile whose span
// would not fit lds_bytes writes nothing (any_prepare sizes it; uniform).
TFP_RS_HD void any_tile(const uint8_t* __restrict__ data, const AnyClipDev& d, const ResamplePlan& P_in,
                        const int16_t* __restrict__ taps, int64_t tile, void* lds, int64_t lds_bytes, int16_t* __restrict__ out,
                        int32_t tid, int32_t nthr) {
  const int64_t n_in = d.nframes, n0 = tile * kRsTile;
  const int64_t n1 = n0 + kRsTile < d.n_out ? n0 + kRsTile : d.n_out;
  if (n0 >= n1) return;  // (uniform; resample_tiles gives no such tile)
  const int32_t C = d.channels;
  const uint8_t* __restrict__ src = data + d.byte_off;  // the clip's first sample
  int16_t* __restrict__ y = out + d.out_off;
  const ResamplePlan P = any_form_plain(d.form) ? ResamplePlan{1, 1, 0, 1} : P_in;  // plain: the identity span
  // frames [lo, hi) of the clip: the first output's first tap to the last output's last tap
  const int64_t lo = (n0 * P.M) / P.L + P.k_lo, hi = ((n1 - 1) * P.M) / P.L + P.k_lo + P.ntaps;
  const int32_t len = (int32_t)(hi - lo);  // <= any_span_max(P)
  switch (d.form) {  // (uniform: the clip's)
    case kAnyCopy: {
      const int16_t* __restrict__ x = reinterpret_cast<const int16_t*>(src);
      for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = x[n];
      return;
    }
    case kAnyExpand: {
      if (d.law == kG711Alaw)
        for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = (int16_t)g711_expand<kG711Alaw>(src[n]);
      else
        for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = (int16_t)g711_expand<kG711Ulaw>(src[n]);
      return;
    }
    case kAnyWideRound: {
      const int32_t* __restrict__ x = reinterpret_cast<const int32_t*>(src);
      for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_wide_mean((int64_t)x[n], 1);
      return;
    }
    case kAnyMonoGlobal: {
      const int16_t* __restrict__ x = reinterpret_cast<const int16_t*>(src);
      for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_sample(P, taps, x, 0, n_in, n);
      return;
    }
    case kAnyMixGlobal: {
      const int16_t* __restrict__ x = reinterpret_cast<const int16_t*>(src);
      for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_mix_sample_frames(P, taps, x, n_in, n, C);
      return;
    }
    case kAnyWideGlobal: {
      const int32_t* __restrict__ x = reinterpret_cast<const int32_t*>(src);
      for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_wide_sample_frames(P, taps, x, n_in, n, C);
      return;
    }
    case kAnyMono:
    case kAnyG711: {
      if ((int64_t)len * 2 > lds_bytes) return;
      int16_t* __restrict__ s = static_cast<int16_t*>(lds);
      if (d.form == kAnyMono) {
        const int16_t* __restrict__ x = reinterpret_cast<const int16_t*>(src);
        for (int32_t i = tid; i < len; i += nthr) {
          const int64_t f = lo + i;
          s[i] = f >= 0 && f < n_in ? x[f] : (int16_t)0;
        }
      } else if (d.law == kG711Alaw) {
        for (int32_t i = tid; i < len; i += nthr) {
          const int64_t f = lo + i;
          s[i] = f >= 0 && f < n_in ? (int16_t)g711_expand<kG711Alaw>(src[f]) : (int16_t)0;
        }
      } else {
        for (int32_t i = tid; i < len; i += nthr) {
          const int64_t f = lo + i;
          s[i] = f >= 0 && f < n_in ? (int16_t)g711_expand<kG711Ulaw>(src[f]) : (int16_t)0;
        }
      }
      TFP_ANY_SYNC();
      for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_sample(P, taps, s, lo, hi, n);
      return;
    }
    case kAnyMix:
    case kAnyMixMean: {
      if ((int64_t)len * 4 > lds_bytes) return;
      int32_t* __restrict__ sums = static_cast<int32_t*>(lds);
      any_stage_mix(reinterpret_cast<const int16_t*>(src), n_in, C, lo, len, sums, tid, nthr);
      if (d.form == kAnyMixMean) {
        for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_mix_mean(sums[n - lo], C);
      } else {
        for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_mix_sample(P, taps, sums, lo, hi, n, C);
      }
      return;
    }
    case kAnyWideMono: {
      if ((int64_t)len * 4 > lds_bytes) return;
      int32_t* __restrict__ s = static_cast<int32_t*>(lds);
      const int32_t* __restrict__ x = reinterpret_cast<const int32_t*>(src);
      for (int32_t i = tid; i < len; i += nthr) {
        const int64_t f = lo + i;
        s[i] = f >= 0 && f < n_in ? x[f] : 0;
      }
      TFP_ANY_SYNC();
      for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_wide_sample(P, taps, s, lo, hi, n, 1);
      return;
    }
    case kAnyWideSums:
    case kAnyWideMean: {
      if ((int64_t)len * 8 > lds_bytes) return;
      int64_t* __restrict__ sums = static_cast<int64_t*>(lds);
      any_stage_wide(reinterpret_cast<const int32_t*>(src), n_in, C, lo, len, sums, tid, nthr);
      if (d.form == kAnyWideMean) {
        for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_wide_mean(sums[n - lo], C);
      } else {
        for (int64_t n = n0 + tid; n < n1; n += nthr) y[n] = resample_wide_sample(P, taps, sums, lo, hi, n, C);
      }
      return;
    }
    default:
      return;
  }
}

#if defined(__HIPCC__) || defined(__HIP__)
// One launch for the whole call (tfp_resample_any.hip). d_data: the call's bytes, 4-byte aligned. d_clips:
// any_prepare's clips; d_plans: its plans (at least one entry allocated); d_taps: the plans' tables laid
// end to end at their taps_off. d_toff / d_tclip: resample_tiles of out_off, ntiles = toff[nclips].
// lds_bytes: AnyBatch::lds_bytes. ntiles = 0 launches nothing.
hipError_t launch_resample_any(const uint8_t* d_data, const AnyClipDev* d_clips, const AnyPlanDev* d_plans, const int16_t* d_taps,
                               const int32_t* d_toff, const int32_t* d_tclip, int32_t ntiles, int64_t lds_bytes, int16_t* d_out,
                               hipStream_t stream);
#endif

}  // namespace tfp
