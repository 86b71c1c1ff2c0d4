// check_resample_any.cpp — the host arithmetic of a mixed batch (csrc/tfp_resample_any.hpp), stand-alone:
// descriptor validation rule by rule, plan de-duplication up to and past TFP_ANY_RATES_MAX, the tile counts and
// each clip's form at the staging constants' edges, and the kernel's own tile routine (any_tile, the statements
// the device runs, here with one thread and plain adds) over every tile of a batch of every class, in exactly
// sized buffers, against tfp_resample_any_pcm. Linked with csrc/tfp_resample.cpp and csrc/tfp_wav.cpp (host
// code). Built with -fsanitize=address,undefined -fno-sanitize-recover=all and run on the CPU: any finding aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tfp_resample_any.hpp"

using namespace tfp;

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      return 1;                                                     \
    }                                                               \
  } while (0)

static uint32_t rng_state = 2024u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static tfp_audio_clip clip(int64_t off, int64_t nfr, int32_t rate, int32_t ch, int32_t kind) {
  tfp_audio_clip k;
  k.offset = off;
  k.nframes = nfr;
  k.rate_in = rate;
  k.channels = ch;
  k.kind = kind;
  k.reserved = 0;
  return k;
}

static bool prepare(const std::vector<tfp_audio_clip>& v, int64_t nbytes, int32_t rate_out, AnyBatch* B, std::string* err) {
  return any_prepare(v.data(), (int32_t)v.size(), nbytes, rate_out, resample_table, B, err);
}

static bool refused(tfp_audio_clip k, int32_t rate_out, const char* what) {
  AnyBatch B;
  std::string err;
  const std::vector<tfp_audio_clip> v = {clip(0, 4, 16000, 1, TFP_AUDIO_S16), k};
  if (prepare(v, 4096, rate_out, &B, &err)) return false;
  return err.rfind("clip 1: ", 0) == 0 && err.find(what) != std::string::npos;
}

// in_len such that the clip has exactly n_out outputs where some length gives it
static int64_t in_len_for(const ResamplePlan& P, int64_t n_out) {
  int64_t n = (n_out * P.M) / P.L;
  if (n > 0) n--;
  while (resample_count(P, n) < n_out) n++;
  return n;
}

int main() {
  // ---- the rules, one by one, and that the clip named is the offender
  CHECK(refused(clip(0, 4, 0, 1, TFP_AUDIO_S16), 8000, "bad sample rate 0"));
  CHECK(refused(clip(0, 4, 7999, 1, TFP_AUDIO_S16), 44100, "unsupported rate ratio 7999 -> 44100"));
  CHECK(refused(clip(0, 4, 16000, 0, TFP_AUDIO_S16), 8000, "unsupported channel count 0"));
  CHECK(refused(clip(0, 4, 16000, 33, TFP_AUDIO_Q31), 8000, "unsupported channel count 33"));
  CHECK(refused(clip(0, 4, 16000, 2, TFP_AUDIO_ULAW), 8000, "G.711 of 2 channels"));
  CHECK(refused(clip(0, 4, 16000, 1, 4), 8000, "unknown sample kind 4"));
  CHECK(refused(clip(1, 4, 16000, 1, TFP_AUDIO_S16), 8000, "multiple of the sample size 2"));
  CHECK(refused(clip(6, 4, 16000, 1, TFP_AUDIO_Q31), 8000, "multiple of the sample size 4"));
  CHECK(refused(clip(-4, 4, 16000, 1, TFP_AUDIO_Q31), 8000, "multiple of the sample size"));
  CHECK(refused(clip(0, -1, 16000, 1, TFP_AUDIO_S16), 8000, "negative frame count"));
  CHECK(refused(clip(4094, 2, 16000, 1, TFP_AUDIO_S16), 8000, "reaches past"));
  CHECK(refused(clip(4097, 0, 16000, 1, TFP_AUDIO_ULAW), 8000, "reaches past"));
  CHECK(refused(clip(0, INT64_MAX, 16000, 32, TFP_AUDIO_Q31), 8000, "reaches past"));
  CHECK(refused(clip(0, 4, 256000, 1, TFP_AUDIO_ALAW), 8000, "for G.711 codes"));
  {
    tfp_audio_clip k = clip(0, 4, 16000, 1, TFP_AUDIO_S16);
    k.reserved = 7;
    CHECK(refused(k, 8000, "reserved is 7"));
    AnyBatch B;
    std::string err;
    CHECK(!prepare({k}, 4096, 0, &B, &err) && err == "bad sample rate 0");
    CHECK(!any_prepare(&k, -1, 4096, 8000, resample_table, &B, &err) && err == "bad arguments");
    CHECK(!any_prepare((const tfp_audio_clip*)nullptr, 1, 4096, 8000, resample_table, &B, &err) && err == "bad arguments");
    CHECK(any_prepare((const tfp_audio_clip*)nullptr, 0, 0, 8000, resample_table, &B, &err) && B.out_off.size() == 1);
    // a clip that ends exactly at nbytes, and an empty one exactly there, are inside
    CHECK(prepare({clip(4092, 2, 16000, 1, TFP_AUDIO_S16), clip(4096, 0, 16000, 1, TFP_AUDIO_Q31)}, 4096, 8000, &B, &err));
  }
  // the Q31 range: a table whose absolute sum leaves it is refused for the Q31 clip alone
  {
    auto big = [](int32_t rin, int32_t rout, bool* bad) {
      std::shared_ptr<const ResampleTable> t = resample_table(rin, rout, bad);
      if (!t) return t;
      auto u = std::make_shared<ResampleTable>(*t);
      u->abs_sum = ((int64_t)1 << 30) / 32;
      return std::shared_ptr<const ResampleTable>(u);
    };
    AnyBatch B;
    std::string err;
    const tfp_audio_clip ok[] = {clip(0, 4, 16000, 32, TFP_AUDIO_S16), clip(0, 4, 16000, 31, TFP_AUDIO_Q31)};
    CHECK(any_prepare(ok, 2, 4096, 8000, big, &B, &err));
    const tfp_audio_clip no[] = {clip(0, 4, 16000, 32, TFP_AUDIO_S16), clip(0, 4, 16000, 32, TFP_AUDIO_Q31)};
    CHECK(!any_prepare(no, 2, 4096, 8000, big, &B, &err) && err.find("clip 1: unsupported rate ratio 16000 -> 8000 for 32 wide") == 0);
  }
  // ---- plans: one per distinct rate_in other than rate_out, in order of first use; the rate limit
  {
    std::vector<tfp_audio_clip> v;
    for (int i = 0; i < 2 * TFP_ANY_RATES_MAX; i++) v.push_back(clip(0, 8, 8000 + 8 * (i % TFP_ANY_RATES_MAX), 1, i % 2 ? TFP_AUDIO_ULAW : TFP_AUDIO_S16));
    AnyBatch B;
    std::string err;
    CHECK(prepare(v, 64, 8000, &B, &err));
    CHECK((int)B.plans.size() == TFP_ANY_RATES_MAX - 1 && B.tables.size() == B.plans.size());
    int64_t off = 0;
    for (size_t i = 0; i < B.plans.size(); i++) {
      CHECK(B.plans[i].taps_off == off && B.tables[i]->plan.L == B.plans[i].P.L && B.tables[i]->plan.M == B.plans[i].P.M);
      off += (int64_t)B.tables[i]->taps.size();
    }
    CHECK(off == B.taps_total);
    for (int i = 0; i < 2 * TFP_ANY_RATES_MAX; i++) CHECK(B.clips[(size_t)i].plan == i % TFP_ANY_RATES_MAX - 1);
    v.push_back(clip(0, 8, 8000 + 8 * TFP_ANY_RATES_MAX, 1, TFP_AUDIO_S16));
    CHECK(!prepare(v, 64, 8000, &B, &err) && err.find("clip 128: more than 64 distinct input rates") == 0);
  }
  // ---- the form at the staging constants' edges (spans, not pairs: the rule itself)
  {
    int64_t lds = -1;
    CHECK(any_form(TFP_AUDIO_S16, 1, false, kRsSpanMax, &lds) == kAnyMono && lds == 2 * (int64_t)kRsSpanMax);
    CHECK(any_form(TFP_AUDIO_S16, 1, false, kRsSpanMax + 1, &lds) == kAnyMonoGlobal && lds == 0);
    CHECK(any_form(TFP_AUDIO_ULAW, 1, false, kRsSpanMax, &lds) == kAnyG711 && any_form(TFP_AUDIO_ALAW, 1, false, kRsSpanMax + 1, &lds) == kAnyForms);
    CHECK(any_form(TFP_AUDIO_S16, 2, false, kRsMixSpanMax, &lds) == kAnyMix && lds == 4 * (int64_t)kRsMixSpanMax);
    CHECK(any_form(TFP_AUDIO_S16, 32, false, kRsMixSpanMax + 1, &lds) == kAnyMixGlobal && lds == 0);
    CHECK(any_form(TFP_AUDIO_Q31, 1, false, kRsMixSpanMax, &lds) == kAnyWideMono && lds == 4 * (int64_t)kRsMixSpanMax);
    CHECK(any_form(TFP_AUDIO_Q31, 1, false, kRsMixSpanMax + 1, &lds) == kAnyWideGlobal);
    CHECK(any_form(TFP_AUDIO_Q31, 2, false, kRsWideSpanMax, &lds) == kAnyWideSums && lds == 8 * (int64_t)kRsWideSpanMax);
    CHECK(any_form(TFP_AUDIO_Q31, 2, false, kRsWideSpanMax + 1, &lds) == kAnyWideGlobal && lds == 0);
    CHECK(any_form(TFP_AUDIO_S16, 1, true, 0, &lds) == kAnyCopy && any_form(TFP_AUDIO_ULAW, 1, true, 0, &lds) == kAnyExpand);
    CHECK(any_form(TFP_AUDIO_Q31, 1, true, 0, &lds) == kAnyWideRound && lds == 0);
    CHECK(any_form(TFP_AUDIO_S16, 3, true, 0, &lds) == kAnyMixMean && lds == 4 * (kRsTile + 1));
    CHECK(any_form(TFP_AUDIO_Q31, 3, true, 0, &lds) == kAnyWideMean && lds == 8 * (kRsTile + 1));
    for (int f = 0; f < kAnyForms; f++) CHECK(any_form_plain(f) + any_form_staged(f) + any_form_global(f) == 1);
  }
  // ---- every tile of a batch of every class through the kernel's tile routine, against the host map
  struct Class {
    int32_t kind, ch, rate;
    int32_t form;
  };
  const Class classes[] = {
      {TFP_AUDIO_S16, 1, 8000, kAnyCopy},      {TFP_AUDIO_S16, 1, 16000, kAnyMono},      {TFP_AUDIO_S16, 2, 44100, kAnyMix},
      {TFP_AUDIO_S16, 32, 16000, kAnyMix},     {TFP_AUDIO_Q31, 1, 48000, kAnyWideMono},  {TFP_AUDIO_Q31, 2, 44100, kAnyWideSums},
      {TFP_AUDIO_Q31, 2, 96000, kAnyWideGlobal}, {TFP_AUDIO_Q31, 1, 192000, kAnyWideGlobal}, {TFP_AUDIO_ULAW, 1, 16000, kAnyG711},
      {TFP_AUDIO_ALAW, 1, 8000, kAnyExpand},   {TFP_AUDIO_S16, 3, 8000, kAnyMixMean},    {TFP_AUDIO_Q31, 1, 8000, kAnyWideRound},
      {TFP_AUDIO_Q31, 5, 8000, kAnyWideMean},  {TFP_AUDIO_S16, 1, 256000, kAnyMonoGlobal}, {TFP_AUDIO_S16, 2, 192000, kAnyMixGlobal},
      {TFP_AUDIO_ALAW, 1, 11025, kAnyG711},    {TFP_AUDIO_S16, 3, 11025, kAnyMix}};
  const int32_t rate_out = 8000;
  const int64_t outs[] = {0, 1, kRsTile - 1, kRsTile, kRsTile + 1, 2 * kRsTile + 37};
  // the bytes: clips laid end to end in a vector of exactly their size (a read past the end is a finding), odd
  // G.711 lengths leaving the next S16 / Q31 clip to be aligned by padding of its own
  std::vector<uint8_t> bytes;
  std::vector<tfp_audio_clip> v;
  int64_t want_staged = 0, want_global = 0, want_plain = 0;
  for (int64_t no : outs) {
    for (const Class& c : classes) {
      ResamplePlan P{1, 1, 0, 1};
      bool bad = false;
      if (c.rate != rate_out) CHECK(resample_plan(c.rate, rate_out, &P, &bad));
      const int64_t nfr = c.rate == rate_out ? no : in_len_for(P, no);
      CHECK((c.rate == rate_out ? nfr : resample_count(P, nfr)) == no);
      const int32_t ss = any_sample_size(c.kind);
      while (bytes.size() % (size_t)ss) bytes.push_back(0xA5);
      v.push_back(clip((int64_t)bytes.size(), nfr, c.rate, c.ch, c.kind));
      for (int64_t i = 0; i < nfr * c.ch * ss; i++) bytes.push_back((uint8_t)rnd());
      const int64_t nt = (no + kRsTile - 1) / kRsTile;
      (any_form_plain(c.form) ? want_plain : any_form_staged(c.form) ? want_staged : want_global) += nt;
    }
    const tfp_audio_clip twin = v[v.size() - 3];
    v.push_back(twin);  // a second descriptor naming the same bytes
    const int32_t f = classes[sizeof(classes) / sizeof(classes[0]) - 3].form;
    (any_form_plain(f) ? want_plain : any_form_staged(f) ? want_staged : want_global) += (no + kRsTile - 1) / kRsTile;
  }
  // any_tile reads Q31 and word pairs at their natural alignment from the start of the bytes
  std::vector<uint32_t> aligned((bytes.size() + 3) / 4);
  uint8_t* data = reinterpret_cast<uint8_t*>(aligned.data());
  if (!bytes.empty()) std::memcpy(data, bytes.data(), bytes.size());
  AnyBatch B;
  std::string err;
  CHECK(prepare(v, (int64_t)bytes.size(), rate_out, &B, &err));
  CHECK(B.tiles_staged == want_staged && B.tiles_global == want_global && B.tiles_plain == want_plain);
  CHECK(B.lds_bytes > 0 && B.lds_bytes <= 61440);
  {
    size_t i = 0;
    for (size_t r = 0; r < sizeof(outs) / sizeof(outs[0]); r++) {
      for (const Class& c : classes) CHECK(B.clips[i++].form == c.form);
      i++;
    }
  }
  std::vector<int16_t> taps((size_t)B.taps_total);
  for (size_t i = 0; i < B.plans.size(); i++)
    std::copy(B.tables[i]->taps.begin(), B.tables[i]->taps.end(), taps.begin() + B.plans[i].taps_off);
  std::vector<int32_t> toff, tclip;
  resample_tiles(B.out_off.data(), (int32_t)v.size(), &toff, &tclip);
  CHECK((int64_t)tclip.size() == want_staged + want_global + want_plain);
  std::vector<int16_t> out((size_t)B.out_off.back(), (int16_t)0x7e7e);
  std::vector<int64_t> lds((size_t)(B.lds_bytes + 7) / 8);  // exactly the launch's size
  for (size_t t = 0; t < tclip.size(); t++) {
    const int32_t c = tclip[t];
    const AnyClipDev& d = B.clips[(size_t)c];
    const ResamplePlan P = d.plan >= 0 ? B.plans[(size_t)d.plan].P : ResamplePlan{1, 1, 0, 1};
    const int16_t* tp = d.plan >= 0 ? taps.data() + B.plans[(size_t)d.plan].taps_off : nullptr;
    std::fill(lds.begin(), lds.end(), (int64_t)0x5a5a5a5a5a5a5a5a);  // a tile relies on nothing left in LDS
    any_tile(data, d, P, tp, (int64_t)((int32_t)t - toff[(size_t)c]), lds.data(), B.lds_bytes, out.data(), 0, 1);
  }
  for (size_t c = 0; c < v.size(); c++) {
    int64_t n = -1;
    CHECK(tfp_resample_any_pcm(data, &v[c], rate_out, nullptr, 0, &n) == TFP_OK && n == B.clips[c].n_out);
    std::vector<int16_t> y((size_t)n);
    CHECK(tfp_resample_any_pcm(data, &v[c], rate_out, y.data(), n, &n) == TFP_OK);
    CHECK(n == 0 || std::memcmp(y.data(), out.data() + B.out_off[c], sizeof(int16_t) * (size_t)n) == 0);
  }
  // a launch whose LDS were sized too small writes nothing instead of past its buffer
  {
    const AnyClipDev& d = B.clips[1 + 2 * (sizeof(classes) / sizeof(classes[0]) + 1)];  // int16 mono 16000, kRsTile - 1 outputs
    CHECK(d.form == kAnyMono && d.n_out == kRsTile - 1);
    std::vector<int16_t> o((size_t)B.out_off.back(), (int16_t)0x1111);
    std::vector<int64_t> small(8);
    any_tile(data, d, B.plans[(size_t)d.plan].P, taps.data() + B.plans[(size_t)d.plan].taps_off, 0, small.data(), 64, o.data(), 0, 1);
    for (int16_t s : o) CHECK(s == 0x1111);
  }
  std::printf("OK\n");
  return 0;
}
