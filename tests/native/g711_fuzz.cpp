// Stand-alone robustness run of the G.711 ingest (csrc/tfp_wav.cpp, host code only), meant to be
// built with -fsanitize=address,undefined and run as a child process: every truncation of valid
// mu-law / A-law WAVs (plain and EXTENSIBLE headers, odd data sizes, unpatched sizes), then random
// bytes and randomly damaged valid files, go through tfp_wav_decode_g711 (size query and decode)
// and tfp_g711_decode. Each buffer is an exact-size heap block, so a read past the bytes given is
// an AddressSanitizer report. Prints "g711_fuzz ok <cases>" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tiresias_fp.h"

namespace {

void put16(std::vector<uint8_t>& v, uint16_t x) {
  v.push_back((uint8_t)x);
  v.push_back((uint8_t)(x >> 8));
}
void put32(std::vector<uint8_t>& v, uint32_t x) {
  put16(v, (uint16_t)x);
  put16(v, (uint16_t)(x >> 16));
}

std::vector<uint8_t> make_wav(uint16_t tag, bool extensible, uint32_t ndata, uint32_t stated_size) {
  std::vector<uint8_t> v;
  const char* riff = "RIFF";
  v.insert(v.end(), riff, riff + 4);
  put32(v, 0);
  const char* wave = "WAVEfmt ";
  v.insert(v.end(), wave, wave + 8);
  put32(v, extensible ? 40 : 16);
  put16(v, extensible ? 0xFFFE : tag);
  put16(v, 1);
  put32(v, 8000);
  put32(v, 8000);
  put16(v, 1);
  put16(v, 8);
  if (extensible) {
    put16(v, 22);
    put16(v, 8);
    put32(v, 4);
    put16(v, tag);
    const uint8_t guid[14] = {0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xaa, 0, 0x38, 0x9b, 0x71};
    v.insert(v.end(), guid, guid + 14);
  }
  const char* data = "data";
  v.insert(v.end(), data, data + 4);
  put32(v, stated_size);
  for (uint32_t i = 0; i < ndata; i++) v.push_back((uint8_t)(i * 37 + 11));
  if (ndata & 1) v.push_back(0);
  return v;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}

long g_cases = 0;

// One input through both decoders; consistency of what they report is checked, never the verdict.
int feed(const uint8_t* src, size_t n) {
  uint8_t* bytes = new uint8_t[n ? n : 1];  // exact size: an overread is a sanitizer report
  if (n) memcpy(bytes, src, n);
  int64_t ns = -1;
  int32_t sr = 0, law = -1;
  int rc = tfp_wav_decode_g711(bytes, (int64_t)n, nullptr, 0, &ns, &sr, &law);
  g_cases++;
  if (rc == TFP_OK) {
    if (ns < 0 || (uint64_t)ns > n || (law != TFP_G711_ULAW && law != TFP_G711_ALAW) || sr <= 0) {
      fprintf(stderr, "inconsistent size query: ns %lld law %d rate %d for %zu bytes\n", (long long)ns, law, sr, n);
      return 1;
    }
    uint8_t* codes = new uint8_t[ns ? ns : 1];
    int16_t* pcm = new int16_t[ns ? ns : 1];
    int64_t ns2 = -1;
    rc = tfp_wav_decode_g711(bytes, (int64_t)n, codes, ns, &ns2, &sr, &law);
    if (rc != TFP_OK || ns2 != ns) {
      fprintf(stderr, "decode after a good size query: rc %d, %lld vs %lld samples\n", rc, (long long)ns2, (long long)ns);
      return 1;
    }
    if (tfp_g711_decode(codes, ns, law, pcm) != TFP_OK) return 1;
    if (ns > 0) {  // one short: TFP_E_CAPACITY, nothing written past the buffer
      uint8_t* small = new uint8_t[ns - 1 ? ns - 1 : 1];
      if (tfp_wav_decode_g711(bytes, (int64_t)n, small, ns - 1, &ns2, &sr, &law) != TFP_E_CAPACITY && ns - 1 > 0) {
        fprintf(stderr, "a short buffer was not TFP_E_CAPACITY\n");
        return 1;
      }
      delete[] small;
    }
    delete[] codes;
    delete[] pcm;
  } else if (rc != TFP_E_FORMAT) {
    fprintf(stderr, "unexpected code %d for %zu bytes\n", rc, n);
    return 1;
  }
  delete[] bytes;
  return 0;
}

}  // namespace

int main() {
  std::vector<std::vector<uint8_t>> valid;
  for (uint16_t tag : {(uint16_t)6, (uint16_t)7})
    for (bool ext : {false, true})
      for (uint32_t nd : {0u, 1u, 7u, 256u}) {
        valid.push_back(make_wav(tag, ext, nd, nd));
        valid.push_back(make_wav(tag, ext, nd, 0));
        valid.push_back(make_wav(tag, ext, nd, 0xFFFFFFFFu));
      }
  // every truncation of every valid file (all header truncations among them)
  for (const auto& w : valid)
    for (size_t n = 0; n <= w.size(); n++)
      if (feed(w.data(), n)) return 1;
  // random bytes, with and without a RIFF/WAVE start
  std::vector<uint8_t> buf;
  for (int it = 0; it < 4000; it++) {
    const size_t n = rnd() % 96;
    buf.resize(n);
    for (auto& b : buf) b = (uint8_t)rnd();
    if ((it & 1) && n >= 12) {
      memcpy(buf.data(), "RIFF", 4);
      memcpy(buf.data() + 8, "WAVE", 4);
      if (n >= 16 && (it & 2)) memcpy(buf.data() + 12, (it & 4) ? "fmt " : "data", 4);
    }
    if (feed(buf.data(), n)) return 1;
  }
  // valid files with a few bytes damaged
  for (int it = 0; it < 4000; it++) {
    buf = valid[rnd() % valid.size()];
    const int hits = 1 + (int)(rnd() % 3);
    for (int h = 0; h < hits && !buf.empty(); h++) buf[rnd() % buf.size()] = (uint8_t)rnd();
    if (feed(buf.data(), buf.size())) return 1;
  }
  // the code map's argument rules
  int16_t one = 0;
  const uint8_t code = 0x55;
  if (tfp_g711_decode(nullptr, 0, TFP_G711_ULAW, nullptr) != TFP_OK || tfp_g711_decode(&code, 1, 2, &one) != TFP_E_ARG ||
      tfp_g711_decode(nullptr, 1, TFP_G711_ALAW, &one) != TFP_E_ARG || tfp_g711_decode(&code, 1, TFP_G711_ALAW, &one) != TFP_OK ||
      one != -8) {
    fprintf(stderr, "tfp_g711_decode argument rules\n");
    return 1;
  }
  printf("g711_fuzz ok %ld\n", g_cases);
  return 0;
}
