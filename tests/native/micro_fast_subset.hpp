// The float bit patterns every run of check_micro_fast (.cpp on the host, .hip on the GPU) checks
// besides its strided walk: the special inputs, the neighbours of 1.0 (10 log10|c| next to 0), and
// the patterns of a list file (tests/golden/micro_fast_boundary.txt: the floats whose 10 log10|c|
// lies nearest a half-micro boundary, as the exhaustive host run printed them).
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

inline std::vector<uint32_t> micro_fast_extras(const char* list) {
  std::vector<uint32_t> v;
  const uint32_t pos[] = {
      0x00000000u,                            // 0
      0x00000001u, 0x00000002u, 0x007fffffu,  // smallest and largest subnormals
      0x00800000u, 0x00800001u,               // FLT_MIN
      0x7f7fffffu, 0x7f7ffffeu,               // FLT_MAX
      0x7f800000u,                            // inf
      0x7f800001u, 0x7fc00000u, 0x7fffffffu,  // NaNs
  };
  for (uint32_t p : pos) {
    v.push_back(p);
    v.push_back(p | 0x80000000u);
  }
  for (int32_t d = -64; d <= 64; d++) {  // 1.0 and its 64 neighbours on each side, both signs
    v.push_back(0x3f800000u + (uint32_t)d);
    v.push_back((0x3f800000u + (uint32_t)d) | 0x80000000u);
  }
  for (uint32_t i = 0; i < 128; i++) {  // both ends of every table bucket, at three exponents
    for (uint32_t e : {1u, 127u, 254u}) {
      v.push_back((e << 23) | (i << 16));
      v.push_back((e << 23) | (i << 16) | 0xffffu);
    }
  }
  if (list) {
    FILE* f = fopen(list, "r");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", list);
      return {};
    }
    unsigned u;
    while (fscanf(f, "%x", &u) == 1) v.push_back((uint32_t)u);
    fclose(f);
  }
  return v;
}
