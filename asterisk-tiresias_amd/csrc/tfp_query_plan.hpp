// tfp_query_plan.hpp — the offset arithmetic of a search batch, host only (no HIP, no engine):
// what the entry points work out from the caller's offsets before anything touches the device.
// A batch is n queries (or recordings) laid end to end; off[0..n] are the caller's offsets into its
// frames or its samples, and every form works on the relative frame offsets fo[0..n], fo[0] = 0.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace tfp {

constexpr int64_t kPlanHop = 256;  // TFP_HOP

// ceil(n / TFP_HOP): tfp_frame_count.
inline int64_t plan_frames(int64_t nsamples) { return nsamples <= 0 ? 0 : (nsamples + kPlanHop - 1) / kPlanHop; }

// off[0..n] never falls (equal neighbours: an empty query). n <= 0 reads nothing.
inline bool offsets_monotone(const int64_t* off, int32_t n) {
  for (int32_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}

// Frame offsets from off[0]. n <= 0 reads nothing and gives {0}.
inline std::vector<int64_t> relative_offsets(const int64_t* off, int32_t n) {
  std::vector<int64_t> fo((size_t)std::max(n, 0) + 1, 0);
  for (int32_t i = 0; i < n; i++) fo[i + 1] = off[i + 1] - off[0];
  return fo;
}

// Sample offsets to frame offsets: query i has plan_frames(its samples) frames. n <= 0 as above.
inline std::vector<int64_t> sample_frame_offsets(const int64_t* off, int32_t n) {
  std::vector<int64_t> fo((size_t)std::max(n, 0) + 1, 0);
  for (int32_t i = 0; i < n; i++) fo[i + 1] = fo[i] + plan_frames(off[i + 1] - off[i]);
  return fo;
}

// Full windows of `window` frames, `hop` apart, in nframes frames: tfp_sliding_windows.
inline int64_t plan_windows(int64_t nframes, int64_t window, int64_t hop) {
  return (nframes <= 0 || window <= 0 || hop <= 0 || nframes < window) ? 0 : (nframes - window) / hop + 1;
}

// woff[r] = the first window of recording r of frame offsets fo[0..nrec]; woff[nrec] = their total.
inline std::vector<int64_t> window_offsets(const std::vector<int64_t>& fo, int32_t nrec, int32_t window, int32_t hop) {
  std::vector<int64_t> woff((size_t)std::max(nrec, 0) + 1, 0);
  for (int32_t i = 0; i < nrec; i++) woff[i + 1] = woff[i] + plan_windows(fo[i + 1] - fo[i], window, hop);
  return woff;
}

// The windows fit the caller's room and the launches' 32-bit window index.
inline bool windows_fit(int64_t nwindows, int64_t cap_windows) { return nwindows <= cap_windows && nwindows <= INT32_MAX; }

// The census's bins for frame offsets fo[0..nq]: the longest query's frames + 1, at least 1.
inline int64_t census_need(const int64_t* fo, int32_t nq) {
  int64_t need = 1;
  for (int32_t i = 0; i < nq; i++) need = std::max<int64_t>(need, fo[i + 1] - fo[i] + 1);
  return need;
}

}  // namespace tfp
