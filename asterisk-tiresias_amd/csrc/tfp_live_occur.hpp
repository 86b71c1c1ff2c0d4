// tfp_live_occur.hpp — the host steps of tfp_live_occurrences an engine and a device group share (no
// HIP in this header): the argument rules, and step 4, the selection of occurrences among tracks already
// advanced (occur_select of tfp_occur.hpp: the batch form's thinning and output order).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/tiresias_fp.h"
#include "tfp_occur.hpp"

namespace tfp {

// One track as step 4 sees it: `clip` numbers the clip for the caller (an engine's clip id, a group's
// member), uuid orders the output's ties.
struct LiveOccTrack {
  int32_t ch, clip, shard_clip, s, windows;
  TraceOut t;
  const char* uuid;
};

// Step 4 over tracks already filtered by enrolment and scope: occur_select's thinning and order.
inline int live_occ_select(std::vector<LiveOccTrack>& tr, int32_t min_hits, tfp_occurrence* out, int64_t cap, int64_t* nocc,
                    std::string* err) {
  std::sort(tr.begin(), tr.end(), [](const LiveOccTrack& a, const LiveOccTrack& b) {
    return std::tie(a.ch, a.clip, a.s) < std::tie(b.ch, b.clip, b.s);
  });
  std::vector<OccurCand> cands(tr.size());
  std::vector<TraceOut> traces(tr.size() + 1);
  for (size_t i = 0; i < tr.size(); i++) {
    cands[i] = OccurCand{tr[i].ch, tr[i].clip, tr[i].s, tr[i].windows};
    traces[i] = tr[i].t;
  }
  // (occur_select asks for a clip's uuid by its number: the first track of that number answers)
  const std::vector<int64_t> kept = occur_select(cands, traces.data(), min_hits, [&](int32_t clip) {
    for (const LiveOccTrack& t : tr)
      if (t.clip == clip) return t.uuid;
    return "";
  });
  *nocc = (int64_t)kept.size();
  if (*nocc > cap) {
    *err = "live occurrences: " + std::to_string(*nocc) + " occurrences, room for " + std::to_string(cap);
    return TFP_E_CAPACITY;
  }
  for (size_t i = 0; i < kept.size(); i++) {
    const LiveOccTrack& k = tr[(size_t)kept[i]];
    tfp_occurrence& o = out[i];
    memset(&o, 0, sizeof o);
    o.recording = k.ch;
    o.clip_id = k.shard_clip;
    o.clip_start_frame = k.s;
    o.first_frame = k.t.seg_first;
    o.last_frame = k.t.seg_last;
    o.hits = k.t.seg_hits;
    o.diagonal_hits = k.t.hits;
    o.overlap = k.t.overlap;
    o.windows = k.windows;
    snprintf(o.uuid, sizeof o.uuid, "%s", k.uuid);
  }
  return TFP_OK;
}

// The argument rules of tfp_live_occurrences (the group's form checks the same): nullptr when they hold.
inline const char* live_occ_args(const tfp_search_params* P, const int32_t* scopes, int32_t nch, int32_t K, int32_t window,
                          int32_t max_gap, int32_t min_hits, int32_t max_tracks, const tfp_occurrence* out, int64_t cap,
                          const int64_t* nocc) {
  if (!P || !nocc || (cap > 0 && !out)) return "NULL params, out or noccurrences";
  if (cap < 0) return "cap < 0";
  if (K < 1 || K > TFP_RANK_MAX) return "k outside [1, TFP_RANK_MAX]";
  if (window < 1) return "window < 1";
  if (max_gap < 0) return "max_gap < 0";
  if (min_hits < 1) return "min_hits < 1";
  if (max_tracks < 1 || max_tracks > TFP_LIVE_TRACKS_MAX) return "max_tracks outside [1, TFP_LIVE_TRACKS_MAX]";
  for (int32_t c = 0; scopes && c < nch; c++)
    if (scopes[c] < TFP_SCOPE_ANY) return "a scope below TFP_SCOPE_ANY";
  return nullptr;
}

}  // namespace tfp
