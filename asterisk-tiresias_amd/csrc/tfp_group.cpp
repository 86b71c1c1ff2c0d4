// tfp_group.cpp — several engines (one per GPU of the node) behind one index and one search
// (include/tiresias_fp.h, "device groups").
//
// The reference's fp_search_fingerprint_info is one SQL pipeline over the whole audio_fingerprint
// table (fp_handler.c:287-374). Here the enrolled clips are sharded over the engines — a clip is
// never split, because the per-frame GROUP BY audio_uuid (:353) is not additive over a split clip —
// and every search runs on all shards in parallel, one worker thread per engine. Each shard's
// per-query winner is the key (count << 32 | global uuid rank): the engines carry the group-wide
// uuid ranks as their tie-break keys (tfp_index_set_tiebreak), so the greatest key over the shards
// is the reference's winner (count(*) DESC, ties to the greatest audio_uuid, :367-374) and the
// combine is an integer max on the host (the results leave the GPUs for the caller anyway).
//
// Batches of host PCM large enough to be throughput-bound are query-sharded: shard s fingerprints
// queries [s·nq/N, (s+1)·nq/N) on its GPU, the frame values are exchanged device to device
// (hipMemcpyPeerAsync over xGMI; a plain device copy when a device repeats), and every shard
// searches the whole batch against its clips (tfp_search_q_device). Smaller batches (batch-1
// latency) are fingerprinted by every shard itself: no exchange on the latency path. Stream
// channels are split over the shards (channel c on shard c mod N): each shard keeps its channels'
// rings and fingerprints their full windows, the windows' frame values are exchanged as for a
// query-sharded batch, and every shard matches all of them against its clips. (TFP_GROUP_STREAM=
// replicate: every shard runs every channel, no exchange; the round-3 form.)
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/tiresias_fp.h"
#include "tfp_coalesce.hpp"
#include "tfp_g711.hpp"
#include "tfp_resample.hpp"
#include "tfp_resample_any.hpp"
#include "tfp_internal.hpp"
#include "tfp_kernels.hpp"
#include "tfp_live_occur.hpp"
#include "tfp_live_plan.hpp"
#include "tfp_live_rate.hpp"
#include "tfp_occur.hpp"
#include "tfp_rank_merge.hpp"
#include "tfp_shardpool.hpp"

namespace {

struct Member {
  std::string uuid;
  int32_t shard;
  int32_t id;        // the engine's clip id
  int32_t key = -1;  // its tie-break key (ordered like the uuids, sparse; -1 until assigned)
};

// Device buffers of the query-sharded batch path, one set per shard.
struct ShardBufs {
  void* pcm = nullptr;      // this shard's queries (int16)
  void* codes = nullptr;    // ... as G.711 codes, expanded into pcm (tfp_group_search_g711_batch)
  void* micro = nullptr;    // their stored values (unused by the search, written by the kernel)
  void* q = nullptr;        // the whole batch's frame values (2 doubles per frame)
  void* keys = nullptr;     // per-query keys
  void* sfp = nullptr;      // split streams: this shard's channels' window values of the tick
  size_t b_pcm = 0, b_codes = 0, b_micro = 0, b_q = 0, b_keys = 0, b_sfp = 0;
  hipStream_t stream = nullptr;
  hipEvent_t fp_done = nullptr;
  tfp_plan* plan = nullptr;  // this shard's share of the last batch shape (k queries of qn samples)
  int64_t plan_k = -1, plan_qn = -1;
  int32_t plan_sr = 0;
};

hipError_t grow(void** p, size_t* have, size_t want) {
  if (want <= *have) return hipSuccess;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  hipError_t e = hipMalloc(p, want);
  if (e == hipSuccess) *have = want;
  return e;
}

}  // namespace

struct tfp_group {
  std::vector<tfp_engine*> eng;
  std::vector<int32_t> dev;
  tfp::ShardPool* pool = nullptr;
  std::recursive_mutex mu;
  tfp::ErrorSlot err;  // last-error messages (tfp_internal.hpp)
  std::unordered_map<std::string, int32_t> where;     // uuid -> index in members
  std::vector<Member> members;                         // every clip ever added (uuid "" once removed)
  std::vector<std::vector<int32_t>> id2member;         // [shard][engine clip id] -> member index (-1 removed)
  std::vector<int64_t> rows;                           // live rows per shard (placement)
  std::vector<int32_t> by_uuid;                        // live members in uuid order (global ranks)
  // Tie-break keys (round 6): every live member's key orders like its uuid with gaps between
  // neighbours, so a new clip takes the middle of its neighbours' gap and no other key changes; the
  // shards then get the new clips' keys only (tfp_index_update_tiebreak), an enrolment stays
  // O(new clips). A gap of 1 (or a large batch) respaces every key evenly over [0, 2^31) instead.
  std::unordered_map<int32_t, int32_t> key2member;     // key -> member
  std::vector<size_t> pushed;                          // per shard: engine clip ids whose keys it has
  bool keys_full = true;                               // respace every key and send every shard all its keys
  bool ranks_dirty = true;                             // some shard lacks keys (keys_full or new clip ids)
  int64_t n_respaces = 0, n_partial_pushes = 0;        // full key refreshes / new-clip-only pushes
  std::vector<ShardBufs> bufs;
  tfp::Coalescer coal;   // concurrent channel searches share one batch per shard (tfp_coalesce.hpp)
  bool coalesce = true;  // TFP_COALESCE=0: every call alone
  // ordered pairs of distinct devices; of them, peer-accessible; of those, peer access enabled
  // (tfp_group_peer_stats: the 8-GPU bench line reports them)
  int32_t peer_pairs = 0, peer_can = 0, peer_enabled = 0;
  ~tfp_group() {
    delete pool;
    for (size_t s = 0; s < bufs.size(); s++) {
      (void)hipSetDevice(dev[s]);
      for (void* p : {bufs[s].pcm, bufs[s].codes, bufs[s].micro, bufs[s].q, bufs[s].keys, bufs[s].sfp})
        if (p) (void)hipFree(p);
      if (bufs[s].fp_done) (void)hipEventDestroy(bufs[s].fp_done);
      tfp_plan_destroy(bufs[s].plan);
      if (bufs[s].stream) (void)hipStreamDestroy(bufs[s].stream);
    }
    for (auto* e : eng) tfp_engine_destroy(e);
  }
};

struct tfp_group_stream {
  tfp_group* g = nullptr;
  std::vector<tfp_stream*> st;  // one per shard: every channel (replicated) or its own (split; null if none)
  int32_t nch = 0;
  int64_t W = 0;
  bool split = false;
  std::vector<std::vector<int32_t>> chans;  // split: shard -> its channels (c mod N == s), ascending
  std::vector<std::vector<int16_t>> tick;   // split: the shard's rows of the tick
  std::vector<std::vector<int32_t>> act;    // split: the shard's windows of the tick (local channel indices)
  std::vector<int32_t> nact;
  std::vector<std::vector<unsigned long long>> keys;
  std::vector<std::vector<tfp_result>> res;
};

namespace {

int gfail(tfp_group* g, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int gfail(tfp_group* g, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (g) g->err.note(g, buf);
  return code;
}

// The error of shard s's failed call made on this thread, into the group's message.
int shard_fail(tfp_group* g, int rc, int s) {
  return gfail(g, rc, "shard %d (device %d): %s", s, g->dev[s], tfp_engine_last_error(g->eng[s]));
}

// f(s) on every shard in parallel; a failure becomes the group's error with the failing shard's
// message, read on the thread that ran that shard's call (the engine's per-thread slot).
int run_all(tfp_group* g, const std::function<int(int)>& f) {
  const int n = (int)g->eng.size();
  std::vector<std::string> why(n);
  int bad = 0;
  const int rc = g->pool->run(
      [&](int s) {
        tfp_internal_engine_clear_error(g->eng[s]);
        g->err.clear_own();  // (this pool thread's: f may note a group-level failure, a peer copy's)
        const int r = f(s);
        if (r) {  // the message this call recorded on this thread: the shard engine's, else the group's
          const char* m = tfp_internal_engine_own_error(g->eng[s]);
          if (!m) m = g->err.own();
          why[s] = m ? m : r == TFP_E_NOMEM ? "out of memory" : "device call failed";
        }
        return r;
      },
      &bad);
  return rc ? gfail(g, rc, "shard %d (device %d): %s", bad, g->dev[bad], why[bad].c_str()) : TFP_OK;
}

constexpr int64_t kKeySpan = int64_t(1) << 31;  // tie-break keys lie in [0, 2^31)

// Every shard's tie-break keys (before any search after a change): after a respace, all of each
// shard's clips' keys; otherwise only the clip ids enrolled since (tfp_index_update_tiebreak).
int refresh_ranks(tfp_group* g) {
  if (!g->ranks_dirty) return TFP_OK;
  const int n = (int)g->eng.size();
  const bool full = g->keys_full;
  if (full) {  // even spacing over [0, 2^31) in uuid order
    const int64_t N = (int64_t)g->by_uuid.size(), step = kKeySpan / (N + 1);
    g->key2member.clear();
    g->key2member.reserve(N);
    for (int64_t r = 0; r < N; r++) {
      Member& m = g->members[g->by_uuid[r]];
      m.key = (int32_t)((r + 1) * step);
      g->key2member[m.key] = g->by_uuid[r];
    }
  }
  g->pushed.resize(n, 0);
  auto key_of_id = [&](int s, size_t id) {
    const int32_t mi = g->id2member[s][id];
    return mi < 0 ? -1 : g->members[mi].key;
  };
  const int rc = run_all(g, [&](int s) -> int {
    const size_t have = g->id2member[s].size(), from = full ? 0 : std::min(g->pushed[s], have);
    if (!full && from == have) return TFP_OK;
    std::vector<int32_t> keys(std::max<size_t>(have - from, 1));
    for (size_t id = from; id < have; id++) keys[id - from] = key_of_id(s, id);
    const int r = full ? tfp_index_set_tiebreak(g->eng[s], keys.data(), (int32_t)have)
                       : tfp_index_update_tiebreak(g->eng[s], (int32_t)from, keys.data(), (int32_t)(have - from));
    if (!r) g->pushed[s] = have;
    return r;
  });
  if (rc) {
    g->keys_full = true;  // (the next refresh sends everything again)
    return rc;
  }
  (full ? g->n_respaces : g->n_partial_pushes)++;
  g->keys_full = false;
  g->ranks_dirty = false;
  return TFP_OK;
}

bool uuid_less(const tfp_group* g, int32_t a, int32_t b) { return g->members[a].uuid < g->members[b].uuid; }

// A member into the uuid order; its key: the middle of its neighbours' gap (keys_full: the next
// refresh respaces every key instead).
void insert_live(tfp_group* g, int32_t mi) {
  auto it = std::lower_bound(g->by_uuid.begin(), g->by_uuid.end(), mi,
                             [&](int32_t a, int32_t b) { return uuid_less(g, a, b); });
  const size_t pos = (size_t)(it - g->by_uuid.begin());
  g->by_uuid.insert(it, mi);
  g->ranks_dirty = true;
  if (g->keys_full) return;
  const int64_t lo = pos > 0 ? g->members[g->by_uuid[pos - 1]].key : -1;
  const int64_t hi = pos + 1 < g->by_uuid.size() ? g->members[g->by_uuid[pos + 1]].key : kKeySpan;
  if (hi - lo < 2) {
    g->keys_full = true;
    return;
  }
  Member& m = g->members[mi];
  m.key = (int32_t)(lo + (hi - lo) / 2);
  g->key2member[m.key] = mi;
}

void erase_live(tfp_group* g, int32_t mi) {
  auto it = std::lower_bound(g->by_uuid.begin(), g->by_uuid.end(), mi,
                             [&](int32_t a, int32_t b) { return uuid_less(g, a, b); });
  if (it != g->by_uuid.end() && *it == mi) g->by_uuid.erase(it);
  Member& m = g->members[mi];
  if (m.key >= 0) {
    auto k = g->key2member.find(m.key);
    if (k != g->key2member.end() && k->second == mi) g->key2member.erase(k);
    m.key = -1;
  }
  // (no other key changes: the shards' keys stay valid, the removed clip's is never read again)
}

int32_t lightest(const tfp_group* g) {
  return (int32_t)(std::min_element(g->rows.begin(), g->rows.end()) - g->rows.begin());
}

// A shard's result -> its key (count << 32 | global rank); 0 = no hit.
unsigned long long key_of(const tfp_group* g, int s, const tfp_result& r) {
  if (!r.found || r.clip_id < 0 || (size_t)r.clip_id >= g->id2member[s].size()) return 0ull;
  const int32_t mi = g->id2member[s][r.clip_id];
  if (mi < 0 || g->members[mi].key < 0) return 0ull;
  return ((unsigned long long)(uint32_t)r.match_count << 32) | (uint32_t)g->members[mi].key;
}

// Per query, the greatest key over the shards' results -> the group's result.
void combine(tfp_group* g, const std::vector<std::vector<tfp_result>>& res, int32_t nq, tfp_result* out) {
  for (int32_t i = 0; i < nq; i++) {
    int best_s = -1;
    unsigned long long best = 0ull;
    for (size_t s = 0; s < res.size(); s++) {
      const unsigned long long k = key_of(g, (int)s, res[s][i]);
      if (k > best) best = k, best_s = (int)s;
    }
    out[i] = best_s >= 0 ? res[best_s][i] : res[0][i];
    if (best_s >= 0) out[i].clip_id = best_s;  // the shard holding the winner
    else out[i].found = 0, out[i].match_count = 0, out[i].clip_id = -1, out[i].uuid[0] = 0;
  }
}

// Global key -> result (uuid, count) for the query-sharded path.
void fill_from_key(const tfp_group* g, unsigned long long k, int32_t frame_count, tfp_result* r) {
  memset(r, 0, sizeof *r);
  r->frame_count = frame_count;
  r->clip_id = -1;
  if (!k) return;
  const auto it = g->key2member.find((int32_t)(uint32_t)(k & 0xffffffffu));
  if (it == g->key2member.end()) return;
  const Member& m = g->members[it->second];
  r->found = 1;
  r->match_count = (int32_t)(k >> 32);
  r->clip_id = m.shard;
  snprintf(r->uuid, sizeof r->uuid, "%s", m.uuid.c_str());
}

bool valid_params(const tfp_search_params* P) { return P && P->coefs >= 1 && P->coefs <= 2; }

int add_members(tfp_group* g, int32_t s, int32_t n, const char* const* uuids) {
  // (a large batch: one even respace at the next refresh instead of many halved gaps)
  if (n > 64) g->keys_full = true;
  // the engine assigns clip ids in order of addition (tfp_index_add / _add_batch)
  for (int32_t c = 0; c < n; c++) {
    const int32_t mi = (int32_t)g->members.size();
    g->members.push_back(Member{uuids[c], s, (int32_t)g->id2member[s].size()});
    g->id2member[s].push_back(mi);
    g->where[uuids[c]] = mi;
    insert_live(g, mi);
  }
  return TFP_OK;
}

// Query-sharded batch over host int16 PCM of equal-length queries: shard s fingerprints its share,
// the frame values are exchanged, every shard searches the whole batch. law >= 0: pcm holds G.711
// codes of that law instead; a shard copies its share at one byte per sample and expands it on its
// device in front of the same fingerprint launch.
int search_sharded(tfp_group* g, const void* pcm, int32_t law, const int64_t* offsets, int32_t nq, int32_t sr,
                   const tfp_search_params* P, tfp_result* out) {
  const int n = (int)g->eng.size();
  const int64_t qn = offsets[1] - offsets[0];
  const int64_t nfq = tfp_frame_count(qn), nf = nfq * nq;
  std::vector<int32_t> share(n + 1);
  for (int s = 0; s <= n; s++) share[s] = (int32_t)(((int64_t)nq * s) / n);
  std::vector<int64_t> qoff(nq + 1);
  for (int32_t i = 0; i <= nq; i++) qoff[i] = nfq * i;
  std::vector<std::vector<unsigned long long>> keys(n, std::vector<unsigned long long>(nq));
  // 1: each shard fingerprints its queries into its part of its own q buffer
  int rc = run_all(g, [&](int s) -> int {
    ShardBufs& b = g->bufs[s];
    if (hipSetDevice(g->dev[s]) != hipSuccess) return TFP_E_HIP;
    if (!b.stream && hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking) != hipSuccess) return TFP_E_HIP;
    if (!b.fp_done && hipEventCreateWithFlags(&b.fp_done, hipEventDisableTiming) != hipSuccess) return TFP_E_HIP;
    const int32_t k = share[s + 1] - share[s];
    if (grow(&b.pcm, &b.b_pcm, sizeof(int16_t) * (size_t)(k * qn + 1)) != hipSuccess ||
        grow(&b.micro, &b.b_micro, sizeof(int32_t) * 2 * (size_t)(k * nfq + 1)) != hipSuccess ||
        grow(&b.q, &b.b_q, sizeof(double) * 2 * (size_t)(nf + 1)) != hipSuccess ||
        grow(&b.keys, &b.b_keys, sizeof(unsigned long long) * (size_t)(nq + 1)) != hipSuccess)
      return TFP_E_NOMEM;
    if (!k) return hipEventRecord(b.fp_done, b.stream) == hipSuccess ? TFP_OK : TFP_E_HIP;
    if (law < 0) {
      // (offsets index the caller's buffer, as in every other form: query i lies at pcm + offsets[i])
      if (hipMemcpyAsync(b.pcm, (const int16_t*)pcm + offsets[share[s]], sizeof(int16_t) * (size_t)(k * qn),
                         hipMemcpyHostToDevice, b.stream) != hipSuccess)
        return TFP_E_HIP;
    } else {
      if (grow(&b.codes, &b.b_codes, (size_t)(k * qn + 1)) != hipSuccess) return TFP_E_NOMEM;
      if (hipMemcpyAsync(b.codes, (const uint8_t*)pcm + offsets[share[s]], (size_t)(k * qn), hipMemcpyHostToDevice,
                         b.stream) != hipSuccess)
        return TFP_E_HIP;
      const int r = tfp_internal_g711_expand_device(g->eng[s], (const uint8_t*)b.codes, k * qn, law, (int16_t*)b.pcm, b.stream);
      if (r) return r;
    }
    if (!b.plan || b.plan_k != k || b.plan_qn != qn || b.plan_sr != sr) {
      std::vector<int64_t> off(k + 1);
      for (int32_t i = 0; i <= k; i++) off[i] = qn * i;
      tfp_plan_destroy(b.plan);
      b.plan = nullptr;
      const int r = tfp_plan_create(g->eng[s], off.data(), k, sr, &b.plan);
      if (r) return r;
      b.plan_k = k, b.plan_qn = qn, b.plan_sr = sr;
    }
    const int r = tfp_fingerprint_device(g->eng[s], b.plan, (const int16_t*)b.pcm, (int32_t*)b.micro,
                                         (double*)b.q + 2 * nfq * share[s], b.stream);
    if (r) return r;
    if (hipEventRecord(b.fp_done, b.stream) != hipSuccess || hipStreamSynchronize(b.stream) != hipSuccess)
      return TFP_E_HIP;
    return TFP_OK;
  });
  if (rc) return rc;
  // 2: every shard pulls the other shards' frame values, searches the batch, keys to the host
  rc = run_all(g, [&](int s) -> int {
    ShardBufs& b = g->bufs[s];
    if (hipSetDevice(g->dev[s]) != hipSuccess) return TFP_E_HIP;
    for (int o = 0; o < n; o++) {
      const int32_t k = share[o + 1] - share[o];
      if (o == s || !k) continue;
      const size_t off = sizeof(double) * 2 * (size_t)(nfq * share[o]), bytes = sizeof(double) * 2 * (size_t)(nfq * k);
      if (const hipError_t pe = hipMemcpyPeerAsync((char*)b.q + off, g->dev[s], (const char*)g->bufs[o].q + off, g->dev[o],
                                                   bytes, b.stream);
          pe != hipSuccess)
        return gfail(g, TFP_E_HIP, "frame values of shard %d (device %d) to shard %d (device %d): hipMemcpyPeerAsync: %s", o,
                     g->dev[o], s, g->dev[s], hipGetErrorString(pe));
    }
    int r = tfp_search_q_device(g->eng[s], (const double*)b.q, qoff.data(), nq, P, (uint64_t*)b.keys, b.stream);
    if (r) return r;
    if (hipMemcpyAsync(keys[s].data(), b.keys, sizeof(unsigned long long) * nq, hipMemcpyDeviceToHost, b.stream) !=
            hipSuccess ||
        hipStreamSynchronize(b.stream) != hipSuccess)
      return TFP_E_HIP;
    return TFP_OK;
  });
  if (rc) return rc;
  for (int32_t i = 0; i < nq; i++) {
    unsigned long long k = 0ull;
    for (int s = 0; s < n; s++) k = std::max(k, keys[s][i]);
    fill_from_key(g, k, (int32_t)nfq, &out[i]);
  }
  return TFP_OK;
}

}  // namespace

extern "C" {

int tfp_group_create(const int32_t* devices, int32_t n, tfp_group** out) {
  if (!devices || n <= 0 || !out) return TFP_E_ARG;
  *out = nullptr;
  tfp_group* g = new tfp_group();
  for (int32_t s = 0; s < n; s++) {
    tfp_engine* e = nullptr;
    const int rc = tfp_engine_create(devices[s], &e);
    if (rc) {
      delete g;
      return rc;
    }
    g->eng.push_back(e);
    g->dev.push_back(devices[s]);
  }
  // peer access between the distinct devices (xGMI), for the query-sharded batches and split
  // streams. Counted per ordered pair (tfp_group_peer_stats); a pair without it still copies
  // (hipMemcpyPeerAsync stages through the host), and a failed copy fails the call loudly.
  for (int32_t a = 0; a < n; a++)
    for (int32_t b = 0; b < n; b++) {
      if (devices[a] == devices[b]) continue;
      bool seen = false;  // (a repeated pair of devices counts once)
      for (int32_t a2 = 0; a2 < n && !seen; a2++)
        for (int32_t b2 = 0; b2 < n && !seen; b2++)
          seen = (a2 < a || (a2 == a && b2 < b)) && devices[a2] == devices[a] && devices[b2] == devices[b];
      if (seen) continue;
      g->peer_pairs++;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) == hipSuccess && can && hipSetDevice(devices[a]) == hipSuccess) {
        g->peer_can++;
        const hipError_t e = hipDeviceEnablePeerAccess(devices[b], 0);
        if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) g->peer_enabled++;
        if (e != hipSuccess) (void)hipGetLastError();
      }
    }
  g->id2member.assign(n, {});
  g->rows.assign(n, 0);
  g->bufs.resize(n);
  g->pool = new tfp::ShardPool(n);
  if (const char* v = tfp::op_env("TFP_COALESCE")) g->coalesce = atoi(v) != 0;
  *out = g;
  return TFP_OK;
}

void tfp_group_destroy(tfp_group* g) { delete g; }

int tfp_group_peer_stats(const tfp_group* g, int32_t* pairs, int32_t* can_access, int32_t* enabled) {
  if (!g) return TFP_E_ARG;
  if (pairs) *pairs = g->peer_pairs;
  if (can_access) *can_access = g->peer_can;
  if (enabled) *enabled = g->peer_enabled;
  return TFP_OK;
}

int tfp_group_tiebreak_stats(tfp_group* g, int64_t* respaces, int64_t* partial_pushes, int64_t* shard_full_key_updates) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  if (respaces) *respaces = g->n_respaces;
  if (partial_pushes) *partial_pushes = g->n_partial_pushes;
  if (shard_full_key_updates) {
    int64_t t = 0;
    for (tfp_engine* e : g->eng) t += tfp_internal_delta_main_keys(e);
    *shard_full_key_updates = t;
  }
  return TFP_OK;
}

int32_t tfp_group_size(const tfp_group* g) { return g ? (int32_t)g->eng.size() : 0; }

const char* tfp_group_last_error(const tfp_group* g) { return g ? const_cast<tfp_group*>(g)->err.read(g) : ""; }

tfp_engine* tfp_group_engine(tfp_group* g, int32_t shard) {
  return g && shard >= 0 && shard < (int32_t)g->eng.size() ? g->eng[shard] : nullptr;
}

namespace {
// law >= 0: x holds G.711 codes of that law (each shard expands its clips on its device).
int group_fingerprint(tfp_group* g, const void* x, bool f32, const int64_t* offsets, int32_t nclips, int32_t sr,
                      tfp_frame* out, int64_t cap, int64_t* nframes, int32_t law = -1) {
  if (!g || !offsets || nclips < 0 || !nframes) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int n = (int)g->eng.size();
  std::vector<int64_t> foff(nclips + 1, 0);
  for (int32_t c = 0; c < nclips; c++) {
    if (offsets[c + 1] < offsets[c]) return gfail(g, TFP_E_ARG, "offsets not monotone");
    foff[c + 1] = foff[c] + tfp_frame_count(offsets[c + 1] - offsets[c]);
  }
  *nframes = foff[nclips];
  if (foff[nclips] > 0 && (!out || cap < foff[nclips])) return gfail(g, TFP_E_CAPACITY, "need %lld frames", (long long)foff[nclips]);
  if (!foff[nclips]) return TFP_OK;
  // contiguous clip ranges with about equal frames per shard
  std::vector<int32_t> cut(n + 1, nclips);
  cut[0] = 0;
  for (int s = 1; s < n; s++)
    cut[s] = (int32_t)(std::lower_bound(foff.begin(), foff.end(), foff[nclips] * s / n) - foff.begin());
  for (int s = 1; s <= n; s++) cut[s] = std::max(cut[s], cut[s - 1]);
  return run_all(g, [&](int s) -> int {
    const int32_t a = cut[s], b = cut[s + 1];
    if (a >= b) return TFP_OK;
    int64_t got = 0;
    if (law >= 0)
      return tfp_fingerprint_g711_batch(g->eng[s], (const uint8_t*)x, offsets + a, b - a, law, sr, out + foff[a],
                                        foff[b] - foff[a], &got);
    return f32 ? tfp_fingerprint_f32_batch(g->eng[s], (const float*)x, offsets + a, b - a, sr, out + foff[a],
                                           foff[b] - foff[a], &got)
               : tfp_fingerprint_batch(g->eng[s], (const int16_t*)x, offsets + a, b - a, sr, out + foff[a],
                                       foff[b] - foff[a], &got);
  });
}
}  // namespace

int tfp_group_fingerprint_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nclips, int32_t sr,
                                tfp_frame* out, int64_t cap, int64_t* nframes) {
  return group_fingerprint(g, pcm, false, offsets, nclips, sr, out, cap, nframes);
}

int tfp_group_fingerprint_f32_batch(tfp_group* g, const float* x, const int64_t* offsets, int32_t nclips, int32_t sr,
                                    tfp_frame* out, int64_t cap, int64_t* nframes) {
  return group_fingerprint(g, x, true, offsets, nclips, sr, out, cap, nframes);
}

int tfp_group_fingerprint_g711_batch(tfp_group* g, const uint8_t* codes, const int64_t* offsets, int32_t nclips, int32_t law,
                                     int32_t sr, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!g) return TFP_E_ARG;
  if (!tfp::g711_law_ok(law)) return gfail(g, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  return group_fingerprint(g, codes, false, offsets, nclips, sr, out, cap, nframes, law);
}

namespace {
// A rate form's pair on a group: the plan, or the engine forms' own refusals.
int group_rate_plan(tfp_group* g, int32_t rate_in, int32_t rate_out, tfp::ResamplePlan* P) {
  bool bad = false;
  if (tfp::resample_plan(rate_in, rate_out, P, &bad)) return TFP_OK;
  if (bad) return gfail(g, TFP_E_ARG, "bad sample rate %d", rate_in < 1 ? rate_in : rate_out);
  return gfail(g, TFP_E_ARG, "unsupported rate ratio %d -> %d", rate_in, rate_out);
}
}  // namespace

// int16 at another rate on a group (tfp_resample.hpp): the clips are cut by their frames at rate_out as
// tfp_group_fingerprint_batch cuts its own, and each shard resamples the clips it fingerprints.
int tfp_group_fingerprint_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                                     int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!g) return TFP_E_ARG;
  tfp::ResamplePlan P;
  if (int rc = group_rate_plan(g, rate_in, rate_out, &P)) return rc;
  if (rate_in == rate_out) return tfp_group_fingerprint_batch(g, pcm, offsets, nclips, rate_out, out, cap, nframes);
  if (!offsets || nclips < 0 || !nframes) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int n = (int)g->eng.size();
  std::vector<int64_t> foff(nclips + 1, 0);
  for (int32_t c = 0; c < nclips; c++) {
    if (offsets[c + 1] < offsets[c]) return gfail(g, TFP_E_ARG, "offsets not monotone");
    const int64_t no = tfp::resample_count(P, offsets[c + 1] - offsets[c]);
    if (no < 0) return gfail(g, TFP_E_ARG, "clip %d: samples past the index range", c);
    foff[c + 1] = foff[c] + tfp_frame_count(no);
  }
  *nframes = foff[nclips];
  if (foff[nclips] > 0 && (!out || cap < foff[nclips])) return gfail(g, TFP_E_CAPACITY, "need %lld frames", (long long)foff[nclips]);
  if (!foff[nclips]) return TFP_OK;
  std::vector<int32_t> cut(n + 1, nclips);
  cut[0] = 0;
  for (int s = 1; s < n; s++)
    cut[s] = (int32_t)(std::lower_bound(foff.begin(), foff.end(), foff[nclips] * s / n) - foff.begin());
  for (int s = 1; s <= n; s++) cut[s] = std::max(cut[s], cut[s - 1]);
  return run_all(g, [&](int s) -> int {
    const int32_t a = cut[s], b = cut[s + 1];
    if (a >= b) return TFP_OK;
    int64_t got = 0;
    return tfp_fingerprint_rate_batch(g->eng[s], pcm, offsets + a, b - a, rate_in, rate_out, out + foff[a], foff[b] - foff[a],
                                      &got);
  });
}

namespace {
// A mix form's channel count and pair on a group: the engine forms' own refusals, in their order.
int group_mix_plan(tfp_group* g, int32_t channels, int32_t rate_in, int32_t rate_out, tfp::ResamplePlan* P) {
  if (channels < 1 || channels > TFP_MIX_CHANNELS_MAX) return gfail(g, TFP_E_ARG, "unsupported channel count %d", channels);
  return group_rate_plan(g, rate_in, rate_out, P);
}

// A wide form's pair on a group: the mix refusals, then the range the wide accumulator needs (A C < 2^30).
int group_wide_plan(tfp_group* g, int32_t channels, int32_t rate_in, int32_t rate_out, tfp::ResamplePlan* P) {
  if (int rc = group_mix_plan(g, channels, rate_in, rate_out, P)) return rc;
  if (rate_in == rate_out) return TFP_OK;
  bool bad = false;
  const std::shared_ptr<const tfp::ResampleTable> t = tfp::resample_table(rate_in, rate_out, &bad);
  if (!t) return gfail(g, TFP_E_ARG, "unsupported rate ratio %d -> %d", rate_in, rate_out);
  if (!tfp::resample_wide_in_range(*t, channels))
    return gfail(g, TFP_E_ARG, "unsupported rate ratio %d -> %d for %d wide channels", rate_in, rate_out, channels);
  return TFP_OK;
}

// The fingerprint split of the interleaved forms: the clips (offsets in frames) are cut by their frames at
// rate_out exactly as tfp_group_fingerprint_rate_batch cuts its own, and shard s runs
// call(s, first clip, clips, out, cap) on the clips it fingerprints.
extern "C++" template <typename Call>
int group_fingerprint_frames(tfp_group* g, const tfp::ResamplePlan& P, const int64_t* offsets, int32_t nclips, int32_t rate_in,
                             int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes, Call call) {
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int n = (int)g->eng.size();
  std::vector<int64_t> foff(nclips + 1, 0);
  for (int32_t c = 0; c < nclips; c++) {
    if (offsets[c + 1] < offsets[c]) return gfail(g, TFP_E_ARG, "offsets not monotone");
    const int64_t len = offsets[c + 1] - offsets[c], no = rate_in == rate_out ? len : tfp::resample_count(P, len);
    if (no < 0) return gfail(g, TFP_E_ARG, "clip %d: frames past the index range", c);
    foff[c + 1] = foff[c] + tfp_frame_count(no);
  }
  *nframes = foff[nclips];
  if (foff[nclips] > 0 && (!out || cap < foff[nclips])) return gfail(g, TFP_E_CAPACITY, "need %lld frames", (long long)foff[nclips]);
  if (!foff[nclips]) return TFP_OK;
  std::vector<int32_t> cut(n + 1, nclips);
  cut[0] = 0;
  for (int s = 1; s < n; s++)
    cut[s] = (int32_t)(std::lower_bound(foff.begin(), foff.end(), foff[nclips] * s / n) - foff.begin());
  for (int s = 1; s <= n; s++) cut[s] = std::max(cut[s], cut[s - 1]);
  return run_all(g, [&](int s) -> int {
    const int32_t a = cut[s], b = cut[s + 1];
    if (a >= b) return TFP_OK;
    return call(s, a, b - a, out + foff[a], foff[b] - foff[a]);
  });
}
}  // namespace

// Interleaved multichannel int16 on a group (tfp_resample.hpp, "the multichannel form"): offsets count
// frames; each shard downmixes and converts the clips it fingerprints. One channel is the rate form.
int tfp_group_fingerprint_mix_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                                         int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                         int64_t* nframes) {
  if (!g) return TFP_E_ARG;
  if (channels == 1) return tfp_group_fingerprint_rate_batch(g, pcm, offsets, nclips, rate_in, rate_out, out, cap, nframes);
  tfp::ResamplePlan P;
  if (int rc = group_mix_plan(g, channels, rate_in, rate_out, &P)) return rc;
  if (!offsets || nclips < 0 || !nframes) return TFP_E_ARG;
  return group_fingerprint_frames(g, P, offsets, nclips, rate_in, rate_out, out, cap, nframes,
                                  [&](int s, int32_t a, int32_t n, tfp_frame* o, int64_t ocap) {
                                    int64_t got = 0;
                                    return tfp_fingerprint_mix_rate_batch(g->eng[s], pcm, offsets + a, n, channels, rate_in,
                                                                          rate_out, o, ocap, &got);
                                  });
}

// Interleaved int32 Q31 on a group (tfp_resample.hpp, "the wide form"), split as the mix twin's clips are.
int tfp_group_fingerprint_wide_rate_batch(tfp_group* g, const int32_t* q31, const int64_t* offsets, int32_t nclips,
                                          int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                          int64_t* nframes) {
  if (!g) return TFP_E_ARG;
  tfp::ResamplePlan P;
  if (int rc = group_wide_plan(g, channels, rate_in, rate_out, &P)) return rc;
  if (!offsets || nclips < 0 || !nframes) return TFP_E_ARG;
  return group_fingerprint_frames(g, P, offsets, nclips, rate_in, rate_out, out, cap, nframes,
                                  [&](int s, int32_t a, int32_t n, tfp_frame* o, int64_t ocap) {
                                    int64_t got = 0;
                                    return tfp_fingerprint_wide_rate_batch(g->eng[s], q31, offsets + a, n, channels, rate_in,
                                                                           rate_out, o, ocap, &got);
                                  });
}

namespace {
// A mixed batch's rules on a group: any_prepare's, with the engine forms' messages.
int group_any_batch(tfp_group* g, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t n, int32_t rate_out,
                    tfp::AnyBatch* B) {
  std::string err;
  if (!tfp::any_prepare(clips, n, nbytes, rate_out, tfp::resample_table, B, &err)) return gfail(g, TFP_E_ARG, "%s", err.c_str());
  if (!data && B->in_off[(size_t)n] > 0) return gfail(g, TFP_E_ARG, "samples are NULL");
  return TFP_OK;
}
}  // namespace

// A mixed batch on a group (tfp_resample_any.hpp): the clips are cut by their frames at rate_out as
// tfp_group_fingerprint_rate_batch cuts its own, and each shard converts the clips it fingerprints in one
// launch of its own. A shard is handed the byte range its clips span (from a 4-byte aligned start, so every
// offset keeps its alignment), not the whole call's bytes.
int tfp_group_fingerprint_any_batch(tfp_group* g, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nclips,
                                    int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);  // (before the first message is written)
  if (!nframes) return gfail(g, TFP_E_ARG, "bad arguments");
  tfp::AnyBatch B;
  if (int rc = group_any_batch(g, data, nbytes, clips, nclips, rate_out, &B)) return rc;
  const int n = (int)g->eng.size();
  std::vector<int64_t> foff(nclips + 1, 0);
  for (int32_t c = 0; c < nclips; c++) foff[c + 1] = foff[c] + tfp_frame_count(B.clips[c].n_out);
  *nframes = foff[nclips];
  if (foff[nclips] > 0 && (!out || cap < foff[nclips])) return gfail(g, TFP_E_CAPACITY, "need %lld frames", (long long)foff[nclips]);
  if (!foff[nclips]) return TFP_OK;
  std::vector<int32_t> cut(n + 1, nclips);
  cut[0] = 0;
  for (int s = 1; s < n; s++)
    cut[s] = (int32_t)(std::lower_bound(foff.begin(), foff.end(), foff[nclips] * s / n) - foff.begin());
  for (int s = 1; s <= n; s++) cut[s] = std::max(cut[s], cut[s - 1]);
  return run_all(g, [&](int s) -> int {
    const int32_t a = cut[s], b = cut[s + 1];
    if (a >= b) return TFP_OK;
    int64_t lo = INT64_MAX, hi = 0;
    for (int32_t c = a; c < b; c++) {
      const int64_t len = clips[c].nframes * clips[c].channels * tfp::any_sample_size(clips[c].kind);
      lo = std::min(lo, clips[c].offset);
      hi = std::max(hi, clips[c].offset + len);
    }
    lo &= ~(int64_t)3;
    std::vector<tfp_audio_clip> mine(clips + a, clips + b);
    for (tfp_audio_clip& k : mine) k.offset -= lo;
    int64_t got = 0;
    return tfp_fingerprint_any_batch(g->eng[s], data ? static_cast<const char*>(data) + lo : nullptr, hi - lo, mine.data(), b - a,
                                     rate_out, out + foff[a], foff[b] - foff[a], &got);
  });
}

int tfp_group_index_add(tfp_group* g, const char* uuid, const int32_t* m1, const int32_t* m2, int32_t nframes) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  if (!uuid || g->where.count(uuid)) return gfail(g, uuid ? TFP_E_EXISTS : TFP_E_ARG, "uuid %s already indexed", uuid ? uuid : "(null)");
  const int32_t s = lightest(g);
  int32_t id = -1;
  const int rc = tfp_index_add(g->eng[s], uuid, m1, m2, nframes, &id);
  if (rc) return shard_fail(g, rc, s);
  if (id != (int32_t)g->id2member[s].size()) {  // (never expected) undo the engine's add: no clip without a member
    (void)tfp_index_remove(g->eng[s], uuid);
    return gfail(g, TFP_E_HIP, "shard %d clip id %d out of step", s, id);
  }
  g->rows[s] += nframes;
  return add_members(g, s, 1, &uuid);
}

int tfp_group_index_add_batch(tfp_group* g, int32_t nclips, const char* const* uuids, const int64_t* foff,
                              const int32_t* m1, const int32_t* m2) {
  if (!g || nclips < 0 || !uuids || !foff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int n = (int)g->eng.size();
  std::unordered_map<std::string, int> seen;
  for (int32_t c = 0; c < nclips; c++) {
    if (!uuids[c] || !*uuids[c] || strlen(uuids[c]) >= 64) return gfail(g, TFP_E_ARG, "bad uuid %d", c);
    if (foff[c + 1] < foff[c]) return gfail(g, TFP_E_ARG, "frame_offsets not monotone at %d", c);
    if (g->where.count(uuids[c]) || !seen.emplace(uuids[c], c).second)
      return gfail(g, TFP_E_EXISTS, "uuid %s already indexed", uuids[c]);
  }
  // each clip to the shard with the fewest rows so far; per shard one tfp_index_add_batch
  std::vector<std::vector<int32_t>> pick(n);
  std::vector<int64_t> rows = g->rows;
  for (int32_t c = 0; c < nclips; c++) {
    const int32_t s = (int32_t)(std::min_element(rows.begin(), rows.end()) - rows.begin());
    pick[s].push_back(c);
    rows[s] += foff[c + 1] - foff[c];
  }
  std::vector<std::vector<const char*>> uu(n);
  std::vector<std::vector<int64_t>> fo(n);
  std::vector<std::vector<int32_t>> a1(n), a2(n);
  for (int s = 0; s < n; s++) {
    fo[s].push_back(0);
    for (int32_t c : pick[s]) {
      uu[s].push_back(uuids[c]);
      a1[s].insert(a1[s].end(), m1 + foff[c], m1 + foff[c + 1]);
      a2[s].insert(a2[s].end(), m2 + foff[c], m2 + foff[c + 1]);
      fo[s].push_back((int64_t)a1[s].size());
    }
  }
  std::vector<int> rcs(n, TFP_OK);
  const int rc = run_all(g, [&](int s) -> int {
    if (uu[s].empty()) return TFP_OK;
    return rcs[s] = tfp_index_add_batch(g->eng[s], (int32_t)uu[s].size(), uu[s].data(), fo[s].data(), a1[s].data(),
                                        a2[s].data());
  });
  // All-or-nothing over the group, as each engine's add_batch is per call: when a shard failed (a
  // device error: the arguments were checked above), the shards that succeeded drop the batch's
  // clips again, so no clip stays on a GPU without a member (or a catalog row: the shim deletes
  // the batch's rows on failure).
  if (rc) {
    for (int s = 0; s < n; s++)
      if (!uu[s].empty() && rcs[s] == TFP_OK) {
        for (const char* u : uu[s]) (void)tfp_index_remove(g->eng[s], u);
        // the engine's clip ids of the dropped clips stay used: keep the group's id map in step
        g->id2member[s].insert(g->id2member[s].end(), uu[s].size(), -1);
        g->ranks_dirty = true;
      }
    return rc;
  }
  for (int s = 0; s < n; s++)
    if (!uu[s].empty()) {
      add_members(g, s, (int32_t)uu[s].size(), uu[s].data());
      g->rows[s] += fo[s].back();
    }
  return TFP_OK;
}

int tfp_group_index_remove(tfp_group* g, const char* uuid) {
  if (!g || !uuid) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  auto it = g->where.find(uuid);
  if (it == g->where.end()) return gfail(g, TFP_E_NOENT, "uuid %s not indexed", uuid);
  const int32_t mi = it->second;
  Member& m = g->members[mi];
  int64_t nr = 0;
  (void)tfp_index_rows(g->eng[m.shard], uuid, nullptr, nullptr, 0, &nr);
  const int rc = tfp_index_remove(g->eng[m.shard], uuid);
  if (rc) return shard_fail(g, rc, m.shard);
  erase_live(g, mi);
  g->rows[m.shard] -= nr;
  g->id2member[m.shard][m.id] = -1;
  g->where.erase(it);
  m.uuid.clear();
  return TFP_OK;
}

int tfp_group_index_clear(tfp_group* g) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int n = (int)g->eng.size();
  std::vector<int> rcs(n, TFP_OK);
  const int rc = run_all(g, [&](int s) { return rcs[s] = tfp_index_clear(g->eng[s]); });
  g->ranks_dirty = true;
  g->keys_full = true;
  if (rc == TFP_OK) {
    g->where.clear();
    g->members.clear();
    g->by_uuid.clear();
    for (auto& v : g->id2member) v.clear();
    std::fill(g->rows.begin(), g->rows.end(), 0);
    return TFP_OK;
  }
  // a shard whose clear failed keeps its clips, and the group keeps them as its members
  for (int s = 0; s < n; s++) {
    if (rcs[s] != TFP_OK) continue;
    for (int32_t mi : g->id2member[s]) {
      if (mi < 0) continue;
      Member& m = g->members[mi];
      erase_live(g, mi);
      g->where.erase(m.uuid);
      m.uuid.clear();
    }
    g->id2member[s].clear();
    g->rows[s] = 0;
  }
  return rc;
}

int tfp_group_index_rows(tfp_group* g, const char* uuid, int32_t* m1, int32_t* m2, int64_t cap, int64_t* nframes) {
  if (!g || !uuid) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  auto it = g->where.find(uuid);
  if (it == g->where.end()) return gfail(g, TFP_E_NOENT, "uuid %s not indexed", uuid);
  const int s = g->members[it->second].shard;
  const int rc = tfp_index_rows(g->eng[s], uuid, m1, m2, cap, nframes);
  return rc ? shard_fail(g, rc, s) : TFP_OK;
}

int tfp_group_index_stats(tfp_group* g, int64_t* nrows, int32_t* nclips) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int64_t r = 0;
  int32_t c = 0;
  for (auto* e : g->eng) {
    int64_t a = 0;
    int32_t b = 0;
    const int rc = tfp_index_stats(e, &a, &b);
    if (rc) return rc;
    r += a;
    c += b;
  }
  if (nrows) *nrows = r;
  if (nclips) *nclips = c;
  return TFP_OK;
}

int tfp_group_index_commit(tfp_group* g) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  return run_all(g, [&](int s) { return tfp_index_commit(g->eng[s]); });
}

int tfp_group_search_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                           const tfp_search_params* P, tfp_result* out) {
  if (!g || !qoff || nq < 0 || !out) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  std::vector<std::vector<tfp_result>> res(n, std::vector<tfp_result>(std::max(nq, 1)));
  rc = run_all(g, [&](int s) { return tfp_search_batch(g->eng[s], frames, qoff, nq, P, res[s].data()); });
  if (rc) return rc;
  combine(g, res, nq, out);
  return TFP_OK;
}

namespace {
// Ranked search on a group: every shard's first k rows (search(s, out, counts)) mapped to their
// global keys as key_of does; per query the at most n * k keys sorted descending and k kept
// (rank_merge_keep). A failing shard fails the call: no partial list goes out.
// kept (optional): the member behind each row of out, -1 past counts[q] (the aligned search reads
// the shard and the shard-local clip id from it).
int group_rank(tfp_group* g, int32_t nq, const tfp_search_params* P, int32_t k, tfp_candidate* out, int32_t* counts,
               const std::function<int(int, tfp_candidate*, int32_t*)>& search, std::vector<int32_t>* kept = nullptr) {
  if (nq < 0 || !out || !counts) return gfail(g, TFP_E_ARG, "ranked search: bad query count or NULL output");
  if (k < 1 || k > TFP_RANK_MAX) return gfail(g, TFP_E_ARG, "ranked search: k = %d outside [1, %d]", k, TFP_RANK_MAX);
  if (!valid_params(P)) return gfail(g, TFP_E_ARG, "ranked search: coefs outside [1, 2]");
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  const size_t per = (size_t)std::max(nq, 1) * k;
  std::vector<std::vector<tfp_candidate>> res(n, std::vector<tfp_candidate>(per));
  std::vector<std::vector<int32_t>> cnt(n, std::vector<int32_t>(std::max(nq, 1), 0));
  rc = run_all(g, [&](int s) { return search(s, res[s].data(), cnt[s].data()); });
  if (rc) return rc;
  memset(out, 0, sizeof(tfp_candidate) * (size_t)nq * k);
  if (kept) kept->assign((size_t)nq * k, -1);
  std::vector<unsigned long long> keys((size_t)n * k), top(k);
  for (int32_t i = 0; i < nq; i++) {
    int64_t nk = 0;
    for (int s = 0; s < n; s++)
      for (int32_t r = 0; r < cnt[s][i]; r++) {
        const tfp_candidate& c = res[s][(size_t)i * k + r];
        tfp_result as_result;
        as_result.found = 1, as_result.match_count = c.match_count, as_result.clip_id = c.clip_id;
        keys[nk++] = key_of(g, s, as_result);
      }
    const int32_t m = tfp::rank_merge_keep(keys.data(), nk, k, top.data());
    int32_t w = 0;
    for (int32_t r = 0; r < m; r++) {
      const auto it = g->key2member.find((int32_t)(uint32_t)(top[r] & 0xffffffffu));
      if (it == g->key2member.end()) continue;
      const Member& mb = g->members[it->second];
      if (kept) (*kept)[(size_t)i * k + w] = it->second;
      tfp_candidate& c = out[(size_t)i * k + w++];
      c.match_count = (int32_t)(top[r] >> 32);
      c.clip_id = mb.shard;
      snprintf(c.uuid, sizeof c.uuid, "%s", mb.uuid.c_str());
    }
    counts[i] = w;
  }
  return TFP_OK;
}
}  // namespace

int tfp_group_search_ranked_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                                  const tfp_search_params* P, int32_t k, tfp_candidate* out, int32_t* counts) {
  if (!g || !qoff) return TFP_E_ARG;
  return group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_ranked_batch(g->eng[s], frames, qoff, nq, P, k, o, c);
  });
}

int tfp_group_search_ranked_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                                      const tfp_search_params* P, int32_t k, tfp_candidate* out, int32_t* counts) {
  if (!g || !offsets) return TFP_E_ARG;
  return group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_ranked_pcm_batch(g->eng[s], pcm, offsets, nq, sr, P, k, o, c);
  });
}

// Scoped search on a group (tfp_scope.hpp): a scope lives with its clip on the clip's shard.
int tfp_group_index_set_scope(tfp_group* g, int32_t n, const char* const* uuids, const int32_t* scopes) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  if (n < 0 || (n && (!uuids || !scopes))) return gfail(g, TFP_E_ARG, "set scope: bad count or NULL array");
  const int ns = (int)g->eng.size();
  std::vector<std::vector<const char*>> u(ns);
  std::vector<std::vector<int32_t>> sc(ns);
  for (int32_t i = 0; i < n; i++) {  // all or nothing: every entry checked before any shard is told
    if (!uuids[i]) return gfail(g, TFP_E_ARG, "set scope: uuid %d is NULL", i);
    if (scopes[i] < 0) return gfail(g, TFP_E_ARG, "set scope: scope %d of %s", scopes[i], uuids[i]);
    const auto it = g->where.find(uuids[i]);
    if (it == g->where.end()) return gfail(g, TFP_E_NOENT, "uuid %s not indexed", uuids[i]);
    const int s = g->members[it->second].shard;
    u[s].push_back(uuids[i]);
    sc[s].push_back(scopes[i]);
  }
  for (int s = 0; s < ns; s++) {
    if (u[s].empty()) continue;
    const int rc = tfp_index_set_scope(g->eng[s], (int32_t)u[s].size(), u[s].data(), sc[s].data());
    if (rc) return shard_fail(g, rc, s);  // (checked above: a shard refuses only what the group's own maps would)
  }
  return TFP_OK;
}

int tfp_group_index_scope(tfp_group* g, const char* uuid, int32_t* scope) {
  if (!g || !uuid || !scope) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  auto it = g->where.find(uuid);
  if (it == g->where.end()) return gfail(g, TFP_E_NOENT, "uuid %s not indexed", uuid);
  const int s = g->members[it->second].shard;
  const int rc = tfp_index_scope(g->eng[s], uuid, scope);
  return rc ? shard_fail(g, rc, s) : TFP_OK;
}

namespace {
int group_scope_args(tfp_group* g, const int32_t* scopes, int32_t nq) {
  if (nq > 0 && !scopes) return gfail(g, TFP_E_ARG, "scoped search: scopes is NULL");
  for (int32_t i = 0; i < nq; i++)
    if (scopes[i] < TFP_SCOPE_ANY) return gfail(g, TFP_E_ARG, "scoped search: scope %d of query %d", scopes[i], i);
  return TFP_OK;
}
}  // namespace

int tfp_group_search_scoped_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                                  const tfp_search_params* P, const int32_t* scopes, int32_t k, tfp_candidate* out,
                                  int32_t* counts) {
  if (!g || !qoff) return TFP_E_ARG;
  if (int rc = group_scope_args(g, scopes, nq)) return rc;
  return group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_scoped_batch(g->eng[s], frames, qoff, nq, P, scopes, k, o, c);
  });
}

int tfp_group_search_scoped_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                                      const tfp_search_params* P, const int32_t* scopes, int32_t k, tfp_candidate* out,
                                      int32_t* counts) {
  if (!g || !offsets) return TFP_E_ARG;
  if (int rc = group_scope_args(g, scopes, nq)) return rc;
  return group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_scoped_pcm_batch(g->eng[s], pcm, offsets, nq, sr, P, scopes, k, o, c);
  });
}

// Every shard resamples and fingerprints the batch, as every shard fingerprints the pcm form's.
int tfp_group_search_scoped_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t rate_in,
                                       int32_t rate_out, const tfp_search_params* P, const int32_t* scopes, int32_t k,
                                       tfp_candidate* out, int32_t* counts, int32_t* frame_counts) {
  if (!g || !offsets) return TFP_E_ARG;
  tfp::ResamplePlan rp;
  if (int rc = group_rate_plan(g, rate_in, rate_out, &rp)) return rc;
  if (int rc = group_scope_args(g, scopes, nq)) return rc;
  const int rc = group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_scoped_rate_batch(g->eng[s], pcm, offsets, nq, rate_in, rate_out, P, scopes, k, o, c, nullptr);
  });
  if (rc) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) {
    const int64_t len = offsets[i + 1] - offsets[i];
    frame_counts[i] = (int32_t)tfp_frame_count(rate_in == rate_out ? len : tfp::resample_count(rp, len));
  }
  return TFP_OK;
}

// Every shard downmixes, converts and fingerprints the batch, as the rate twin's shards do.
int tfp_group_search_scoped_mix_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq,
                                           int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* P,
                                           const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                           int32_t* frame_counts) {
  if (!g || !offsets) return TFP_E_ARG;
  if (channels == 1)
    return tfp_group_search_scoped_rate_batch(g, pcm, offsets, nq, rate_in, rate_out, P, scopes, k, out, counts, frame_counts);
  tfp::ResamplePlan rp;
  if (int rc = group_mix_plan(g, channels, rate_in, rate_out, &rp)) return rc;
  if (int rc = group_scope_args(g, scopes, nq)) return rc;
  const int rc = group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_scoped_mix_rate_batch(g->eng[s], pcm, offsets, nq, channels, rate_in, rate_out, P, scopes, k, o, c,
                                            nullptr);
  });
  if (rc) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) {
    const int64_t len = offsets[i + 1] - offsets[i];
    frame_counts[i] = (int32_t)tfp_frame_count(rate_in == rate_out ? len : tfp::resample_count(rp, len));
  }
  return TFP_OK;
}

// The wide twin: every shard converts and fingerprints the Q31 batch.
int tfp_group_search_scoped_wide_rate_batch(tfp_group* g, const int32_t* q31, const int64_t* offsets, int32_t nq,
                                            int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* P,
                                            const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                            int32_t* frame_counts) {
  if (!g || !offsets) return TFP_E_ARG;
  tfp::ResamplePlan rp;
  if (int rc = group_wide_plan(g, channels, rate_in, rate_out, &rp)) return rc;
  if (int rc = group_scope_args(g, scopes, nq)) return rc;
  const int rc = group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_scoped_wide_rate_batch(g->eng[s], q31, offsets, nq, channels, rate_in, rate_out, P, scopes, k, o, c,
                                             nullptr);
  });
  if (rc) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) {
    const int64_t len = offsets[i + 1] - offsets[i];
    frame_counts[i] = (int32_t)tfp_frame_count(rate_in == rate_out ? len : tfp::resample_count(rp, len));
  }
  return TFP_OK;
}

// The mixed twin: every shard converts (one launch) and fingerprints the batch.
int tfp_group_search_scoped_any_batch(tfp_group* g, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nq,
                                      int32_t rate_out, const tfp_search_params* P, const int32_t* scopes, int32_t k,
                                      tfp_candidate* out, int32_t* counts, int32_t* frame_counts) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);  // (before the first message is written)
  tfp::AnyBatch B;
  if (int rc = group_any_batch(g, data, nbytes, clips, nq, rate_out, &B)) return rc;
  if (int rc = group_scope_args(g, scopes, nq)) return rc;
  const int rc = group_rank(g, nq, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    return tfp_search_scoped_any_batch(g->eng[s], data, nbytes, clips, nq, rate_out, P, scopes, k, o, c, nullptr);
  });
  if (rc) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) frame_counts[i] = (int32_t)tfp_frame_count(B.clips[i].n_out);
  return TFP_OK;
}

// Catalog neighbours on a group (tfp_neighbour.hpp). The shard that holds a named clip produces its
// frame values (the gather kernel over its staged rows); they travel to every shard as a frames batch
// does, from the host. Every shard returns its first k rows over its own clips, the owner with the
// clip's own row deleted from k + 1 (no other shard has a row to delete), so the merged first k are
// one engine's over all the clips. The rows are aligned on the shard that holds their clip.
int tfp_group_index_neighbours(tfp_group* g, int32_t nclips, const char* const* uuids, const tfp_search_params* P,
                               const int32_t* scopes, int32_t k, tfp_candidate* out, tfp_alignment* align, int32_t* counts,
                               int32_t* frame_counts) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  if (nclips < 0 || (nclips && (!uuids || !out || !counts))) return gfail(g, TFP_E_ARG, "neighbours: bad clip count or NULL array");
  if (k < 1 || k > TFP_RANK_MAX) return gfail(g, TFP_E_ARG, "neighbours: k = %d outside [1, %d]", k, TFP_RANK_MAX);
  if (!valid_params(P)) return gfail(g, TFP_E_ARG, "neighbours: coefs outside [1, 2]");
  for (int32_t i = 0; scopes && i < nclips; i++)
    if (scopes[i] < TFP_SCOPE_ANY) return gfail(g, TFP_E_ARG, "neighbours: scope %d of clip %d", scopes[i], i);
  const int n = (int)g->eng.size();
  std::vector<std::vector<const char*>> names(n);
  std::vector<std::vector<int32_t>> which(n), self(n, std::vector<int32_t>((size_t)std::max(nclips, 1), -1));
  for (int32_t i = 0; i < nclips; i++) {  // all or nothing: every name resolved before anything is written
    if (!uuids[i]) return gfail(g, TFP_E_ARG, "neighbours: uuid %d is NULL", i);
    const auto it = g->where.find(uuids[i]);
    if (it == g->where.end()) return gfail(g, TFP_E_NOENT, "uuid %s not indexed", uuids[i]);
    const Member& mb = g->members[it->second];
    names[mb.shard].push_back(uuids[i]);
    which[mb.shard].push_back(i);
    self[mb.shard][i] = mb.id;
  }
  if (!nclips) return TFP_OK;
  std::vector<int64_t> qoff((size_t)nclips + 1, 0);
  for (int s = 0; s < n; s++) {
    if (names[s].empty()) continue;
    std::vector<int64_t> nr(names[s].size());
    const int rc = tfp_internal_neighbour_rows(g->eng[s], (int32_t)names[s].size(), names[s].data(), nr.data());
    if (rc) return shard_fail(g, rc, s);
    for (size_t j = 0; j < nr.size(); j++) qoff[which[s][j] + 1] = nr[j];
  }
  for (int32_t i = 0; i < nclips; i++) qoff[i + 1] += qoff[i];
  std::vector<tfp_frame> frames((size_t)std::max<int64_t>(qoff[nclips], 1));
  int rc = run_all(g, [&](int s) {
    if (names[s].empty()) return (int)TFP_OK;
    std::vector<int64_t> foff(names[s].size());
    for (size_t j = 0; j < foff.size(); j++) foff[j] = qoff[which[s][j]];
    return tfp_internal_neighbour_frames(g->eng[s], (int32_t)names[s].size(), names[s].data(), foff.data(), frames.data());
  });
  if (rc) return rc;
  std::vector<int32_t> sv((size_t)nclips, TFP_SCOPE_ANY);
  if (scopes) sv.assign(scopes, scopes + nclips);
  std::vector<int32_t> kept;
  std::vector<tfp_candidate> rows((size_t)nclips * k);
  std::vector<int32_t> cnt((size_t)nclips);
  rc = group_rank(
      g, nclips, P, k, rows.data(), cnt.data(),
      [&](int s, tfp_candidate* o, int32_t* c) {
        return tfp_internal_neighbours_of_frames(g->eng[s], frames.data(), qoff.data(), nclips, P, sv.data(), self[s].data(), k,
                                                 o, c);
      },
      &kept);
  if (rc) return rc;
  const size_t np = (size_t)nclips * k;
  std::vector<tfp_alignment> al(np);
  if (align) {
    std::vector<std::vector<int32_t>> ids(n, std::vector<int32_t>(np, -1));
    std::vector<char> used(n, 0);
    for (size_t p = 0; p < np; p++)
      if (kept[p] >= 0) {
        const Member& mb = g->members[kept[p]];
        ids[mb.shard][p] = mb.id;
        used[mb.shard] = 1;
      }
    std::vector<std::vector<tfp_alignment>> res(n, std::vector<tfp_alignment>(np));
    rc = run_all(g, [&](int s) {
      return used[s] ? tfp_internal_neighbour_align(g->eng[s], frames.data(), qoff.data(), nclips, P, ids[s].data(), k,
                                                    res[s].data())
                     : (int)TFP_OK;
    });
    if (rc) return rc;
    memset(al.data(), 0, sizeof(tfp_alignment) * np);
    for (size_t p = 0; p < np; p++)
      if (kept[p] >= 0) al[p] = res[g->members[kept[p]].shard][p];
    std::copy(al.begin(), al.end(), align);
  }
  std::copy(rows.begin(), rows.end(), out);
  std::copy(cnt.begin(), cnt.end(), counts);
  for (int32_t i = 0; frame_counts && i < nclips; i++) frame_counts[i] = (int32_t)(qoff[i + 1] - qoff[i]);
  return TFP_OK;
}

// Match census on a group (tfp_census.hpp): each shard's census of its own clips runs on its worker
// and the rows are summed on the host, bin 0 (the shard's live clips of the scope with count 0)
// included. A clip lies on one shard, so the sum is exact.
namespace {
int group_census(tfp_group* g, int32_t nq, const tfp_search_params* P, const int32_t* scopes, int32_t nbins, int32_t* hist,
                 int32_t* need_bins, const std::function<int(int, int32_t*, int32_t*)>& census) {
  if (nq < 0 || !need_bins) return gfail(g, TFP_E_ARG, "census: bad query count or NULL need_bins");
  if (!valid_params(P)) return gfail(g, TFP_E_ARG, "census: coefs outside [1, 2]");
  for (int32_t i = 0; scopes && i < nq; i++)
    if (scopes[i] < TFP_SCOPE_ANY) return gfail(g, TFP_E_ARG, "census: scope %d of query %d", scopes[i], i);
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  const size_t per = (size_t)std::max(nq, 1) * (size_t)std::max(nbins, 1);
  std::vector<std::vector<int32_t>> res(n, std::vector<int32_t>(per, 0));
  std::vector<int32_t> need(n, 0);
  // (every shard sees the same queries: all return TFP_E_CAPACITY with the same need_bins, or none)
  rc = run_all(g, [&](int s) { return census(s, res[s].data(), &need[s]); });
  if (rc && rc != TFP_E_CAPACITY) return rc;
  *need_bins = need[0];
  if (rc) return rc;
  if (nq && !hist) return gfail(g, TFP_E_ARG, "census: hist is NULL");
  for (size_t i = 0; i < (size_t)nq * nbins; i++) {
    int64_t sum = 0;
    for (int s = 0; s < n; s++) sum += res[s][i];
    hist[i] = (int32_t)sum;
  }
  return TFP_OK;
}
}  // namespace

int tfp_group_census_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nq, const tfp_search_params* P,
                           const int32_t* scopes, int32_t nbins, int32_t* hist, int32_t* need_bins) {
  if (!g || !qoff) return TFP_E_ARG;
  return group_census(g, nq, P, scopes, nbins, hist, need_bins, [&](int s, int32_t* h, int32_t* nb) {
    return tfp_census_batch(g->eng[s], frames, qoff, nq, P, scopes, nbins, h, nb);
  });
}

int tfp_group_census_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                               const tfp_search_params* P, const int32_t* scopes, int32_t nbins, int32_t* hist,
                               int32_t* need_bins) {
  if (!g || !offsets) return TFP_E_ARG;
  return group_census(g, nq, P, scopes, nbins, hist, need_bins, [&](int s, int32_t* h, int32_t* nb) {
    return tfp_census_pcm_batch(g->eng[s], pcm, offsets, nq, sr, P, scopes, nbins, h, nb);
  });
}

// Sliding search on a group (tfp_slide.hpp): every shard slides over every recording, and per window
// the shards' rows merge as a query's do (group_rank, a window in a query's place).
namespace {
// The windows of the recordings at off[0..nrec] (frames, or samples with pcm) counted as the shards
// will count them, after the argument checks that decide the count.
int group_slide_windows(tfp_group* g, const int64_t* off, int32_t nrec, bool pcm, int32_t window, int32_t hop,
                        const int32_t* scopes, int64_t cap_windows, int64_t* nwindows, int32_t* nw) {
  if (nrec < 0 || !nwindows) return gfail(g, TFP_E_ARG, "sliding search: bad recording count or NULL nwindows");
  if (window < 1 || hop < 1) return gfail(g, TFP_E_ARG, "sliding search: window = %d, hop = %d", window, hop);
  for (int32_t i = 0; scopes && i < nrec; i++)
    if (scopes[i] < TFP_SCOPE_ANY) return gfail(g, TFP_E_ARG, "sliding search: scope %d of recording %d", scopes[i], i);
  int64_t total = 0;
  for (int32_t i = 0; i < nrec; i++) {
    if (off[i + 1] < off[i]) return gfail(g, TFP_E_ARG, "sliding search: offsets not monotone");
    const int64_t n = off[i + 1] - off[i];
    total += tfp_sliding_windows(pcm ? tfp_frame_count(n) : n, window, hop);
  }
  *nwindows = total;
  if (total > cap_windows || total > INT32_MAX)
    return gfail(g, TFP_E_CAPACITY, "sliding search: %lld windows, room for %lld", (long long)total, (long long)cap_windows);
  *nw = (int32_t)total;
  return TFP_OK;
}
}  // namespace

int tfp_group_search_sliding_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nrec,
                                   const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes, int32_t k,
                                   tfp_candidate* out, int32_t* counts, int64_t cap_windows, int64_t* nwindows) {
  if (!g || !qoff) return TFP_E_ARG;
  if (k < 1 || k > TFP_RANK_MAX || !valid_params(P)) return gfail(g, TFP_E_ARG, "sliding search: k or coefs out of range");
  int32_t nw = 0;
  if (int rc = group_slide_windows(g, qoff, nrec, false, window, hop, scopes, cap_windows, nwindows, &nw)) return rc;
  if (!nw) return TFP_OK;
  return group_rank(g, nw, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    int64_t n = 0;
    return tfp_search_sliding_batch(g->eng[s], frames, qoff, nrec, P, window, hop, scopes, k, o, c, nw, &n);
  });
}

int tfp_group_search_sliding_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nrec, int32_t sr,
                                       const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes,
                                       int32_t k, tfp_candidate* out, int32_t* counts, int64_t cap_windows,
                                       int64_t* nwindows) {
  if (!g || !offsets) return TFP_E_ARG;
  if (k < 1 || k > TFP_RANK_MAX || !valid_params(P)) return gfail(g, TFP_E_ARG, "sliding search: k or coefs out of range");
  int32_t nw = 0;
  if (int rc = group_slide_windows(g, offsets, nrec, true, window, hop, scopes, cap_windows, nwindows, &nw)) return rc;
  if (!nw) return TFP_OK;
  return group_rank(g, nw, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
    int64_t n = 0;
    return tfp_search_sliding_pcm_batch(g->eng[s], pcm, offsets, nrec, sr, P, window, hop, scopes, k, o, c, nw, &n);
  });
}

// Aligned search on a group: the ranked search above, then every kept row aligned on the shard
// that holds its clip (tfp_align_batch with the shard-local clip id; -1 for the other shards' rows).
int tfp_group_search_aligned_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                                   const tfp_search_params* P, int32_t k, tfp_candidate* cand, tfp_alignment* align,
                                   int32_t* counts) {
  if (!g || !qoff) return TFP_E_ARG;
  if (!align) return gfail(g, TFP_E_ARG, "aligned search: NULL output");
  std::lock_guard<std::recursive_mutex> lk(g->mu);  // (the shards' clips stay as ranked until they are aligned)
  std::vector<int32_t> kept;
  int rc = group_rank(
      g, nq, P, k, cand, counts,
      [&](int s, tfp_candidate* o, int32_t* c) { return tfp_search_ranked_batch(g->eng[s], frames, qoff, nq, P, k, o, c); },
      &kept);
  if (rc) return rc;
  const size_t np = (size_t)nq * k;
  memset(align, 0, sizeof(tfp_alignment) * np);
  if (!np) return TFP_OK;
  const int n = (int)g->eng.size();
  std::vector<std::vector<int32_t>> ids(n, std::vector<int32_t>(np, -1));
  std::vector<char> used(n, 0);
  for (size_t p = 0; p < np; p++)
    if (kept[p] >= 0) {
      const Member& mb = g->members[kept[p]];
      ids[mb.shard][p] = mb.id;
      used[mb.shard] = 1;
    }
  std::vector<std::vector<tfp_alignment>> res(n, std::vector<tfp_alignment>(np));
  rc = run_all(g, [&](int s) {
    return used[s] ? tfp_align_batch(g->eng[s], frames, qoff, nq, P, ids[s].data(), k, res[s].data()) : TFP_OK;
  });
  if (rc) return rc;
  for (size_t p = 0; p < np; p++)
    if (kept[p] >= 0) align[p] = res[g->members[kept[p]].shard][p];
  return TFP_OK;
}

// Sliding aligned search on a group (tfp_slide_align.hpp): the sliding search above, then every kept
// row aligned on the shard that holds its clip (tfp_align_sliding_batch with the shard-local clip id;
// -1 for the other shards' rows), a window in a query's place.
int tfp_group_search_sliding_aligned_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nrec,
                                           const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes,
                                           int32_t k, tfp_candidate* out, int32_t* counts, tfp_alignment* align,
                                           int64_t cap_windows, int64_t* nwindows) {
  if (!g || !qoff) return TFP_E_ARG;
  if (k < 1 || k > TFP_RANK_MAX || !valid_params(P)) return gfail(g, TFP_E_ARG, "sliding search: k or coefs out of range");
  int32_t nw = 0;
  if (int rc = group_slide_windows(g, qoff, nrec, false, window, hop, scopes, cap_windows, nwindows, &nw)) return rc;
  if (!nw) return TFP_OK;
  if (!align) return gfail(g, TFP_E_ARG, "sliding aligned search: NULL output");
  std::lock_guard<std::recursive_mutex> lk(g->mu);  // (the shards' clips stay as ranked until they are aligned)
  std::vector<int32_t> kept;
  int rc = group_rank(
      g, nw, P, k, out, counts,
      [&](int s, tfp_candidate* o, int32_t* c) {
        int64_t n = 0;
        return tfp_search_sliding_batch(g->eng[s], frames, qoff, nrec, P, window, hop, scopes, k, o, c, nw, &n);
      },
      &kept);
  if (rc) return rc;
  const size_t np = (size_t)nw * k;
  memset(align, 0, sizeof(tfp_alignment) * np);
  const int n = (int)g->eng.size();
  std::vector<std::vector<int32_t>> ids(n, std::vector<int32_t>(np, -1));
  std::vector<char> used(n, 0);
  for (size_t p = 0; p < np; p++)
    if (kept[p] >= 0) {
      const Member& mb = g->members[kept[p]];
      ids[mb.shard][p] = mb.id;
      used[mb.shard] = 1;
    }
  std::vector<std::vector<tfp_alignment>> res(n, std::vector<tfp_alignment>(np));
  rc = run_all(g, [&](int s) {
    int64_t got = 0;
    return used[s] ? tfp_align_sliding_batch(g->eng[s], frames, qoff, nrec, P, window, hop, ids[s].data(), k,
                                             res[s].data(), nw, &got)
                   : TFP_OK;
  });
  if (rc) return rc;
  for (size_t p = 0; p < np; p++)
    if (kept[p] >= 0) align[p] = res[g->members[kept[p]].shard][p];
  return TFP_OK;
}

// Occurrence search on a group (tfp_occur.hpp): the rows of the sliding aligned search above, each
// candidate (recording, clip, start) traced on the shard that holds its clip (tfp_trace_batch with
// the shard-local clip id), then the suppression per (recording, audio_uuid) and the output order over
// all shards' candidates. A clip is numbered by its member index here; clip_id out is its shard.
int tfp_group_search_occurrences_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoff, int32_t nrec,
                                       const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes,
                                       int32_t k, int32_t max_gap, int32_t min_hits, tfp_occurrence* out, int64_t cap,
                                       int64_t* nocc) {
  if (!g || !qoff) return TFP_E_ARG;
  if (!nocc) return gfail(g, TFP_E_ARG, "occurrence search: NULL noccurrences");
  if (max_gap < 0 || min_hits < 1)
    return gfail(g, TFP_E_ARG, "occurrence search: max_gap = %d, min_hits = %d", max_gap, min_hits);
  if (k < 1 || k > TFP_RANK_MAX || !valid_params(P)) return gfail(g, TFP_E_ARG, "sliding search: k or coefs out of range");
  int32_t nw = 0;
  int64_t got = 0;
  if (int rc = group_slide_windows(g, qoff, nrec, false, window, hop, scopes, INT32_MAX, &got, &nw)) return rc;
  *nocc = 0;
  if (!nw) return TFP_OK;
  std::lock_guard<std::recursive_mutex> lk(g->mu);  // (the shards' clips stay as ranked until they are traced)
  std::vector<tfp_candidate> cand((size_t)nw * k);
  std::vector<int32_t> counts((size_t)nw);
  std::vector<tfp_alignment> align((size_t)nw * k);
  int rc = tfp_group_search_sliding_aligned_batch(g, frames, qoff, nrec, P, window, hop, scopes, k, cand.data(), counts.data(),
                                                  align.data(), nw, &got);
  if (rc) return rc;
  std::vector<tfp::OccurRow> rows;
  int64_t j = 0;
  for (int32_t r = 0; r < nrec; r++) {
    const int64_t n = tfp_sliding_windows(qoff[r + 1] - qoff[r], window, hop);
    for (int64_t w = 0; w < n; w++, j++)
      for (int32_t i = 0; i < counts[j]; i++)
        rows.push_back(tfp::OccurRow{r, g->where.at(cand[j * k + i].uuid), w, align[j * k + i].offset});
  }
  const std::vector<tfp::OccurCand> cands = tfp::occur_candidates(rows, hop);
  const int n = (int)g->eng.size();
  std::vector<std::vector<tfp_trace_req>> reqs(n);
  std::vector<std::vector<size_t>> slot(n);
  for (size_t i = 0; i < cands.size(); i++) {
    const Member& mb = g->members[cands[i].clip];
    reqs[mb.shard].push_back(tfp_trace_req{cands[i].rec, mb.id, cands[i].s, 0});
    slot[mb.shard].push_back(i);
  }
  std::vector<std::vector<tfp_trace>> res(n);
  for (int s = 0; s < n; s++) res[s].resize(reqs[s].size());
  rc = run_all(g, [&](int s) {
    return reqs[s].empty() ? TFP_OK
                           : tfp_trace_batch(g->eng[s], frames, qoff, nrec, P, reqs[s].data(), (int64_t)reqs[s].size(),
                                             max_gap, res[s].data());
  });
  if (rc) return rc;
  std::vector<tfp::TraceOut> tr(cands.size());
  static_assert(sizeof(tfp_trace) == sizeof(tfp::TraceOut), "tfp_occur.hpp and the public header agree");
  for (int s = 0; s < n; s++)
    for (size_t i = 0; i < slot[s].size(); i++) memcpy(&tr[slot[s][i]], &res[s][i], sizeof(tfp_trace));
  const std::vector<int64_t> kept =
      tfp::occur_select(cands, tr.data(), min_hits, [&](int32_t mi) { return g->members[mi].uuid.c_str(); });
  *nocc = (int64_t)kept.size();
  if (*nocc > cap)
    return gfail(g, TFP_E_CAPACITY, "occurrence search: %lld occurrences, room for %lld", (long long)*nocc, (long long)cap);
  if (*nocc && !out) return gfail(g, TFP_E_ARG, "occurrence search: NULL output");
  for (size_t i = 0; i < kept.size(); i++) {
    const tfp::OccurCand& c = cands[(size_t)kept[i]];
    const tfp::TraceOut& t = tr[(size_t)kept[i]];
    const Member& mb = g->members[c.clip];
    tfp_occurrence& o = out[i];
    memset(&o, 0, sizeof o);
    o.recording = c.rec;
    o.clip_id = mb.shard;
    o.clip_start_frame = c.s;
    o.first_frame = t.seg_first;
    o.last_frame = t.seg_last;
    o.hits = t.seg_hits;
    o.diagonal_hits = t.hits;
    o.overlap = t.overlap;
    o.windows = c.windows;
    snprintf(o.uuid, sizeof o.uuid, "%s", mb.uuid.c_str());
  }
  return TFP_OK;
}

namespace {
// One search over host samples on every shard (each fingerprints the whole batch: no exchange on
// the latency path), combined by the integer max of the keys.
int group_search_direct(tfp_group* g, const void* const* ptrs, const int64_t* lens, int32_t nq, bool f32, int32_t sr,
                        const tfp_search_params* P, tfp_result* out) {
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  std::vector<std::vector<tfp_result>> res(n, std::vector<tfp_result>(std::max(nq, 1)));
  rc = run_all(g, [&](int s) { return tfp_internal_search_gather(g->eng[s], ptrs, lens, nq, f32, sr, P, res[s].data()); });
  if (rc) return rc;
  combine(g, res, nq, out);
  return TFP_OK;
}

int group_search_gather(tfp_group* g, const void* const* ptrs, const int64_t* lens, int32_t nq, bool f32, int32_t sr,
                        const tfp_search_params* P, tfp_result* out) {
  if (!g || nq < 0 || !out || (nq && (!ptrs || !lens))) return TFP_E_ARG;
  for (int32_t i = 0; i < nq; i++)
    if (lens[i] < 0 || (lens[i] && !ptrs[i])) return gfail(g, TFP_E_ARG, "bad query %d", i);
  if (!g->coalesce || nq == 0 || nq > tfp::Coalescer::kMaxCallQueries)
    return group_search_direct(g, ptrs, lens, nq, f32, sr, P, out);
  tfp::SearchReq r;
  r.ptrs.assign(ptrs, ptrs + nq);
  r.lens.assign(lens, lens + nq);
  r.f32 = f32;
  r.sr = sr;
  if (P) r.P = *P;
  else r.P.coefs = 0;  // (invalid: NULL results, fp_handler.c:247-250)
  r.out = out;
  const int rc = g->coal.submit(&r, [g](std::vector<tfp::SearchReq*>& batch) {
    tfp::exec_batch(
        batch,
        [g](const void* const* p, const int64_t* l, int32_t n, bool f, int32_t rate, const tfp_search_params* q,
            tfp_result* o) { return group_search_direct(g, p, l, n, f, rate, q, o); },
        [g] { return std::string(tfp_group_last_error(g)); });
  });
  if (rc) g->err.note(g, r.err.c_str());  // (the leader ran it: the message into this caller's slot)
  return rc;
}

int group_search_samples(tfp_group* g, const void* x, bool f32, const int64_t* offsets, int32_t nq, int32_t sr,
                         const tfp_search_params* P, tfp_result* out) {
  if (!g || !offsets || nq < 0 || !out) return TFP_E_ARG;
  for (int32_t i = 0; i < nq; i++)
    if (offsets[i + 1] < offsets[i]) return gfail(g, TFP_E_ARG, "offsets not monotone");
  if (!x && nq && offsets[nq] > offsets[0]) return gfail(g, TFP_E_ARG, "samples are NULL");
  const int n = (int)g->eng.size();
  // throughput batches of equal-length int16 queries: query-sharded (fingerprint once, exchange)
  bool equal = nq > 0;
  for (int32_t i = 0; i < nq && equal; i++) equal = offsets[i + 1] - offsets[i] == offsets[1] - offsets[0];
  if (!f32 && n > 1 && equal && nq >= 64 * n && offsets[1] > offsets[0] && valid_params(P)) {
    std::lock_guard<std::recursive_mutex> lk(g->mu);
    const int rc = refresh_ranks(g);
    return rc ? rc : search_sharded(g, x, -1, offsets, nq, sr, P, out);
  }
  const size_t ss = f32 ? sizeof(float) : sizeof(int16_t);
  std::vector<const void*> ptrs(nq);
  std::vector<int64_t> lens(nq);
  for (int32_t i = 0; i < nq; i++) {
    ptrs[i] = static_cast<const char*>(x) + ss * offsets[i];
    lens[i] = offsets[i + 1] - offsets[i];
  }
  return group_search_gather(g, ptrs.data(), lens.data(), nq, f32, sr, P, out);
}
}  // namespace

int tfp_group_search_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                               const tfp_search_params* P, tfp_result* out) {
  return group_search_samples(g, pcm, false, offsets, nq, sr, P, out);
}

int tfp_group_search_f32_batch(tfp_group* g, const float* x, const int64_t* offsets, int32_t nq, int32_t sr,
                               const tfp_search_params* P, tfp_result* out) {
  return group_search_samples(g, x, true, offsets, nq, sr, P, out);
}

// Codes in: throughput batches of equal-length queries are query-sharded as the int16 form's are
// (each shard expands and fingerprints its share, the frame values are exchanged); every other batch
// is expanded and fingerprinted by every shard. Not coalesced (as tfp_search_g711_batch).
int tfp_group_search_g711_batch(tfp_group* g, const uint8_t* codes, const int64_t* offsets, int32_t nq, int32_t law,
                                int32_t sr, const tfp_search_params* P, tfp_result* out) {
  if (!g || !offsets || nq < 0 || !out) return TFP_E_ARG;
  if (!tfp::g711_law_ok(law)) return gfail(g, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  for (int32_t i = 0; i < nq; i++)
    if (offsets[i + 1] < offsets[i]) return gfail(g, TFP_E_ARG, "offsets not monotone");
  if (!codes && nq && offsets[nq] > offsets[0]) return gfail(g, TFP_E_ARG, "codes are NULL");
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  bool equal = nq > 0;
  for (int32_t i = 0; i < nq && equal; i++) equal = offsets[i + 1] - offsets[i] == offsets[1] - offsets[0];
  if (n > 1 && equal && nq >= 64 * n && offsets[1] > offsets[0] && valid_params(P))
    return search_sharded(g, codes, law, offsets, nq, sr, P, out);
  std::vector<std::vector<tfp_result>> res(n, std::vector<tfp_result>(std::max(nq, 1)));
  rc = run_all(g, [&](int s) { return tfp_internal_search_g711(g->eng[s], codes, offsets, nq, law, sr, P, res[s].data()); });
  if (rc) return rc;
  combine(g, res, nq, out);
  return TFP_OK;
}

// int16 at another rate: every shard resamples and fingerprints the batch (no exchange), combined as the
// direct pcm search's results are. Equal rates are the pcm form. Not coalesced (as tfp_search_rate_batch).
int tfp_group_search_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t rate_in,
                                int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!g) return TFP_E_ARG;
  tfp::ResamplePlan rp;
  if (int rc = group_rate_plan(g, rate_in, rate_out, &rp)) return rc;
  if (rate_in == rate_out) return tfp_group_search_pcm_batch(g, pcm, offsets, nq, rate_out, P, out);
  if (!offsets || nq < 0 || !out) return TFP_E_ARG;
  for (int32_t i = 0; i < nq; i++)
    if (offsets[i + 1] < offsets[i]) return gfail(g, TFP_E_ARG, "offsets not monotone");
  if (!pcm && nq && offsets[nq] > offsets[0]) return gfail(g, TFP_E_ARG, "samples are NULL");
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  std::vector<std::vector<tfp_result>> res(n, std::vector<tfp_result>(std::max(nq, 1)));
  rc = run_all(g, [&](int s) { return tfp_search_rate_batch(g->eng[s], pcm, offsets, nq, rate_in, rate_out, P, res[s].data()); });
  if (rc) return rc;
  combine(g, res, nq, out);
  return TFP_OK;
}

// Interleaved multichannel int16: every shard downmixes, converts and fingerprints the batch, combined
// as the rate twin's results are. One channel is the rate form. Not coalesced.
int tfp_group_search_mix_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t channels,
                                    int32_t rate_in, int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!g) return TFP_E_ARG;
  if (channels == 1) return tfp_group_search_rate_batch(g, pcm, offsets, nq, rate_in, rate_out, P, out);
  tfp::ResamplePlan rp;
  if (int rc = group_mix_plan(g, channels, rate_in, rate_out, &rp)) return rc;
  if (!offsets || nq < 0 || !out) return TFP_E_ARG;
  for (int32_t i = 0; i < nq; i++)
    if (offsets[i + 1] < offsets[i]) return gfail(g, TFP_E_ARG, "offsets not monotone");
  if (!pcm && nq && offsets[nq] > offsets[0]) return gfail(g, TFP_E_ARG, "samples are NULL");
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  std::vector<std::vector<tfp_result>> res(n, std::vector<tfp_result>(std::max(nq, 1)));
  rc = run_all(g, [&](int s) {
    return tfp_search_mix_rate_batch(g->eng[s], pcm, offsets, nq, channels, rate_in, rate_out, P, res[s].data());
  });
  if (rc) return rc;
  combine(g, res, nq, out);
  return TFP_OK;
}

// The wide twin: every shard converts and fingerprints the Q31 batch. Not coalesced.
int tfp_group_search_wide_rate_batch(tfp_group* g, const int32_t* q31, const int64_t* offsets, int32_t nq, int32_t channels,
                                     int32_t rate_in, int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!g) return TFP_E_ARG;
  tfp::ResamplePlan rp;
  if (int rc = group_wide_plan(g, channels, rate_in, rate_out, &rp)) return rc;
  if (!offsets || nq < 0 || !out) return TFP_E_ARG;
  for (int32_t i = 0; i < nq; i++)
    if (offsets[i + 1] < offsets[i]) return gfail(g, TFP_E_ARG, "offsets not monotone");
  if (!q31 && nq && offsets[nq] > offsets[0]) return gfail(g, TFP_E_ARG, "samples are NULL");
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  std::vector<std::vector<tfp_result>> res(n, std::vector<tfp_result>(std::max(nq, 1)));
  rc = run_all(g, [&](int s) {
    return tfp_search_wide_rate_batch(g->eng[s], q31, offsets, nq, channels, rate_in, rate_out, P, res[s].data());
  });
  if (rc) return rc;
  combine(g, res, nq, out);
  return TFP_OK;
}

// The mixed twin: every shard converts (one launch) and fingerprints the batch. Not coalesced.
int tfp_group_search_any_batch(tfp_group* g, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nq,
                               int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!g) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);  // (before the first message is written)
  if (!out) return gfail(g, TFP_E_ARG, "bad arguments");
  tfp::AnyBatch B;
  if (int rc = group_any_batch(g, data, nbytes, clips, nq, rate_out, &B)) return rc;
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  std::vector<std::vector<tfp_result>> res(n, std::vector<tfp_result>(std::max(nq, 1)));
  rc = run_all(g, [&](int s) { return tfp_search_any_batch(g->eng[s], data, nbytes, clips, nq, rate_out, P, res[s].data()); });
  if (rc) return rc;
  combine(g, res, nq, out);
  return TFP_OK;
}

int tfp_group_search_pcm_gather(tfp_group* g, const int16_t* const* pcms, const int64_t* nsamples, int32_t nq,
                                int32_t sr, const tfp_search_params* P, tfp_result* out) {
  return group_search_gather(g, reinterpret_cast<const void* const*>(pcms), nsamples, nq, false, sr, P, out);
}

int tfp_group_search_coalesce_stats(tfp_group* g, int64_t* calls, int64_t* batches) {
  if (!g) return TFP_E_ARG;
  g->coal.stats(calls, batches);
  return TFP_OK;
}

int tfp_group_stream_create(tfp_group* g, int32_t nch, int32_t sr, int64_t W, tfp_group_stream** out) {
  if (!g || nch <= 0 || W <= 0 || !out) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  *out = nullptr;
  tfp_group_stream* st = new tfp_group_stream();
  const int n = (int)g->eng.size();
  st->g = g;
  st->nch = nch;
  st->W = W;
  const char* mode = tfp::op_env("TFP_GROUP_STREAM");  // operational switch
  st->split = n > 1 && !(mode && !strcmp(mode, "replicate"));
  st->st.assign(n, nullptr);
  if (st->split) {
    st->chans.assign(n, {});
    for (int32_t c = 0; c < nch; c++) st->chans[c % n].push_back(c);
    st->tick.assign(n, {});
    st->act.assign(n, {});
    st->nact.assign(n, 0);
    st->keys.assign(n, {});
    for (int s = 0; s < n; s++) st->act[s].assign(st->chans[s].size(), 0);
  }
  const int rc = run_all(g, [&](int s) {
    if (!st->split) return tfp_stream_create(g->eng[s], nch, sr, W, &st->st[s]);
    return st->chans[s].empty() ? TFP_OK : tfp_stream_create(g->eng[s], (int32_t)st->chans[s].size(), sr, W, &st->st[s]);
  });
  if (rc) {
    for (auto* p : st->st) tfp_stream_destroy(p);
    delete st;
    return rc;
  }
  st->res.assign(g->eng.size(), std::vector<tfp_result>(nch));
  *out = st;
  return TFP_OK;
}

void tfp_group_stream_destroy(tfp_group_stream* st) {
  if (!st) return;
  for (auto* p : st->st) tfp_stream_destroy(p);
  delete st;
}

int tfp_group_stream_reset(tfp_group_stream* st, int32_t ch) {
  if (!st || ch >= st->nch) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(st->g->mu);
  if (st->split) {
    const int n = (int)st->g->eng.size();
    if (ch >= 0) return tfp_stream_reset(st->st[ch % n], ch / n);  // channel c is local channel c / N of shard c mod N
    return run_all(st->g, [&](int s) { return st->st[s] ? tfp_stream_reset(st->st[s], -1) : TFP_OK; });
  }
  return run_all(st->g, [&](int s) { return tfp_stream_reset(st->st[s], ch); });
}

namespace {

// A tick of a split-channel stream: (1) every shard pushes its channels' rows and fingerprints its
// full windows into its sfp buffer; (2) every shard gathers all shards' window values in shard
// order (hipMemcpyPeerAsync; a device copy when a device repeats) and matches them against its
// clips; (3) per window, the greatest key over the shards.
// law < 0: pcm is int16[nch][T]; else G.711 codes uint8[nch][T] (the shards' rows are regrouped as
// bytes and each shard's scatter expands them).
int split_stream_push(tfp_group_stream* st, const void* pcm, int32_t law, int32_t T, const tfp_search_params* P,
                      tfp_result* out) {
  tfp_group* g = st->g;
  const int n = (int)g->eng.size();
  const size_t row = (law < 0 ? sizeof(int16_t) : sizeof(uint8_t)) * (size_t)T;  // bytes of a channel's tick
  for (int s = 0; s < n; s++) {
    const auto& ch = st->chans[s];
    st->tick[s].resize((ch.size() * row + 1) / sizeof(int16_t));
    for (size_t j = 0; j < ch.size(); j++)
      memcpy(reinterpret_cast<char*>(st->tick[s].data()) + j * row, static_cast<const char*>(pcm) + (size_t)ch[j] * row, row);
  }
  const bool match = valid_params(P);
  const int64_t F = tfp_frame_count(st->W);
  int rc = run_all(g, [&](int s) -> int {
    st->nact[s] = 0;
    if (!st->st[s]) return TFP_OK;
    ShardBufs& b = g->bufs[s];
    if (hipSetDevice(g->dev[s]) != hipSuccess) return TFP_E_HIP;
    const int64_t cap = (int64_t)st->chans[s].size() * F;
    if (match && grow(&b.sfp, &b.b_sfp, sizeof(double) * 2 * (size_t)(cap + 1)) != hipSuccess) return TFP_E_NOMEM;
    int64_t fw = 0;
    return tfp_internal_stream_fp(st->st[s], st->tick[s].data(), law, T, match ? P : nullptr, (double*)b.sfp, cap,
                                  st->act[s].data(), &st->nact[s], &fw);
  });
  if (rc || !P) return rc;
  for (int32_t c = 0; c < st->nch; c++) {
    memset(&out[c], 0, sizeof out[c]);
    out[c].clip_id = -1;
  }
  std::vector<int32_t> base(n + 1, 0);
  for (int s = 0; s < n; s++) base[s + 1] = base[s] + st->nact[s];
  const int32_t na = base[n];
  if (!match || !na) return TFP_OK;
  std::vector<int64_t> qoff(na + 1);
  for (int32_t i = 0; i <= na; i++) qoff[i] = F * i;
  rc = run_all(g, [&](int s) -> int {
    ShardBufs& b = g->bufs[s];
    if (hipSetDevice(g->dev[s]) != hipSuccess) return TFP_E_HIP;
    if (!b.stream && hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking) != hipSuccess) return TFP_E_HIP;
    if (grow(&b.q, &b.b_q, sizeof(double) * 2 * (size_t)(na * F + 1)) != hipSuccess ||
        grow(&b.keys, &b.b_keys, sizeof(unsigned long long) * (size_t)(na + 1)) != hipSuccess)
      return TFP_E_NOMEM;
    for (int o = 0; o < n; o++) {
      if (!st->nact[o]) continue;
      const size_t off = sizeof(double) * 2 * (size_t)(F * base[o]), bytes = sizeof(double) * 2 * (size_t)(F * st->nact[o]);
      if (const hipError_t pe = hipMemcpyPeerAsync((char*)b.q + off, g->dev[s], g->bufs[o].sfp, g->dev[o], bytes, b.stream);
          pe != hipSuccess)
        return gfail(g, TFP_E_HIP, "stream windows of shard %d (device %d) to shard %d (device %d): hipMemcpyPeerAsync: %s", o,
                     g->dev[o], s, g->dev[s], hipGetErrorString(pe));
    }
    st->keys[s].resize(na);
    int r = tfp_search_q_device(g->eng[s], (const double*)b.q, qoff.data(), na, P, (uint64_t*)b.keys, b.stream);
    if (r) return r;
    if (hipMemcpyAsync(st->keys[s].data(), b.keys, sizeof(unsigned long long) * na, hipMemcpyDeviceToHost, b.stream) !=
            hipSuccess ||
        hipStreamSynchronize(b.stream) != hipSuccess)
      return TFP_E_HIP;
    return TFP_OK;
  });
  if (rc) return rc;
  for (int o = 0; o < n; o++)
    for (int32_t j = 0; j < st->nact[o]; j++) {
      const int32_t i = base[o] + j;
      unsigned long long k = 0ull;
      for (int s = 0; s < n; s++) k = std::max(k, st->keys[s][i]);
      fill_from_key(g, k, (int32_t)F, &out[st->chans[o][st->act[o][j]]]);
    }
  return TFP_OK;
}

}  // namespace

namespace {
int group_stream_push(tfp_group_stream* st, const void* pcm, int32_t law, int32_t tick, const tfp_search_params* P,
                      tfp_result* out) {
  if (!st || !pcm || tick <= 0 || (P && !out)) return TFP_E_ARG;
  tfp_group* g = st->g;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  int rc = P ? refresh_ranks(g) : TFP_OK;
  if (rc) return rc;
  if (st->split) return split_stream_push(st, pcm, law, tick, P, out);
  rc = run_all(g, [&](int s) {
    tfp_result* r = P ? st->res[s].data() : nullptr;
    return law < 0 ? tfp_stream_push(st->st[s], (const int16_t*)pcm, tick, P, r)
                   : tfp_stream_push_g711(st->st[s], (const uint8_t*)pcm, tick, law, P, r);
  });
  if (rc || !P) return rc;
  combine(g, st->res, st->nch, out);
  return TFP_OK;
}
}  // namespace

int tfp_group_stream_push(tfp_group_stream* st, const int16_t* pcm, int32_t tick, const tfp_search_params* P,
                          tfp_result* out) {
  return group_stream_push(st, pcm, -1, tick, P, out);
}

int tfp_group_stream_push_g711(tfp_group_stream* st, const uint8_t* codes, int32_t tick, int32_t law,
                               const tfp_search_params* P, tfp_result* out) {
  if (!st) return TFP_E_ARG;
  if (!tfp::g711_law_ok(law)) return gfail(st->g, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  return group_stream_push(st, codes, law, tick, P, out);
}

// ---- live calls on a group (tfp_live.hpp): every shard keeps every channel ------------------------

struct tfp_group_live {
  tfp_group* g = nullptr;
  std::vector<tfp_live*> lv;     // one per shard
  int32_t nch = 0;
  int64_t max_samples = 0;
  std::vector<int64_t> samples;  // per channel, as every shard counts them (the capacity check before any shard is told)
  // a rate object (tfp_live_rate.hpp): the shards take the tick at rate_in; samples is then the settled
  // count and in_samples the input samples, both as every shard counts them
  bool rated = false;
  tfp::ResamplePlan rs_plan{};
  std::vector<int64_t> in_samples;
  // tfp_group_live_occurrences: per channel the merged list, each track also on its clip's shard (whose
  // engine carries its trace); `windows` is counted here, over the merged rows
  struct Track {
    int32_t member;
    std::string uuid;  // the member's, checked with the index (tfp_group_index_clear starts them again)
    int32_t s, windows;
    tfp_trace last;    // its trace as of the last occurrence call
  };
  std::vector<std::vector<Track>> tracks;
  int64_t n_occ_calls = 0, n_tr_added = 0, n_tr_dropped = 0;
};

int tfp_group_live_create(tfp_group* g, int32_t nch, int32_t sr, int64_t max_samples, tfp_group_live** out) {
  return tfp_group_live_create_rate(g, nch, sr, sr, max_samples, out);
}

int tfp_group_live_create_rate(tfp_group* g, int32_t nch, int32_t rate_in, int32_t sr, int64_t max_samples,
                               tfp_group_live** out) {
  if (!g || !out) return TFP_E_ARG;
  *out = nullptr;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  tfp_group_live* gl = new tfp_group_live();
  gl->g = g;
  gl->nch = nch;
  gl->max_samples = max_samples;
  gl->lv.assign(g->eng.size(), nullptr);
  bool bad = false;  // (a pair the plan refuses is refused by every shard, with the message)
  gl->rated = rate_in != sr && tfp::resample_plan(rate_in, sr, &gl->rs_plan, &bad);
  gl->in_samples.assign(gl->rated && nch > 0 ? nch : 0, 0);
  const int rc = run_all(g, [&](int s) { return tfp_live_create_rate(g->eng[s], nch, rate_in, sr, max_samples, &gl->lv[s]); });
  if (rc) {
    for (auto* p : gl->lv) tfp_live_destroy(p);
    delete gl;
    return rc;
  }
  gl->samples.assign(nch, 0);
  gl->tracks.assign(nch, {});
  *out = gl;
  return TFP_OK;
}

void tfp_group_live_destroy(tfp_group_live* gl) {
  if (!gl) return;
  for (auto* p : gl->lv) tfp_live_destroy(p);
  delete gl;
}

int tfp_group_live_reset(tfp_group_live* gl, int32_t ch) {
  if (!gl || ch >= gl->nch) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(gl->g->mu);
  const int rc = run_all(gl->g, [&](int s) { return tfp_live_reset(gl->lv[s], ch); });
  if (rc) return rc;
  for (int32_t c = ch < 0 ? 0 : ch; c < (ch < 0 ? gl->nch : ch + 1); c++) {
    gl->samples[c] = 0, gl->tracks[c].clear();
    if (gl->rated) gl->in_samples[c] = 0;
  }
  return TFP_OK;
}

int tfp_group_live_input_samples(tfp_group_live* gl, int32_t ch, int64_t* nsamples) {
  if (!gl || ch < 0 || ch >= gl->nch || !nsamples) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(gl->g->mu);
  *nsamples = gl->rated ? gl->in_samples[ch] : gl->samples[ch];
  return TFP_OK;
}

int tfp_group_live_rate_info(tfp_group_live* gl, int32_t* rate_in, int64_t* lag_in) {
  if (!gl) return TFP_E_ARG;
  return tfp_live_rate_info(gl->lv[0], rate_in, lag_in);  // (every shard was created alike)
}

int tfp_group_live_rate_stats(tfp_group_live* gl, int32_t shard, int64_t* launches, int64_t* samples_in, int64_t* samples_out) {
  if (!gl || shard < 0 || (size_t)shard >= gl->lv.size()) return TFP_E_ARG;
  return tfp_live_rate_stats(gl->lv[shard], launches, samples_in, samples_out);
}

int tfp_group_live_samples(tfp_group_live* gl, int32_t ch, int64_t* nsamples) {
  if (!gl || ch < 0 || ch >= gl->nch || !nsamples) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(gl->g->mu);
  *nsamples = gl->samples[ch];
  return TFP_OK;
}

int tfp_group_live_stats(tfp_group_live* gl, int32_t shard, int64_t* incremental_pushes, int64_t* general_pushes,
                         int64_t* rebuilds, int64_t* frames_fingerprinted, int64_t* frames_added) {
  if (!gl || shard < 0 || (size_t)shard >= gl->lv.size()) return TFP_E_ARG;
  return tfp_live_stats(gl->lv[shard], incremental_pushes, general_pushes, rebuilds, frames_fingerprinted, frames_added);
}

}  // extern "C"

namespace {
// One shard's push: int16 samples (law < 0) or G.711 codes of that law.
int shard_live_push(tfp_live* lv, const void* pcm, int32_t law, int32_t T, const int32_t* nsamples, const tfp_search_params* P,
                    const int32_t* scopes, int32_t k, tfp_candidate* o, int32_t* c, int32_t* frame_counts) {
  return law < 0 ? tfp_live_push(lv, (const int16_t*)pcm, T, nsamples, P, scopes, k, o, c, frame_counts)
                 : tfp_live_push_g711(lv, (const uint8_t*)pcm, T, law, nsamples, P, scopes, k, o, c, frame_counts);
}

// tfp_group_live_push (law < 0) and tfp_group_live_push_g711: the tick's source is the only difference.
int group_live_push(tfp_group_live* gl, const void* pcm, int32_t law, int32_t T, const int32_t* nsamples,
                    const tfp_search_params* P, const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                    int32_t* frame_counts) {
  tfp_group* g = gl->g;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int32_t nch = gl->nch;
  if (!pcm || T <= 0) return gfail(g, TFP_E_ARG, "live push: NULL samples or tick_samples %d", T);
  for (int32_t c = 0; nsamples && c < nch; c++)
    if (nsamples[c] < 0 || nsamples[c] > T)
      return gfail(g, TFP_E_ARG, "live push: nsamples[%d] = %d outside [0, %d]", c, nsamples[c], T);
  if (P) {
    if (!out || !counts) return gfail(g, TFP_E_ARG, "live push: NULL output");
    if (k < 1 || k > TFP_RANK_MAX) return gfail(g, TFP_E_ARG, "live push: k = %d outside [1, %d]", k, TFP_RANK_MAX);
    if (scopes)
      if (int rc = group_scope_args(g, scopes, nch)) return rc;
  }
  std::vector<int64_t> settled(nch);  // what each channel's history gains (a rate object: its newly settled samples)
  for (int32_t c = 0; c < nch; c++) {  // before any shard is told: a capacity failure leaves every shard unchanged
    settled[c] = nsamples ? nsamples[c] : T;
    if (gl->rated) {
      tfp::LiveRateStep st;
      if (!tfp::live_rate_step(gl->rs_plan, gl->in_samples[c], settled[c], &st))
        return gfail(g, TFP_E_ARG, "live push: channel %d past the index range", c);
      settled[c] = st.n_new;  // (st.n_old = gl->samples[c])
    }
    if (gl->samples[c] + settled[c] > gl->max_samples)
      return gfail(g, TFP_E_CAPACITY, "live push: channel %d past %lld samples", c, (long long)gl->max_samples);
  }
  int rc;
  if (P && valid_params(P)) {
    // each shard's first k rows of every channel, merged as scoped search's (shard 0 reports the frame counts)
    rc = group_rank(g, nch, P, k, out, counts, [&](int s, tfp_candidate* o, int32_t* c) {
      return shard_live_push(gl->lv[s], pcm, law, T, nsamples, P, scopes, k, o, c, s == 0 ? frame_counts : nullptr);
    });
  } else {
    // ingest only; with invalid params the rows come out empty (fp_handler.c:247-250)
    std::vector<tfp_candidate> o(P ? (size_t)nch * k : 0);
    std::vector<int32_t> cn(P ? nch : 0);
    rc = run_all(g, [&](int s) {
      return shard_live_push(gl->lv[s], pcm, law, T, nsamples, s == 0 ? P : nullptr, scopes, k, o.data(), cn.data(), frame_counts);
    });
    if (!rc && P) {
      memset(out, 0, sizeof(tfp_candidate) * (size_t)nch * k);
      memset(counts, 0, sizeof(int32_t) * nch);
    }
  }
  if (rc) return rc;
  for (int32_t c = 0; c < nch; c++) {
    gl->samples[c] += settled[c];
    if (gl->rated) gl->in_samples[c] += nsamples ? nsamples[c] : T;
  }
  return TFP_OK;
}
}  // namespace

extern "C" {

int tfp_group_live_push(tfp_group_live* gl, const int16_t* pcm, int32_t T, const int32_t* nsamples,
                        const tfp_search_params* P, const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                        int32_t* frame_counts) {
  if (!gl) return TFP_E_ARG;
  return group_live_push(gl, pcm, -1, T, nsamples, P, scopes, k, out, counts, frame_counts);
}

int tfp_group_live_push_g711(tfp_group_live* gl, const uint8_t* codes, int32_t T, int32_t law, const int32_t* nsamples,
                             const tfp_search_params* P, const int32_t* scopes, int32_t k, tfp_candidate* out,
                             int32_t* counts, int32_t* frame_counts) {
  if (!gl) return TFP_E_ARG;
  if (!tfp::g711_law_ok(law)) return gfail(gl->g, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  return group_live_push(gl, codes, law, T, nsamples, P, scopes, k, out, counts, frame_counts);
}

int tfp_group_live_verdict(tfp_group_live* gl, const int64_t* total, const tfp_search_params* P, const int32_t* scopes,
                           struct tfp_live_verdict* out) {
  if (!gl || !out) return TFP_E_ARG;
  tfp_group* g = gl->g;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int32_t nch = gl->nch;
  // before any shard is told: a refused call brings no shard's count rows up to date
  char msg[160];
  if (!tfp::live_verdict_args_ok(total, P ? &P->coefs : nullptr, scopes, gl->samples.data(), nch, gl->max_samples, msg, sizeof msg))
    return gfail(g, TFP_E_ARG, "%s", msg);
  int rc = refresh_ranks(g);
  if (rc) return rc;
  const int n = (int)g->eng.size();
  std::vector<std::vector<unsigned long long>> keys(n, std::vector<unsigned long long>((size_t)nch * 2, 0ull));
  std::vector<int32_t> bad(n, 0);
  rc = run_all(g, [&](int s) { return tfp_internal_live_verdict_keys(gl->lv[s], total, P, scopes, keys[s].data(), &bad[s]); });
  if (rc) return rc;
  const bool any_bad = std::any_of(bad.begin(), bad.end(), [](int32_t b) { return b != 0; });
  std::vector<struct tfp_live_verdict> res(nch);  // copied out on success: every failure leaves out untouched
  for (int32_t c = 0; c < nch; c++) {
    unsigned long long top[2] = {0ull, 0ull};  // the two greatest of the shards' keys (distinct: the tie keys are)
    for (int s = 0; s < n && !any_bad; s++)
      for (int r = 0; r < 2; r++) {
        const unsigned long long k = keys[s][(size_t)c * 2 + r];
        if (k > top[0]) top[1] = top[0], top[0] = k;
        else if (k > top[1]) top[1] = k;
      }
    const tfp::LiveVerdictRule r = tfp::live_verdict_rule(top[0], top[1], gl->samples[c], total[c]);
    struct tfp_live_verdict& v = res[c];
    memset(&v, 0, sizeof v);
    v.remaining = r.remaining;
    v.complete = r.complete;
    v.decided = r.decided;
    const unsigned long long side[2] = {r.leader, r.rival};
    for (int i = 0; i < 2; i++) {
      if (!(i ? r.has_rival : r.has_leader)) continue;
      const auto it = g->key2member.find((int32_t)(uint32_t)(side[i] & 0xffffffffu));
      if (it == g->key2member.end())
        return gfail(g, TFP_E_HIP, "live verdict: tie-break key %u names no clip", (unsigned)(side[i] & 0xffffffffu));
      const Member& mb = g->members[it->second];
      tfp_candidate& cd = i ? v.rival : v.leader;
      cd.match_count = (int32_t)(side[i] >> 32);
      cd.clip_id = mb.shard;
      snprintf(cd.uuid, sizeof cd.uuid, "%s", mb.uuid.c_str());
      (i ? v.has_rival : v.has_leader) = 1;
    }
  }
  std::copy(res.begin(), res.end(), out);
  return TFP_OK;
}

}  // extern "C"

namespace {
// tfp_group_live_window (aligned false) and tfp_group_live_window_aligned: the same arguments, rows, counts
// and frame ranges. Every shard keeps every channel: each answers for its own clips from its own window
// table, and the rows merge as a push's do. The frame counts and first frames come from the group's
// sample counts. Aligned: every shard aligns its own rows (tfp_live_window_aligned), and a kept row
// takes the alignment its shard computed for it, found by the shard-local clip id.
int group_live_window_call(tfp_group_live* gl, const tfp_search_params* P, const int32_t* scopes, int32_t k, int32_t window,
                           tfp_candidate* out, tfp_alignment* align, bool aligned, int32_t* counts, int32_t* frame_counts,
                           int32_t* first_frames) {
  tfp_group* g = gl->g;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int32_t nch = gl->nch;
  if (!P || !out || !counts || (aligned && !align)) return gfail(g, TFP_E_ARG, "live window: NULL params or output");
  if (window < 1) return gfail(g, TFP_E_ARG, "live window: window = %d frames", window);
  if (k < 1 || k > TFP_RANK_MAX) return gfail(g, TFP_E_ARG, "live window: k = %d outside [1, %d]", k, TFP_RANK_MAX);
  if (scopes)
    if (int rc = group_scope_args(g, scopes, nch)) return rc;
  const size_t np = (size_t)nch * k;
  if (valid_params(P)) {
    const int n = (int)g->eng.size();
    std::vector<std::vector<tfp_alignment>> sal(aligned ? n : 0, std::vector<tfp_alignment>(np));
    // each shard's rows as shard-local clip ids (-1 past its count): group_rank's own buffers end with it
    std::vector<std::vector<int32_t>> sid(aligned ? n : 0, std::vector<int32_t>(np, -1));
    std::vector<int32_t> kept;
    const int rc = group_rank(
        g, nch, P, k, out, counts,
        [&](int s, tfp_candidate* o, int32_t* c) {
          if (!aligned) return tfp_live_window(gl->lv[s], P, scopes, k, window, o, c, nullptr, nullptr);
          const int rs = tfp_live_window_aligned(gl->lv[s], P, scopes, k, window, o, sal[s].data(), c, nullptr, nullptr);
          for (int32_t ch = 0; !rs && ch < nch; ch++)
            for (int32_t r = 0; r < c[ch]; r++) sid[s][(size_t)ch * k + r] = o[(size_t)ch * k + r].clip_id;
          return rs;
        },
        aligned ? &kept : nullptr);
    if (rc) return rc;
    if (aligned) memset(align, 0, sizeof(tfp_alignment) * np);
    for (size_t p = 0; aligned && p < np; p++) {
      if (kept[p] < 0) continue;
      const Member& mb = g->members[kept[p]];
      const size_t c0 = p / k * k;
      for (size_t r = c0; r < c0 + k; r++)
        if (sid[mb.shard][r] == mb.id) {
          align[p] = sal[mb.shard][r];
          break;
        }
    }
  } else {  // empty rows (fp_handler.c:247-250)
    memset(out, 0, sizeof(tfp_candidate) * np);
    if (aligned) memset(align, 0, sizeof(tfp_alignment) * np);
    memset(counts, 0, sizeof(int32_t) * nch);
  }
  for (int32_t c = 0; c < nch; c++) {
    const int64_t F = tfp::live_frames(gl->samples[c]), first = F > window ? F - window : 0;
    if (frame_counts) frame_counts[c] = (int32_t)(F - first);
    if (first_frames) first_frames[c] = (int32_t)first;
  }
  return TFP_OK;
}
}  // namespace

extern "C" {

int tfp_group_live_window(tfp_group_live* gl, const tfp_search_params* P, const int32_t* scopes, int32_t k, int32_t window,
                          tfp_candidate* out, int32_t* counts, int32_t* frame_counts, int32_t* first_frames) {
  if (!gl) return TFP_E_ARG;
  return group_live_window_call(gl, P, scopes, k, window, out, nullptr, false, counts, frame_counts, first_frames);
}

int tfp_group_live_window_aligned(tfp_group_live* gl, const tfp_search_params* P, const int32_t* scopes, int32_t k,
                                  int32_t window, tfp_candidate* out, tfp_alignment* align, int32_t* counts,
                                  int32_t* frame_counts, int32_t* first_frames) {
  if (!gl) return TFP_E_ARG;
  return group_live_window_call(gl, P, scopes, k, window, out, align, true, counts, frame_counts, first_frames);
}

int tfp_group_live_frames(tfp_group_live* gl, int32_t ch, int64_t first, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!gl || !nframes) return TFP_E_ARG;
  tfp_group* g = gl->g;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int rc = tfp_live_frames(gl->lv[0], ch, first, out, cap, nframes);  // (every shard keeps the same values)
  return rc ? gfail(g, rc, "%s", tfp_engine_last_error(g->eng[0])) : TFP_OK;
}

int tfp_group_live_window_stats(tfp_group_live* gl, int32_t shard, int64_t* slid_calls, int64_t* general_calls,
                                int64_t* rebuilds, int64_t* frames_added, int64_t* frames_removed, int64_t* rows_restarted) {
  if (!gl || shard < 0 || (size_t)shard >= gl->lv.size()) return TFP_E_ARG;
  return tfp_live_window_stats(gl->lv[shard], slid_calls, general_calls, rebuilds, frames_added, frames_removed, rows_restarted);
}

int tfp_group_live_window_aligned_stats(tfp_group_live* gl, int32_t shard, int64_t* inplace_calls, int64_t* general_calls,
                                        int64_t* pairs) {
  if (!gl || shard < 0 || (size_t)shard >= gl->lv.size()) return TFP_E_ARG;
  return tfp_live_window_aligned_stats(gl->lv[shard], inplace_calls, general_calls, pairs);
}

}  // extern "C"

// ---- tfp_live_occurrences on a group: the rows are tfp_group_live_window_aligned's merged rows, the offer
// rule runs once on them (max_tracks bounds a channel's list over all shards together), every shard
// advances its own clips' tracks on its own engine, and the selection runs on the union.
extern "C" {

int tfp_group_live_occurrences(tfp_group_live* gl, const tfp_search_params* P, const int32_t* scopes, int32_t k,
                               int32_t window, int32_t max_gap, int32_t min_hits, int32_t max_tracks, tfp_occurrence* out,
                               int64_t cap, int64_t* nocc, int32_t* dropped) {
  if (!gl) return TFP_E_ARG;
  tfp_group* g = gl->g;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  const int32_t nch = gl->nch;
  if (const char* bad = tfp::live_occ_args(P, scopes, nch, k, window, max_gap, min_hits, max_tracks, out, cap, nocc))
    return gfail(g, TFP_E_ARG, "live occurrences: %s", bad);
  if (dropped) memset(dropped, 0, sizeof(int32_t) * nch);
  *nocc = 0;
  gl->n_occ_calls++;
  if (!valid_params(P)) return TFP_OK;  // no rows, nothing offered, the lists stay
  // step 1: the merged rows with their alignments
  const size_t np = (size_t)nch * k;
  std::vector<tfp_candidate> rows(np);
  std::vector<tfp_alignment> al(np);
  std::vector<int32_t> counts(nch, 0), first(nch, 0);
  int rc = group_live_window_call(gl, P, scopes, k, window, rows.data(), al.data(), true, counts.data(), nullptr, first.data());
  if (rc) return rc;
  // step 2: the offer, a new track also onto its clip's shard
  for (int32_t c = 0; c < nch; c++)
    for (int32_t r = 0; r < counts[c]; r++) {
      const size_t p = (size_t)c * k + r;
      if (al[p].aligned_count < 1) continue;
      const auto it = g->where.find(rows[p].uuid);
      if (it == g->where.end()) continue;
      const int32_t mi = it->second, s = first[c] - al[p].offset;
      std::vector<tfp_group_live::Track>& list = gl->tracks[c];
      auto at = std::find_if(list.begin(), list.end(),
                             [&](const tfp_group_live::Track& t) { return t.member == mi && t.s == s && t.uuid == rows[p].uuid; });
      if (at != list.end()) {
        at->windows++;
      } else if ((int64_t)list.size() < max_tracks) {
        const Member& mb = g->members[mi];
        if ((rc = tfp_internal_live_occ_add(gl->lv[mb.shard], c, mb.id, s))) return shard_fail(g, rc, mb.shard);
        list.push_back(tfp_group_live::Track{mi, mb.uuid, s, 1, tfp_trace{0, 0, 0, 0, 0, 0}});
        gl->n_tr_added++;
      } else {
        gl->n_tr_dropped++;
        if (dropped) dropped[c]++;
      }
    }
  // step 3: the tracks of removed clips leave (the shards drop their own), every shard advances its tracks
  for (int32_t c = 0; c < nch; c++) {
    std::vector<tfp_group_live::Track>& list = gl->tracks[c];
    list.erase(std::remove_if(list.begin(), list.end(),
                              [&](const tfp_group_live::Track& t) {
                                return t.member < 0 || (size_t)t.member >= g->members.size() || g->members[t.member].uuid != t.uuid ||
                                       t.uuid.empty();
                              }),
               list.end());
  }
  if ((rc = run_all(g, [&](int s) { return tfp_internal_live_occ_advance(gl->lv[s], P, max_gap); }))) return rc;
  const int n = (int)g->eng.size();
  std::vector<tfp_trace_req> sreq(TFP_LIVE_TRACKS_MAX);
  std::vector<tfp_trace> strace(TFP_LIVE_TRACKS_MAX);
  std::vector<tfp::LiveOccTrack> tr;
  for (int32_t c = 0; c < nch; c++) {
    std::vector<tfp_group_live::Track>& list = gl->tracks[c];
    std::vector<bool> found(list.size(), false);
    for (int s = 0; s < n; s++) {
      int64_t nt = 0;
      if ((rc = tfp_live_tracks(gl->lv[s], c, sreq.data(), strace.data(), nullptr, TFP_LIVE_TRACKS_MAX, &nt)))
        return shard_fail(g, rc, s);
      for (int64_t i = 0; i < nt; i++)
        for (size_t j = 0; j < list.size(); j++) {
          const Member& mb = g->members[list[j].member];
          if (mb.shard == s && mb.id == sreq[i].clip_id && list[j].s == sreq[i].start) list[j].last = strace[i], found[j] = true;
        }
    }
    const int32_t scope = scopes ? scopes[c] : TFP_SCOPE_ANY;
    for (size_t j = 0; j < list.size(); j++) {
      const Member& mb = g->members[list[j].member];
      if (!found[j]) return gfail(g, TFP_E_HIP, "live occurrences: shard %d has no track of %s", mb.shard, mb.uuid.c_str());
      int32_t cs = 0;
      if (scope != TFP_SCOPE_ANY && (rc = tfp_index_scope(g->eng[mb.shard], mb.uuid.c_str(), &cs))) return shard_fail(g, rc, mb.shard);
      if (scope != TFP_SCOPE_ANY && cs != scope) continue;
      tfp::TraceOut t;
      memcpy(&t, &list[j].last, sizeof t);
      tr.push_back(tfp::LiveOccTrack{c, list[j].member, mb.shard, list[j].s, list[j].windows, t, mb.uuid.c_str()});
    }
  }
  // step 4: on the union
  std::string err;
  if ((rc = tfp::live_occ_select(tr, min_hits, out, cap, nocc, &err))) return gfail(g, rc, "%s", err.c_str());
  return TFP_OK;
}

int tfp_group_live_tracks(tfp_group_live* gl, int32_t ch, tfp_trace_req* reqs, tfp_trace* traces, int32_t* windows,
                          int64_t cap, int64_t* ntracks) {
  if (!gl || !ntracks) return TFP_E_ARG;
  tfp_group* g = gl->g;
  std::lock_guard<std::recursive_mutex> lk(g->mu);
  if (ch < 0 || ch >= gl->nch) return gfail(g, TFP_E_ARG, "live tracks: channel %d outside [0, %d)", ch, gl->nch);
  const std::vector<tfp_group_live::Track>& list = gl->tracks[ch];
  *ntracks = (int64_t)list.size();
  if (cap < *ntracks) return gfail(g, TFP_E_CAPACITY, "live tracks: %lld tracks, room for %lld", (long long)*ntracks, (long long)cap);
  for (size_t i = 0; i < list.size(); i++) {
    const bool ok = list[i].member >= 0 && (size_t)list[i].member < g->members.size() && g->members[list[i].member].uuid == list[i].uuid;
    if (reqs) reqs[i] = tfp_trace_req{ch, ok ? g->members[list[i].member].shard : -1, list[i].s, ok ? g->members[list[i].member].id : -1};
    if (traces) traces[i] = list[i].last;
    if (windows) windows[i] = list[i].windows;
  }
  return TFP_OK;
}

int tfp_group_live_occurrence_stats(tfp_group_live* gl, int32_t shard, int64_t* calls, int64_t* tracks_added,
                                    int64_t* tracks_dropped, int64_t* frames_traced, int64_t* retraces) {
  if (!gl || shard < 0 || (size_t)shard >= gl->lv.size()) return TFP_E_ARG;
  const int rc = tfp_live_occurrence_stats(gl->lv[shard], calls, tracks_added, nullptr, frames_traced, retraces);
  if (rc) return rc;
  std::lock_guard<std::recursive_mutex> lk(gl->g->mu);
  if (tracks_dropped) *tracks_dropped = gl->n_tr_dropped;  // (the offer runs on the group: dropped by it, not by a shard)
  return TFP_OK;
}

}  // extern "C"
