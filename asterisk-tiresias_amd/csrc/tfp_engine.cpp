// tfp_engine.cpp — C-ABI implementation (include/tiresias_fp.h) on top of the gfx950 kernels.
//
// Owns one HIP device + stream per engine, the per-sample-rate DSP tables, the enrolled
// index (staging rows + the m1-sorted device index rebuilt lazily after changes) and the
// search scratch. Every entry point takes the engine mutex, so concurrent channel threads
// (the reference runs one tiresias_exec per channel, application_handler.c:66) are safe.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/tiresias_fp.h"
#include "tfp_align.hpp"
#include "tfp_coalesce.hpp"
#include "tfp_g711.hpp"
#include "tfp_resample.hpp"
#include "tfp_resample_any.hpp"
#include "tfp_index.hpp"
#include "tfp_internal.hpp"
#include "tfp_kernels.hpp"
#include "tfp_live.hpp"
#include "tfp_live_occur.hpp"
#include "tfp_live_rate.hpp"
#include "tfp_math.hpp"
#include "tfp_query_plan.hpp"
#include "tfp_rank.hpp"
#include "tfp_census.hpp"
#include "tfp_scope.hpp"
#include "tfp_slide.hpp"
#include "tfp_neighbour.hpp"
#include "tfp_slide_align.hpp"
#include "tfp_trace.hpp"
#include "tfp_synth.hpp"
#include "tfp_tables.hpp"
#include "tfp_tolcache.hpp"

using namespace tfp;

namespace {

// Grow-only device buffer.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t reserve(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    size_t want = n < 256 ? 256 : n;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) bytes = want;
    return e;
  }
  // for buffers that grow a little per call (the merged index): 1/8 headroom, so a run of
  // enrolments does not free and reallocate hundreds of MB each time
  hipError_t reserve_grow(size_t n) { return n <= bytes ? hipSuccess : reserve(n + n / 8); }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
  void swap_with(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
};

// One tolerance's key row ranges (of every key's box) and the key-presence bitsets built from them
// (launch_key_bits; the vote paths), cached per index version (tfp_engine::tc.ranges).
struct KeyRanges {
  DevBuf rng_all, key_bits;
  bool bits_valid = false;
  int32_t bits_cols = -1;  // the column count key_bits was laid out for (its row width)
};

// The index rows in clip order (tfp_kernels.hpp), the source of the clip-set caches at tolerances up
// to kOrderMaxTol: built on the first search that needs it, then carried through every merge.
struct ClipOrder {
  DevBuf key, m1, key_b, m1_b, newcol;
  int64_t rows = 0;
  bool valid = false;
  int64_t n_builds = 0, n_merges = 0;
  CacheBuf sort_tmp;
  OrderScratch merge;
};

// The index delta's staged rows in clip order (sorted once per delta version, for any tolerance).
struct DeltaOrder {
  DevBuf key, m1, key_b, m1_b;
  CacheBuf sort_tmp;
};

// Index delta (round 4, tfp_index.hpp): the live clips added since the last build, searched by the
// coefs = 1 vote paths beside the main index instead of merged into it per enrolment.
struct IndexDelta {
  static constexpr int32_t kMaxClips = 512;        // columns reserved for them
  static constexpr int64_t kMaxRows = 1ll << 20;  // beyond either limit the next update merges
  bool use = true;  // TFP_INDEX_DELTA=0: every update merges (A/B, tests)
  // The delta pads the main columns to a multiple of 1024 and reserves kMaxClips columns after
  // them, which a small DB's vote passes would pay for on every search (300 clips -> 1,536
  // columns); below this many main columns an update merges instead (cheap at that size).
  // TFP_INDEX_DELTA=1 (tests) takes the delta at any size.
  int64_t min_cols = 4096;
  bool force_merge = false;  // consolidate(): the next rebuild merges the delta
  bool wide = true;          // TFP_DELTA_WIDE=0: coefs = 2 searches merge the delta first (A/B, tests)
  std::vector<int32_t> clip;  // delta column col0 + j -> clip id (uuid order)
  std::vector<int32_t> at;    // delta j's insertion point among the main columns' uuids
  int32_t col0 = 0;           // first delta column (a multiple of 1024)
  int64_t rows = 0;           // staged rows of the delta's clips
  int64_t n_updates = 0;
  std::unordered_map<int32_t, int32_t> key_col;  // tie-break key -> delta column (with an override)
  DevBuf d_clips, d_at;
  void reset(int32_t c0) { clip.clear(), at.clear(), key_col.clear(), col0 = c0, rows = 0; }  // no clip beside the c0 main columns
};

// The search-side caches, served only at the (tolerance, version) they were committed at (tfp_tolcache.hpp).
struct SearchCaches {
  TolCache<KeyRanges, 4> ranges;  // per index_version (every index update; merge_index and delta_update carry the active one)
  // general path: the clip-set caches (tfp_scan.hip), per main_version: they hold main-index rows
  // only, so they stay valid across delta updates
  TolCache<CellCache, 4> cells;
  // coefs = 2 with an index delta (round 6): the delta's own clip-set cache (its staged rows in clip
  // order, columns numbered from 0 in uuid order), swept after the main cache into the same maxima,
  // so an enrolment followed by a coefs = 2 search does not merge the index (fp_handler.c:559-571:
  // the reference's INSERT makes a clip searchable for the cost of its own rows)
  TolEntry<CellCache> dcells;  // per index_version
  TolEntry<DeltaOrder> dorder;  // per index_version (committed at tolerance 0: it serves every tolerance)
  TolEntry<DevBuf> kbox;        // the keys' "%f" boxes (launch_key_boxes); version 0: they do not depend on the index
  int64_t n_builds = 0, n_hits = 0, n_from_order = 0, n_delta_builds = 0, n_delta_sweeps = 0;
};

// Pinned host staging (one H2D copy per small call instead of one per array).
struct HostBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~HostBuf() { if (p) (void)hipHostFree(p); }
  hipError_t reserve(size_t n, unsigned flags = hipHostMallocDefault) {
    if (n <= bytes) return hipSuccess;
    if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
    size_t want = n < 65536 ? 65536 : n;
    hipError_t e = hipHostMalloc(&p, want, flags);
    if (e == hipSuccess) bytes = want;
    return e;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct Clip {
  std::string uuid;
  bool alive = true;
  int64_t nrows = 0;
  int64_t off = 0;  // first staging row (a clip's rows are contiguous, in frame order)
  int32_t scope = 0;  // tfp_index_set_scope (tfp_scope.hpp); kept by clip id, so through every index update
};

// tfp_host_alloc's buffers: host address -> (bytes, generation), so a call whose samples lie
// inside one hands the GPU the samples in place. The device address is resolved per engine
// (hipHostGetDevicePointer on the engine's own device, cached by base and generation), not taken
// from whichever device was current at allocation.
struct HostAllocs {
  std::mutex mu;
  std::map<uintptr_t, std::pair<size_t, uint64_t>> m;
  uint64_t next_gen = 1;
  // the buffer holding [p, p + n): its base and generation, or false
  bool find(const void* p, size_t n, uintptr_t* base, uint64_t* gen) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lk(mu);
    auto it = m.upper_bound(a);
    if (it == m.begin()) return false;
    --it;
    if (a + n > it->first + it->second.first) return false;
    *base = it->first;
    *gen = it->second.second;
    return true;
  }
};
HostAllocs& host_allocs() {
  static HostAllocs h;
  return h;
}

}  // namespace

struct tfp_plan {
  int32_t nclips = 0, ntiles = 0, sample_rate = 0, tile_frames = 0;
  bool long_clip = false;  // a clip of >= kDirectMaxSamples: the generic kernel
  int64_t nsamples = 0, nframes = 0;
  std::vector<int64_t> soff, foff;
  std::vector<int32_t> toff, tclip;
  DevBuf d_soff, d_foff, d_toff, d_tclip;
  std::vector<int64_t> qoff;  // == foff (frames per clip as queries)
  DevBuf d_qoff;
  tfp_engine* eng = nullptr;
};

struct tfp_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  std::recursive_mutex mu;
  tfp::ErrorSlot err;  // last-error messages (tfp_internal.hpp)
  std::map<int, DevBuf> tables;  // sample rate -> device DspTables
  std::map<int, bool> tables_fixed8k;  // sample rate -> DspTables_fixed8k (kernel variant)

  // staging (append-only) rows of every clip ever added
  std::vector<Clip> clips;
  std::unordered_map<std::string, int32_t> by_uuid;
  DevBuf st_m1, st_m2, st_clip;
  int64_t n_staged = 0, cap_staged = 0;
  bool dirty = true;

  // sorted index
  DevBuf m1s, m2s, cols, rank_of_clip, tiekey;
  // incremental maintenance (merge_index): the last build's clips and staged rows, the merge's
  // output buffers (swapped with m1s/m2s/cols) and scratch
  bool built = false;        // m1s/m2s/cols/col_clip describe clips [0, built_clips) as of the last build
  bool force_full = false;   // TFP_INDEX_FULL: every update is a full build (A/B, tests)
  size_t built_clips = 0;
  int64_t built_staged = 0;
  bool removed_built = false;  // a clip of the last build was removed since (else an update only adds)
  int64_t live_rows = 0;       // staged rows of live clips (kept per add / remove, not counted per build)
  int64_t n_merges = 0, n_full_builds = 0;
  DevBuf m1s_b, m2s_b, cols_b, remap;
  MergeScratch merge;
  int64_t nrows = 0;       // rows that can match (live clip, non-NULL max1)
  int32_t ncols = 0;       // live clips
  std::vector<int32_t> col_clip;                 // column (uuid rank) -> clip id
  std::unordered_map<int32_t, int32_t> key_col;  // tie-break key -> main column (with an override)
  bool key_identity = true;                      // no override: key == column
  std::vector<int32_t> tiebreak_override;        // clip id -> key (empty = uuid rank)
  // with an override: key_col / the device tie keys of the main columns no longer match it (a full
  // tfp_index_set_tiebreak, or new keys for clips of the last build); tfp_index_update_tiebreak of
  // clips added since leaves them standing, so a delta update costs the delta's clips only
  bool ovr_main_stale = true;
  int64_t n_delta_main_keys = 0;  // delta updates that re-sent every main column's key (tests)

  // scratch
  DevBuf sort_tmp, keys_a, keys_b, vals_a, vals_b, cnt;
  DevBuf pcm, q, qoff, boxes, vote_part, mask, maxc, A, Bt, best, stamp, score, micro, db;
  DevBuf soff, foff, toff, tclip, specs;
  // small host calls: packed upload + the small-batch search workspace
  HostBuf hstage;
  DevBuf dstage;
  HostBuf zstage;                   // mapped + coherent: small 8 kHz calls are read by the kernel in place
  void* zstage_host = nullptr;      // the allocation zstage_dev was taken for
  char* zstage_dev = nullptr;
  DevBuf zlayout;                   // device copy of the last zero-copy call's tile layout
  std::vector<char> zlayout_host;   // ... and its bytes (re-uploaded when they change)
  bool stage_pending = false;  // hstage / zstage may still be read by a copy or kernel on e->stream
  std::unordered_map<uintptr_t, std::pair<uint64_t, char*>> host_dev;  // tfp_host_alloc base -> (generation, device address)
  HostBuf qoff_pin;                   // pinned source of the qoff copy
  std::vector<int64_t> qoff_host;     // what e->qoff holds (copied on stream qoff_stream)
  hipStream_t qoff_stream = nullptr;
  hipEvent_t qoff_ev = nullptr;
  bool qoff_pending = false;
  DevBuf key_bits_b;         // the other buffer of a key-bitset update (merge_index, delta_update)
  int64_t tiekey_ident = -1; // tiekey on the device holds the identity over this many columns (-1: not known)
  HostBuf vres_pin;         // pinned (VoteMeta, best[]) of the vote path
  HostBuf spec_pin;         // pinned copy of the speculative sweep's counts (WideScratch::info), host-mapped
  void* spec_pin_host = nullptr;   // the allocation spec_pin_dev was taken for
  int32_t* spec_pin_dev = nullptr; // its device address (the sweep's last kernel writes it)
  HostBuf small_res;        // host-mapped SmallResult, written by small_vote_kernel (no copy back)
  SmallResult* small_res_dev = nullptr;
  void* small_res_host = nullptr;  // the allocation small_res_dev was taken for
  // index_version changes with every index update (rebuild, delta update); main_version is the main
  // index's own (builds and merges; a delta update leaves it)
  uint64_t index_version = 1, main_version = 1;
  SearchCaches tc;
  WideScratch wide;         // the general path's sweep by groups
  double wide_min_tol = 0;  // TFP_WIDE_MIN_TOL: general-path batches below it take the clip-set cells (tests)
  // the coefs = 2 sweep's sort path per batch (tfp_sweep_stats): the bin sort's speculative pass
  // stood, the library sort ran, a speculative pass was redone; crowd bins the bin sort copied
  int64_t n_sweep_bins = 0, n_sweep_lib = 0, n_sweep_redo = 0, n_sweep_crowd = 0;
  // plain search's form per batch (tfp_search_path_stats): the small vote, the vote by pattern classes
  // or by the GEMM, a vote the host had to redo (VoteMeta::ok clear), a pass of the general path
  int64_t n_path_small = 0, n_path_class = 0, n_path_gemm = 0, n_path_redone = 0, n_path_general = 0;
  ClipOrder order;
  // scan scratch: stamp / score / touched nq x ncols int32 each, tcnt nq int32; kept all-zero
  // by the scan kernels themselves
  DevBuf touched, tcnt;
  size_t scan_zeroed = 0;  // bytes of stamp / score / touched known to be zero
  // ranked search (rank_core): the vote form's per-block partial keys, the batch's keys [nq][k] with
  // the vote form's bad flag after them, their pinned copy, and the batches each form served
  DevBuf rank_part, rank_keys;
  HostBuf rank_pin;
  int64_t n_rank_vote = 0, n_rank_general = 0;
  // scoped search (tfp_scope.hpp): the clips' scopes and the columns' clips as uploaded, the
  // per-column scope table built from them, the batch's per-query scopes; the table stands for
  // index version scope_version until a scope changes (scope_dirty)
  DevBuf scope_clip, scope_colclip, scope_table, scope_q;
  std::unordered_map<int32_t, int64_t> scope_pop;  // scope -> live clips, as of the table's build (the census's bin 0)
  int64_t scope_live = 0;                          // live clips
  uint64_t scope_version = 0;
  bool scope_dirty = true;
  int64_t n_scope_vote = 0, n_scope_general = 0, n_scope_builds = 0;
  // catalog neighbours (tfp_neighbour.hpp): the launch's named clips, the columns' staged rows and the
  // clips' columns (host) as of index version nbr_version with the longest live clip's rows, the
  // selected rows' columns, the frame boxes / gathered frame values, the pairs, the bands' partial keys,
  // [keys][bad flag][alignments] and their pinned copy; the calls each form served, the pairs aligned
  // and the stored rows used as query frames
  DevBuf nbr_clips, nbr_colrows, nbr_cols, nbr_boxes, nbr_q, nbr_pairs, nbr_part, nbr_res;
  HostBuf nbr_pin;
  std::vector<int32_t> nbr_col_of_clip;
  uint64_t nbr_version = 0;
  int64_t nbr_nmax = 0;
  int64_t n_nbr_vote = 0, n_nbr_general = 0, n_nbr_pairs = 0, n_nbr_frames = 0;
  // match census (tfp_census.hpp): the batch's bins [nq][nbins] with the vote form's bad flag after
  // them, their pinned copy, and the batches each form served
  DevBuf census_hist;
  HostBuf census_pin;
  int64_t n_census_vote = 0, n_census_general = 0;
  // sliding search (tfp_slide.hpp): the recordings' key slots, the launch's runs, the general form's
  // window starts and gathered frame values, and the batches / windows served so far
  DevBuf slide_slots, slide_runs, slide_wsrc, slide_q;
  int64_t n_slide_vote = 0, n_slide_general = 0, n_slide_windows = 0;
  // aligned search (align_core): the batch's frame boxes (its own: a device-form search may still
  // read e->boxes on the caller's stream), the pairs, the bands' partial keys, the results, the
  // pinned copy of pairs and results, and the batches / pairs aligned so far
  DevBuf align_boxes, align_pairs, align_part, align_out;
  HostBuf align_pin;
  int64_t n_align_batches = 0, n_align_pairs = 0;
  // sliding aligned search (slide_align_core): the launch's runs, their step tables and the entries'
  // band counts (the boxes, pairs, partials and results are aligned search's buffers), and the
  // batches / entries aligned so far by form
  DevBuf sa_runs, sa_steps, sa_nb;
  int64_t n_sa_batches = 0, n_sa_slid = 0, n_sa_direct = 0;
  // diagonal trace (trace_core): the launch's requests and results (the boxes are aligned search's),
  // and the batches that launched the kernel / the requests it computed so far
  DevBuf trace_reqs, trace_out;
  int64_t n_trace_batches = 0, n_traces = 0;
  DevBuf g711_codes;  // a large G.711 batch's codes, expanded into pcm
  int64_t n_g711_expand = 0, n_g711_stream = 0, n_g711_codes = 0;  // tfp_g711_stats
  // rate-normalised ingest (tfp_resample.hpp): the tables by (M, L) with their device copies, kept for
  // the engine's lifetime as the rate tables are; a large batch's input samples, converted into pcm
  struct RsTable {
    std::shared_ptr<const ResampleTable> host;
    DevBuf dev;
  };
  std::map<std::pair<int32_t, int32_t>, RsTable> rs_tables;
  DevBuf rs_in;
  int64_t n_rs_launch = 0, n_rs_in = 0, n_rs_out = 0;  // tfp_resample_stats
  int64_t n_mix_launch = 0, n_mix_in = 0, n_mix_out = 0, n_mix_staged = 0;  // tfp_resample_mix_stats
  int64_t n_wide_launch = 0, n_wide_in = 0, n_wide_out = 0, n_wide_staged = 0;  // tfp_resample_wide_stats
  // mixed batches (tfp_resample_any.hpp): the last call's plans' tables laid end to end on the device, kept
  // while the next call names the same plans in the same order (any_taps_key: their (M, L))
  DevBuf any_taps;
  std::vector<std::pair<int32_t, int32_t>> any_taps_key;
  int64_t n_any_launch = 0, n_any_clips = 0, n_any_in = 0, n_any_out = 0;  // tfp_resample_any_stats
  int64_t n_any_staged = 0, n_any_global = 0, n_any_plain = 0;             // ... its tiles by form
  // launch configuration and test/A-B knobs, read once at engine creation
  FpLaunchCfg fpcfg;
  FpLaunchStats fpstats;  // fingerprint launches so far per kernel (tfp_fingerprint_stats)
  int32_t class_ku_max = 10;  // TFP_VOTE_CLASS_MAX: pattern-class vote up to this many used keys (-1: always the GEMM)
  bool dbg_vote = false;      // TFP_DEBUG_VOTE: log the vote path's shape per batch
  bool dbg_index = false;     // TFP_DEBUG_INDEX: log each index update's phases (host ms)
  int32_t fail_compact = 0;   // TFP_TEST_FAIL_COMPACT=n: the next n staging compactions fail (tests)
  // TFP_TEST_FAIL_CELLS=k / TFP_TEST_FAIL_DELTA_CELLS=k: the k-th main / delta clip-set cache build
  // fails in its preparation, as an allocation failure of the clip order would (tests)
  int64_t fail_cells = 0, fail_delta_cells = 0;
  int quiet = 0;  // > 0: failures are not recorded in err (quietly(): an optional cache's build)
  int64_t fail_query_len = -1;  // TFP_TEST_FAIL_QUERY_SAMPLES=n: a search with a query of n samples fails (tests)
  int32_t kb_win = 0;           // TFP_KEYBITS_WIN: LDS words per column window of launch_key_bits (tests; 0 = default)
  int64_t kb_direct = -1;       // TFP_KEYBITS_DIRECT: pieces below this many rows use global atomics (tests; -1 = default)
  DevBuf logfix_key, logfix_val, logfix_bits;  // device copy of the glibc log correction table (LogFix)
  LogFix logfix{nullptr, nullptr, 0};
  IndexDelta delta;
  Coalescer coal;          // concurrent small host-sample searches share one batch (tfp_coalesce.hpp)
  bool coalesce = true;    // TFP_COALESCE=0: every call runs alone (A/B)
  hipEvent_t null_in = nullptr, null_out = nullptr;  // (NullStreamOrder)
  ~tfp_engine() {
    if (qoff_ev) (void)hipEventDestroy(qoff_ev);
    if (null_in) (void)hipEventDestroy(null_in);
    if (null_out) (void)hipEventDestroy(null_out);
  }
};

namespace {

int fail(tfp_engine* e, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int fail(tfp_engine* e, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (e && !e->quiet) e->err.note(e, buf);
  return code;
}

// f() with its failures left out of the last-error messages: the build of an optional cache, whose
// failure the search recovers from (the caller holds the engine mutex).
template <class F>
int quietly(tfp_engine* e, F f) {
  e->quiet++;
  const int rc = f();
  e->quiet--;
  return rc;
}

#define HIPCHK(e, expr)                                                                          \
  do {                                                                                           \
    hipError_t _st = (expr);                                                                     \
    if (_st != hipSuccess)                                                                       \
      return fail((e), _st == hipErrorOutOfMemory ? TFP_E_NOMEM : TFP_E_HIP, "%s: %s", #expr,   \
                  hipGetErrorString(_st));                                                       \
  } while (0)

// A device-form call given no stream (NULL) runs on the engine's own stream, ordered after the work
// queued on the HIP null stream before the call and before the null stream's later work: the
// null stream is the default stream of torch and of CUDA-style callers, and the engine's stream
// is non-blocking, so without this a caller's default-stream producers and consumers (a torch
// copy, a gloo all_gather of the frame values) could race the engine's kernels. Two event
// records and two stream waits, no host wait.
class NullStreamOrder {
 public:
  NullStreamOrder(tfp_engine* e, void* stream) : e_(e), on_(stream == nullptr) {
    if (!on_) return;
    if (!e_->null_in && hipEventCreateWithFlags(&e_->null_in, hipEventDisableTiming) != hipSuccess) e_->null_in = nullptr;
    if (!e_->null_out && hipEventCreateWithFlags(&e_->null_out, hipEventDisableTiming) != hipSuccess) e_->null_out = nullptr;
    ok_ = e_->null_in && e_->null_out && hipEventRecord(e_->null_in, nullptr) == hipSuccess &&
          hipStreamWaitEvent(e_->stream, e_->null_in, 0) == hipSuccess;
  }
  bool ok() const { return !on_ || ok_; }
  ~NullStreamOrder() {
    if (on_ && ok_ && hipEventRecord(e_->null_out, e_->stream) == hipSuccess) (void)hipStreamWaitEvent(nullptr, e_->null_out, 0);
  }

 private:
  tfp_engine* e_;
  bool on_, ok_ = false;
};

// The device copy of the glibc log correction table (frame values == glibc's 10*log10|c|).
int ensure_logfix(tfp_engine* e) {
  if (e->logfix.n) return TFP_OK;
  const uint32_t* k;
  const double* v;
  int32_t n;
  log_fix_hash(&k, &v, &n);  // (the hashed form: one or two key loads per lookup on the device)
  if (n <= 0) return TFP_OK;
  const size_t slots = (size_t)1 << kLogFixHashBits;
  HIPCHK(e, e->logfix_key.reserve(sizeof(uint32_t) * slots));
  HIPCHK(e, e->logfix_val.reserve(sizeof(double) * slots));
  HIPCHK(e, hipMemcpyAsync(e->logfix_key.p, k, sizeof(uint32_t) * slots, hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipMemcpyAsync(e->logfix_val.p, v, sizeof(double) * slots, hipMemcpyHostToDevice, e->stream));
  // the keys present as a bitmap over the 2^24 reduced arguments (2 MiB)
  std::vector<uint32_t> bits(1u << 19, 0u);
  for (size_t j = 0; j < slots; j++)
    if (k[j] != kLogFixEmpty) bits[k[j] >> 5] |= 1u << (k[j] & 31);
  HIPCHK(e, e->logfix_bits.reserve(sizeof(uint32_t) * bits.size()));
  HIPCHK(e, hipMemcpyAsync(e->logfix_bits.p, bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->logfix = LogFix{e->logfix_key.as<uint32_t>(), e->logfix_val.as<double>(), n, 1, e->logfix_bits.as<uint32_t>()};
  return TFP_OK;
}

int ensure_tables(tfp_engine* e, int sr, const DspTables** out, bool* fixed8k = nullptr) {
  int rc0 = ensure_logfix(e);
  if (rc0) return rc0;
  auto it = e->tables.find(sr);
  if (it == e->tables.end()) {
    DspTables host;
    if (!build_tables(sr, &host)) return fail(e, TFP_E_ARG, "bad sample rate %d", sr);
    e->tables_fixed8k[sr] = DspTables_fixed8k(host);
    DevBuf& d = e->tables[sr];
    HIPCHK(e, d.reserve(sizeof(DspTables)));
    HIPCHK(e, hipMemcpyAsync(d.p, &host, sizeof host, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    it = e->tables.find(sr);
  }
  *out = it->second.as<DspTables>();
  if (fixed8k) *fixed8k = e->tables_fixed8k[sr];
  return TFP_OK;
}

// Clip layout: sample, frame and 16-frame-tile offsets.
void layout(const int64_t* offsets, int32_t nclips, std::vector<int64_t>& soff, std::vector<int64_t>& foff,
            std::vector<int32_t>& toff, std::vector<int32_t>* tclip = nullptr, int tile_frames = kFramesPerBlock) {
  soff.assign(offsets, offsets + nclips + 1);
  const int64_t base = soff[0];
  for (auto& v : soff) v -= base;
  foff.assign(nclips + 1, 0);
  toff.assign(nclips + 1, 0);
  for (int32_t c = 0; c < nclips; c++) {
    const int64_t nf = tfp_frame_count(soff[c + 1] - soff[c]);
    foff[c + 1] = foff[c] + nf;
    toff[c + 1] = toff[c] + (int32_t)((nf + tile_frames - 1) / tile_frames);
  }
  if (tclip) {
    tclip->assign(std::max<int32_t>(toff[nclips], 1), 0);
    for (int32_t c = 0; c < nclips; c++)
      for (int32_t t = toff[c]; t < toff[c + 1]; t++) (*tclip)[t] = c;
  }
}

int upload(tfp_engine* e, DevBuf& d, const void* h, size_t bytes, hipStream_t s = nullptr) {
  HIPCHK(e, d.reserve(bytes));
  if (bytes) HIPCHK(e, hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, s ? s : e->stream));
  return TFP_OK;
}

// The engine's device address of [p, p + n) if it lies inside one tfp_host_alloc buffer, else
// nullptr. Resolved on the engine's device (current here) once per buffer and cached.
const char* engine_host_ptr(tfp_engine* e, const void* p, size_t n) {
  uintptr_t base;
  uint64_t gen;
  if (!host_allocs().find(p, n, &base, &gen)) return nullptr;
  auto& slot = e->host_dev[base];
  if (slot.first != gen) {
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, reinterpret_cast<void*>(base), 0) != hipSuccess) {
      (void)hipGetLastError();
      e->host_dev.erase(base);
      return nullptr;  // (the call copies the samples instead)
    }
    slot = {gen, static_cast<char*>(d)};
  }
  return slot.second + (reinterpret_cast<uintptr_t>(p) - base);
}

// A batch of G.711 codes laid end to end (clip c = lens[c] codes, in order) and their law.
struct G711Src {
  const uint8_t* codes;
  int32_t law;
};

// A batch of int16 clips at another rate laid end to end (clip c = the samples [in_off[c], in_off[c + 1])
// of pcm, in_off[0] = 0), and the table that brings them to the call's rate. The call's lens are the
// output lengths (resample_count of the input lengths).
struct RateSrc {
  const int16_t* pcm;
  std::vector<int64_t> in_off;
  const ResampleTable* tab;
  const int16_t* d_taps;
};

// A batch of interleaved int16 clips of `channels` channels laid end to end (clip c = the frames
// [in_off[c], in_off[c + 1]) of pcm, channels samples each, in_off[0] = 0) and the table that brings
// their channel sums to the call's rate; tab == nullptr at equal rates (the downmix alone, in_off = the
// call's own offsets). The call's lens are the output lengths. The wide forms (wide_source) hand over int32
// Q31 frames instead: q31 is set, pcm is not read, and the launch is tfp_resample_wide.hip's.
struct MixSrc {
  const int16_t* pcm;
  const int32_t* q31 = nullptr;
  std::vector<int64_t> in_off;
  int32_t channels;
  const ResampleTable* tab;
  const int16_t* d_taps;
};

// A mixed batch (tfp_resample_any.hpp): the call's bytes as the caller gave them, the validated call and
// its plans' tables on the device. The call's lens are the output lengths (B->out_off).
struct AnySrc {
  const void* data;
  int64_t nbytes;
  const AnyBatch* B;
  const int16_t* d_taps;
};

// Fingerprint host samples (int16 PCM, or with f32 the fp32 values aubio_source produced):
// clip c is the lens[c] samples at ptrs[c] (the clips may lie anywhere: a coalesced batch gathers
// the queries of several callers); leaves micro/db on the device in e->micro / e->db.
// exact_q: the frame values (e->db) equal glibc's 10*log10|c| bit for bit (LogFix lookups); a
// coefs = 1 search needs only their truncation, which is exact either way.
// g711: the clips are G.711 codes laid end to end at g711->codes (ptrs is not read). The codes go to
// the device at one byte per sample and g711_expand_kernel writes their int16 into e->pcm; from
// there on (layout, tile choice, launch) the call is the int16 call of the same lengths.
// rate: the clips are int16 at another rate laid end to end at rate->pcm (ptrs is not read) and lens
// are their lengths at sr. The samples go to the device as they are and resample_kernel writes their
// conversion into e->pcm; the layout, tile choice and launch are the int16 call's of lens.
// mix: the same for interleaved multichannel int16 at mix->pcm, by resample_mix_kernel (offsets in frames),
// or for interleaved int32 Q31 at mix->q31, by resample_wide_kernel.
// any: a mixed batch: the call's bytes go to the device as they are and resample_any_kernel writes every
// clip's conversion into e->pcm.
int fingerprint_host(tfp_engine* e, const void* const* ptrs, const int64_t* lens, bool f32, int32_t nclips, int32_t sr,
                     int64_t* nframes_out, std::vector<int64_t>* foff_out, bool exact_q = true,
                     const G711Src* g711 = nullptr, const RateSrc* rate = nullptr, const MixSrc* mix = nullptr,
                     const AnySrc* any = nullptr) {
  const size_t ss = f32 ? sizeof(float) : sizeof(int16_t);
  const bool wide = mix && mix->q31;
  const size_t hs = g711 || any ? sizeof(uint8_t) : wide ? sizeof(int32_t) : ss;  // bytes per sample as the host hands them over
  const bool flat = g711 || rate || mix || any;   // one flat source array in front of e->pcm
  const std::vector<int64_t>* rs_in_off =  // a converting launch's input offsets (a mixed batch: its running frames)
      rate ? &rate->in_off : mix ? &mix->in_off : any ? &any->B->in_off : nullptr;
  const DspTables* T;
  bool fx = false;
  int rc = ensure_tables(e, sr, &T, &fx);
  if (rc) return rc;
  std::vector<int64_t> foff(nclips + 1, 0);
  std::vector<int32_t> toff(nclips + 1, 0), tclip;
  // small batches at 8 kHz: 4-frame wave tiles (more waves, fewer passes per wave)
  bool small = false;
  for (int32_t c = 0; c < nclips; c++)
    if (lens[c] >= kDirectMaxSamples) fx = false;  // (the 8 kHz kernel's 32-bit buffer offsets)
  if (fx && !f32) {
    int64_t nf16 = 0;
    for (int32_t c = 0; c < nclips; c++) nf16 += (tfp_frame_count(lens[c]) + 15) / 16;
    small = nf16 <= 256;
  }
  const int tile_frames = fp_tile_frames(e->fpcfg, fx, f32, small);
  for (int32_t c = 0; c < nclips; c++) {
    const int64_t nfc = tfp_frame_count(lens[c]);
    foff[c + 1] = foff[c] + nfc;
    toff[c + 1] = toff[c] + (int32_t)((nfc + tile_frames - 1) / tile_frames);
  }
  tclip.assign(std::max<int32_t>(toff[nclips], 1), 0);
  for (int32_t c = 0; c < nclips; c++)
    for (int32_t t = toff[c]; t < toff[c + 1]; t++) tclip[t] = c;
  const int64_t nf = foff[nclips];
  HIPCHK(e, e->micro.reserve(sizeof(int32_t) * 2 * (nf + 1)));
  HIPCHK(e, e->db.reserve(sizeof(double) * 2 * (nf + 1)));
  // Where the samples come from:
  //  - in place: every clip lies in a tfp_host_alloc buffer (the shim's WAV reads): the kernel reads
  //    them through their device mapping, clip c at sample offset sbeg[c] from the lowest address;
  //  - else packed (sbeg = prefix sums): into the pinned staging (small calls) or the device buffer.
  // Throughput batches that are one contiguous buffer keep the DMA copy into HBM.
  bool contiguous = true;
  int64_t ns = 0;
  for (int32_t c = 0; c < nclips; c++) {
    ns += lens[c];
    if (!flat && c + 1 < nclips && static_cast<const char*>(ptrs[c]) + ss * lens[c] != ptrs[c + 1]) contiguous = false;
  }
  const int64_t n_src = rate  ? rate->in_off[nclips]  // samples (a mixed batch: bytes) the host hands over
                        : mix ? mix->in_off[nclips] * mix->channels
                        : any ? any->nbytes
                              : ns;
  std::vector<int64_t> sbeg(nclips + 1, 0), send(nclips + 1, 0);
  const char* base_dev = nullptr;
  bool in_place = !flat && ns > 0 && (small || !contiguous);
  if (in_place) {
    std::vector<const char*> dv(nclips, nullptr);
    for (int32_t c = 0; c < nclips && in_place; c++) {
      if (!lens[c]) continue;
      dv[c] = engine_host_ptr(e, ptrs[c], ss * lens[c]);
      in_place = dv[c] != nullptr;
      if (in_place && (!base_dev || dv[c] < base_dev)) base_dev = dv[c];
    }
    for (int32_t c = 0; c < nclips && in_place; c++) {
      const int64_t d = lens[c] ? (int64_t)(dv[c] - base_dev) : 0;
      in_place = d % (int64_t)ss == 0;
      sbeg[c] = d / (int64_t)ss;
      send[c] = sbeg[c] + lens[c];
    }
  }
  if (!in_place) {
    for (int32_t c = 0; c < nclips; c++) {
      sbeg[c + 1] = sbeg[c] + lens[c];
      send[c] = sbeg[c + 1];
    }
  }
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  // the resample launch's own layout, after the fingerprint launch's: the input offsets, the output
  // offsets (sbeg, all nclips + 1 of them) and the tiles of kRsTile outputs
  std::vector<int32_t> rs_toff, rs_tclip;
  if (rs_in_off) resample_tiles(sbeg.data(), nclips, &rs_toff, &rs_tclip);
  const size_t b_pcm = in_place ? 0 : al(hs * n_src), b_sb = al(sizeof(int64_t) * nclips),
               b_fo = al(sizeof(int64_t) * foff.size()), b_to = al(sizeof(int32_t) * toff.size()),
               b_tc = al(sizeof(int32_t) * tclip.size());
  const size_t b_ro = rs_in_off ? al(sizeof(int64_t) * (nclips + 1)) : 0, b_rt = rs_in_off ? al(sizeof(int32_t) * rs_toff.size()) : 0,
               b_rc = rs_in_off ? al(sizeof(int32_t) * rs_tclip.size()) : 0;
  // a mixed batch's clip descriptors and plans, behind the resample layout (one plan slot at least)
  const size_t b_ad = any ? al(sizeof(AnyClipDev) * std::max<size_t>(any->B->clips.size(), 1)) : 0,
               b_ap = any ? al(sizeof(AnyPlanDev) * std::max<size_t>(any->B->plans.size(), 1)) : 0;
  const size_t lay_fp = 2 * b_sb + b_fo + b_to + b_tc, lay_rs = lay_fp + 2 * b_ro + b_rt + b_rc, lay = lay_rs + b_ad + b_ap,
               total = b_pcm + lay;
  auto pack_layout = [&](char* h) {
    memcpy(h, sbeg.data(), sizeof(int64_t) * nclips);
    memcpy(h + b_sb, send.data(), sizeof(int64_t) * nclips);
    memcpy(h + 2 * b_sb, foff.data(), sizeof(int64_t) * foff.size());
    memcpy(h + 2 * b_sb + b_fo, toff.data(), sizeof(int32_t) * toff.size());
    memcpy(h + 2 * b_sb + b_fo + b_to, tclip.data(), sizeof(int32_t) * tclip.size());
    if (!rs_in_off) return;
    memcpy(h + lay_fp, rs_in_off->data(), sizeof(int64_t) * (nclips + 1));
    memcpy(h + lay_fp + b_ro, sbeg.data(), sizeof(int64_t) * (nclips + 1));
    memcpy(h + lay_fp + 2 * b_ro, rs_toff.data(), sizeof(int32_t) * rs_toff.size());
    if (!rs_tclip.empty()) memcpy(h + lay_fp + 2 * b_ro + b_rt, rs_tclip.data(), sizeof(int32_t) * rs_tclip.size());
    if (!any) return;
    memset(h + lay_rs, 0, b_ad + b_ap);
    if (!any->B->clips.empty()) memcpy(h + lay_rs, any->B->clips.data(), sizeof(AnyClipDev) * any->B->clips.size());
    if (!any->B->plans.empty()) memcpy(h + lay_rs + b_ad, any->B->plans.data(), sizeof(AnyPlanDev) * any->B->plans.size());
  };
  auto pack_samples = [&](char* h) {
    if (contiguous) {
      const void* src = g711   ? static_cast<const void*>(g711->codes)
                        : rate ? static_cast<const void*>(rate->pcm)
                        : wide ? static_cast<const void*>(mix->q31)
                        : mix  ? static_cast<const void*>(mix->pcm)
                        : any  ? any->data
                               : ptrs[0];
      if (n_src) memcpy(h, src, hs * n_src);
      return;
    }
    for (int32_t c = 0; c < nclips; c++)
      if (lens[c]) memcpy(h + ss * sbeg[c], ptrs[c], ss * lens[c]);
  };
  const void* d_pcm;
  const char* lay_d;
  if (total <= ((size_t)8 << 20)) {
    // small call: pack every array into pinned staging, one H2D copy. The 4-frame-tile calls
    // (a query, batch-1 latency) skip the copy: the kernel reads the mapped, coherent staging in
    // place (a copy plus its hand-off to the kernel cost ~16 us before the first kernel started).
    // Every caller waits for e->stream before it returns and then clears stage_pending, so the
    // staging buffer is free here; after an error return the stream is drained first.
    if (e->stage_pending) HIPCHK(e, hipStreamSynchronize(e->stream));
    const bool zero_copy = small || in_place;
    char* h;
    if (zero_copy) {
      HIPCHK(e, e->zstage.reserve(total, hipHostMallocMapped | hipHostMallocCoherent));
      if (e->zstage.p != e->zstage_host) {
        HIPCHK(e, hipHostGetDevicePointer(reinterpret_cast<void**>(&e->zstage_dev), e->zstage.p, 0));
        e->zstage_host = e->zstage.p;
      }
      h = e->zstage.as<char>();
    } else {
      HIPCHK(e, e->hstage.reserve(total));
      HIPCHK(e, e->dstage.reserve(total));
      h = e->hstage.as<char>();
    }
    if (!in_place) pack_samples(h);
    pack_layout(h + b_pcm);
    if (!zero_copy) HIPCHK(e, hipMemcpyAsync(e->dstage.p, h, total, hipMemcpyHostToDevice, e->stream));
    e->stage_pending = true;
    char* d = zero_copy ? e->zstage_dev : e->dstage.as<char>();
    d_pcm = in_place ? base_dev : d;
    lay_d = d + b_pcm;  // the layout arrays' device address
    if (zero_copy) {
      // The tile layout is read first and in a dependent chain (tile -> clip -> its bounds -> the
      // PCM address): keep it in device memory. It depends only on the query lengths (and, in
      // place, the buffers' relative positions), so it is uploaded only when it changes (from the
      // pinned staging; the PCM stays in place).
      if (e->zlayout_host.size() != lay || memcmp(e->zlayout_host.data(), h + b_pcm, lay) != 0) {
        HIPCHK(e, e->zlayout.reserve(lay));
        HIPCHK(e, hipMemcpyAsync(e->zlayout.p, h + b_pcm, lay, hipMemcpyHostToDevice, e->stream));
        e->zlayout_host.assign(h + b_pcm, h + total);
      }
      lay_d = e->zlayout.as<char>();
    }
  } else {
    std::vector<char> hl(lay);
    pack_layout(hl.data());
    if ((rc = upload(e, e->soff, hl.data(), lay))) return rc;
    if (in_place) {
      d_pcm = base_dev;
    } else if (g711) {
      if ((rc = upload(e, e->g711_codes, g711->codes, hs * ns))) return rc;
      d_pcm = e->g711_codes.p;
    } else if (rs_in_off) {
      if ((rc = upload(e, e->rs_in,
                       rate   ? static_cast<const void*>(rate->pcm)
                       : wide ? static_cast<const void*>(mix->q31)
                       : mix  ? static_cast<const void*>(mix->pcm)
                              : any->data,
                       hs * n_src))) return rc;
      d_pcm = e->rs_in.p;
    } else {
      HIPCHK(e, e->pcm.reserve(ss * ns));
      if (contiguous) {
        if ((rc = upload(e, e->pcm, ptrs[0], ss * ns))) return rc;
      } else {
        for (int32_t c = 0; c < nclips; c++)
          if (lens[c])
            HIPCHK(e, hipMemcpyAsync(e->pcm.as<char>() + ss * sbeg[c], ptrs[c], ss * lens[c], hipMemcpyHostToDevice,
                                     e->stream));
      }
      d_pcm = e->pcm.p;
    }
    lay_d = e->soff.as<char>();
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (hl is released on return)
  }
  if (g711 && ns) {
    // d_pcm holds the codes so far (staging, or g711_codes): their int16 into the device PCM buffer
    HIPCHK(e, e->pcm.reserve(ss * ns));
    HIPCHK(e, launch_g711_expand(static_cast<const uint8_t*>(d_pcm), ns, g711->law, e->pcm.as<int16_t>(), e->stream));
    e->n_g711_expand++;
    e->n_g711_codes += ns;
    d_pcm = e->pcm.p;
  }
  if (rate && ns) {
    // d_pcm holds the input samples so far (staging, or rs_in): their conversion into the device PCM buffer
    HIPCHK(e, e->pcm.reserve(ss * ns));
    const char* r = lay_d + lay_fp;
    HIPCHK(e, launch_resample(rate->tab->plan, rate->d_taps, static_cast<const int16_t*>(d_pcm),
                              reinterpret_cast<const int64_t*>(r), reinterpret_cast<const int64_t*>(r + b_ro),
                              reinterpret_cast<const int32_t*>(r + 2 * b_ro),
                              reinterpret_cast<const int32_t*>(r + 2 * b_ro + b_rt), rs_toff[nclips], e->pcm.as<int16_t>(),
                              e->stream));
    e->n_rs_launch++;
    e->n_rs_in += n_src;
    e->n_rs_out += ns;
    d_pcm = e->pcm.p;
  }
  if (wide && ns) {
    // d_pcm holds the interleaved Q31 frames so far (staging, or rs_in): their conversion into the device PCM buffer
    HIPCHK(e, e->pcm.reserve(ss * ns));
    const char* r = lay_d + lay_fp;
    ResampleWideForm form = kRsWideNone;
    HIPCHK(e, launch_resample_wide(mix->tab ? mix->tab->plan : ResamplePlan{1, 1, 0, 1}, mix->d_taps, !mix->tab, mix->channels,
                                   static_cast<const int32_t*>(d_pcm), reinterpret_cast<const int64_t*>(r),
                                   reinterpret_cast<const int64_t*>(r + b_ro), reinterpret_cast<const int32_t*>(r + 2 * b_ro),
                                   reinterpret_cast<const int32_t*>(r + 2 * b_ro + b_rt), rs_toff[nclips],
                                   e->pcm.as<int16_t>(), e->stream, &form));
    e->n_wide_launch++;
    e->n_wide_in += mix->in_off[nclips];
    e->n_wide_out += ns;
    e->n_wide_staged += form != kRsWideGlobal ? 1 : 0;
    d_pcm = e->pcm.p;
  }
  if (any && ns) {
    // d_pcm holds the call's bytes so far (staging, or rs_in: 256-byte aligned, as the Q31 and word reads
    // need): every clip's conversion into the device PCM buffer, one launch
    HIPCHK(e, e->pcm.reserve(ss * ns));
    const char* r = lay_d + lay_fp;
    HIPCHK(e, launch_resample_any(static_cast<const uint8_t*>(d_pcm), reinterpret_cast<const AnyClipDev*>(lay_d + lay_rs),
                                  reinterpret_cast<const AnyPlanDev*>(lay_d + lay_rs + b_ad), any->d_taps,
                                  reinterpret_cast<const int32_t*>(r + 2 * b_ro),
                                  reinterpret_cast<const int32_t*>(r + 2 * b_ro + b_rt), rs_toff[nclips], any->B->lds_bytes,
                                  e->pcm.as<int16_t>(), e->stream));
    e->n_any_launch++;
    e->n_any_clips += nclips;
    e->n_any_in += any->B->in_off[nclips];
    e->n_any_out += ns;
    e->n_any_staged += any->B->tiles_staged;
    e->n_any_global += any->B->tiles_global;
    e->n_any_plain += any->B->tiles_plain;
    d_pcm = e->pcm.p;
  }
  if (mix && !wide && ns) {
    // d_pcm holds the interleaved frames so far (staging, or rs_in): their downmix and conversion into the
    // device PCM buffer (the staging and rs_in are 256-byte aligned, as the launch's word reads need)
    HIPCHK(e, e->pcm.reserve(ss * ns));
    const char* r = lay_d + lay_fp;
    bool staged = false;
    HIPCHK(e, launch_resample_mix(mix->tab ? mix->tab->plan : ResamplePlan{1, 1, 0, 1}, mix->d_taps, !mix->tab, mix->channels,
                                  static_cast<const int16_t*>(d_pcm), reinterpret_cast<const int64_t*>(r),
                                  reinterpret_cast<const int64_t*>(r + b_ro), reinterpret_cast<const int32_t*>(r + 2 * b_ro),
                                  reinterpret_cast<const int32_t*>(r + 2 * b_ro + b_rt), rs_toff[nclips],
                                  e->pcm.as<int16_t>(), e->stream, &staged));
    e->n_mix_launch++;
    e->n_mix_in += mix->in_off[nclips];
    e->n_mix_out += ns;
    e->n_mix_staged += staged ? 1 : 0;
    d_pcm = e->pcm.p;
  }
  const int64_t* d_sbeg = reinterpret_cast<const int64_t*>(lay_d);
  const int64_t* d_send = reinterpret_cast<const int64_t*>(lay_d + b_sb);
  const int64_t* d_foff = reinterpret_cast<const int64_t*>(lay_d + 2 * b_sb);
  const int32_t* d_toff = reinterpret_cast<const int32_t*>(lay_d + 2 * b_sb + b_fo);
  const int32_t* d_tclip = reinterpret_cast<const int32_t*>(lay_d + 2 * b_sb + b_fo + b_to);
  if (f32)
    HIPCHK(e, launch_fingerprint_f32(e->fpcfg, T, static_cast<const float*>(d_pcm), d_sbeg, d_send, d_foff, d_toff, d_tclip,
                                     toff[nclips], e->micro.as<int32_t>(), e->db.as<double>(), e->stream,
                                     exact_q ? e->logfix : LogFix{}, &e->fpstats));
  else
    HIPCHK(e, launch_fingerprint(e->fpcfg, T, fx, tile_frames, static_cast<const int16_t*>(d_pcm), d_sbeg, d_send, d_foff,
                                 d_toff, d_tclip, toff[nclips], nf, e->micro.as<int32_t>(), e->db.as<double>(),
                                 e->stream, exact_q ? e->logfix : LogFix{}, &e->fpstats,
                                 nclips == 1 && sbeg[0] == 0 ? send[0] : -1));
  *nframes_out = nf;
  if (foff_out) *foff_out = foff;
  return TFP_OK;
}

// The clips of one buffer at sample offsets offsets[0..nclips] as (pointer, length) lists.
void split_offsets(const void* pcm, size_t ss, const int64_t* offsets, int32_t nclips, std::vector<const void*>* ptrs,
                   std::vector<int64_t>* lens) {
  ptrs->resize(nclips);
  lens->resize(nclips);
  for (int32_t c = 0; c < nclips; c++) {
    (*ptrs)[c] = static_cast<const char*>(pcm) + ss * offsets[c];
    (*lens)[c] = offsets[c + 1] - offsets[c];
  }
}

int copy_frames_out(tfp_engine* e, int64_t nf, const std::vector<int64_t>& foff, tfp_frame* out) {
  std::vector<int32_t> m(2 * nf);
  std::vector<double> d(2 * nf);
  if (nf) {
    HIPCHK(e, hipMemcpyAsync(m.data(), e->micro.p, sizeof(int32_t) * 2 * nf, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(d.data(), e->db.p, sizeof(double) * 2 * nf, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->stage_pending = false;
  size_t c = 0;
  for (int64_t g = 0; g < nf; g++) {
    while (c + 1 < foff.size() && foff[c + 1] <= g) c++;
    out[g].frame_idx = (int32_t)(g - foff[c]);
    out[g].m1 = m[2 * g];
    out[g].m2 = m[2 * g + 1];
    out[g].reserved = 0;
    out[g].q1 = d[2 * g];
    out[g].q2 = d[2 * g + 1];
  }
  return TFP_OK;
}

// ---- index -------------------------------------------------------------------------------

int stage_reserve(tfp_engine* e, int64_t extra) {
  const int64_t need = e->n_staged + extra;
  if (need <= e->cap_staged) return TFP_OK;
  int64_t cap = std::max<int64_t>(need, std::max<int64_t>(1 << 16, e->cap_staged * 2));
  DevBuf n1, n2, nc;
  HIPCHK(e, n1.reserve(sizeof(int32_t) * cap));
  HIPCHK(e, n2.reserve(sizeof(int32_t) * cap));
  HIPCHK(e, nc.reserve(sizeof(int32_t) * cap));
  if (e->n_staged) {
    HIPCHK(e, hipMemcpyAsync(n1.p, e->st_m1.p, sizeof(int32_t) * e->n_staged, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(n2.p, e->st_m2.p, sizeof(int32_t) * e->n_staged, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(nc.p, e->st_clip.p, sizeof(int32_t) * e->n_staged, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  e->st_m1.swap_with(n1);
  e->st_m2.swap_with(n2);
  e->st_clip.swap_with(nc);
  e->cap_staged = cap;
  return TFP_OK;
}

int new_clip(tfp_engine* e, const char* uuid, int64_t nrows, int64_t off, int32_t* id) {
  if (!uuid || !*uuid || strlen(uuid) >= 64) return fail(e, TFP_E_ARG, "bad uuid");
  if (e->by_uuid.count(uuid)) return fail(e, TFP_E_EXISTS, "uuid %s already indexed", uuid);
  Clip c;
  c.uuid = uuid;
  c.nrows = nrows;
  c.off = off;
  *id = (int32_t)e->clips.size();
  e->clips.push_back(c);
  e->by_uuid[uuid] = *id;
  e->live_rows += nrows;
  e->dirty = true;
  return TFP_OK;
}

// Staging rows of live clips, moved down over the rows of removed clips (clip ids and row order
// kept): one block per run of rows.
__global__ void compact_rows_kernel(const int64_t* __restrict__ runs /*[n][3]: src, dst, len*/, const int32_t* m1,
                                    const int32_t* m2, const int32_t* cl, int32_t* o1, int32_t* o2, int32_t* oc) {
  const int64_t src = runs[3 * blockIdx.x], dst = runs[3 * blockIdx.x + 1], len = runs[3 * blockIdx.x + 2];
  for (int64_t i = threadIdx.x; i < len; i += blockDim.x) {
    o1[dst + i] = m1[src + i];
    o2[dst + i] = m2[src + i];
    oc[dst + i] = cl[src + i];
  }
}

// Drops the staging rows of removed clips once they outnumber a quarter of the live rows (else
// delete/re-enrol cycles grow the staging area, and every rebuild sorts the dead rows too).
int compact_staging(tfp_engine* e) {
  int64_t live = 0;
  for (const auto& c : e->clips)
    if (c.alive) live += c.nrows;
  const int64_t dead = e->n_staged - live;
  if (dead <= std::max<int64_t>(1 << 16, live / 4)) return TFP_OK;
  // The new layout is built aside and written into e->clips only once the copy has succeeded: a
  // failure below (allocation, launch) leaves the staging rows and every clip's offset as they were.
  std::vector<int64_t> runs, new_off(e->clips.size(), 0);
  int64_t dst = 0;
  for (size_t i = 0; i < e->clips.size(); i++) {
    const Clip& c = e->clips[i];
    if (!c.alive || !c.nrows) continue;
    const size_t nr = runs.size();
    if (nr && runs[nr - 3] + runs[nr - 1] == c.off && runs[nr - 2] + runs[nr - 1] == dst) runs[nr - 1] += c.nrows;
    else runs.insert(runs.end(), {c.off, dst, c.nrows});
    new_off[i] = dst;
    dst += c.nrows;
  }
  DevBuf n1, n2, nc, d_runs;
  const int64_t cap = std::max<int64_t>(live, 1 << 16);
  HIPCHK(e, n1.reserve(sizeof(int32_t) * cap));
  HIPCHK(e, n2.reserve(sizeof(int32_t) * cap));
  HIPCHK(e, nc.reserve(sizeof(int32_t) * cap));
  const int32_t nruns = (int32_t)(runs.size() / 3);
  if (e->fail_compact > 0) {  // TFP_TEST_FAIL_COMPACT: an allocation failure here, for the tests
    e->fail_compact--;
    return fail(e, TFP_E_NOMEM, "compact_staging: injected allocation failure");
  }
  if (nruns) {
    int rc = upload(e, d_runs, runs.data(), sizeof(int64_t) * runs.size());
    if (rc) return rc;
    hipLaunchKernelGGL(compact_rows_kernel, dim3(nruns), dim3(256), 0, e->stream, d_runs.as<int64_t>(),
                       e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), e->st_clip.as<int32_t>(), n1.as<int32_t>(),
                       n2.as<int32_t>(), nc.as<int32_t>());
    HIPCHK(e, hipGetLastError());
  }
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->st_m1.swap_with(n1);
  e->st_m2.swap_with(n2);
  e->st_clip.swap_with(nc);
  for (size_t i = 0; i < e->clips.size(); i++) {
    Clip& c = e->clips[i];
    if (c.alive) c.off = new_off[i];
    else c.nrows = 0, c.off = 0;
  }
  e->n_staged = live;
  e->cap_staged = cap;
  return TFP_OK;
}

// Live clips in uuid order (the columns: the tie-break order of SQLite's result sort) and each
// clip's rank (-1 when dead). Incremental: the previous build's order with the clips added since
// merged in (no re-sort of every uuid).
// Returns true for an update that only adds (no clip of the last build removed) with at most
// kMergeBreaks new uuids placed before an old one: the old columns are then col_clip as it stands
// (no alive filter), *brk is the merge's column map (old col c -> c + breakpoints <= c) and rank
// holds the new clips' ranks only (the merge and the device rank table read no other; skipping
// the scatter over every clip is most of an enrolment's host time at 100k clips).
bool live_order(const tfp_engine* e, bool incremental, std::vector<int32_t>* live, std::vector<int32_t>* rank,
                MergeBreaks* brk) {
  auto by_uuid = [&](int32_t a, int32_t b) { return e->clips[a].uuid < e->clips[b].uuid; };
  live->clear();
  brk->n = -1;
  if (incremental) {
    const bool add_only = !e->removed_built;
    std::vector<int32_t> kept, add;
    if (!add_only) {
      kept.reserve(e->col_clip.size());
      for (int32_t c : e->col_clip)
        if (e->clips[c].alive) kept.push_back(c);
    }
    const std::vector<int32_t>& old = add_only ? e->col_clip : kept;
    for (int32_t i = (int32_t)e->built_clips; i < (int32_t)e->clips.size(); i++)
      if (e->clips[i].alive) add.push_back(i);
    std::sort(add.begin(), add.end(), by_uuid);
    // each new uuid's place by binary search, the old runs between them copied whole: log C
    // string compares per new clip instead of a linear merge (each compare is two uuid strings
    // on the heap, a cache miss apiece: ~10 ms at 100k clips)
    live->reserve(old.size() + add.size());
    std::vector<int32_t> at_col(add.size());
    int32_t before_old = 0;  // new uuids placed before some old one
    auto from = old.begin();
    for (size_t j = 0; j < add.size(); j++) {
      const auto at = std::lower_bound(from, old.end(), add[j], by_uuid);
      live->insert(live->end(), from, at);
      live->push_back(add[j]);
      from = at;
      at_col[j] = (int32_t)(at - old.begin());
      before_old += at != old.end();
    }
    live->insert(live->end(), from, old.end());
    if (add_only && before_old <= kMergeBreaks) {
      brk->n = 0;
      for (int32_t p : at_col)
        if ((size_t)p < old.size()) brk->p[brk->n++] = p;
      rank->assign(std::max<size_t>(e->clips.size(), 1), -1);
      for (size_t j = 0; j < add.size(); j++) (*rank)[add[j]] = at_col[j] + (int32_t)j;
      return true;
    }
  } else {
    for (int32_t i = 0; i < (int32_t)e->clips.size(); i++)
      if (e->clips[i].alive) live->push_back(i);
    std::sort(live->begin(), live->end(), by_uuid);
  }
  rank->assign(std::max<size_t>(e->clips.size(), 1), -1);
  for (size_t r = 0; r < live->size(); r++) (*rank)[(*live)[r]] = (int32_t)r;
  return false;
}

// Staging rows [b, b + n) sorted by m1 with the rows that cannot match (dead clip or NULL max1,
// key INT32_MAX) last: m1 in keys_b, m2 in vals_a, col in keys_a; the count of the others (the
// first ones) in e->cnt. Asynchronous: the merge runs over all n rows (those with key INT32_MAX
// land after every index row, past the new row count) and the count is read with its result,
// one host wait per update instead of two.
int sort_staged_rows(tfp_engine* e, int64_t b, int64_t n) {
  HIPCHK(e, e->keys_a.reserve(sizeof(int32_t) * (n + 1)));
  HIPCHK(e, e->keys_b.reserve(sizeof(int32_t) * (n + 1)));
  HIPCHK(e, e->vals_a.reserve(sizeof(int32_t) * (n + 1)));
  HIPCHK(e, e->vals_b.reserve(sizeof(int32_t) * (n + 1)));
  HIPCHK(e, launch_index_keys(e->st_m1.as<int32_t>() + b, e->st_clip.as<int32_t>() + b, e->rank_of_clip.as<int32_t>(), n,
                              e->keys_a.as<int32_t>(), e->vals_a.as<int32_t>(), e->stream));
  size_t tb = 0;
  HIPCHK(e, radix_sort_pairs(nullptr, &tb, nullptr, nullptr, nullptr, nullptr, n, e->stream));
  HIPCHK(e, e->sort_tmp.reserve(tb));
  HIPCHK(e, radix_sort_pairs(e->sort_tmp.p, &tb, e->keys_a.as<int32_t>(), e->keys_b.as<int32_t>(),
                             e->vals_a.as<int32_t>(), e->vals_b.as<int32_t>(), n, e->stream));
  HIPCHK(e, e->cnt.reserve(sizeof(int64_t)));
  HIPCHK(e, launch_count_below(e->keys_b.as<int32_t>(), n, INT32_MAX, e->cnt.as<int64_t>(), e->stream));
  HIPCHK(e, launch_index_gather(e->vals_b.as<int32_t>(), e->st_m2.as<int32_t>() + b, e->st_clip.as<int32_t>() + b,
                                e->rank_of_clip.as<int32_t>(), n, e->vals_a.as<int32_t>(), e->keys_a.as<int32_t>(), e->stream));
  return TFP_OK;
}

// e->cnt (sort_staged_rows' row count) after the work queued on e->stream. Synchronous.
int read_sorted_count(tfp_engine* e, int64_t* valid) {
  HIPCHK(e, hipMemcpyAsync(valid, e->cnt.p, sizeof *valid, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  return TFP_OK;
}

// Index update without a full re-sort (tfp_index.hip): the rows staged since the last build are
// sorted alone and merged into (m1s, m2s, cols) in one pass that also drops removed clips' rows
// and renumbers the columns around the inserted / removed uuids. Commits nothing on failure.
// fast_brk: live_order's column map of an update that only adds (rank then holds the new clips'
// ranks only), else nullptr (the map from rank over every old column).
int merge_index(tfp_engine* e, const std::vector<int32_t>& rank, const MergeBreaks* fast_brk, int32_t new_cols,
                bool* carried) {
  *carried = false;
  const int64_t b = e->built_staged, n = e->n_staged - e->built_staged;
  bool removed = false;
  MergeBreaks brk;
  int rc = TFP_OK;
  if (fast_brk) {
    brk = *fast_brk;
  } else {
    // old column -> new column (-1: the clip was removed)
    std::vector<int32_t> remap(std::max<size_t>(e->col_clip.size(), 1), -1);
    for (size_t c = 0; c < e->col_clip.size(); c++) {
      remap[c] = rank[e->col_clip[c]];
      removed |= remap[c] < 0;
    }
    // without removals remap[c] - c only steps up (uuid order is kept): its breakpoints, when few
    brk.n = removed ? -1 : 0;
    for (size_t c = 0, shift = 0; brk.n >= 0 && c < e->col_clip.size(); c++)
      while ((size_t)remap[c] - c > shift) {
        if (brk.n == kMergeBreaks) {
          brk.n = -1;
          break;
        }
        brk.p[brk.n++] = (int32_t)c;
        shift++;
      }
    if (brk.n < 0 && (rc = upload(e, e->remap, remap.data(), sizeof(int32_t) * remap.size())))  // (only when gathered)
      return rc;
  }
  // (e.g. new tie-break keys only: the rows and their columns are unchanged; a clip without rows
  // placed before an old one still renumbers the columns)
  if (n == 0 && !removed && brk.n == 0) return TFP_OK;
  if (n > 0 && (rc = sort_staged_rows(e, b, n))) return rc;
  const int64_t R = e->nrows;
  HIPCHK(e, e->m1s_b.reserve_grow(sizeof(int32_t) * (R + n + 1)));
  HIPCHK(e, e->m2s_b.reserve_grow(sizeof(int32_t) * (R + n + 1)));
  HIPCHK(e, e->cols_b.reserve_grow(sizeof(int32_t) * (R + n + 1)));
  int64_t kept = R;
  HIPCHK(e, launch_merge_update(e->m1s.as<int32_t>(), e->m2s.as<int32_t>(), e->cols.as<int32_t>(), R, e->remap.as<int32_t>(),
                                removed, brk, e->keys_b.as<int32_t>(), e->vals_a.as<int32_t>(), e->keys_a.as<int32_t>(), n,
                                &e->merge, e->m1s_b.as<int32_t>(), e->m2s_b.as<int32_t>(), e->cols_b.as<int32_t>(), &kept,
                                e->stream));
  int64_t valid = 0;
  if (n > 0 && (rc = read_sorted_count(e, &valid))) return rc;
  HIPCHK(e, hipStreamSynchronize(e->stream));
  e->m1s.swap_with(e->m1s_b);
  e->m2s.swap_with(e->m2s_b);
  e->cols.swap_with(e->cols_b);
  e->nrows = kept + valid;
  // The clip order (when built) through the same update: its old rows renumbered, the new rows
  // inserted (tfp_index.hpp). Best effort: on failure it is rebuilt when next needed.
  if (e->order.valid) {
    e->order.valid = false;
    auto by_uuid = [&](int32_t a, int32_t c) { return e->clips[a].uuid < e->clips[c].uuid; };
    std::vector<int32_t> add;
    for (int32_t i = (int32_t)e->built_clips; i < (int32_t)e->clips.size(); i++)
      if (e->clips[i].alive) add.push_back(i);
    std::sort(add.begin(), add.end(), by_uuid);
    const int32_t D = (int32_t)add.size();
    std::vector<int32_t> nca(2 * (size_t)std::max(D, 1));  // new columns, then their insertion points among the old columns
    for (int32_t j = 0; j < D; j++) {
      nca[j] = rank[add[j]];
      nca[D + j] = fast_brk ? rank[add[j]] - j
                            : (int32_t)(std::lower_bound(e->col_clip.begin(), e->col_clip.end(), add[j], by_uuid) - e->col_clip.begin());
    }
    int64_t orows = 0;
    const size_t on = (size_t)std::max<int64_t>(e->order.rows + valid, 1);
    if ((!D || upload(e, e->order.newcol, nca.data(), sizeof(int32_t) * nca.size()) == TFP_OK) &&
        e->order.key_b.reserve_grow(sizeof(unsigned long long) * on) == hipSuccess &&
        e->order.m1_b.reserve_grow(sizeof(int32_t) * on) == hipSuccess &&
        launch_order_merge(e->order.key.as<unsigned long long>(), e->order.m1.as<int32_t>(), e->order.rows, e->remap.as<int32_t>(), removed,
                           brk, e->keys_b.as<int32_t>(), e->vals_a.as<int32_t>(), e->keys_a.as<int32_t>(), valid,
                           e->order.newcol.as<int32_t>(), e->order.newcol.as<int32_t>() + D, D, &e->merge, &e->order.merge,
                           e->order.key_b.as<unsigned long long>(), e->order.m1_b.as<int32_t>(), &orows, e->stream) == hipSuccess &&
        hipStreamSynchronize(e->stream) == hipSuccess && orows == e->nrows) {  // (nca is read by then)
      e->order.key.swap_with(e->order.key_b);
      e->order.m1.swap_with(e->order.m1_b);
      e->order.rows = orows;
      e->order.valid = true;
      e->order.n_merges++;
    } else {
      (void)hipGetLastError();
    }
  }
  // The small path's key ranges and bitsets, carried to the merged index at their tolerance
  // instead of rebuilt from every box row (tfp_index.hpp): the ranges are searched again, every
  // surviving column's bits move to its new column (removed clips' and an index delta's columns
  // dropped: the delta's clips are among the new rows), then the new rows' bits are set. Best
  // effort: on any failure the bitsets are rebuilt when next needed.
  const int32_t W = key_bits_words(new_cols);
  const int32_t Cm = (int32_t)e->col_clip.size();
  KeyRanges& kr = e->tc.ranges.active();
  if (e->tc.ranges.active_valid() && kr.bits_valid && kr.bits_cols >= Cm &&
      kr.key_bits.bytes >= sizeof(uint32_t) * (size_t)kKeyRange * key_bits_words(kr.bits_cols)) {
    hipStream_t s = e->stream;
    bool ok = launch_key_ranges_all(e->m1s.as<int32_t>(), e->nrows, e->tc.ranges.active_tol(), kr.rng_all.as<int64_t>(), s) == hipSuccess &&
              e->key_bits_b.reserve(sizeof(uint32_t) * (size_t)kKeyRange * W) == hipSuccess &&
              launch_key_bits_remap(kr.key_bits.as<uint32_t>(), key_bits_words(kr.bits_cols), Cm,
                                    brk.n >= 0 ? nullptr : e->remap.as<int32_t>(), brk, e->key_bits_b.as<uint32_t>(), W,
                                    s) == hipSuccess;
    if (ok) kr.key_bits.swap_with(e->key_bits_b);
    if (ok && valid > 0)
      ok = launch_key_bits_add(kr.rng_all.as<int64_t>(), e->m1s.as<int32_t>(), e->keys_b.as<int32_t>(), e->keys_a.as<int32_t>(),
                               valid, W, kr.key_bits.as<uint32_t>(), s) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    *carried = ok;
  }
  return TFP_OK;
}

// A live clip's tie-break key is in [0, INT32_MAX] (tiresias_fp.h): the packed result key carries it
// as its unsigned low half, where a negative key would outrank every other clip's.
int fail_negative_key(tfp_engine* e, int32_t clip, int32_t k) {
  return fail(e, TFP_E_ARG, "tie-break key %d given to live clip %s: keys lie in [0, 2^31 - 1]", k,
              e->clips[clip].uuid.c_str());
}

int full_index(tfp_engine* e);

int delta_update(tfp_engine* e);
bool delta_eligible(const tfp_engine* e);

int rebuild(tfp_engine* e) {
  if (!e->dirty) return TFP_OK;
  if (delta_eligible(e)) return delta_update(e);
  int rc;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
  // Incremental (merge) when there is an index to merge into, the new rows are few next to it, and
  // the staging area needs no compaction (the staged rows since the last build are then exactly
  // rows [built_staged, n_staged)); otherwise the full build.
  const int64_t live_rows = e->live_rows;
  const int64_t dead = e->n_staged - live_rows, fresh = e->n_staged - e->built_staged;
  const bool incremental = e->built && !e->force_full && fresh <= std::max<int64_t>(e->nrows / 2, 0) &&
                           dead <= std::max<int64_t>(1 << 16, live_rows / 4) && e->n_staged < INT32_MAX;
  if (!incremental) {
    e->built = false;  // a failure below leaves the next attempt a full build as well
    if ((rc = compact_staging(e))) return rc;
    // the sort and the index rows use 32-bit row numbers
    if (e->n_staged >= INT32_MAX)
      return fail(e, TFP_E_CAPACITY, "%lld staged rows (limit 2^31 - 1)", (long long)e->n_staged);
  }
  std::vector<int32_t> live, rank;
  MergeBreaks brk;
  const bool add_only = live_order(e, incremental, &live, &rank, &brk);
  const double t_order = ms_since(t0);
  const size_t nkeys = std::max<size_t>(live.size(), 1);
  std::vector<int32_t> tiekey;  // column -> tie-break key: with an override every column, else the identity's new tail
  // key -> column: the identity without an override (the key is the uuid rank), so no map is built
  // (a 100k-entry hash map was most of an enrolment's host time); with one, a map that also
  // rejects a key given twice
  std::unordered_map<int32_t, int32_t> key_col;
  const bool ovr = !e->tiebreak_override.empty();
  if (ovr) {
    key_col.reserve(live.size());
    tiekey.assign(nkeys, 0);
  }
  for (size_t r = 0; ovr && r < live.size(); r++) {
    const int32_t clip = live[r];
    // With an override every live clip needs its own key (a clip added after the override would
    // otherwise take its local rank, which can equal another shard's global key).
    if ((size_t)clip >= e->tiebreak_override.size())
      return fail(e, TFP_E_ARG, "clip %s was added after tfp_index_set_tiebreak: set the tie-break keys again",
                  e->clips[clip].uuid.c_str());
    const int32_t k = e->tiebreak_override[clip];
    if (k < 0) return fail_negative_key(e, clip, k);
    if (!key_col.emplace(k, (int32_t)r).second) return fail(e, TFP_E_ARG, "tie-break key %d given to two live clips", k);
    tiekey[r] = k;
  }
  // Device copies, only the parts that changed (two 400 KB pageable uploads were a tenth of an
  // enrolment at 100k clips): a merge reads the ranks of the clips added since the last build
  // only (their staged rows), and identity tie keys keep their prefix.
  {
    const size_t rb = incremental ? std::min(e->built_clips, rank.size()) : 0;
    HIPCHK(e, e->rank_of_clip.reserve_grow(sizeof(int32_t) * rank.size()));
    HIPCHK(e, hipMemcpyAsync(e->rank_of_clip.as<int32_t>() + rb, rank.data() + rb, sizeof(int32_t) * (rank.size() - rb),
                             hipMemcpyHostToDevice, e->stream));
    const void* before = e->tiekey.p;
    const int64_t ident = e->tiekey_ident;
    e->tiekey_ident = -1;
    HIPCHK(e, e->tiekey.reserve_grow(sizeof(int32_t) * nkeys));
    const size_t tb = !ovr && e->tiekey.p == before && ident > 0 ? std::min<size_t>((size_t)ident, nkeys) : 0;
    if (!ovr) {
      tiekey.resize(nkeys - tb);
      std::iota(tiekey.begin(), tiekey.end(), (int32_t)tb);
    }
    if (nkeys > tb)
      HIPCHK(e, hipMemcpyAsync(e->tiekey.as<int32_t>() + tb, tiekey.data(), sizeof(int32_t) * (nkeys - tb),
                               hipMemcpyHostToDevice, e->stream));
    if (!ovr) e->tiekey_ident = (int64_t)nkeys;
  }
  const double t_keys = ms_since(t0);
  bool carried = false;
  if (incremental) {
    if ((rc = merge_index(e, rank, add_only ? &brk : nullptr, (int32_t)live.size(), &carried))) return rc;
    e->n_merges++;
  } else {
    e->nrows = 0;
    e->order.valid = false;  // (the clip order is rebuilt from the new index when next needed)
    if ((rc = full_index(e))) return rc;
    e->n_full_builds++;
  }
  e->ncols = (int32_t)live.size();
  e->col_clip = std::move(live);
  e->delta.reset(e->ncols);  // (every clip is in the main index now)
  e->key_col = std::move(key_col);
  e->ovr_main_stale = !ovr;  // (with an override: its keys for these columns are on the device now)
  e->key_identity = !ovr;
  e->built = true;
  e->built_clips = e->clips.size();
  e->built_staged = e->n_staged;
  e->removed_built = false;
  e->dirty = false;
  // the key-range and clip-set caches follow the index: every entry is for the previous versions
  // now, but the active ranges and bitsets when merge_index carried them
  e->index_version++;
  e->main_version++;
  if (carried) {
    e->tc.ranges.carry(e->index_version);
    e->tc.ranges.active().bits_cols = e->ncols;
  } else {
    e->tc.ranges.invalidate_active();
  }
  if (e->dbg_index)
    fprintf(stderr, "[tfp] index %s: %lld rows, %d clips; order %.3f keys %.3f total %.3f ms\n",
            incremental ? "merge" : "full build", (long long)e->nrows, e->ncols, t_order, t_keys, ms_since(t0));
  return TFP_OK;
}

// The full build: every staged row of a live clip, radix-sorted by m1 (the sorted arrays become
// the index buffers).
int full_index(tfp_engine* e) {
  const int64_t n = e->n_staged;
  int64_t valid = 0;
  if (n > 0) {
    int rc = sort_staged_rows(e, 0, n);
    if (!rc) rc = read_sorted_count(e, &valid);
    if (rc) return rc;
    e->m1s.swap_with(e->keys_b);
    e->m2s.swap_with(e->vals_a);
    e->cols.swap_with(e->keys_a);
  } else {
    HIPCHK(e, e->m1s.reserve(4));
    HIPCHK(e, e->m2s.reserve(4));
    HIPCHK(e, e->cols.reserve(4));
  }
  e->nrows = valid;
  return TFP_OK;
}

// Row ranges of every key's box at tolerance tole, cached per index version and tolerance
// (tc.ranges); a tolerance first seen gets the ranges only: its bitsets are built when a vote path
// asks for them (ensure_key_bits).
int ensure_ranges(tfp_engine* e, double tole, hipStream_t s) {
  if (e->tc.ranges.find(tole, e->index_version)) return TFP_OK;
  KeyRanges* kr = e->tc.ranges.claim(e->index_version);
  kr->bits_valid = false;
  HIPCHK(e, kr->rng_all.reserve(sizeof(int64_t) * 2 * kKeyRange));
  HIPCHK(e, launch_key_ranges_all(e->m1s.as<int32_t>(), e->nrows, tole, kr->rng_all.as<int64_t>(), s));
  e->tc.ranges.commit(tole, e->index_version);
  return TFP_OK;
}

// The small path's key-presence bitsets, from the cached row ranges (after ensure_ranges).
int delta_bits(tfp_engine* e, hipStream_t s);

int ensure_key_bits(tfp_engine* e, hipStream_t s) {
  KeyRanges& kr = e->tc.ranges.active();
  if (kr.bits_valid) return TFP_OK;
  HIPCHK(e, kr.key_bits.reserve(sizeof(uint32_t) * (size_t)kKeyRange * key_bits_words(e->ncols)));
  // the boxes' rows in all: a row is in the boxes of the keys within tol of its m1
  const double tl = e->tc.ranges.active_tol();
  const int64_t per_row = std::isfinite(tl) && tl >= 0 && tl < kKeyRange ? 2 * (int64_t)ceil(tl) + 2 : kKeyRange;
  HIPCHK(e, launch_key_bits(kr.rng_all.as<int64_t>(), e->cols.as<int32_t>(), e->ncols, e->nrows * std::min<int64_t>(per_row, kKeyRange),
                            e->kb_win, e->kb_direct, kr.key_bits.as<uint32_t>(), s));
  int rc = delta_bits(e, s);  // (the delta's columns, from its staged rows)
  if (rc) return rc;
  kr.bits_valid = true;
  kr.bits_cols = e->ncols;
  return TFP_OK;
}

// ---- index delta ---------------------------------------------------------------------------

// The keys' "%f" boxes at tolerance tole (launch_key_boxes), for the caches built from a clip order
// and the delta's key bits.
int ensure_kbox(tfp_engine* e, double tole, hipStream_t s) {
  if (e->tc.kbox.holds(tole, 0)) return TFP_OK;
  DevBuf* kbox = e->tc.kbox.begin();
  HIPCHK(e, kbox->reserve(sizeof(int64_t) * 2 * kKeyRange));
  HIPCHK(e, launch_key_boxes(tole, kbox->as<int64_t>(), s));
  e->tc.kbox.commit(tole, 0);
  return TFP_OK;
}

// The delta's key bits at the active bitsets' tolerance, into columns that hold no bit.
int delta_bits(tfp_engine* e, hipStream_t s) {
  if (e->delta.clip.empty()) return TFP_OK;
  const double tole = e->tc.ranges.active_tol();
  int rc = ensure_kbox(e, tole, s);
  if (rc) return rc;
  const int32_t kspan = (int32_t)ceil(tole) + 1;  // (delta_tol_ok: tol <= 8)
  HIPCHK(e, launch_delta_bits(e->delta.d_clips.as<DeltaClip>(), (int32_t)e->delta.clip.size(), e->st_m1.as<int32_t>(),
                              e->tc.kbox.p.as<int64_t>(), kspan, key_bits_words(e->ncols),
                              e->tc.ranges.active().key_bits.as<uint32_t>(), s));
  return TFP_OK;
}

// Tolerances the delta's bits are set for: finite, 0 <= tol <= 8 (a row is in at most 2 ceil(tol) + 3
// keys' boxes); other searches merge the delta first.
bool delta_tol_ok(double tol) { return std::isfinite(tol) && tol >= 0.0 && tol <= 8.0; }

bool delta_eligible(const tfp_engine* e) {
  if (!e->delta.use || !e->built || e->force_full || e->delta.force_merge || e->removed_built || e->n_staged >= INT32_MAX ||
      (int64_t)e->col_clip.size() < e->delta.min_cols)
    return false;
  int64_t n = 0, rows = 0;
  for (size_t i = e->built_clips; i < e->clips.size(); i++)
    if (e->clips[i].alive) {
      n++;
      rows += e->clips[i].nrows;
    }
  return n <= IndexDelta::kMaxClips && rows <= IndexDelta::kMaxRows;
}

// An update that only adds (or removes clips added since the last build): the new clips become the
// delta, in uuid order after the main columns; the tie keys are re-derived (global uuid ranks, or
// the override's keys), and the key bits get the delta's columns. The main index, its row ranges
// and its columns' bits stay as they are: the cost is the new clips' rows, not a pass over the DB.
int delta_update(tfp_engine* e) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  hipStream_t s = e->stream;
  auto by_uuid = [&](int32_t a, int32_t b) { return e->clips[a].uuid < e->clips[b].uuid; };
  std::vector<int32_t> add;
  int64_t rows = 0;
  for (int32_t i = (int32_t)e->built_clips; i < (int32_t)e->clips.size(); i++)
    if (e->clips[i].alive) {
      add.push_back(i);
      rows += e->clips[i].nrows;
    }
  std::sort(add.begin(), add.end(), by_uuid);
  const int32_t Cm = (int32_t)e->col_clip.size(), D = (int32_t)add.size();
  std::vector<int32_t> at(std::max(D, 1));
  for (int32_t j = 0; j < D; j++)
    at[j] = (int32_t)(std::lower_bound(e->col_clip.begin(), e->col_clip.end(), add[j], by_uuid) - e->col_clip.begin());
  const int32_t col0 = D ? (Cm + 1023) / 1024 * 1024 : Cm;
  const int32_t ncols = D ? col0 + IndexDelta::kMaxClips : Cm;
  // tie keys (and the key -> column maps with an override)
  const bool ovr = !e->tiebreak_override.empty();
  const void* tk_before = e->tiekey.p;
  HIPCHK(e, e->tiekey.reserve_grow(sizeof(int32_t) * std::max(ncols, 1)));
  std::unordered_map<int32_t, int32_t> key_col_delta;
  std::vector<int32_t> tk;  // host staging of the keys uploaded (kept until the sync below)
  if (ovr) {
    auto key_of_clip = [&](int32_t clip, int32_t* k) -> int {
      if ((size_t)clip >= e->tiebreak_override.size())
        return fail(e, TFP_E_ARG, "clip %s was added after tfp_index_set_tiebreak: set the tie-break keys again",
                    e->clips[clip].uuid.c_str());
      *k = e->tiebreak_override[clip];
      return *k < 0 ? fail_negative_key(e, clip, *k) : TFP_OK;
    };
    // the main columns' keys: only when the override changed for them (or their device copy was
    // lost to a larger buffer); otherwise the delta's clips alone (O(new clips), round 6)
    const bool main_up = e->ovr_main_stale || e->tiekey.p != tk_before;
    e->n_delta_main_keys += main_up;
    if (e->ovr_main_stale) {
      std::unordered_map<int32_t, int32_t> key_col;
      key_col.reserve(Cm);
      for (int32_t c = 0; c < Cm; c++) {
        int32_t k;
        if (int rc = key_of_clip(e->col_clip[c], &k)) return rc;
        if (!key_col.emplace(k, c).second) return fail(e, TFP_E_ARG, "tie-break key %d given to two live clips", k);
      }
      e->key_col = std::move(key_col);
    }
    tk.assign(main_up ? std::max(ncols, 1) : std::max(D, 1), 0);
    key_col_delta.reserve(D);
    for (int32_t j = 0; j < D; j++) {
      int32_t k;
      if (int rc = key_of_clip(add[j], &k)) return rc;
      if (e->key_col.count(k) || !key_col_delta.emplace(k, col0 + j).second)
        return fail(e, TFP_E_ARG, "tie-break key %d given to two live clips", k);
      tk[main_up ? col0 + j : j] = k;
    }
    if (main_up) {
      for (int32_t c = 0; c < Cm; c++) tk[c] = e->tiebreak_override[e->col_clip[c]];
      HIPCHK(e, hipMemcpyAsync(e->tiekey.p, tk.data(), sizeof(int32_t) * ncols, hipMemcpyHostToDevice, s));
    } else if (D) {
      HIPCHK(e, hipMemcpyAsync(e->tiekey.as<int32_t>() + col0, tk.data(), sizeof(int32_t) * D, hipMemcpyHostToDevice, s));
    }
    e->ovr_main_stale = false;
    e->tiekey_ident = -1;
  } else {
    HIPCHK(e, e->delta.d_at.reserve(sizeof(int32_t) * std::max(D, 1)));
    if (D) HIPCHK(e, hipMemcpyAsync(e->delta.d_at.p, at.data(), sizeof(int32_t) * D, hipMemcpyHostToDevice, s));
    HIPCHK(e, launch_delta_tiekey(e->delta.d_at.as<int32_t>(), D, Cm, col0, ncols, e->tiekey.as<int32_t>(), s));
    e->tiekey_ident = D ? -1 : Cm;
  }
  // the delta's clips for the bits kernel
  std::vector<DeltaClip> dc(std::max(D, 1));
  for (int32_t j = 0; j < D; j++) {
    const Clip& c = e->clips[add[j]];
    dc[j] = DeltaClip{c.off, (int32_t)c.nrows, col0 + j};
  }
  HIPCHK(e, e->delta.d_clips.reserve(sizeof(DeltaClip) * std::max(D, 1)));
  if (D) HIPCHK(e, hipMemcpyAsync(e->delta.d_clips.p, dc.data(), sizeof(DeltaClip) * D, hipMemcpyHostToDevice, s));
  e->delta.clip = std::move(add);
  e->delta.at.assign(at.begin(), at.begin() + D);
  e->delta.col0 = col0;
  e->delta.rows = rows;
  e->ncols = ncols;
  e->delta.key_col = std::move(key_col_delta);
  e->key_identity = !ovr;
  // key bits: the first delta after a build widens the rows (the delta's columns start at a
  // multiple of 1024): the main columns' words move to the wider rows in one 2-D device copy
  // (~13 MB at 100k clips) instead of a rebuild from the index rows (46 ms at 100k clips)
  KeyRanges& kr = e->tc.ranges.active();
  const bool bits = e->tc.ranges.active_valid() && kr.bits_valid;
  if (bits && D > 0 && kr.bits_cols != ncols && kr.bits_cols <= col0) {
    const int32_t Wo = key_bits_words(kr.bits_cols), Wn = key_bits_words(ncols);
    if (Wn > Wo) {
      const size_t nb = sizeof(uint32_t) * (size_t)kKeyRange * Wn;
      HIPCHK(e, e->key_bits_b.reserve(nb));
      HIPCHK(e, hipMemsetAsync(e->key_bits_b.p, 0, nb, s));
      HIPCHK(e, hipMemcpy2DAsync(e->key_bits_b.p, sizeof(uint32_t) * Wn, kr.key_bits.p, sizeof(uint32_t) * Wo,
                                 sizeof(uint32_t) * Wo, kKeyRange, hipMemcpyDeviceToDevice, s));
      kr.key_bits.swap_with(e->key_bits_b);
    }
    kr.bits_cols = ncols;
  }
  // the delta columns cleared and set again when the layout stands, else rebuilt later
  if (bits && kr.bits_cols == ncols && D > 0) {
    const int32_t W = key_bits_words(ncols);
    HIPCHK(e, hipMemset2DAsync(kr.key_bits.as<uint32_t>() + col0 / 32, sizeof(uint32_t) * W, 0,
                               sizeof(uint32_t) * (IndexDelta::kMaxClips / 32), kKeyRange, s));
    int rc = delta_bits(e, s);
    if (rc) return rc;
  } else {
    kr.bits_valid = false;
  }
  HIPCHK(e, hipStreamSynchronize(s));  // (dc and at are released on return)
  e->dirty = false;
  e->index_version++;  // (other tolerances' cached ranges and bitsets are for the previous index;
  e->tc.ranges.carry(e->index_version);  // the main index, so the active ones, stand)
  e->delta.n_updates++;
  if (e->dbg_index)
    fprintf(stderr, "[tfp] index delta: %d clips (%lld rows) beside %d main columns; %.3f ms\n", D, (long long)rows, Cm,
            std::chrono::duration<double, std::milli>(clk::now() - t0).count());
  return TFP_OK;
}

// The delta merged into the main index now (coefs = 2, a fallback to the row scan, a tolerance the
// delta's bits do not cover).
int consolidate(tfp_engine* e) {
  if (e->delta.clip.empty() && !e->dirty) return TFP_OK;
  e->delta.force_merge = true;
  e->dirty = true;
  const int rc = rebuild(e);
  e->delta.force_merge = false;
  return rc;
}

// The clip order of the current index (tfp_kernels.hpp), built when first needed: the index rows'
// keys (nearest-integer key, column, m2) radix-sorted once; merge_index carries it afterwards.
int ensure_order(tfp_engine* e, hipStream_t s) {
  if (e->order.valid) return TFP_OK;
  const int64_t R = e->nrows;
  if (R >= INT32_MAX) return fail(e, TFP_E_CAPACITY, "clip order: %lld rows", (long long)R);
  const size_t n = (size_t)std::max<int64_t>(R, 1);
  HIPCHK(e, e->order.key.reserve_grow(sizeof(unsigned long long) * n));
  HIPCHK(e, e->order.m1.reserve_grow(sizeof(int32_t) * n));
  HIPCHK(e, e->order.key_b.reserve_grow(sizeof(unsigned long long) * n));
  HIPCHK(e, e->order.m1_b.reserve_grow(sizeof(int32_t) * n));
  HIPCHK(e, launch_order_fill(e->m1s.as<int32_t>(), e->m2s.as<int32_t>(), e->cols.as<int32_t>(), R,
                              e->order.key_b.as<unsigned long long>(), e->order.m1_b.as<int32_t>(), s));
  HIPCHK(e, order_sort(e->order.key_b.as<unsigned long long>(), e->order.key.as<unsigned long long>(), e->order.m1_b.as<int32_t>(),
                       e->order.m1.as<int32_t>(), R, &e->order.sort_tmp, s));
  e->order.rows = R;
  e->order.valid = true;
  e->order.n_builds++;
  return TFP_OK;
}

// One build of the main clip-set cache at tolerance tole into c (after ensure_ranges at tole): from
// the clip order for tolerances up to kOrderMaxTol (no sort), else from the boxes' rows.
int build_cells(tfp_engine* e, CellCache* c, double tole, hipStream_t s) {
  if (e->fail_cells > 0 && --e->fail_cells == 0)  // TFP_TEST_FAIL_CELLS
    return fail(e, TFP_E_NOMEM, "clip order: injected allocation failure");
  if (tole >= 0.0 && tole <= kOrderMaxTol && e->nrows > 0 && e->nrows < INT32_MAX) {
    int rc = ensure_order(e, s);
    if (rc || (rc = ensure_kbox(e, tole, s))) return rc;
    HIPCHK(e, c->build_from_order(e->order.key.as<unsigned long long>(), e->order.m1.as<int32_t>(), e->order.rows,
                                  e->tc.kbox.p.as<int64_t>(), (int32_t)e->col_clip.size(), tole, s));
    if (c->valid) e->tc.n_from_order++;
  } else {
    const DevBuf& rng_all = e->tc.ranges.active().rng_all;
    std::vector<int64_t> rng(2 * kKeyRange), off(kKeyRange + 1, 0);
    HIPCHK(e, hipMemcpyAsync(rng.data(), rng_all.p, sizeof(int64_t) * rng.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    for (int k = 0; k < kKeyRange; k++) off[k + 1] = off[k] + std::max<int64_t>(0, rng[2 * k + 1] - rng[2 * k]);
    HIPCHK(e, c->build(rng_all.as<int64_t>(), off.data(), e->m2s.as<int32_t>(), e->cols.as<int32_t>(),
                       (int32_t)e->col_clip.size(), e->nrows, tole, s));
  }
  return TFP_OK;
}

// The general path's clip-set cache at tolerance tole, per main index version and tolerance
// (tc.cells): afterwards tc.cells.active() is the cache to search with. It is optional: if preparing
// or building it fails (an allocation, a library call), nothing is committed or recorded, the active
// cache is left not valid and the batch takes the row scan (tfp_scan.hip); the next search tries again.
int ensure_cells(tfp_engine* e, double tole, hipStream_t s) {
  const CellCache* was = &e->tc.cells.active();
  if (const CellCache* c = e->tc.cells.find(tole, e->main_version)) {
    e->tc.n_hits += c != was;  // (taken from beside the active one)
    return TFP_OK;
  }
  CellCache* c = e->tc.cells.claim(e->main_version);
  e->tc.n_builds++;
  if (quietly(e, [&] { return build_cells(e, c, tole, s); }) == TFP_OK) {
    e->tc.cells.commit(tole, e->main_version);
    return TFP_OK;
  }
  (void)hipGetLastError();
  if (e->dbg_vote) fprintf(stderr, "[tfp] clip-set cache not built: row scan\n");
  c->invalidate();
  HIPCHK(e, hipStreamSynchronize(s));
  return TFP_OK;
}

// The index delta's clip-set cache at tolerance tole (<= kOrderMaxTol): the delta's staged rows in
// clip order (sorted once per delta version, for any tolerance), then the main cache's filter.
// Valid (or known empty: no delta row in a box) at the current index version.
int ensure_delta_cells(tfp_engine* e, double tole, hipStream_t s) {
  if (e->tc.dcells.holds(tole, e->index_version)) return TFP_OK;
  CellCache* dc = e->tc.dcells.begin();
  dc->invalidate();
  const int32_t D = (int32_t)e->delta.clip.size();
  const int64_t n = e->delta.rows;
  if (D > 0 && n > 0) {
    if (e->fail_delta_cells > 0 && --e->fail_delta_cells == 0)  // TFP_TEST_FAIL_DELTA_CELLS
      return fail(e, TFP_E_NOMEM, "delta clip order: injected allocation failure");
    if (!e->tc.dorder.holds(0.0, e->index_version)) {
      DeltaOrder* o = e->tc.dorder.begin();
      HIPCHK(e, o->key.reserve_grow(sizeof(unsigned long long) * n));
      HIPCHK(e, o->m1.reserve_grow(sizeof(int32_t) * n));
      HIPCHK(e, o->key_b.reserve_grow(sizeof(unsigned long long) * n));
      HIPCHK(e, o->m1_b.reserve_grow(sizeof(int32_t) * n));
      HIPCHK(e, launch_delta_order_fill(e->delta.d_clips.as<DeltaClip>(), D, e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(),
                                        o->key_b.as<unsigned long long>(), o->m1_b.as<int32_t>(), s));
      HIPCHK(e, order_sort(o->key_b.as<unsigned long long>(), o->key.as<unsigned long long>(), o->m1_b.as<int32_t>(),
                           o->m1.as<int32_t>(), n, &o->sort_tmp, s));
      e->tc.dorder.commit(0.0, e->index_version);
    }
    int rc = ensure_kbox(e, tole, s);
    if (rc) return rc;
    const DeltaOrder& o = e->tc.dorder.p;
    HIPCHK(e, dc->build_from_order(o.key.as<unsigned long long>(), o.m1.as<int32_t>(), n, e->tc.kbox.p.as<int64_t>(), D, tole,
                                   s));
    e->tc.n_delta_builds++;
  }
  e->tc.dcells.commit(tole, e->index_version);
  return TFP_OK;
}

// Can the sweep serve a search at tolerance tole with the index delta beside the main index?
bool delta_wide_ok(const tfp_engine* e, double tole) {
  return e->delta.wide && tole >= 0.0 && tole <= kOrderMaxTol && tole >= e->wide_min_tol;
}

// ---- search core: frames' q values already on device (e->q, 2 doubles per frame) -----------

// What a search form returns besides TFP_OK (the results are out) and an error (< 0):
constexpr int kNext = 1;         // not for this batch, or it could not finish it: the next form
constexpr int kNeedsSorted = 2;  // it needs the sorted rows to hold every clip: merge the index delta, start over

// fp_search_fingerprint_info's arguments as the kernels take them (search_core, rank_core).
SearchConsts search_consts(const tfp_search_params* P) {
  SearchConsts sc;
  memset(&sc, 0, sizeof sc);
  sc.coefs = P->coefs;
  sc.tole = P->tolerance < 0 ? TFP_DEFAULT_TOLERANCE : P->tolerance;  // fp_handler.c:252-256
  sc.has_low = P->freq_ignore_low > 0;
  sc.has_high = P->freq_ignore_high > 0;
  if (sc.has_low) sc.thr_low = 10 * log10((double)P->freq_ignore_low);
  if (sc.has_high) sc.thr_high = 10 * log10((double)P->freq_ignore_high);
  return sc;
}

// The batch's relative query offsets qo on the device (e->qoff), copied when they change.
int ensure_qoff(tfp_engine* e, const std::vector<int64_t>& qo, hipStream_t s) {
  if (qo == e->qoff_host && s == e->qoff_stream) return TFP_OK;
  const size_t bytes = sizeof(int64_t) * qo.size();
  if (e->qoff_pending) HIPCHK(e, hipEventSynchronize(e->qoff_ev));  // previous copy done reading
  HIPCHK(e, e->qoff.reserve(bytes));
  HIPCHK(e, e->qoff_pin.reserve(bytes));
  memcpy(e->qoff_pin.p, qo.data(), bytes);
  HIPCHK(e, hipMemcpyAsync(e->qoff.p, e->qoff_pin.p, bytes, hipMemcpyHostToDevice, s));
  if (!e->qoff_ev) HIPCHK(e, hipEventCreateWithFlags(&e->qoff_ev, hipEventDisableTiming));
  HIPCHK(e, hipEventRecord(e->qoff_ev, s));
  e->qoff_pending = true;
  e->qoff_host = qo;
  e->qoff_stream = s;
  return TFP_OK;
}

// The row scan's scratch for queries in chunks of <= 256 MB per array (*chunk queries at a time):
// stamp / score / touched chunk x C int32, tcnt chunk int32, zero here and after every scan.
int ensure_scan_scratch(tfp_engine* e, int32_t nq, int32_t C, int64_t* chunk_out, hipStream_t s) {
  int64_t chunk = (int64_t)(256ll << 20) / (4ll * C);
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, nq));
  *chunk_out = chunk;
  const size_t bytes = sizeof(int32_t) * chunk * C;
  if (bytes > e->scan_zeroed || bytes > e->stamp.bytes || bytes > e->score.bytes || bytes > e->touched.bytes ||
      sizeof(int32_t) * chunk > e->tcnt.bytes) {
    HIPCHK(e, e->stamp.reserve(bytes));
    HIPCHK(e, e->score.reserve(bytes));
    HIPCHK(e, e->touched.reserve(bytes));
    HIPCHK(e, e->tcnt.reserve(sizeof(int32_t) * chunk));
    const size_t z = std::min(std::min(e->stamp.bytes, e->score.bytes), e->touched.bytes);
    HIPCHK(e, hipMemsetAsync(e->stamp.p, 0, z, s));
    HIPCHK(e, hipMemsetAsync(e->score.p, 0, z, s));
    HIPCHK(e, hipMemsetAsync(e->tcnt.p, 0, e->tcnt.bytes, s));
    e->scan_zeroed = z;  // (touched is written before it is read)
  }
  return TFP_OK;
}

// One batch on its way through the forms (search_core): the call's arguments, then the set-up the
// forms share.
struct Batch {
  int32_t nq;
  const double* d_q;
  std::vector<unsigned long long>& keys;
  unsigned long long* d_keys_out;
  hipStream_t s;
  SearchConsts sc;
  std::vector<int64_t> qo;  // query offsets from 0
  int64_t nf = 0, max_frames = 0;
  bool has_delta = false;
  int32_t C = 0;             // columns (with a delta: its reserved ones too)
  int64_t R = 0, R_all = 0;  // rows of the main index; with the delta's
  // one buffer: the vote path's key mask (32 words), max count (1), pad (1), VoteMeta (4), then
  // best[Qp] (u64); zeroed by prep_boxes. VoteMeta directly before best[]: one copy brings both back.
  static constexpr int kMaskWords = kKeyRange / 32, kMetaWord = kMaskWords + 2, kMiscWords = kMetaWord + 4;
  static_assert(sizeof(VoteMeta) == 16 && kMiscWords % 2 == 0, "meta + 8-byte aligned best[]");
  int32_t Qp = 0, nzero = 0;
  uint32_t* d_mask = nullptr;
  int32_t* d_max = nullptr;
  unsigned long long* d_best = nullptr;
};

// Small batch (batch-1 latency): one vote launch over the cached key bitsets, results into
// host-mapped memory.
int search_small(tfp_engine* e, Batch& b) {
  const int32_t nq = b.nq;
  hipStream_t s = b.s;
  if (b.d_keys_out || b.sc.coefs != 1 || nq < 1 || nq > kSmallQ || b.C <= 0 || b.R_all <= 0) return kNext;
  for (int32_t i = 0; i < nq; i++)
    if (b.qo[i + 1] - b.qo[i] > 2048) return kNext;  // counts bounded like the fp16 path
  SmallQueries sq;
  memset(&sq, 0, sizeof sq);
  sq.nq = nq;
  for (int32_t i = 0; i <= nq; i++) sq.qoff[i] = b.qo[i];
  const int32_t C = b.C;
  HIPCHK(e, e->small_res.reserve(small_result_bytes(C), hipHostMallocMapped | hipHostMallocCoherent));
  if (e->small_res.p != e->small_res_host) {
    HIPCHK(e, hipHostGetDevicePointer(reinterpret_cast<void**>(&e->small_res_dev), e->small_res.p, 0));
    e->small_res_host = e->small_res.p;
  }
  int rc;
  if ((rc = ensure_ranges(e, b.sc.tole, s)) || (rc = ensure_key_bits(e, s))) return rc;
  HIPCHK(e, launch_search_small(b.d_q, sq, b.sc, e->tc.ranges.active().key_bits.as<uint32_t>(), C, e->tiekey.as<int32_t>(),
                                e->small_res_dev, s));
  HIPCHK(e, hipStreamSynchronize(s));
  // the vote ran after the fingerprint kernel, which read the staged upload: it is free again
  e->stage_pending = false;
  // the vote's blocks wrote their per-query maxima into host memory: the max over the blocks
  SmallResult* h = e->small_res.as<SmallResult>();
  if (h->bad) return b.has_delta ? kNeedsSorted : kNext;  // a key outside the vote range: the general path (over the index's rows)
  if (h->ku > 0) {
    const unsigned long long* part = small_result_parts(h);
    const int32_t nb = small_vote_blocks(C);
    for (int32_t i = 0; i < nq; i++) {
      unsigned long long k = 0ull;
      for (int32_t blk = 0; blk < nb; blk++) k = std::max(k, part[(size_t)blk * kSmallQ + i]);
      b.keys[i] = k;
    }
  }
  e->n_path_small++;
  return TFP_OK;
}

// Vote-matrix path (after prep_boxes' zeroing), no host round trip: key mask -> used-key compaction
// -> A (per-query counts) and Bt -> GEMM.
int search_vote(tfp_engine* e, Batch& b) {
  const int32_t nq = b.nq, Qp = b.Qp, C = b.C;
  hipStream_t s = b.s;
  const SearchConsts& sc = b.sc;
  const int32_t Cp = ((C + 31) / 32) * 32;
  HIPCHK(e, e->A.reserve(sizeof(_Float16) * (size_t)Qp * kVoteKpMax));
  HIPCHK(e, e->Bt.reserve(sizeof(_Float16) * (size_t)Cp * kVoteKpMax));
  VoteMeta* d_meta = reinterpret_cast<VoteMeta*>(b.d_mask + Batch::kMetaWord);
  int rc;
  if ((rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_key_bits(e, s))) return rc;
  const uint32_t* key_bits = e->tc.ranges.active().key_bits.as<uint32_t>();
  HIPCHK(e, launch_key_mask(b.d_q, sc, b.nf, b.d_mask, b.d_max, d_meta, s));
  HIPCHK(e, launch_build_A(b.d_q, sc, e->qoff.as<int64_t>(), nq, Qp, b.d_mask, b.d_max, d_meta, e->class_ku_max,
                           e->A.as<_Float16>(), e->Bt.as<_Float16>(), Cp, s));
  HIPCHK(e, launch_build_B(b.d_mask, key_bits, C, d_meta, Cp, e->Bt.as<_Float16>(), s));
  HIPCHK(e, e->vote_part.reserve(sizeof(unsigned long long) * (size_t)vote_chunks(Cp) * Qp));
  HIPCHK(e, launch_vote_gemm(e->A.as<_Float16>(), e->Bt.as<_Float16>(), Qp, Cp, d_meta, e->tiekey.as<int32_t>(),
                             e->vote_part.as<unsigned long long>(), b.d_best, b.d_mask, key_bits, C, s));
  // the results go out before the ok flag is known (one host wait); a redo overwrites them.
  // Host results: (VoteMeta, best[nq]) in one copy into pinned memory.
  const size_t back = sizeof(VoteMeta) + (b.d_keys_out ? 0 : sizeof(unsigned long long) * nq);
  HIPCHK(e, e->vres_pin.reserve(back));
  if (b.d_keys_out)
    HIPCHK(e, hipMemcpyAsync(b.d_keys_out, b.d_best, sizeof(unsigned long long) * nq, hipMemcpyDeviceToDevice, s));
  HIPCHK(e, hipMemcpyAsync(e->vres_pin.p, d_meta, back, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  VoteMeta hm;
  memcpy(&hm, e->vres_pin.p, sizeof hm);
  if (!b.d_keys_out && nq)
    memcpy(b.keys.data(), e->vres_pin.as<char>() + sizeof(VoteMeta), sizeof(unsigned long long) * nq);
  if (e->dbg_vote) fprintf(stderr, "[tfp] vote: nq %d Qp %d C %d ku %d kp %d ok %d\n", nq, Qp, C, hm.ku, hm.kp, hm.ok);
  if (hm.ok) {
    (hm.cls ? e->n_path_class : e->n_path_gemm)++;
    return TFP_OK;
  }
  e->n_path_redone++;
  // a count above fp16's exact range or a key outside the vote range: the scan path (over the
  // sorted rows), which needs the frames' boxes too
  if (b.has_delta) return kNeedsSorted;
  HIPCHK(e, launch_prep_boxes(b.d_q, b.nf, sc, e->boxes.as<FrameBox>(), b.d_mask, b.nzero, s));
  return kNext;
}

// General path (tfp_scan.hip), after prep_boxes over every frame: the sweep by groups, run
// speculatively (its sort's counts checked with the results: one host wait per batch) and redone
// when they say so; else the cells form / row scan over the sorted rows.
int search_general(tfp_engine* e, Batch& b) {
  const int32_t nq = b.nq, C = b.C;
  const int64_t nf = b.nf, R = b.R;
  hipStream_t s = b.s;
  const SearchConsts& sc = b.sc;
  unsigned long long *const d_keys_out = b.d_keys_out, *const d_best = b.d_best;
  const bool general = C > 0 && R > 0 && (sc.coefs == 1 || sc.coefs == 2);
  int rc;
  for (int pass = 0;; pass++) {
    bool spec = false;  // the sweep ran without the host reading its sort's counts (checked below)
    bool spec_mapped = false;  // its counts were written to spec_pin by its last kernel
    bool out_written = false;  // the sweep wrote its keys straight into d_keys_out
    bool swept = false;        // the sweep by groups ran (not the cells form / row scan)
    bool bins_used = false;
    CellCache* cells = nullptr;  // this pass's clip-set cache (not valid: none, the row scan)
    if (general) {
      if ((rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_cells(e, sc.tole, s))) return rc;
      cells = &e->tc.cells.active();
    }
    if (general && sc.tole >= e->wide_min_tol) {
      // the sweep by groups, unless a frame needs the row scan
      if (e->dbg_vote && !cells->valid) fprintf(stderr, "[tfp] general path: no clip-set cache (row scan)\n");
      // with a delta: its cache too (a failure to build it is recovered: the delta is merged, below)
      bool dsweep = b.has_delta && cells->valid;
      if (dsweep && quietly(e, [&] { return ensure_delta_cells(e, sc.tole, s); }) != TFP_OK) {
        (void)hipGetLastError();
        dsweep = false;
      }
      if (cells->valid && (dsweep || !b.has_delta)) {
        HIPCHK(e, e->wide.reserve(nf, nq, s));
        bool ok = false;
        // (a device caller's output buffer takes the sweep's keys directly: zeroed by the prepare)
        unsigned long long* wbest = d_keys_out ? d_keys_out : d_best;
        HIPCHK(e, launch_scan_wide_prepare(e->boxes.as<FrameBox>(), e->qoff.as<int64_t>(), nq, nf, b.max_frames, sc.tole,
                                           &e->wide, &ok, s, pass == 0, d_keys_out ? wbest : nullptr));
        bins_used = e->wide.ukeys_ready;  // (the bin sort ran on this pass)
        if (ok) {
          // a speculative sweep's counts come back through host-mapped memory, written by its last kernel
          int32_t* d_info = nullptr;
          if (e->wide.spec) {
            HIPCHK(e, e->spec_pin.reserve(4 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
            if (e->spec_pin.p != e->spec_pin_host) {
              HIPCHK(e, hipHostGetDevicePointer(reinterpret_cast<void**>(&e->spec_pin_dev), e->spec_pin.p, 0));
              e->spec_pin_host = e->spec_pin.p;
            }
            d_info = e->spec_pin_dev;
          }
          HIPCHK(e, launch_scan_wide(nq, nf, cells, e->tiekey.as<int32_t>(), C, &e->wide, wbest, s, d_info, &spec_mapped));
          if (dsweep && e->tc.dcells.p.valid) {  // the delta's clips into the same maxima
            HIPCHK(e, launch_scan_wide(nq, nf, &e->tc.dcells.p, e->tiekey.as<int32_t>(), C, &e->wide, wbest, s, d_info,
                                       &spec_mapped, e->delta.col0));
            e->tc.n_delta_sweeps++;
          }
          swept = true;
          out_written = d_keys_out != nullptr;
          spec = e->wide.spec;
        }
        if (e->dbg_vote) fprintf(stderr, "[tfp] general path: nq %d nf %lld C %d tol %g -> %s%s\n", nq, (long long)nf, C,
                                 sc.tole, ok ? "sweep by groups" : "cells / row scan", spec ? " (speculative)" : "");
      }
    }
    if (!swept && b.has_delta) return kNeedsSorted;  // the cells form and the row scan read the sorted rows
    if (!swept && general) {
      // queries in chunks of <= 256 MB of scratch per array
      int64_t chunk;
      if ((rc = ensure_scan_scratch(e, nq, C, &chunk, s))) return rc;
      if (cells->valid && cells->ensure_entries(s) != hipSuccess) {  // (the cells form's candidates)
        (void)hipGetLastError();
        cells->invalidate();  // every frame takes the row scan
      }
      for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
        const int32_t n = (int32_t)std::min<int64_t>(chunk, nq - q0);
        HIPCHK(e, launch_scan(e->boxes.as<FrameBox>(), e->qoff.as<int64_t>(), b.qo.data(), (int32_t)q0, n,
                              e->m1s.as<int32_t>(), e->m2s.as<int32_t>(), e->cols.as<int32_t>(), R, cells,
                              e->tiekey.as<int32_t>(), C, e->stamp.as<int32_t>(), e->score.as<int32_t>(),
                              e->touched.as<int32_t>(), e->tcnt.as<int32_t>(), d_best, s));
      }
    }
    // the speculative sweep's counts come back with the results (one host wait per batch)
    if (spec && !spec_mapped) {
      HIPCHK(e, e->spec_pin.reserve(4 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
      HIPCHK(e, hipMemcpyAsync(e->spec_pin.p, e->wide.info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (d_keys_out) {
      if (!out_written)
        HIPCHK(e, hipMemcpyAsync(d_keys_out, d_best, sizeof(unsigned long long) * nq, hipMemcpyDeviceToDevice, s));
    } else if (nq) {
      HIPCHK(e, hipMemcpyAsync(b.keys.data(), d_best, sizeof(unsigned long long) * nq, hipMemcpyDeviceToHost, s));
    }
    // (the scan kernels read and write engine scratch: the next call, on any stream or thread, may
    // reuse it only once they are done)
    HIPCHK(e, hipStreamSynchronize(s));
    if (spec) {
      const int32_t* info = e->spec_pin.as<int32_t>();
      if (info[1] > 0 || info[2] > 0) {  // a frame for the row scan, or a window the one-sort key cannot order
        if (e->dbg_vote) fprintf(stderr, "[tfp] speculative sweep redone (info %d %d %d)\n", info[0], info[1], info[2]);
        e->n_sweep_redo++;
        HIPCHK(e, hipMemsetAsync(d_best, 0, sizeof(unsigned long long) * nq, s));
        continue;
      }
      if (bins_used) e->n_sweep_crowd += info[3];
    }
    if (swept) (bins_used ? e->n_sweep_bins : e->n_sweep_lib)++;
    e->n_path_general++;
    return TFP_OK;
  }
}

// The forms in turn: the small batch, the vote GEMM, the general path. The index delta serves the
// coefs = 1 vote paths at the tolerances its bits cover, and the sweep (its own clip-set cache
// beside the main one) at tolerances up to kOrderMaxTol; any other search reads the sorted rows.
// Whether a batch is one of those is known up front, or a form finds out (kNeedsSorted):
// either way the delta is merged here, and the batch starts over on the merged index.
int search_core(tfp_engine* e, const int64_t* h_qoff, int32_t nq, const double* d_q, const tfp_search_params* P,
                std::vector<unsigned long long>& keys, unsigned long long* d_keys_out, hipStream_t s) {
  int rc = rebuild(e);  // synchronous on e->stream
  if (rc) return rc;
  Batch b{nq, d_q, keys, d_keys_out, s};
  SearchConsts& sc = b.sc;
  sc = search_consts(P);
  b.qo.assign(h_qoff, h_qoff + nq + 1);
  for (auto& v : b.qo) v -= h_qoff[0];
  b.nf = b.qo[nq];
  for (int32_t i = 0; i < nq; i++) b.max_frames = std::max<int64_t>(b.max_frames, b.qo[i + 1] - b.qo[i]);
  b.Qp = ((nq + 127) / 128) * 128;
  b.nzero = Batch::kMiscWords + 2 * b.Qp;

  for (bool merge = false;; merge = true) {
    if (merge && (rc = consolidate(e))) return rc;
    keys.assign(nq, 0ull);
    b.has_delta = !e->delta.clip.empty();
    b.C = e->ncols;
    b.R = e->nrows;
    b.R_all = e->nrows + e->delta.rows;  // rows that may match (main index + delta)
    const bool vote = sc.coefs == 1 && b.C > 0 && b.R_all > 0 && b.max_frames < 16384;  // packed scores exact below 16384 frames
    // up front: a tolerance the delta's bits do not cover; a batch for the cells form / row scan
    if (b.has_delta && (sc.coefs == 1 ? !delta_tol_ok(sc.tole) || (!vote && !delta_wide_ok(e, sc.tole))
                                      : !delta_wide_ok(e, sc.tole)))
      continue;
    if ((rc = search_small(e, b)) <= 0) return rc;
    if (rc == kNeedsSorted) continue;
    // Query offsets are the same on every call of one plan or stream: copy them only when they
    // change, from pinned memory so the copy is asynchronous (a pageable copy would make the host
    // wait for the queries' fingerprint kernels before it could launch the search).
    if ((rc = ensure_qoff(e, b.qo, s))) return rc;
    HIPCHK(e, e->boxes.reserve(sizeof(FrameBox) * (b.nf + 1)));
    HIPCHK(e, e->best.reserve(sizeof(uint32_t) * b.nzero));
    b.d_mask = e->best.as<uint32_t>();
    b.d_max = reinterpret_cast<int32_t*>(b.d_mask + Batch::kMaskWords);
    b.d_best = reinterpret_cast<unsigned long long*>(b.d_mask + Batch::kMiscWords);
    // the vote path needs only the zeroing; the scan path the frames' boxes too
    HIPCHK(e, launch_prep_boxes(d_q, vote ? 0 : b.nf, sc, e->boxes.as<FrameBox>(), b.d_mask, b.nzero, s));
    if (vote && (rc = search_vote(e, b)) <= 0) return rc;
    if ((!vote || rc == kNext) && (rc = search_general(e, b)) <= 0) return rc;
  }
}

// The index column of a tie-break key (-1: none). Without an override the key is the clip's rank
// among all live uuids: a main column's, or with a delta (ranks at[j] + j, ascending) either a delta
// column's or main column k - #{delta ranks below k}.
int32_t col_of_key(const tfp_engine* e, int32_t k) {
  if (e->key_identity) {
    const int32_t Cm = (int32_t)e->col_clip.size(), D = (int32_t)e->delta.clip.size();
    if (k < 0 || k >= Cm + D) return -1;
    int32_t lo = 0, hi = D;  // first delta j with rank >= k
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (e->delta.at[mid] + mid < k) lo = mid + 1; else hi = mid;
    }
    if (lo < D && e->delta.at[lo] + lo == k) return e->delta.col0 + lo;
    return k - lo;
  }
  auto it = e->key_col.find(k);
  if (it != e->key_col.end()) return it->second;
  auto jt = e->delta.key_col.find(k);
  return jt == e->delta.key_col.end() ? -1 : jt->second;
}

// The clip of an index column (-1: none): a main column or a delta column.
int32_t clip_of_col(const tfp_engine* e, int32_t col) {
  if (col >= 0 && (size_t)col < e->col_clip.size()) return e->col_clip[col];
  const int32_t j = col - e->delta.col0;
  return j >= 0 && (size_t)j < e->delta.clip.size() ? e->delta.clip[j] : -1;
}

void fill_results(tfp_engine* e, const std::vector<unsigned long long>& keys, const int64_t* qoff, int32_t nq,
                  tfp_result* out) {
  for (int32_t i = 0; i < nq; i++) {
    tfp_result& r = out[i];
    memset(&r, 0, sizeof r);
    r.frame_count = (int32_t)(qoff[i + 1] - qoff[i]);
    r.clip_id = -1;
    const unsigned long long k = keys[i];
    if (!k) continue;
    const int32_t clip = clip_of_col(e, col_of_key(e, (int32_t)(uint32_t)(k & 0xffffffffu)));
    if (clip < 0) continue;
    r.found = 1;
    r.match_count = (int32_t)(k >> 32);
    r.clip_id = clip;
    snprintf(r.uuid, sizeof r.uuid, "%s", e->clips[clip].uuid.c_str());
  }
}

bool valid_params(const tfp_search_params* P) { return P && P->coefs >= 1 && P->coefs <= 2; }

// The queries' frame values (q1, q2) on the device (e->q), as the frames forms search them.
int upload_frames(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq) {
  const int64_t nf = qoff[nq] - qoff[0];
  std::vector<double> q(2 * (nf + 1));
  for (int64_t i = 0; i < nf; i++) {
    q[2 * i] = frames[qoff[0] + i].q1;
    q[2 * i + 1] = frames[qoff[0] + i].q2;
  }
  return upload(e, e->q, q.data(), sizeof(double) * q.size());
}

// ---- the argument checks the forms share; `what` names the form in the message ----
int check_k(tfp_engine* e, const char* what, int32_t k) {
  if (k < 1 || k > TFP_RANK_MAX) return fail(e, TFP_E_ARG, "%s: k = %d outside [1, %d]", what, k, TFP_RANK_MAX);
  return TFP_OK;
}

int check_params(tfp_engine* e, const char* what, const tfp_search_params* P) {
  return valid_params(P) ? TFP_OK : fail(e, TFP_E_ARG, "%s: coefs outside [1, 2]", what);
}

// scopes (or nullptr: none to check): one per `item` ("query", "recording"), TFP_SCOPE_ANY or above.
int check_scopes(tfp_engine* e, const char* what, const int32_t* scopes, int32_t n, const char* item) {
  for (int32_t i = 0; scopes && i < n; i++)
    if (scopes[i] < TFP_SCOPE_ANY) return fail(e, TFP_E_ARG, "%s: scope %d of %s %d", what, scopes[i], item, i);
  return TFP_OK;
}

// The caller's offsets off[0..n] never fall (tfp_query_plan.hpp); the frames forms call theirs qoffsets.
int check_monotone(tfp_engine* e, const int64_t* off, int32_t n, bool samples) {
  if (offsets_monotone(off, n)) return TFP_OK;
  if (samples) return fail(e, TFP_E_ARG, "offsets not monotone");
  return fail(e, TFP_E_ARG, "qoffsets not monotone");
}

// ---- rate-normalised ingest (tfp_resample.hpp) ---------------------------------------------
// The table of a supported pair (P its plan) on the device: uploaded once per pair and kept for the
// engine's lifetime (the entry and its device copy never move).
int ensure_rs_table(tfp_engine* e, const ResamplePlan& P, int32_t rate_in, int32_t rate_out, const tfp_engine::RsTable** tab) {
  HIPCHK(e, hipSetDevice(e->device));
  auto it = e->rs_tables.find({P.M, P.L});
  if (it == e->rs_tables.end()) {
    bool bad = false;
    std::shared_ptr<const ResampleTable> host = resample_table(rate_in, rate_out, &bad);
    if (!host) return fail(e, TFP_E_ARG, "unsupported rate ratio %d -> %d", rate_in, rate_out);
    DevBuf dev;
    if (int rc = upload(e, dev, host->taps.data(), sizeof(int16_t) * host->taps.size())) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    tfp_engine::RsTable& t = e->rs_tables[{P.M, P.L}];
    t.host = host;
    t.dev.swap_with(dev);
    it = e->rs_tables.find({P.M, P.L});
  }
  *tab = &it->second;
  return TFP_OK;
}

// The rate source of a batch at rate_in != rate_out: checks the pair and the offsets, takes the pair's
// table onto the device (once per pair, kept), and gives the clips' offsets at rate_out (out_off[0] = 0).
int rate_source(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t n, int32_t rate_in, int32_t rate_out,
                RateSrc* rs, std::vector<int64_t>* out_off) {
  if (rate_in < 1 || rate_out < 1) return fail(e, TFP_E_ARG, "bad sample rate %d", rate_in < 1 ? rate_in : rate_out);
  if (int rc = check_monotone(e, offsets, n, true)) return rc;
  ResamplePlan P;
  bool bad = false;
  if (!resample_plan(rate_in, rate_out, &P, &bad))
    return fail(e, TFP_E_ARG, "unsupported rate ratio %d -> %d", rate_in, rate_out);
  const tfp_engine::RsTable* tab;
  if (int rc = ensure_rs_table(e, P, rate_in, rate_out, &tab)) return rc;
  rs->pcm = pcm && n ? pcm + offsets[0] : pcm;
  rs->tab = tab->host.get();
  rs->d_taps = tab->dev.as<int16_t>();
  rs->in_off.assign((size_t)std::max(n, 0) + 1, 0);
  out_off->assign((size_t)std::max(n, 0) + 1, 0);
  for (int32_t c = 0; c < n; c++) {
    const int64_t len = offsets[c + 1] - offsets[c], no = resample_count(P, len);
    if (no < 0) return fail(e, TFP_E_ARG, "clip %d: %lld samples past the index range", c, (long long)len);
    rs->in_off[c + 1] = rs->in_off[c] + len;
    (*out_off)[c + 1] = (*out_off)[c] + no;
  }
  return TFP_OK;
}

// ---- ranked search (tfp_rank.hpp): keys[q * K + r] = row r of query q's result set, 0 past the last

// The per-column scope table (tfp_scope.hpp) of the current index: built when the index version or a
// clip's scope changed since the last build (the columns' clips and the clips' scopes uploaded, one
// kernel), else it stands and a search does no per-clip work.
int ensure_scope_table(tfp_engine* e, hipStream_t s) {
  if (e->scope_version == e->index_version && !e->scope_dirty) return TFP_OK;
  const int32_t C = e->ncols, Cp = scope_table_cols(C);
  std::vector<int32_t> cc((size_t)std::max(Cp, 1), -1), cs(std::max<size_t>(e->clips.size(), 1), 0);
  std::copy(e->col_clip.begin(), e->col_clip.end(), cc.begin());  // (col_clip.size() <= ncols)
  for (size_t j = 0; j < e->delta.clip.size(); j++) cc[(size_t)e->delta.col0 + j] = e->delta.clip[j];
  e->scope_pop.clear();
  e->scope_live = 0;
  for (size_t i = 0; i < e->clips.size(); i++) {
    cs[i] = e->clips[i].scope;
    if (e->clips[i].alive) {
      e->scope_pop[cs[i]]++;
      e->scope_live++;
    }
  }
  HIPCHK(e, e->scope_colclip.reserve_grow(sizeof(int32_t) * cc.size()));
  HIPCHK(e, e->scope_clip.reserve_grow(sizeof(int32_t) * cs.size()));
  HIPCHK(e, e->scope_table.reserve_grow(sizeof(int32_t) * cc.size()));
  HIPCHK(e, hipMemcpyAsync(e->scope_colclip.p, cc.data(), sizeof(int32_t) * cc.size(), hipMemcpyHostToDevice, s));
  HIPCHK(e, hipMemcpyAsync(e->scope_clip.p, cs.data(), sizeof(int32_t) * cs.size(), hipMemcpyHostToDevice, s));
  HIPCHK(e, launch_scope_table(e->scope_colclip.as<int32_t>(), e->scope_clip.as<int32_t>(), C, e->scope_table.as<int32_t>(), s));
  HIPCHK(e, hipStreamSynchronize(s));  // (cc and cs are released on return)
  e->scope_version = e->index_version;
  e->scope_dirty = false;
  e->n_scope_builds++;
  return TFP_OK;
}

// A scoped batch's set-up: the table, and the queries' scopes on the device (read from the
// caller's array, which outlives the batch: every form waits for the stream before it returns).
int ensure_scopes(tfp_engine* e, const int32_t* scopes, int32_t nq, hipStream_t s) {
  int rc = ensure_scope_table(e, s);
  if (rc) return rc;
  return upload(e, e->scope_q, scopes, sizeof(int32_t) * (size_t)nq, s);
}

// The vote forms' result: nkeys keys with the bad flag after them (rank_keys, and rank_pin for the copy
// back). vote_keys_begin reserves both and zeroes the flag; vote_keys_end copies keys and flag back, waits,
// and fills keys unless the flag is set (*bad).
int vote_keys_begin(tfp_engine* e, size_t nkeys, unsigned long long** d_keys, int32_t** d_bad, hipStream_t s) {
  HIPCHK(e, e->rank_keys.reserve(sizeof(unsigned long long) * (nkeys + 1)));
  HIPCHK(e, e->rank_pin.reserve(sizeof(unsigned long long) * (nkeys + 1)));
  *d_keys = e->rank_keys.as<unsigned long long>();
  *d_bad = reinterpret_cast<int32_t*>(*d_keys + nkeys);
  HIPCHK(e, hipMemsetAsync(*d_bad, 0, sizeof(unsigned long long), s));
  return TFP_OK;
}

int vote_keys_end(tfp_engine* e, size_t nkeys, std::vector<unsigned long long>& keys, bool* bad, hipStream_t s) {
  HIPCHK(e, hipMemcpyAsync(e->rank_pin.p, e->rank_keys.p, sizeof(unsigned long long) * (nkeys + 1), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  const unsigned long long* h = e->rank_pin.as<unsigned long long>();
  *bad = (uint32_t)h[nkeys] != 0;
  if (!*bad) std::copy(h, h + nkeys, keys.begin());
  return TFP_OK;
}

// The general forms' set-up over the merged index (C > 0 columns): the batch's offsets and frame boxes on
// the device, the tolerance's ranges and clip-set cells (*cells), the scan scratch for *chunk queries at a
// time and, with scopes, the scope table and the queries' scopes.
int general_setup(tfp_engine* e, const std::vector<int64_t>& qo, int32_t nq, const double* d_q, const SearchConsts& sc,
                  const int32_t* scopes, CellCache** cells, int64_t* chunk, hipStream_t s) {
  const int64_t nf = qo[nq];
  int rc;
  if ((rc = ensure_qoff(e, qo, s))) return rc;
  HIPCHK(e, e->boxes.reserve(sizeof(FrameBox) * (nf + 1)));
  HIPCHK(e, launch_prep_boxes(d_q, nf, sc, e->boxes.as<FrameBox>(), nullptr, 0, s));
  if ((rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_cells(e, sc.tole, s))) return rc;
  *cells = &e->tc.cells.active();
  if ((rc = ensure_scan_scratch(e, nq, e->ncols, chunk, s))) return rc;
  if ((*cells)->valid && (*cells)->ensure_entries(s) != hipSuccess) {  // (the cells form's candidates)
    (void)hipGetLastError();
    (*cells)->invalidate();  // every frame takes the row scan
  }
  return scopes ? ensure_scopes(e, scopes, nq, s) : TFP_OK;
}

// The vote form (coefs = 1): *bad when a frame's key lies outside the vote range (keys undefined).
// scopes (or nullptr): the queries' scopes, for the scoped kernels (tfp_scope.hpp).
int rank_vote(tfp_engine* e, const std::vector<int64_t>& qo, int32_t nq, const double* d_q, const SearchConsts& sc,
              int32_t K, const int32_t* scopes, std::vector<unsigned long long>& keys, bool* bad, hipStream_t s) {
  const int32_t C = e->ncols, nb = rank_vote_blocks(C);
  int rc;
  if ((rc = ensure_qoff(e, qo, s)) || (rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_key_bits(e, s))) return rc;
  if (scopes && (rc = ensure_scopes(e, scopes, nq, s))) return rc;
  // queries in chunks of <= 256 MB of partial keys (and of the launch grid's second dimension)
  int64_t chunk = (int64_t)(256ll << 20) / ((int64_t)sizeof(unsigned long long) * nb * K);
  chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chunk, 65535), nq));
  const size_t nkeys = (size_t)nq * K;
  HIPCHK(e, e->rank_part.reserve(sizeof(unsigned long long) * (size_t)chunk * nb * K));
  unsigned long long* d_keys;
  int32_t* d_bad;
  if ((rc = vote_keys_begin(e, nkeys, &d_keys, &d_bad, s))) return rc;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int32_t n = (int32_t)std::min<int64_t>(chunk, nq - q0);
    if (scopes)
      HIPCHK(e, launch_scope_vote(d_q, e->qoff.as<int64_t>() + q0, e->scope_q.as<int32_t>() + q0, n, sc,
                                  e->tc.ranges.active().key_bits.as<uint32_t>(), C, e->tiekey.as<int32_t>(),
                                  e->scope_table.as<int32_t>(), K, e->rank_part.as<unsigned long long>(), d_keys + q0 * K,
                                  d_bad, s));
    else
      HIPCHK(e, launch_rank_vote(d_q, e->qoff.as<int64_t>() + q0, n, sc, e->tc.ranges.active().key_bits.as<uint32_t>(), C,
                                 e->tiekey.as<int32_t>(), K, e->rank_part.as<unsigned long long>(), d_keys + q0 * K, d_bad,
                                 s));
  }
  return vote_keys_end(e, nkeys, keys, bad, s);
}

// The general form (any coefs / tolerance / key), over the sorted rows of the merged index.
int rank_general(tfp_engine* e, const std::vector<int64_t>& qo, int32_t nq, const double* d_q, const SearchConsts& sc,
                 int32_t K, const int32_t* scopes, std::vector<unsigned long long>& keys, hipStream_t s) {
  const int32_t C = e->ncols;
  const int64_t R = e->nrows;
  if (C <= 0 || R <= 0) return TFP_OK;  // an empty index: no row
  CellCache* cells;
  int64_t chunk;
  if (int rc = general_setup(e, qo, nq, d_q, sc, scopes, &cells, &chunk, s)) return rc;
  const size_t nkeys = (size_t)nq * K;
  HIPCHK(e, e->rank_keys.reserve(sizeof(unsigned long long) * (nkeys + 1)));
  HIPCHK(e, e->rank_pin.reserve(sizeof(unsigned long long) * (nkeys + 1)));
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int32_t n = (int32_t)std::min<int64_t>(chunk, nq - q0);
    if (scopes) {  // the same counts, selected among the scope's clips
      HIPCHK(e, launch_scan_touched(e->boxes.as<FrameBox>(), e->qoff.as<int64_t>(), qo.data(), (int32_t)q0, n,
                                    e->m1s.as<int32_t>(), e->m2s.as<int32_t>(), e->cols.as<int32_t>(), R, cells, C,
                                    e->stamp.as<int32_t>(), e->score.as<int32_t>(), e->touched.as<int32_t>(),
                                    e->tcnt.as<int32_t>(), s));
      HIPCHK(e, launch_scope_final((int32_t)q0, n, e->scope_q.as<int32_t>(), e->tiekey.as<int32_t>(),
                                   e->scope_table.as<int32_t>(), C, e->stamp.as<int32_t>(), e->score.as<int32_t>(),
                                   e->touched.as<int32_t>(), e->tcnt.as<int32_t>(), K, e->rank_keys.as<unsigned long long>(),
                                   s));
      continue;
    }
    HIPCHK(e, launch_scan_ranked(e->boxes.as<FrameBox>(), e->qoff.as<int64_t>(), qo.data(), (int32_t)q0, n,
                                 e->m1s.as<int32_t>(), e->m2s.as<int32_t>(), e->cols.as<int32_t>(), R, cells,
                                 e->tiekey.as<int32_t>(), C, e->stamp.as<int32_t>(), e->score.as<int32_t>(),
                                 e->touched.as<int32_t>(), e->tcnt.as<int32_t>(), K, e->rank_keys.as<unsigned long long>(),
                                 s));
  }
  HIPCHK(e, hipMemcpyAsync(e->rank_pin.p, e->rank_keys.p, sizeof(unsigned long long) * nkeys, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));  // (the scan's scratch is free for the next call)
  const unsigned long long* h = e->rank_pin.as<unsigned long long>();
  std::copy(h, h + nkeys, keys.begin());
  return TFP_OK;
}

// Shaped like search_core. The vote form reads the key bitsets, which hold a live index delta's
// columns at the tolerances delta_tol_ok() names; every other ranked search merges the delta first.
// scopes (or nullptr: ranked search): scopes[q] restricts query q to that scope's clips (tfp_scope.hpp).
// count: the batch is a ranked / scoped search's own (catalog neighbours run the core for theirs and count there).
int rank_core(tfp_engine* e, const int64_t* h_qoff, int32_t nq, const double* d_q, const tfp_search_params* P, int32_t K,
              const int32_t* scopes, std::vector<unsigned long long>& keys, hipStream_t s, bool count = true) {
  int rc = rebuild(e);  // synchronous on e->stream
  if (rc) return rc;
  const SearchConsts sc = search_consts(P);
  const std::vector<int64_t> qo = relative_offsets(h_qoff, nq);
  keys.assign((size_t)nq * K, 0ull);
  if (sc.coefs == 1) {
    if (!e->delta.clip.empty() && !delta_tol_ok(sc.tole) && (rc = consolidate(e))) return rc;
    if (e->ncols <= 0 || e->nrows + e->delta.rows <= 0) return TFP_OK;
    bool bad = false;
    if ((rc = rank_vote(e, qo, nq, d_q, sc, K, scopes, keys, &bad, s))) return rc;
    if (!bad) {
      if (count) (scopes ? e->n_scope_vote : e->n_rank_vote)++;
      return TFP_OK;
    }
  }
  if ((rc = consolidate(e)) || (rc = rank_general(e, qo, nq, d_q, sc, K, scopes, keys, s))) return rc;
  if (count) (scopes ? e->n_scope_general : e->n_rank_general)++;
  return TFP_OK;
}

// ---- match census (tfp_census.hpp): hist[q * nbins + c] = the clips of scopes[q] with count c >= 1

// The vote form (coefs = 1): *bad when a frame's key lies outside the vote range (bins undefined).
int census_vote(tfp_engine* e, const std::vector<int64_t>& qo, int32_t nq, const double* d_q, const SearchConsts& sc,
                const int32_t* scopes, int32_t nbins, int32_t* hist, bool* bad, hipStream_t s) {
  const int32_t C = e->ncols;
  int rc;
  if ((rc = ensure_qoff(e, qo, s)) || (rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_key_bits(e, s)) ||
      (rc = ensure_scopes(e, scopes, nq, s)))
    return rc;
  const size_t n = (size_t)nq * nbins;
  HIPCHK(e, e->census_hist.reserve(sizeof(int32_t) * (n + 1)));
  HIPCHK(e, e->census_pin.reserve(sizeof(int32_t) * (n + 1)));
  int32_t* d_hist = e->census_hist.as<int32_t>();
  HIPCHK(e, hipMemsetAsync(d_hist, 0, sizeof(int32_t) * (n + 1), s));  // the bins and the bad flag after them
  for (int64_t q0 = 0; q0 < nq; q0 += 65535) {  // (the launch grid's second dimension)
    const int32_t m = (int32_t)std::min<int64_t>(65535, nq - q0);
    HIPCHK(e, launch_census_vote(d_q, e->qoff.as<int64_t>() + q0, e->scope_q.as<int32_t>() + q0, m, sc,
                                 e->tc.ranges.active().key_bits.as<uint32_t>(), C, e->scope_table.as<int32_t>(), nbins,
                                 d_hist + q0 * nbins, d_hist + n, s));
  }
  HIPCHK(e, hipMemcpyAsync(e->census_pin.p, d_hist, sizeof(int32_t) * (n + 1), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  const int32_t* h = e->census_pin.as<int32_t>();
  *bad = h[n] != 0;
  if (!*bad) std::copy(h, h + n, hist);
  return TFP_OK;
}

// The general form (any coefs / tolerance / key), over the sorted rows of the merged index.
int census_general(tfp_engine* e, const std::vector<int64_t>& qo, int32_t nq, const double* d_q, const SearchConsts& sc,
                   const int32_t* scopes, int32_t nbins, int32_t* hist, hipStream_t s) {
  const int32_t C = e->ncols;
  const int64_t R = e->nrows;
  if (C <= 0 || R <= 0) return TFP_OK;  // an empty index: no count above 0
  CellCache* cells;
  int64_t chunk;
  if (int rc = general_setup(e, qo, nq, d_q, sc, scopes, &cells, &chunk, s)) return rc;
  const size_t n = (size_t)nq * nbins;
  HIPCHK(e, e->census_hist.reserve(sizeof(int32_t) * (n + 1)));
  HIPCHK(e, e->census_pin.reserve(sizeof(int32_t) * (n + 1)));
  int32_t* d_hist = e->census_hist.as<int32_t>();
  HIPCHK(e, hipMemsetAsync(d_hist, 0, sizeof(int32_t) * n, s));
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    const int32_t m = (int32_t)std::min<int64_t>(chunk, nq - q0);
    HIPCHK(e, launch_scan_touched(e->boxes.as<FrameBox>(), e->qoff.as<int64_t>(), qo.data(), (int32_t)q0, m,
                                  e->m1s.as<int32_t>(), e->m2s.as<int32_t>(), e->cols.as<int32_t>(), R, cells, C,
                                  e->stamp.as<int32_t>(), e->score.as<int32_t>(), e->touched.as<int32_t>(),
                                  e->tcnt.as<int32_t>(), s));
    HIPCHK(e, launch_census_final((int32_t)q0, m, e->scope_q.as<int32_t>(), e->scope_table.as<int32_t>(), C,
                                  e->stamp.as<int32_t>(), e->score.as<int32_t>(), e->touched.as<int32_t>(),
                                  e->tcnt.as<int32_t>(), nbins, d_hist, s));
  }
  HIPCHK(e, hipMemcpyAsync(e->census_pin.p, d_hist, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));  // (the scan's scratch is free for the next call)
  const int32_t* h = e->census_pin.as<int32_t>();
  std::copy(h, h + n, hist);
  return TFP_OK;
}

// Shaped like rank_core (the same forms, the same rule for a live index delta); scopes[nq] holds a
// scope per query. On return hist[nq][nbins] is complete: bin 0 of a query is its scope's live
// clips (row-less ones included, removed ones not) minus the clips the kernels counted.
int census_core(tfp_engine* e, const int64_t* h_qoff, int32_t nq, const double* d_q, const tfp_search_params* P,
                const int32_t* scopes, int32_t nbins, int32_t* hist, hipStream_t s) {
  int rc = rebuild(e);  // synchronous on e->stream
  if (rc) return rc;
  const SearchConsts sc = search_consts(P);
  const std::vector<int64_t> qo = relative_offsets(h_qoff, nq);
  std::fill(hist, hist + (size_t)nq * nbins, 0);
  bool done = qo[nq] == 0;  // no frame: every live clip has count 0, and nothing is launched
  if (!done && sc.coefs == 1) {
    if (!e->delta.clip.empty() && !delta_tol_ok(sc.tole) && (rc = consolidate(e))) return rc;
    if (e->ncols <= 0 || e->nrows + e->delta.rows <= 0) {
      done = true;  // no row: the same
    } else {
      bool bad = false;
      if ((rc = census_vote(e, qo, nq, d_q, sc, scopes, nbins, hist, &bad, s))) return rc;
      if (!bad) {
        e->n_census_vote++;
        done = true;
      }
    }
  }
  if (!done) {
    if ((rc = consolidate(e)) || (rc = census_general(e, qo, nq, d_q, sc, scopes, nbins, hist, s))) return rc;
    e->n_census_general++;
  }
  // the scopes' live-clip populations, counted from e->clips when the scope table was built: current
  // after this (a no-op unless the index or a scope changed since), so a census does no per-clip work
  if ((rc = ensure_scope_table(e, s))) return rc;
  for (int32_t i = 0; i < nq; i++) {
    int32_t* row = hist + (size_t)i * nbins;
    int64_t n = 0;
    if (scopes[i] == kScopeAny) n = e->scope_live;
    else if (const auto it = e->scope_pop.find(scopes[i]); it != e->scope_pop.end()) n = it->second;
    row[0] = (int32_t)(n - tfp_census_at_least(row, nbins, 1));
  }
  return TFP_OK;
}

// The arguments every census entry point checks; fills sv with a scope per query.
int census_args(tfp_engine* e, const tfp_search_params* P, int32_t nq, const int32_t* scopes, const void* need_bins,
                std::vector<int32_t>& sv) {
  if (nq < 0 || !need_bins) return fail(e, TFP_E_ARG, "census: bad query count or NULL need_bins");
  int rc = check_params(e, "census", P);
  if (rc || (rc = check_scopes(e, "census", scopes, nq, "query"))) return rc;
  sv.assign((size_t)nq, kScopeAny);
  if (scopes) sv.assign(scopes, scopes + nq);
  return TFP_OK;
}

// *need_bins = the longest query's frames + 1; TFP_E_CAPACITY when nbins is below it.
int census_bins(tfp_engine* e, const int64_t* off, int32_t nq, int32_t nbins, const int32_t* hist, int32_t* need_bins) {
  const int64_t need = census_need(off, nq);
  if (need > INT32_MAX) return fail(e, TFP_E_ARG, "census: a query of %lld frames", (long long)need - 1);
  *need_bins = (int32_t)need;
  if (nbins < need) return fail(e, TFP_E_CAPACITY, "census: %d bins, the longest query needs %lld", nbins, (long long)need);
  if (nq && !hist) return fail(e, TFP_E_ARG, "census: hist is NULL");
  return TFP_OK;
}

// Keys to rows, as fill_results maps the winner's; counts[q] = the query's rows.
void fill_candidates(tfp_engine* e, const std::vector<unsigned long long>& keys, int32_t nq, int32_t K, tfp_candidate* out,
                     int32_t* counts) {
  memset(out, 0, sizeof(tfp_candidate) * (size_t)nq * K);
  for (int32_t i = 0; i < nq; i++) {
    int32_t n = 0;
    for (int32_t r = 0; r < K; r++) {
      const unsigned long long k = keys[(size_t)i * K + r];
      if (!k) break;
      const int32_t clip = clip_of_col(e, col_of_key(e, (int32_t)(uint32_t)(k & 0xffffffffu)));
      if (clip < 0) continue;
      tfp_candidate& c = out[(size_t)i * K + n++];
      c.match_count = (int32_t)(k >> 32);
      c.clip_id = clip;
      snprintf(c.uuid, sizeof c.uuid, "%s", e->clips[clip].uuid.c_str());
    }
    counts[i] = n;
  }
}

// ---- sliding search (tfp_slide.hpp): keys[j * K + r] = row r of window j, 0 past the last. fo: the
// recordings' relative frame offsets into d_q; woff: the first window of each recording.

// The vote form: *bad when a frame's key lies outside the vote range (keys undefined).
int slide_vote(tfp_engine* e, const std::vector<int64_t>& fo, int32_t nrec, const double* d_q, const SearchConsts& sc,
               int32_t window, int32_t hop, const int32_t* scopes, int32_t K, const std::vector<int64_t>& woff,
               std::vector<unsigned long long>& keys, bool* bad, hipStream_t s) {
  const int32_t C = e->ncols, nb = rank_vote_blocks(C);
  const int64_t nf = fo[nrec], nw = woff[nrec];
  int rc;
  if ((rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_key_bits(e, s)) || (rc = ensure_scope_table(e, s))) return rc;
  // runs of <= kSlideRun windows, launched in groups of <= 256 MB of partial keys (and of the launch
  // grid's second dimension); a run's w0 counts from its group's first window
  const int64_t gwin = std::max<int64_t>(kSlideRun, (int64_t)(256ll << 20) / ((int64_t)sizeof(unsigned long long) * nb * K));
  struct Group { size_t r0, r1; int64_t w0, n; };
  std::vector<SlideRun> runs;
  std::vector<Group> groups;
  for (int32_t r = 0; r < nrec; r++) {
    const int64_t n = woff[r + 1] - woff[r];
    for (int64_t w = 0; w < n; w += kSlideRun) {
      const int32_t len = (int32_t)std::min<int64_t>(kSlideRun, n - w);
      if (groups.empty() || groups.back().n + len > gwin || groups.back().r1 - groups.back().r0 >= 65535)
        groups.push_back(Group{runs.size(), runs.size(), woff[r] + w, 0});
      Group& g = groups.back();
      runs.push_back(SlideRun{fo[r] + w * hop, (int32_t)g.n, len, scopes ? scopes[r] : kScopeAny, 0});
      g.n += len;
      g.r1++;
    }
  }
  int64_t maxw = 0;
  for (const Group& g : groups) maxw = std::max(maxw, g.n);
  const size_t nkeys = (size_t)nw * K;
  HIPCHK(e, e->slide_slots.reserve(sizeof(int16_t) * (size_t)(nf + 1)));
  if ((rc = upload(e, e->slide_runs, runs.data(), sizeof(SlideRun) * runs.size(), s))) return rc;
  HIPCHK(e, e->rank_part.reserve(sizeof(unsigned long long) * (size_t)maxw * nb * K));
  unsigned long long* d_keys;
  int32_t* d_bad;
  if ((rc = vote_keys_begin(e, nkeys, &d_keys, &d_bad, s))) return rc;
  HIPCHK(e, launch_slide_keys(d_q, nf, sc, e->slide_slots.as<int16_t>(), d_bad, s));
  for (const Group& g : groups)
    HIPCHK(e, launch_slide_vote(e->slide_slots.as<int16_t>(), e->slide_runs.as<SlideRun>() + g.r0, (int32_t)(g.r1 - g.r0),
                                (int32_t)g.n, window, hop, e->tc.ranges.active().key_bits.as<uint32_t>(), C,
                                e->tiekey.as<int32_t>(), e->scope_table.as<int32_t>(), K,
                                e->rank_part.as<unsigned long long>(), d_keys + g.w0 * K, s));
  return vote_keys_end(e, nkeys, keys, bad, s);
}

// The general form: the windows' frame values laid end to end in chunks of <= 256 MB, each chunk a
// batch of ranked search's general form (a window in a query's place).
int slide_general(tfp_engine* e, const std::vector<int64_t>& fo, int32_t nrec, const double* d_q, const SearchConsts& sc,
                  int32_t window, int32_t hop, const int32_t* scopes, int32_t K, const std::vector<int64_t>& woff,
                  std::vector<unsigned long long>& keys, hipStream_t s) {
  const int64_t nw = woff[nrec];
  if (e->ncols <= 0 || e->nrows <= 0) return TFP_OK;  // an empty index: no row
  std::vector<int64_t> wsrc((size_t)nw);
  std::vector<int32_t> wscope(scopes ? (size_t)nw : 0);
  for (int32_t r = 0; r < nrec; r++)
    for (int64_t j = woff[r]; j < woff[r + 1]; j++) {
      wsrc[(size_t)j] = fo[r] + (j - woff[r]) * hop;
      if (scopes) wscope[(size_t)j] = scopes[r];
    }
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(nw, (int64_t)(256ll << 20) / (2 * sizeof(double)) / window));
  std::vector<int64_t> qo;
  std::vector<unsigned long long> ck;
  int rc;
  for (int64_t j0 = 0; j0 < nw; j0 += chunk) {
    const int32_t n = (int32_t)std::min<int64_t>(chunk, nw - j0);
    if ((rc = upload(e, e->slide_wsrc, wsrc.data() + j0, sizeof(int64_t) * (size_t)n, s))) return rc;
    HIPCHK(e, e->slide_q.reserve(2 * sizeof(double) * ((size_t)n * window + 1)));
    HIPCHK(e, launch_slide_gather(d_q, e->slide_wsrc.as<int64_t>(), n, window, e->slide_q.as<double>(), s));
    qo.resize((size_t)n + 1);
    for (int32_t i = 0; i <= n; i++) qo[i] = (int64_t)i * window;
    ck.assign((size_t)n * K, 0ull);
    if ((rc = rank_general(e, qo, n, e->slide_q.as<double>(), sc, K, scopes ? wscope.data() + j0 : nullptr, ck, s)))
      return rc;  // (waits for the stream: the chunk's buffers are free again)
    std::copy(ck.begin(), ck.end(), keys.begin() + (size_t)j0 * K);
  }
  return TFP_OK;
}

// Shaped like rank_core. scopes (or nullptr: every clip): scopes[r] restricts recording r's windows.
int slide_core(tfp_engine* e, const std::vector<int64_t>& fo, int32_t nrec, const double* d_q, const tfp_search_params* P,
               int32_t window, int32_t hop, const int32_t* scopes, int32_t K, const std::vector<int64_t>& woff,
               std::vector<unsigned long long>& keys, hipStream_t s) {
  int rc = rebuild(e);  // synchronous on e->stream
  if (rc) return rc;
  const SearchConsts sc = search_consts(P);
  const int64_t nw = woff[nrec];
  keys.assign((size_t)nw * K, 0ull);
  // the vote form runs at the tolerances whose key bitsets hold a live index delta's columns too, so it
  // never needs the delta merged
  if (sc.coefs == 1 && delta_tol_ok(sc.tole)) {
    if (e->ncols <= 0 || e->nrows + e->delta.rows <= 0) return TFP_OK;
    bool bad = false;
    if ((rc = slide_vote(e, fo, nrec, d_q, sc, window, hop, scopes, K, woff, keys, &bad, s))) return rc;
    if (!bad) {
      e->n_slide_vote++;
      e->n_slide_windows += nw;
      return TFP_OK;
    }
  }
  if ((rc = consolidate(e)) || (rc = slide_general(e, fo, nrec, d_q, sc, window, hop, scopes, K, woff, keys, s))) return rc;
  e->n_slide_general++;
  e->n_slide_windows += nw;
  return TFP_OK;
}

// The arguments both sliding forms share; on TFP_OK woff[r] = the first window of recording r of
// the given frame counts and *nwindows = woff[nrec].
int slide_args(tfp_engine* e, const tfp_search_params* P, int32_t window, int32_t hop, int32_t k, int32_t nrec,
               const int32_t* scopes, const std::vector<int64_t>& fo, const void* out, const void* counts,
               int64_t cap_windows, int64_t* nwindows, std::vector<int64_t>& woff) {
  if (nrec < 0 || !nwindows) return fail(e, TFP_E_ARG, "sliding search: bad recording count or NULL nwindows");
  if (window < 1 || hop < 1) return fail(e, TFP_E_ARG, "sliding search: window = %d, hop = %d", window, hop);
  int rc = check_k(e, "sliding search", k);
  if (rc || (rc = check_params(e, "sliding search", P)) || (rc = check_scopes(e, "sliding search", scopes, nrec, "recording")))
    return rc;
  woff = window_offsets(fo, nrec, window, hop);
  *nwindows = woff[nrec];
  if (!windows_fit(woff[nrec], cap_windows))
    return fail(e, TFP_E_CAPACITY, "sliding search: %lld windows, room for %lld", (long long)woff[nrec],
                (long long)cap_windows);
  if (woff[nrec] && (!out || !counts)) return fail(e, TFP_E_ARG, "sliding search: NULL output");
  return TFP_OK;
}

// ---- aligned search (tfp_align.hpp): out[q * K + r] = the alignment of query q with clip
// ids[q * K + r] (-1: none, a zeroed row). The clips' rows are read where they lie in the staging
// arrays (Clip::off under the engine lock), so no index build is needed and a clip of the live
// delta aligns like any other. qo: the queries' relative frame offsets into d_q.
static_assert(sizeof(tfp_alignment) == sizeof(AlignOut), "tfp_align.hpp and the public header agree");

// count: the batch moves tfp_align_stats (catalog neighbours count their own pairs).
int align_core(tfp_engine* e, const std::vector<int64_t>& qo, int32_t nq, const double* d_q, const tfp_search_params* P,
               int32_t K, const int32_t* ids, tfp_alignment* out, hipStream_t s, bool count = true) {
  const int64_t npairs = (int64_t)nq * K;
  memset(out, 0, sizeof(tfp_alignment) * (size_t)npairs);
  std::vector<AlignPair> pairs((size_t)npairs, AlignPair{0, 0, 0, 0});
  int64_t max_bands = 0, named = 0;
  for (int64_t p = 0; p < npairs; p++) {
    const int32_t id = ids[p];
    if (id == -1) continue;
    if (id < 0 || (size_t)id >= e->clips.size() || !e->clips[id].alive)
      return fail(e, TFP_E_NOENT, "aligned search: clip id %d is not in the index", id);
    const Clip& c = e->clips[id];
    const int64_t F = qo[p / K + 1] - qo[p / K], N = c.nrows;
    if (F + N > (int64_t(1) << 31))
      return fail(e, TFP_E_CAPACITY, "aligned search: %lld frames against %lld rows", (long long)F, (long long)N);
    named++;
    if (F <= 0 || N <= 0) continue;
    pairs[p] = AlignPair{c.off, qo[p / K], (int32_t)N, (int32_t)F};
    max_bands = std::max(max_bands, align_bands(F, N));
  }
  if (!max_bands) return TFP_OK;  // nothing to compare: every row stays zero
  const SearchConsts sc = search_consts(P);
  const int64_t nf = qo[nq];
  HIPCHK(e, e->align_boxes.reserve(sizeof(FrameBox) * (nf + 1)));
  HIPCHK(e, launch_prep_boxes(d_q, nf, sc, e->align_boxes.as<FrameBox>(), nullptr, 0, s));
  // pairs in chunks of <= 256 MB of partial keys (and of the launch grid's second dimension)
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({(int64_t(1) << 25) / max_bands, kAlignMaxPairs, npairs}));
  const size_t pbytes = sizeof(AlignPair) * (size_t)npairs, obytes = sizeof(AlignOut) * (size_t)npairs;
  HIPCHK(e, e->align_pairs.reserve(pbytes));
  HIPCHK(e, e->align_part.reserve(sizeof(unsigned long long) * (size_t)(chunk * max_bands)));
  HIPCHK(e, e->align_out.reserve(obytes));
  HIPCHK(e, e->align_pin.reserve(pbytes + obytes));
  char* pin = e->align_pin.as<char>();
  memcpy(pin, pairs.data(), pbytes);
  HIPCHK(e, hipMemcpyAsync(e->align_pairs.p, pin, pbytes, hipMemcpyHostToDevice, s));
  for (int64_t p0 = 0; p0 < npairs; p0 += chunk) {
    const int32_t n = (int32_t)std::min<int64_t>(chunk, npairs - p0);
    HIPCHK(e, launch_align(e->align_pairs.as<AlignPair>() + p0, n, max_bands, e->align_boxes.as<FrameBox>(),
                           e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), sc.coefs == 2,
                           e->align_part.as<unsigned long long>(), e->align_out.as<AlignOut>() + p0, s));
  }
  HIPCHK(e, hipMemcpyAsync(pin + pbytes, e->align_out.p, obytes, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  memcpy(out, pin + pbytes, obytes);
  if (count) {
    e->n_align_batches++;
    e->n_align_pairs += named;
  }
  return TFP_OK;
}

// The candidates' clip ids as align_core takes them: -1 past counts[q].
std::vector<int32_t> candidate_ids(const tfp_candidate* cand, const int32_t* counts, int32_t nq, int32_t K) {
  std::vector<int32_t> ids((size_t)nq * K, -1);
  for (int32_t q = 0; q < nq; q++)
    for (int32_t r = 0; r < counts[q]; r++) ids[(size_t)q * K + r] = cand[(size_t)q * K + r].clip_id;
  return ids;
}

// ---- sliding aligned search (tfp_slide_align.hpp) ----
// The sizes slide_align_core's launches hold, checked against the longest live clip before a call
// writes anything (TFP_E_CAPACITY leaves all but *nwindows untouched): window + N within the 2^31
// align_core allows, and a run's bands within 2^20. A run has at most kSlideAlignRun entries, each
// less than `window` frames after the one before, so it covers fewer than kSlideAlignRun * window
// frames.
int slide_align_limits(tfp_engine* e, int32_t window) {
  int64_t N = 0;
  for (const Clip& c : e->clips)
    if (c.alive) N = std::max(N, c.nrows);
  if (window + N > (int64_t(1) << 31) || align_bands((int64_t)kSlideAlignRun * window, N) > (int64_t(1) << 20))
    return fail(e, TFP_E_CAPACITY, "sliding aligned search: windows of %d frames against clips of up to %lld rows", window,
                (long long)N);
  return TFP_OK;
}

// out[j * K + i] = the alignment of window j of the recordings with clip ids[j * K + i] (-1: none, a
// zeroed row). fo, woff as slide_core takes them; the clips' rows are read where they lie in the
// staging arrays, as align_core reads them. The caller has passed slide_align_limits.
int slide_align_core(tfp_engine* e, const std::vector<int64_t>& fo, int32_t nrec, const double* d_q,
                     const tfp_search_params* P, int32_t window, int32_t hop, int32_t K, const std::vector<int64_t>& woff,
                     const int32_t* ids, tfp_alignment* out, hipStream_t s) {
  const int64_t nw = woff[nrec];
  memset(out, 0, sizeof(tfp_alignment) * (size_t)nw * K);
  // the named entries by (recording, clip), windows ascending
  struct Ent { int32_t rec, clip; int64_t w, slot; };
  std::vector<Ent> ents;
  for (int32_t r = 0; r < nrec; r++)
    for (int64_t j = woff[r]; j < woff[r + 1]; j++)
      for (int32_t i = 0; i < K; i++) {
        const int32_t id = ids[j * K + i];
        if (id == -1) continue;
        if (id < 0 || (size_t)id >= e->clips.size() || !e->clips[id].alive)
          return fail(e, TFP_E_NOENT, "sliding aligned search: clip id %d is not in the index", id);
        if (e->clips[id].nrows > 0) ents.push_back(Ent{r, id, j - woff[r], j * K + i});
      }
  if (ents.empty()) return TFP_OK;  // nothing to compare: every row stays zero
  std::sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) {
    return std::tie(a.rec, a.clip, a.w, a.slot) < std::tie(b.rec, b.clip, b.w, b.slot);
  });
  // direct pairs first, then the slid entries run by run; slot[i]: where work entry i's result goes
  std::vector<AlignPair> direct, slid;
  std::vector<int64_t> dslot, sslot;
  std::vector<std::pair<int64_t, int64_t>> dups;  // (slot, the slot of the same (window, clip) before it)
  std::vector<SlideAlignRun> runs;
  std::vector<int32_t> steps, nbs;
  int64_t bands_d = 0, bands_s = 0;
  const bool slide = 2 * (int64_t)hop < window;
  for (size_t a = 0; a < ents.size();) {
    // one run: successive needed windows of one (recording, clip) that share a frame
    std::vector<size_t> run(1, a);
    size_t b = a + 1;
    for (; b < ents.size() && ents[b].rec == ents[a].rec && ents[b].clip == ents[a].clip; b++) {
      const Ent& prev = ents[run.back()];
      if (ents[b].w == prev.w) {
        dups.emplace_back(ents[b].slot, prev.slot);
        continue;
      }
      if ((ents[b].w - prev.w) * hop >= window) break;
      run.push_back(b);
    }
    const Clip& c = e->clips[ents[a].clip];
    const int64_t N = c.nrows, f0 = fo[ents[a].rec], n = (int64_t)run.size();
    if (n == 1 || !slide) {
      for (const size_t i : run) {
        direct.push_back(AlignPair{c.off, f0 + ents[i].w * hop, (int32_t)N, window});
        dslot.push_back(ents[i].slot);
      }
      bands_d = std::max(bands_d, align_bands(window, N));
    } else {
      const int64_t pieces = (n + kSlideAlignRun - 1) / kSlideAlignRun;  // near-equal, each of >= 2 entries
      for (int64_t p = 0; p < pieces; p++) {
        const int64_t i0 = p * n / pieces, i1 = (p + 1) * n / pieces;
        const int64_t w0 = ents[run[i0]].w, nsteps = ents[run[i1 - 1]].w - w0 + 1;
        const int64_t nb = slide_align_bands(nsteps, window, hop, N);
        runs.push_back(SlideAlignRun{c.off, f0 + w0 * hop, (int32_t)N, (int32_t)nsteps, (int32_t)steps.size(), 0});
        steps.resize(steps.size() + (size_t)nsteps, -1);
        for (int64_t i = i0; i < i1; i++) {
          const Ent& en = ents[run[i]];
          steps[(size_t)runs.back().e0 + (size_t)(en.w - w0)] = (int32_t)slid.size();
          slid.push_back(AlignPair{c.off, f0 + en.w * hop, (int32_t)N, window});
          sslot.push_back(en.slot);
          nbs.push_back((int32_t)nb);
        }
        bands_s = std::max(bands_s, nb);
      }
    }
    a = b;
  }
  const SearchConsts sc = search_consts(P);
  const int64_t nf = fo[nrec], nd = (int64_t)direct.size(), ns = (int64_t)slid.size(), np = nd + ns;
  HIPCHK(e, e->align_boxes.reserve(sizeof(FrameBox) * (nf + 1)));
  HIPCHK(e, launch_prep_boxes(d_q, nf, sc, e->align_boxes.as<FrameBox>(), nullptr, 0, s));  // once per recording frame
  // in chunks of <= 256 MB of partial keys (and of the launch grid's second dimension), as align_core
  const int64_t chunk_d = nd ? std::max<int64_t>(1, std::min<int64_t>({(int64_t(1) << 25) / bands_d, kAlignMaxPairs, nd})) : 0;
  const int64_t chunk_s = ns ? std::max<int64_t>(kSlideAlignRun, (int64_t(1) << 25) / bands_s) : 0;
  const size_t pbytes = sizeof(AlignPair) * (size_t)np, obytes = sizeof(AlignOut) * (size_t)np;
  HIPCHK(e, e->align_pairs.reserve(pbytes));
  HIPCHK(e, e->align_part.reserve(sizeof(unsigned long long) *
                                  (size_t)std::max(chunk_d * bands_d, std::min(chunk_s, ns) * bands_s)));
  HIPCHK(e, e->align_out.reserve(obytes));
  HIPCHK(e, e->align_pin.reserve(pbytes + obytes));
  char* pin = e->align_pin.as<char>();
  memcpy(pin, direct.data(), sizeof(AlignPair) * (size_t)nd);
  memcpy(pin + sizeof(AlignPair) * (size_t)nd, slid.data(), sizeof(AlignPair) * (size_t)ns);
  HIPCHK(e, hipMemcpyAsync(e->align_pairs.p, pin, pbytes, hipMemcpyHostToDevice, s));
  const FrameBox* boxes = e->align_boxes.as<FrameBox>();
  unsigned long long* d_part = e->align_part.as<unsigned long long>();
  for (int64_t p0 = 0; p0 < nd; p0 += chunk_d) {
    const int32_t n = (int32_t)std::min<int64_t>(chunk_d, nd - p0);
    HIPCHK(e, launch_align(e->align_pairs.as<AlignPair>() + p0, n, bands_d, boxes, e->st_m1.as<int32_t>(),
                           e->st_m2.as<int32_t>(), sc.coefs == 2, d_part, e->align_out.as<AlignOut>() + p0, s));
  }
  if (ns) {
    int rc;
    if ((rc = upload(e, e->sa_runs, runs.data(), sizeof(SlideAlignRun) * runs.size(), s)) ||
        (rc = upload(e, e->sa_steps, steps.data(), sizeof(int32_t) * steps.size(), s)) ||
        (rc = upload(e, e->sa_nb, nbs.data(), sizeof(int32_t) * nbs.size(), s)))
      return rc;
    // whole runs per launch: a run's entries are consecutive, steps[run.e0] onwards names them
    for (size_t r0 = 0; r0 < runs.size();) {
      const int64_t ent0 = steps[(size_t)runs[r0].e0];  // (a run's first window is needed)
      int64_t ent1 = ent0;
      size_t r1 = r0;
      for (; r1 < runs.size() && r1 - r0 < (size_t)kSlideAlignMaxRuns; r1++) {
        const int64_t last = steps[(size_t)runs[r1].e0 + (size_t)runs[r1].nsteps - 1] + 1;  // (and its last)
        if (r1 > r0 && last - ent0 > chunk_s) break;
        ent1 = last;
      }
      HIPCHK(e, launch_slide_align(e->sa_runs.as<SlideAlignRun>() + r0, (int32_t)(r1 - r0), e->sa_steps.as<int32_t>(),
                                   (int32_t)ent0, (int32_t)(ent1 - ent0), e->align_pairs.as<AlignPair>() + nd + ent0,
                                   e->sa_nb.as<int32_t>() + ent0, bands_s, window, hop, boxes, e->st_m1.as<int32_t>(),
                                   e->st_m2.as<int32_t>(), sc.coefs == 2, d_part, e->align_out.as<AlignOut>() + nd + ent0,
                                   s));
      r0 = r1;
    }
  }
  HIPCHK(e, hipMemcpyAsync(pin + pbytes, e->align_out.p, obytes, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  const tfp_alignment* res = reinterpret_cast<const tfp_alignment*>(pin + pbytes);
  for (int64_t i = 0; i < nd; i++) out[dslot[(size_t)i]] = res[i];
  for (int64_t i = 0; i < ns; i++) out[sslot[(size_t)i]] = res[nd + i];
  for (const auto& d : dups) out[d.first] = out[d.second];  // (in order: a copy's source is filled before it)
  e->n_sa_batches++;
  e->n_sa_slid += ns;
  e->n_sa_direct += nd;
  return TFP_OK;
}

// ---- diagonal trace and occurrence search (tfp_trace.hpp, tfp_occur.hpp) ----
static_assert(sizeof(tfp_trace) == sizeof(TraceOut), "tfp_occur.hpp and the public header agree");

// out[i] = the trace of reqs[i] over recording reqs[i].recording of fo[0 .. nrec] (checked by the
// caller to lie in range). A clip id of -1 gives a zeroed row, any other id that names no live clip
// TFP_E_NOENT before anything is written; a request that covers no frame is answered here. The rest
// go to the kernel in one launch, after boxes() has put the recordings' frame boxes into
// e->align_boxes (called only then). The clips' rows are read where they lie in the staging arrays,
// as align_core reads them.
template <class Boxes>
int trace_core(tfp_engine* e, const std::vector<int64_t>& fo, const tfp_trace_req* reqs, int64_t n, int32_t max_gap,
               const tfp_search_params* P, Boxes boxes, tfp_trace* out, hipStream_t s) {
  std::vector<TraceReq> work;
  std::vector<int64_t> slot;
  for (int64_t i = 0; i < n; i++) {
    const int32_t id = reqs[i].clip_id;
    if (id == -1) continue;
    if (id < 0 || (size_t)id >= e->clips.size() || !e->clips[id].alive)
      return fail(e, TFP_E_NOENT, "trace: clip id %d is not in the index", id);
  }
  if (n > INT32_MAX) return fail(e, TFP_E_CAPACITY, "trace: %lld requests", (long long)n);
  for (int64_t i = 0; i < n; i++) {
    out[i] = tfp_trace{0, 0, 0, 0, 0, 0};
    if (reqs[i].clip_id == -1) continue;
    const Clip& c = e->clips[reqs[i].clip_id];
    const int64_t f0 = fo[reqs[i].recording], F = fo[reqs[i].recording + 1] - f0;
    int64_t lo, hi;
    trace_span(F, c.nrows, reqs[i].start, &lo, &hi);
    if (hi <= lo) continue;
    out[i].overlap = (int32_t)(hi - lo);
    work.push_back(TraceReq{c.off, f0, (int32_t)c.nrows, (int32_t)F, reqs[i].start, 0});
    slot.push_back(i);
  }
  if (work.empty()) return TFP_OK;  // nothing to trace: nothing is launched
  int rc = boxes();
  if (rc) return rc;
  const size_t obytes = sizeof(TraceOut) * work.size();
  if ((rc = upload(e, e->trace_reqs, work.data(), sizeof(TraceReq) * work.size(), s))) return rc;
  HIPCHK(e, e->trace_out.reserve(obytes));
  HIPCHK(e, launch_trace(e->trace_reqs.as<TraceReq>(), (int32_t)work.size(), max_gap, e->align_boxes.as<FrameBox>(),
                         e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), search_consts(P).coefs == 2,
                         e->trace_out.as<TraceOut>(), s));
  std::vector<tfp_trace> res(work.size());
  HIPCHK(e, hipMemcpyAsync(res.data(), e->trace_out.p, obytes, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  for (size_t i = 0; i < work.size(); i++) out[slot[i]] = res[i];
  e->n_trace_batches++;
  e->n_traces += (int64_t)work.size();
  return TFP_OK;
}

// The occurrences of a sliding aligned search's rows (cand, counts, align: nw windows of K rows,
// the recordings' boxes still in e->align_boxes): tfp_occur.hpp's steps 2-5.
int occur_core(tfp_engine* e, const std::vector<int64_t>& fo, int32_t nrec, const tfp_search_params* P, int32_t window,
               int32_t hop, int32_t K, const tfp_candidate* cand, const int32_t* counts, const tfp_alignment* align,
               int32_t max_gap, int32_t min_hits, tfp_occurrence* out, int64_t cap, int64_t* nocc, hipStream_t s) {
  std::vector<OccurRow> rows;
  int64_t j = 0;
  for (int32_t r = 0; r < nrec; r++) {
    const int64_t nw = plan_windows(fo[r + 1] - fo[r], window, hop);
    for (int64_t w = 0; w < nw; w++, j++)
      for (int32_t i = 0; i < counts[j]; i++) rows.push_back(OccurRow{r, cand[j * K + i].clip_id, w, align[j * K + i].offset});
  }
  const std::vector<OccurCand> cands = occur_candidates(rows, hop);
  std::vector<tfp_trace_req> reqs(cands.size());
  for (size_t i = 0; i < cands.size(); i++) reqs[i] = tfp_trace_req{cands[i].rec, cands[i].clip, cands[i].s, 0};
  std::vector<tfp_trace> tr(cands.size());
  const int rc = trace_core(e, fo, reqs.data(), (int64_t)reqs.size(), max_gap, P, [] { return TFP_OK; }, tr.data(), s);
  if (rc) return rc;
  const std::vector<int64_t> kept = occur_select(cands, reinterpret_cast<const TraceOut*>(tr.data()), min_hits,
                                                 [&](int32_t c) { return e->clips[c].uuid.c_str(); });
  *nocc = (int64_t)kept.size();
  if (*nocc > cap)
    return fail(e, TFP_E_CAPACITY, "occurrence search: %lld occurrences, room for %lld", (long long)*nocc, (long long)cap);
  if (*nocc && !out) return fail(e, TFP_E_ARG, "occurrence search: NULL output");
  for (size_t i = 0; i < kept.size(); i++) {
    const OccurCand& c = cands[(size_t)kept[i]];
    const tfp_trace& t = tr[(size_t)kept[i]];
    tfp_occurrence& o = out[i];
    memset(&o, 0, sizeof o);
    o.recording = c.rec;
    o.clip_id = c.clip;
    o.clip_start_frame = c.s;
    o.first_frame = t.seg_first;
    o.last_frame = t.seg_last;
    o.hits = t.seg_hits;
    o.diagonal_hits = t.hits;
    o.overlap = t.overlap;
    o.windows = c.windows;
    snprintf(o.uuid, sizeof o.uuid, "%s", e->clips[c.clip].uuid.c_str());
  }
  return TFP_OK;
}

}  // namespace

// =========================================================================================
extern "C" {

int tfp_abi_version(void) { return TFP_ABI_VERSION; }

int tfp_device_count(int32_t* count) {
  int n = 0;
  if (!count) return TFP_E_ARG;
  *count = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return TFP_E_NODEV;
  *count = n;
  return TFP_OK;
}

static_assert(kPlanHop == TFP_HOP, "tfp_query_plan.hpp and the public header agree");
int64_t tfp_frame_count(int64_t n) { return plan_frames(n); }

int tfp_engine_create(int32_t device, tfp_engine** out) {
  if (!out) return TFP_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return TFP_E_NODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return TFP_E_NODEV;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return TFP_E_NODEV;  // code objects are gfx950-only
  if (hipSetDevice(device) != hipSuccess) return TFP_E_HIP;
  tfp_engine* e = new tfp_engine();
  e->device = device;
  if (fp_launch_config(device, &e->fpcfg) != hipSuccess) {
    delete e;
    return TFP_E_HIP;
  }
  // test knobs (tfp::knob: only under TFP_TEST_KNOBS)
  if (const char* v = tfp::knob("TFP_VOTE_CLASS_MAX")) e->class_ku_max = (int32_t)atoi(v);
  e->dbg_vote = tfp::knob("TFP_DEBUG_VOTE") != nullptr;
  e->dbg_index = tfp::knob("TFP_DEBUG_INDEX") != nullptr;
  if (const char* v = tfp::knob("TFP_TEST_FAIL_COMPACT")) e->fail_compact = (int32_t)atoi(v);
  if (const char* v = tfp::knob("TFP_TEST_FAIL_CELLS")) e->fail_cells = atoll(v);
  if (const char* v = tfp::knob("TFP_TEST_FAIL_DELTA_CELLS")) e->fail_delta_cells = atoll(v);
  if (const char* v = tfp::knob("TFP_TEST_FAIL_QUERY_SAMPLES")) e->fail_query_len = atoll(v);
  if (const char* v = tfp::knob("TFP_KEYBITS_WIN")) e->kb_win = atoi(v);
  if (const char* v = tfp::knob("TFP_KEYBITS_DIRECT")) e->kb_direct = atoll(v);
  e->force_full = tfp::knob("TFP_INDEX_FULL") != nullptr;
  if (const char* v = tfp::knob("TFP_WIDE_MIN_TOL")) e->wide_min_tol = atof(v);
  e->wide.points_only = tfp::knob("TFP_WIDE_POINTS") != nullptr;
  e->wide.ch128 = tfp::knob("TFP_WIDE_CH128") != nullptr;
  e->wide.unpacked = tfp::knob("TFP_WIDE_UNPACKED") != nullptr;
  e->wide.libsort = tfp::knob("TFP_WIDE_LIBSORT") != nullptr;
  e->wide.debug_bins = tfp::knob("TFP_DEBUG_BINS") != nullptr;
  if (const char* v = tfp::knob("TFP_DELTA_WIDE")) e->delta.wide = atoi(v) != 0;
  // operational switches (documented: tiresias_fp.h), read as plain environment variables
  if (const char* v = tfp::op_env("TFP_COALESCE")) e->coalesce = atoi(v) != 0;
  if (const char* v = tfp::op_env("TFP_INDEX_DELTA")) e->delta.use = atoi(v) != 0;
  // test form: the delta even below delta_min_cols main columns (small test DBs)
  if (const char* v = tfp::knob("TFP_INDEX_DELTA"))
    if (atoi(v) != 0) e->delta.min_cols = 0;
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
    delete e;
    return TFP_E_HIP;
  }
  *out = e;
  return TFP_OK;
}

void tfp_engine_destroy(tfp_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  (void)hipStreamSynchronize(e->stream);
  hipStream_t s = e->stream;
  delete e;
  (void)hipStreamDestroy(s);
}

__attribute__((visibility("hidden"))) const char* tfp_ingest_last_error();  // tfp_wav.cpp: engine-less errors of this thread
const char* tfp_engine_last_error(const tfp_engine* e) {
  return e ? const_cast<tfp_engine*>(e)->err.read(e) : tfp_ingest_last_error();
}

int tfp_host_alloc(size_t bytes, void** out) {
  if (!bytes || !out) return TFP_E_ARG;
  *out = nullptr;
  void* p = nullptr;
  // portable: pinned for every device; each engine maps it on its own device (engine_host_ptr)
  if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess)
    return TFP_E_NOMEM;
  HostAllocs& h = host_allocs();
  std::lock_guard<std::mutex> lk(h.mu);
  h.m[reinterpret_cast<uintptr_t>(p)] = {bytes, h.next_gen++};
  *out = p;
  return TFP_OK;
}

void tfp_host_free(void* p) {
  if (!p) return;
  HostAllocs& h = host_allocs();
  {
    std::lock_guard<std::mutex> lk(h.mu);
    if (!h.m.erase(reinterpret_cast<uintptr_t>(p))) return;  // not ours
  }
  (void)hipHostFree(p);
}

namespace {
// law >= 0: pcm holds G.711 codes of that law (one byte per sample) instead of int16.
int fingerprint_batch_impl(tfp_engine* e, const void* pcm, bool f32, const int64_t* offsets, int32_t nclips,
                           int32_t sr, tfp_frame* out, int64_t cap, int64_t* nframes, int32_t law = -1) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!offsets || nclips < 0 || !nframes || (!pcm && nclips && offsets[nclips] > offsets[0]))
    return fail(e, TFP_E_ARG, "bad arguments");
  if (int rc = check_monotone(e, offsets, nclips, true)) return rc;
  const int64_t need = sample_frame_offsets(offsets, nclips)[nclips];
  *nframes = need;
  if (need > 0 && (!out || cap < need)) return fail(e, TFP_E_CAPACITY, "need %lld frames", (long long)need);
  if (need == 0) return TFP_OK;
  HIPCHK(e, hipSetDevice(e->device));
  int64_t nf;
  std::vector<int64_t> foff;
  std::vector<const void*> ptrs;
  std::vector<int64_t> lens;
  split_offsets(pcm, law >= 0 ? sizeof(uint8_t) : f32 ? sizeof(float) : sizeof(int16_t), offsets, nclips, &ptrs, &lens);
  const G711Src g{static_cast<const uint8_t*>(ptrs[0]), law};
  int rc = fingerprint_host(e, ptrs.data(), lens.data(), f32, nclips, sr, &nf, &foff, true, law >= 0 ? &g : nullptr);
  if (rc) return rc;
  return copy_frames_out(e, nf, foff, out);
}
}  // namespace

int tfp_fingerprint_g711_batch(tfp_engine* e, const uint8_t* codes, const int64_t* offsets, int32_t nclips, int32_t law,
                               int32_t sr, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!e) return TFP_E_ARG;
  if (!g711_law_ok(law)) return fail(e, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  return fingerprint_batch_impl(e, codes, false, offsets, nclips, sr, out, cap, nframes, law);
}

int tfp_g711_stats(tfp_engine* e, int64_t* expand_launches, int64_t* stream_launches, int64_t* codes) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (expand_launches) *expand_launches = e->n_g711_expand;
  if (stream_launches) *stream_launches = e->n_g711_stream;
  if (codes) *codes = e->n_g711_codes;
  return TFP_OK;
}

int tfp_fingerprint_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nclips, int32_t sr,
                          tfp_frame* out, int64_t cap, int64_t* nframes) {
  return fingerprint_batch_impl(e, pcm, false, offsets, nclips, sr, out, cap, nframes);
}

int tfp_fingerprint_f32_batch(tfp_engine* e, const float* x, const int64_t* offsets, int32_t nclips, int32_t sr,
                              tfp_frame* out, int64_t cap, int64_t* nframes) {
  return fingerprint_batch_impl(e, x, true, offsets, nclips, sr, out, cap, nframes);
}

int tfp_fingerprint_pcm(tfp_engine* e, const int16_t* pcm, int64_t n, int32_t sr, tfp_frame* out, int64_t cap,
                        int64_t* nframes) {
  if (n < 0) return TFP_E_ARG;
  int64_t off[2] = {0, n};
  return tfp_fingerprint_batch(e, pcm, off, 1, sr, out, cap, nframes);
}

int tfp_plan_create(tfp_engine* e, const int64_t* offsets, int32_t nclips, int32_t sr, tfp_plan** out) {
  if (!e || !offsets || nclips < 0 || !out) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  const DspTables* T;
  bool fx = false;
  int rc = ensure_tables(e, sr, &T, &fx);
  if (rc) return rc;
  tfp_plan* p = new tfp_plan();
  p->eng = e;
  p->nclips = nclips;
  p->sample_rate = sr;
  for (int32_t c = 0; c < nclips; c++)
    if (offsets[c + 1] - offsets[c] >= kDirectMaxSamples) p->long_clip = true;
  p->tile_frames = fp_tile_frames(e->fpcfg, fx && !p->long_clip, false, false);
  layout(offsets, nclips, p->soff, p->foff, p->toff, &p->tclip, p->tile_frames);
  p->nsamples = p->soff[nclips];
  p->nframes = p->foff[nclips];
  p->ntiles = p->toff[nclips];
  if ((rc = upload(e, p->d_soff, p->soff.data(), sizeof(int64_t) * p->soff.size())) ||
      (rc = upload(e, p->d_foff, p->foff.data(), sizeof(int64_t) * p->foff.size())) ||
      (rc = upload(e, p->d_toff, p->toff.data(), sizeof(int32_t) * p->toff.size())) ||
      (rc = upload(e, p->d_tclip, p->tclip.data(), sizeof(int32_t) * p->tclip.size())) ||
      (rc = upload(e, p->d_qoff, p->foff.data(), sizeof(int64_t) * p->foff.size()))) {
    delete p;
    return rc;
  }
  if (hipStreamSynchronize(e->stream) != hipSuccess) { delete p; return fail(e, TFP_E_HIP, "sync"); }
  *out = p;
  return TFP_OK;
}

void tfp_plan_destroy(tfp_plan* p) { delete p; }
int64_t tfp_plan_frames(const tfp_plan* p) { return p ? p->nframes : -1; }

int tfp_fingerprint_device(tfp_engine* e, const tfp_plan* p, const int16_t* d_pcm, int32_t* d_micro, double* d_db,
                           void* stream) {
  if (!e || !p || !d_micro || (!d_pcm && p->nsamples)) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  NullStreamOrder order(e, stream);
  if (!order.ok()) return fail(e, TFP_E_HIP, "ordering after the null stream failed");
  const DspTables* T;
  bool fx = false;
  int rc = ensure_tables(e, p->sample_rate, &T, &fx);
  if (rc) return rc;
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  HIPCHK(e, launch_fingerprint(e->fpcfg, T, fx && !p->long_clip, p->tile_frames, d_pcm, p->d_soff.as<int64_t>(), p->d_soff.as<int64_t>() + 1,
                               p->d_foff.as<int64_t>(), p->d_toff.as<int32_t>(),
                               p->d_tclip.as<int32_t>(), p->ntiles, p->nframes, d_micro, d_db, s, e->logfix, &e->fpstats));
  return TFP_OK;
}

int tfp_index_add(tfp_engine* e, const char* uuid, const int32_t* m1, const int32_t* m2, int32_t nframes,
                  int32_t* clip_id) {
  if (!e || nframes < 0 || (nframes && (!m1 || !m2))) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int32_t id;
  if (!uuid || !*uuid || strlen(uuid) >= 64) return fail(e, TFP_E_ARG, "bad uuid");
  if (e->by_uuid.count(uuid)) return fail(e, TFP_E_EXISTS, "uuid %s already indexed", uuid);
  int rc = stage_reserve(e, nframes);
  if (rc) return rc;
  // the rows go in past the staged ones first; the clip is registered only once they are there
  // (a failed copy leaves the index as it was)
  const int64_t o = e->n_staged;
  if (nframes) {
    std::vector<int32_t> cl(nframes, (int32_t)e->clips.size());
    HIPCHK(e, hipMemcpyAsync(e->st_m1.as<int32_t>() + o, m1, sizeof(int32_t) * nframes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->st_m2.as<int32_t>() + o, m2, sizeof(int32_t) * nframes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->st_clip.as<int32_t>() + o, cl.data(), sizeof(int32_t) * nframes, hipMemcpyHostToDevice,
                             e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  if ((rc = new_clip(e, uuid, nframes, o, &id))) return rc;
  e->n_staged += nframes;
  if (clip_id) *clip_id = id;
  return TFP_OK;
}

// de-interleave (m1, m2) pairs + clip ids into staging
__global__ void stage_from_micro_kernel(const int32_t* micro, int64_t nf, const int64_t* foff, int32_t nclips,
                                        int32_t clip0, int32_t* m1, int32_t* m2, int32_t* clip) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nf; g += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = nclips;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (foff[mid] <= g) lo = mid; else hi = mid;
    }
    m1[g] = micro[2 * g];
    m2[g] = micro[2 * g + 1];
    clip[g] = clip0 + lo;
  }
}

int tfp_index_add_device(tfp_engine* e, int32_t nclips, const char* const* uuids, const int64_t* frame_offsets,
                         const int32_t* d_micro, void* stream) {
  if (!e || nclips < 0 || !uuids || !frame_offsets || (!d_micro && frame_offsets[nclips] > frame_offsets[0]))
    return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  NullStreamOrder order(e, stream);
  if (!order.ok()) return fail(e, TFP_E_HIP, "ordering after the null stream failed");
  std::unordered_map<std::string, int> seen;
  for (int32_t c = 0; c < nclips; c++) {
    if (!uuids[c] || !*uuids[c] || strlen(uuids[c]) >= 64) return fail(e, TFP_E_ARG, "bad uuid %d", c);
    if (frame_offsets[c + 1] < frame_offsets[c]) return fail(e, TFP_E_ARG, "frame_offsets not monotone at %d", c);
    if (e->by_uuid.count(uuids[c]) || !seen.emplace(uuids[c], c).second)
      return fail(e, TFP_E_EXISTS, "uuid %s already indexed", uuids[c]);
  }
  const int64_t nf = frame_offsets[nclips] - frame_offsets[0];
  int rc = stage_reserve(e, nf);
  if (rc) return rc;
  const int32_t clip0 = (int32_t)e->clips.size();
  // rows first, clips registered once they are staged (a failure leaves the index as it was)
  if (nf) {
    std::vector<int64_t> fo(frame_offsets, frame_offsets + nclips + 1);
    for (auto& v : fo) v -= frame_offsets[0];
    if ((rc = upload(e, e->foff, fo.data(), sizeof(int64_t) * fo.size()))) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    if (s != e->stream) HIPCHK(e, hipStreamSynchronize(e->stream));
    const int64_t o = e->n_staged;
    hipLaunchKernelGGL(stage_from_micro_kernel, dim3(2048), dim3(256), 0, s, d_micro + 2 * frame_offsets[0], nf,
                       e->foff.as<int64_t>(), nclips, clip0, e->st_m1.as<int32_t>() + o, e->st_m2.as<int32_t>() + o,
                       e->st_clip.as<int32_t>() + o);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(s));
  }
  for (int32_t c = 0; c < nclips; c++) {
    int32_t id;
    if ((rc = new_clip(e, uuids[c], frame_offsets[c + 1] - frame_offsets[c],
                       e->n_staged + frame_offsets[c] - frame_offsets[0], &id)))
      return rc;  // (cannot fail: checked above)
  }
  e->n_staged += nf;
  return TFP_OK;
}

// TFP_TEST_FAIL_ADD_BATCH=n (tests): the n-th tfp_index_add_batch call of the process since the
// variable took its value fails as a device error would, before it changes anything.
static bool injected_add_batch_failure() {
  static std::mutex mu;
  static std::string val;
  static int64_t calls = 0;
  const char* v = tfp::knob("TFP_TEST_FAIL_ADD_BATCH");
  std::lock_guard<std::mutex> lk(mu);
  if (!v) return false;
  if (val != v) {
    val = v;
    calls = 0;
  }
  return ++calls == atoll(v);
}

int tfp_index_add_batch(tfp_engine* e, int32_t nclips, const char* const* uuids, const int64_t* frame_offsets,
                        const int32_t* m1, const int32_t* m2) {
  if (!e || nclips < 0 || !uuids || !frame_offsets) return TFP_E_ARG;
  const int64_t nf = frame_offsets[nclips] - frame_offsets[0];
  if (nf < 0 || (nf && (!m1 || !m2))) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  std::unordered_map<std::string, int> seen;
  for (int32_t c = 0; c < nclips; c++) {
    if (!uuids[c] || !*uuids[c] || strlen(uuids[c]) >= 64) return fail(e, TFP_E_ARG, "bad uuid %d", c);
    if (frame_offsets[c + 1] < frame_offsets[c]) return fail(e, TFP_E_ARG, "frame_offsets not monotone at %d", c);
    if (e->by_uuid.count(uuids[c]) || !seen.emplace(uuids[c], c).second)
      return fail(e, TFP_E_EXISTS, "uuid %s already indexed", uuids[c]);
  }
  if (injected_add_batch_failure()) return fail(e, TFP_E_HIP, "tfp_index_add_batch: injected device failure");
  int rc = stage_reserve(e, nf);
  if (rc) return rc;
  // All-or-nothing: the rows go in past the staged ones, and the clips are registered only once
  // every copy has succeeded.
  const int32_t clip0 = (int32_t)e->clips.size();
  if (nf) {
    std::vector<int32_t> cl(nf);
    for (int32_t c = 0; c < nclips; c++)
      std::fill(cl.begin() + (frame_offsets[c] - frame_offsets[0]), cl.begin() + (frame_offsets[c + 1] - frame_offsets[0]),
                clip0 + c);
    const int64_t o = e->n_staged;
    const int32_t* s1 = m1 + frame_offsets[0];
    const int32_t* s2 = m2 + frame_offsets[0];
    HIPCHK(e, hipMemcpyAsync(e->st_m1.as<int32_t>() + o, s1, sizeof(int32_t) * nf, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->st_m2.as<int32_t>() + o, s2, sizeof(int32_t) * nf, hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->st_clip.as<int32_t>() + o, cl.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice,
                             e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  for (int32_t c = 0; c < nclips; c++) {
    int32_t id;
    const int64_t b = frame_offsets[c] - frame_offsets[0], n = frame_offsets[c + 1] - frame_offsets[c];
    if ((rc = new_clip(e, uuids[c], n, e->n_staged + b, &id))) return rc;  // (cannot fail: checked above)
  }
  e->n_staged += nf;
  return TFP_OK;
}

int tfp_index_rows(tfp_engine* e, const char* uuid, int32_t* m1, int32_t* m2, int64_t cap, int64_t* nframes) {
  if (!e || !uuid || cap < 0 || (cap && (!m1 || !m2))) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  auto it = e->by_uuid.find(uuid);
  if (it == e->by_uuid.end()) return fail(e, TFP_E_NOENT, "uuid %s not indexed", uuid);
  const Clip& c = e->clips[it->second];
  if (nframes) *nframes = c.nrows;
  if (cap < c.nrows) return fail(e, TFP_E_CAPACITY, "need %lld rows", (long long)c.nrows);
  if (c.nrows) {
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(m1, e->st_m1.as<int32_t>() + c.off, sizeof(int32_t) * c.nrows, hipMemcpyDeviceToHost,
                             e->stream));
    HIPCHK(e, hipMemcpyAsync(m2, e->st_m2.as<int32_t>() + c.off, sizeof(int32_t) * c.nrows, hipMemcpyDeviceToHost,
                             e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
  }
  return TFP_OK;
}

int tfp_index_remove(tfp_engine* e, const char* uuid) {
  if (!e || !uuid) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  auto it = e->by_uuid.find(uuid);
  if (it == e->by_uuid.end()) return fail(e, TFP_E_NOENT, "uuid %s not indexed", uuid);
  Clip& c = e->clips[it->second];
  c.alive = false;
  e->live_rows -= c.nrows;
  e->removed_built |= (size_t)it->second < e->built_clips;
  e->by_uuid.erase(it);
  e->dirty = true;
  return TFP_OK;
}

int tfp_index_clear(tfp_engine* e) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  e->clips.clear();
  e->by_uuid.clear();
  e->tiebreak_override.clear();
  e->n_staged = 0;
  e->built = false;
  e->built_clips = 0;
  e->built_staged = 0;
  e->removed_built = false;
  e->live_rows = 0;
  e->col_clip.clear();
  e->delta.reset(0);
  e->dirty = true;
  return TFP_OK;
}

int tfp_index_stats(tfp_engine* e, int64_t* nrows, int32_t* nclips) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  int64_t r = 0;
  int32_t c = 0;
  for (const auto& cl : e->clips)
    if (cl.alive) { r += cl.nrows; c++; }
  if (nrows) *nrows = r;
  if (nclips) *nclips = c;
  return TFP_OK;
}

int tfp_index_commit(tfp_engine* e) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  return rebuild(e);
}

int tfp_index_build_stats(tfp_engine* e, int64_t* full_builds, int64_t* merges) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (full_builds) *full_builds = e->n_full_builds;
  if (merges) *merges = e->n_merges;
  return TFP_OK;
}

int tfp_index_delta_stats(tfp_engine* e, int64_t* delta_updates, int32_t* delta_clips) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (delta_updates) *delta_updates = e->delta.n_updates;
  if (delta_clips) *delta_clips = (int32_t)e->delta.clip.size();
  return TFP_OK;
}

int tfp_index_set_tiebreak(tfp_engine* e, const int32_t* keys, int32_t n) {
  if (!e || n < 0 || (n && !keys)) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  e->tiebreak_override.assign(keys, keys + n);
  e->ovr_main_stale = true;
  e->dirty = true;
  return TFP_OK;
}

int tfp_index_update_tiebreak(tfp_engine* e, int32_t first_clip_id, const int32_t* keys, int32_t n) {
  if (!e || first_clip_id < 0 || n < 0 || (n && !keys)) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if ((size_t)first_clip_id > e->tiebreak_override.size() || (e->tiebreak_override.empty() && first_clip_id > 0))
    return fail(e, TFP_E_ARG, "tie-break keys from clip id %d: the keys before it were never set", first_clip_id);
  if ((size_t)first_clip_id + (size_t)n > e->tiebreak_override.size()) e->tiebreak_override.resize((size_t)first_clip_id + n);
  std::copy(keys, keys + n, e->tiebreak_override.begin() + first_clip_id);
  // new keys for clips of the last build change the main columns' keys (a full refresh at the next
  // update); keys of clips added since concern the delta or the next merge only
  if ((size_t)first_clip_id < e->built_clips && n > 0) e->ovr_main_stale = true;
  e->dirty = true;
  return TFP_OK;
}

int tfp_index_uuid_of_key(tfp_engine* e, int32_t key, char* uuid, int32_t len) {
  if (!e || !uuid || len <= 0) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const int32_t clip = clip_of_col(e, col_of_key(e, key));
  if (clip < 0) return fail(e, TFP_E_NOENT, "no clip with key %d", key);
  snprintf(uuid, len, "%s", e->clips[clip].uuid.c_str());
  return TFP_OK;
}

int tfp_search_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                     const tfp_search_params* P, tfp_result* out) {
  if (!e || !qoff || nq < 0 || !out) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const int64_t nf = nq ? qoff[nq] - qoff[0] : 0;
  if (nf && !frames) return fail(e, TFP_E_ARG, "frames is NULL");
  std::vector<unsigned long long> keys(nq, 0ull);
  if (valid_params(P) && nq) {  // coefs out of range: NULL for every query (fp_handler.c:247-250)
    HIPCHK(e, hipSetDevice(e->device));
    int rc = upload_frames(e, frames, qoff, nq);
    if (rc) return rc;
    if ((rc = search_core(e, qoff, nq, e->q.as<double>(), P, keys, nullptr, e->stream))) return rc;
  }
  fill_results(e, keys, qoff, nq, out);
  return TFP_OK;
}

int tfp_search(tfp_engine* e, const tfp_frame* frames, int32_t nframes, const tfp_search_params* P, tfp_result* out) {
  if (nframes < 0) return TFP_E_ARG;
  int64_t qoff[2] = {0, nframes};
  return tfp_search_batch(e, frames, qoff, 1, P, out);
}

// ---- ranked search: the result query's first k rows (fp_handler.c:367-374) ----------------
static_assert(kRankMax == TFP_RANK_MAX, "tfp_rank.hpp and the public header agree");

namespace {
// Where a batch's frame values come from: the caller's frames, or int16 samples fingerprinted here.
// off[0..n] are the caller's offsets into either. Every form's body is written once over this; its
// public entry points build the source and call the body.
struct QuerySrc {
  const void* data;  // query i is off[i] .. off[i + 1] of it: tfp_frame, or with samples int16 at sample rate sr
  const int64_t* off;
  int32_t sr;
  bool samples;
  bool fingerprinted = false;  // materialise() queued a fingerprint that settle() waits for
  // samples at another rate (rate_source): off are the offsets at sr and data is rate->pcm
  const RateSrc* rate = nullptr;
  // interleaved multichannel samples (mix_source): off are the offsets at sr and data is mix->pcm
  const MixSrc* mix = nullptr;
  // a mixed batch (any_source): off are the offsets at sr and data is the call's bytes
  const AnySrc* any = nullptr;

  int check_offsets(tfp_engine* e, int32_t n) const { return check_monotone(e, off, n, samples); }
  int check_data(tfp_engine* e, int64_t nframes) const {  // frames to search need their data
    return nframes > 0 && !data ? fail(e, TFP_E_ARG, "%s", samples ? "samples are NULL" : "frames is NULL") : TFP_OK;
  }
  // the queries' relative frame offsets (n <= 0: {0}, no offset is read)
  std::vector<int64_t> fo(int32_t n) const { return samples ? sample_frame_offsets(off, n) : relative_offsets(off, n); }

  // The frame values on the device, *d_q: frames are uploaded into e->q; samples are fingerprinted once
  // into e->db (nothing to do without a frame). They stay there for an alignment after the search.
  int materialise(tfp_engine* e, int32_t n, const std::vector<int64_t>& fo, const tfp_search_params* P, const double** d_q) {
    HIPCHK(e, hipSetDevice(e->device));
    int rc = TFP_OK;
    if (!samples) {
      rc = upload_frames(e, static_cast<const tfp_frame*>(data), off, n);
    } else if (fo[n] > 0) {
      std::vector<const void*> ptrs;
      std::vector<int64_t> lens;
      split_offsets(data, sizeof(int16_t), off, n, &ptrs, &lens);
      int64_t nf;
      rc = fingerprint_host(e, rate || mix || any ? nullptr : ptrs.data(), lens.data(), false, n, sr, &nf, nullptr,
                            P->coefs == 2, nullptr, rate, mix, any);
      fingerprinted = rc == TFP_OK;
    }
    *d_q = samples ? e->db.as<double>() : e->q.as<double>();
    return rc;
  }

  // After the core: the fingerprint's staging buffer is free again once the stream has drained.
  int settle(tfp_engine* e) {
    if (!fingerprinted) return TFP_OK;
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (an empty index returns before any wait)
    e->stage_pending = false;
    return TFP_OK;
  }
};

// Ranked search (tfp_search_ranked_*_batch); with align its rows' alignments (tfp_search_aligned_*_batch),
// scoped: scoped search (tfp_search_scoped_*_batch), a scope per query of TFP_SCOPE_ANY or above.
int search_ranked(tfp_engine* e, QuerySrc src, int32_t nq, const tfp_search_params* P, int32_t k, tfp_candidate* out,
                  int32_t* counts, tfp_alignment* align, bool scoped = false, const int32_t* scopes = nullptr) {
  if (nq < 0 || !out || !counts) return fail(e, TFP_E_ARG, "ranked search: bad query count or NULL output");
  int rc = check_k(e, "ranked search", k);
  if (rc || (rc = check_params(e, "ranked search", P))) return rc;
  if (scoped && nq && !scopes) return fail(e, TFP_E_ARG, "scoped search: scopes is NULL");
  if ((rc = check_scopes(e, "scoped search", scopes, nq, "query")) || (rc = src.check_offsets(e, nq))) return rc;
  const std::vector<int64_t> fo = src.fo(nq);
  if ((rc = src.check_data(e, fo[nq]))) return rc;
  std::vector<unsigned long long> keys((size_t)nq * k, 0ull);
  const double* d_q = nullptr;
  // frames run the core, hence the index build, for any query; samples only once a frame exists
  const bool run = nq && (!src.samples || fo[nq] > 0);
  if (run && ((rc = src.materialise(e, nq, fo, P, &d_q)) ||
              (rc = rank_core(e, fo.data(), nq, d_q, P, k, scopes, keys, e->stream)) || (rc = src.settle(e))))
    return rc;
  fill_candidates(e, keys, nq, k, out, counts);
  if (align && nq) {
    if (src.samples) memset(align, 0, sizeof(tfp_alignment) * (size_t)nq * k);  // (frames always run: align_core zeroes)
    if (run) return align_core(e, fo, nq, d_q, P, k, candidate_ids(out, counts, nq, k).data(), align, e->stream);
  }
  return TFP_OK;
}
}  // namespace

int tfp_search_ranked_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                            const tfp_search_params* P, int32_t k, tfp_candidate* out, int32_t* counts) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_ranked(e, QuerySrc{frames, qoff, 0, false}, nq, P, k, out, counts, nullptr);
}

int tfp_search_ranked(tfp_engine* e, const tfp_frame* frames, int32_t nframes, const tfp_search_params* P, int32_t k,
                      tfp_candidate* out, int32_t* count) {
  if (nframes < 0) return TFP_E_ARG;
  int64_t qoff[2] = {0, nframes};
  return tfp_search_ranked_batch(e, frames, qoff, 1, P, k, out, count);
}

int tfp_search_ranked_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                                const tfp_search_params* P, int32_t k, tfp_candidate* out, int32_t* counts) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_ranked(e, QuerySrc{pcm, offsets, sr, true}, nq, P, k, out, counts, nullptr);
}

// ---- aligned search (tfp_align.hpp) -------------------------------------------------------
int tfp_align_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq, const tfp_search_params* P,
                    const int32_t* clip_ids, int32_t k, tfp_alignment* out) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (nq < 0 || !out) return fail(e, TFP_E_ARG, "aligned search: bad query count or NULL output");
  int rc = check_k(e, "aligned search", k);
  if (rc || (rc = check_params(e, "aligned search", P))) return rc;
  if (nq && !clip_ids) return fail(e, TFP_E_ARG, "aligned search: clip_ids is NULL");
  QuerySrc src{frames, qoff, 0, false};
  if ((rc = src.check_offsets(e, nq)) || !nq) return rc;
  const std::vector<int64_t> fo = src.fo(nq);
  const double* d_q;
  if ((rc = src.check_data(e, fo[nq])) || (rc = src.materialise(e, nq, fo, P, &d_q))) return rc;
  return align_core(e, fo, nq, d_q, P, k, clip_ids, out, e->stream);
}

int tfp_search_aligned_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                             const tfp_search_params* P, int32_t k, tfp_candidate* cand, tfp_alignment* align,
                             int32_t* counts) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!align) return fail(e, TFP_E_ARG, "aligned search: NULL output");
  return search_ranked(e, QuerySrc{frames, qoff, 0, false}, nq, P, k, cand, counts, align);
}

int tfp_search_aligned_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                                 const tfp_search_params* P, int32_t k, tfp_candidate* cand, tfp_alignment* align,
                                 int32_t* counts) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!align) return fail(e, TFP_E_ARG, "aligned search: NULL output");
  return search_ranked(e, QuerySrc{pcm, offsets, sr, true}, nq, P, k, cand, counts, align);
}

int tfp_align_stats(tfp_engine* e, int64_t* batches, int64_t* pairs) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (batches) *batches = e->n_align_batches;
  if (pairs) *pairs = e->n_align_pairs;
  return TFP_OK;
}

int tfp_rank_stats(tfp_engine* e, int64_t* vote_batches, int64_t* general_batches) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (vote_batches) *vote_batches = e->n_rank_vote;
  if (general_batches) *general_batches = e->n_rank_general;
  return TFP_OK;
}

int tfp_fingerprint_stats(tfp_engine* e, int64_t* small8k, int64_t* throughput8k, int64_t* generic_i16,
                          int64_t* generic_f32) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (small8k) *small8k = e->fpstats.small8k;
  if (throughput8k) *throughput8k = e->fpstats.throughput8k;
  if (generic_i16) *generic_i16 = e->fpstats.generic_i16;
  if (generic_f32) *generic_f32 = e->fpstats.generic_f32;
  return TFP_OK;
}

// ---- scoped search (tfp_scope.hpp): fp_handler.c:367-374 over one context's clips ----------
static_assert(kScopeAny == TFP_SCOPE_ANY, "tfp_scope.hpp and the public header agree");

int tfp_index_set_scope(tfp_engine* e, int32_t n, const char* const* uuids, const int32_t* scopes) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (n < 0 || (n && (!uuids || !scopes))) return fail(e, TFP_E_ARG, "set scope: bad count or NULL array");
  std::vector<int32_t> ids((size_t)n);
  for (int32_t i = 0; i < n; i++) {  // all or nothing: every entry checked before any scope changes
    if (!uuids[i]) return fail(e, TFP_E_ARG, "set scope: uuid %d is NULL", i);
    if (scopes[i] < 0) return fail(e, TFP_E_ARG, "set scope: scope %d of %s", scopes[i], uuids[i]);
    const auto it = e->by_uuid.find(uuids[i]);
    if (it == e->by_uuid.end()) return fail(e, TFP_E_NOENT, "uuid %s not indexed", uuids[i]);
    ids[i] = it->second;
  }
  for (int32_t i = 0; i < n; i++) {
    Clip& c = e->clips[ids[i]];
    e->scope_dirty |= c.scope != scopes[i];
    c.scope = scopes[i];
  }
  return TFP_OK;
}

int tfp_index_scope(tfp_engine* e, const char* uuid, int32_t* scope) {
  if (!e || !uuid || !scope) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const auto it = e->by_uuid.find(uuid);
  if (it == e->by_uuid.end()) return fail(e, TFP_E_NOENT, "uuid %s not indexed", uuid);
  *scope = e->clips[it->second].scope;
  return TFP_OK;
}

int tfp_search_scoped_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                            const tfp_search_params* P, const int32_t* scopes, int32_t k, tfp_candidate* out,
                            int32_t* counts) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_ranked(e, QuerySrc{frames, qoff, 0, false}, nq, P, k, out, counts, nullptr, true, scopes);
}

int tfp_search_scoped_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                                const tfp_search_params* P, const int32_t* scopes, int32_t k, tfp_candidate* out,
                                int32_t* counts) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_ranked(e, QuerySrc{pcm, offsets, sr, true}, nq, P, k, out, counts, nullptr, true, scopes);
}

int tfp_scope_stats(tfp_engine* e, int64_t* vote_batches, int64_t* general_batches, int64_t* table_builds) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (vote_batches) *vote_batches = e->n_scope_vote;
  if (general_batches) *general_batches = e->n_scope_general;
  if (table_builds) *table_builds = e->n_scope_builds;
  return TFP_OK;
}

// ---- catalog neighbours (tfp_neighbour.hpp): fp_handler.c:367-374 for a clip's own stored rows ----
namespace {

// The columns' staged rows on the device and the clips' columns on the host, for the current index
// (caller has run rebuild): rebuilt when the index version changed, else they stand.
int ensure_neighbour_cols(tfp_engine* e, hipStream_t s) {
  if (e->nbr_version == e->index_version) return TFP_OK;
  const int32_t Cp = scope_table_cols(e->ncols);
  std::vector<NeighbourCol> rows((size_t)std::max(Cp, 1), NeighbourCol{0, 0});
  e->nbr_col_of_clip.assign(e->clips.size(), -1);
  e->nbr_nmax = 0;
  auto put = [&](size_t col, int32_t clip) {
    if (clip < 0 || !e->clips[clip].alive) return;
    rows[col] = NeighbourCol{e->clips[clip].off, e->clips[clip].nrows};
    e->nbr_col_of_clip[clip] = (int32_t)col;
    e->nbr_nmax = std::max(e->nbr_nmax, e->clips[clip].nrows);
  };
  for (size_t c = 0; c < e->col_clip.size(); c++) put(c, e->col_clip[c]);
  for (size_t j = 0; j < e->delta.clip.size(); j++) put((size_t)e->delta.col0 + j, e->delta.clip[j]);
  HIPCHK(e, e->nbr_colrows.reserve_grow(sizeof(NeighbourCol) * rows.size()));
  HIPCHK(e, hipMemcpyAsync(e->nbr_colrows.p, rows.data(), sizeof(NeighbourCol) * rows.size(), hipMemcpyHostToDevice, s));
  HIPCHK(e, hipStreamSynchronize(s));  // (rows is released on return)
  e->nbr_version = e->index_version;
  return TFP_OK;
}

// The launch descriptors of named clips ids[0, n): boxes laid end to end from 0. with_cols: the own
// columns from ensure_neighbour_cols (the vote form), else -1. *total = the clips' rows, *longest = the
// longest clip's.
void neighbour_clips(const tfp_engine* e, const int32_t* ids, const int32_t* scopes, int32_t n, bool with_cols,
                     std::vector<NeighbourClip>& nc, int64_t* total, int64_t* longest) {
  nc.resize((size_t)n);
  int64_t box0 = 0, mx = 0;
  for (int32_t i = 0; i < n; i++) {
    const Clip& c = e->clips[ids[i]];
    nc[i] = NeighbourClip{c.off, box0, (int32_t)c.nrows, scopes ? scopes[i] : kScopeAny,
                          with_cols ? e->nbr_col_of_clip[ids[i]] : -1, 0};
    box0 += c.nrows;
    mx = std::max(mx, c.nrows);
  }
  *total = box0;
  *longest = mx;
}

// The vote form for named clips ids[0, n) (a batch the partial keys' scratch holds): keys[n * K] and, with
// al, the rows' alignments, one upload, one read-back, one wait. *bad: a row's key lay outside the vote
// range (nothing written). Caller has run the ensure_* of the vote and ensure_neighbour_cols.
int neighbour_vote(tfp_engine* e, const int32_t* ids, const int32_t* scopes, int32_t n, const SearchConsts& sc, int32_t K,
                   unsigned long long* keys, AlignOut* al, bool* bad, hipStream_t s) {
  const int32_t C = e->ncols, nb = rank_vote_blocks(C);
  const size_t nkeys = (size_t)n * K;
  int64_t total, longest;
  std::vector<NeighbourClip> nc;
  neighbour_clips(e, ids, scopes, n, true, nc, &total, &longest);
  if (longest + e->nbr_nmax > (int64_t(1) << 31))  // align_core's limit
    return fail(e, TFP_E_CAPACITY, "neighbours: %lld rows against %lld rows", (long long)longest, (long long)e->nbr_nmax);
  const int64_t max_bands = std::max<int64_t>(align_bands(longest, e->nbr_nmax), 1);
  // pairs in chunks of <= 256 MB of partial keys (and of the launch grid's second dimension), as align_core
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>({(int64_t(1) << 25) / max_bands, kAlignMaxPairs, (int64_t)nkeys}));
  const size_t rbytes = (sizeof(unsigned long long) + sizeof(AlignOut)) * nkeys + 8;
  int rc;
  if ((rc = upload(e, e->nbr_clips, nc.data(), sizeof(NeighbourClip) * nc.size(), s))) return rc;
  HIPCHK(e, e->rank_part.reserve(sizeof(unsigned long long) * (size_t)n * nb * K));
  HIPCHK(e, e->nbr_res.reserve(rbytes));
  HIPCHK(e, e->nbr_pin.reserve(rbytes));
  unsigned long long* d_keys = e->nbr_res.as<unsigned long long>();  // [keys][bad flag][AlignOut]
  int32_t* d_flag = reinterpret_cast<int32_t*>(d_keys + nkeys);
  AlignOut* d_out = reinterpret_cast<AlignOut*>(d_keys + nkeys + 1);
  HIPCHK(e, hipMemsetAsync(d_flag, 0, sizeof(unsigned long long), s));
  const NeighbourClip* d_nc = e->nbr_clips.as<NeighbourClip>();
  HIPCHK(e, launch_neighbour_vote(e->st_m1.as<int32_t>(), d_nc, n, sc, e->tc.ranges.active().key_bits.as<uint32_t>(), C,
                                  e->tiekey.as<int32_t>(), e->scope_table.as<int32_t>(), K,
                                  e->rank_part.as<unsigned long long>(), d_keys, d_flag, s));
  size_t back = sizeof(unsigned long long) * (nkeys + 1);
  if (al) {
    HIPCHK(e, e->nbr_cols.reserve(sizeof(int32_t) * nkeys));
    HIPCHK(e, e->nbr_boxes.reserve(sizeof(FrameBox) * (size_t)(total + 1)));
    HIPCHK(e, e->nbr_pairs.reserve(sizeof(AlignPair) * nkeys));
    HIPCHK(e, e->nbr_part.reserve(sizeof(unsigned long long) * (size_t)(chunk * max_bands)));
    HIPCHK(e, hipMemsetAsync(e->nbr_cols.p, 0xff, sizeof(int32_t) * nkeys, s));  // -1: no column
    HIPCHK(e, launch_neighbour_boxes(e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), d_nc, n, longest, sc,
                                     e->nbr_boxes.as<FrameBox>(), s));
    HIPCHK(e, launch_neighbour_key_cols(d_keys, d_nc, n, K, e->tiekey.as<int32_t>(), e->scope_table.as<int32_t>(),
                                        e->nbr_colrows.as<NeighbourCol>(), C, e->nbr_cols.as<int32_t>(), s));
    HIPCHK(e, launch_neighbour_pairs(d_keys, e->nbr_cols.as<int32_t>(), e->nbr_colrows.as<NeighbourCol>(), C, d_nc, n, K,
                                     e->nbr_pairs.as<AlignPair>(), s));
    for (int64_t p0 = 0; p0 < (int64_t)nkeys; p0 += chunk) {
      const int32_t m = (int32_t)std::min<int64_t>(chunk, (int64_t)nkeys - p0);
      HIPCHK(e, launch_align(e->nbr_pairs.as<AlignPair>() + p0, m, max_bands, e->nbr_boxes.as<FrameBox>(),
                             e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), false, e->nbr_part.as<unsigned long long>(),
                             d_out + p0, s));
    }
    back = rbytes;
  }
  HIPCHK(e, hipMemcpyAsync(e->nbr_pin.p, d_keys, back, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));  // (nc is released on return)
  const unsigned long long* hk = e->nbr_pin.as<unsigned long long>();
  *bad = (uint32_t)hk[nkeys] != 0;
  if (*bad) return TFP_OK;
  std::copy(hk, hk + nkeys, keys);
  if (al) {
    const AlignOut* ho = reinterpret_cast<const AlignOut*>(hk + nkeys + 1);
    for (size_t p = 0; p < nkeys; p++) {
      al[p] = AlignOut{0, 0, 0, 0};
      if (!keys[p]) continue;
      // a row has a frame that hits one of its clip's rows, so its best diagonal holds a hit
      if (ho[p].aligned_count <= 0)
        return fail(e, TFP_E_HIP, "neighbours: no staged rows found for tie-break key %u", (unsigned)(keys[p] & 0xffffffffu));
      al[p] = ho[p];
    }
  }
  return TFP_OK;
}

// The clip behind a row's key (-1: none).
int32_t clip_of_key(const tfp_engine* e, unsigned long long key) {
  return clip_of_col(e, col_of_key(e, (int32_t)(uint32_t)(key & 0xffffffffu)));
}

// The general form over frame values on the device (query i at qo[i] .. qo[i + 1] of d_q): the scoped
// search's core at k + 1 rows (the one caller of the ranked launchers' internal bound), self_ids[i] (-1:
// none on this engine) deleted on the host, k rows kept; with al their alignments as aligned search's.
// The cores run uncounted: these are not the scoped and aligned searches' batches.
int neighbour_general(tfp_engine* e, const std::vector<int64_t>& qo, int32_t n, const double* d_q, const tfp_search_params* P,
                      const int32_t* scopes, const int32_t* self_ids, int32_t K, unsigned long long* keys, AlignOut* al,
                      hipStream_t s) {
  std::vector<unsigned long long> wide;
  int rc = rank_core(e, qo.data(), n, d_q, P, K + 1, scopes, wide, s, false);
  if (rc) return rc;
  std::vector<int32_t> ids((size_t)n * K, -1), row((size_t)K + 1), keep((size_t)K);
  for (int32_t i = 0; i < n; i++) {
    int32_t nr = 0;
    while (nr <= K && wide[(size_t)i * (K + 1) + nr]) {
      row[nr] = clip_of_key(e, wide[(size_t)i * (K + 1) + nr]);
      nr++;
    }
    const int32_t m = neighbour_drop_self(row.data(), nr, self_ids ? self_ids[i] : -1, K, keep.data());
    for (int32_t r = 0; r < K; r++) {
      keys[(size_t)i * K + r] = r < m ? wide[(size_t)i * (K + 1) + keep[r]] : 0ull;
      if (r < m) ids[(size_t)i * K + r] = row[keep[r]];
    }
  }
  if (!al) return TFP_OK;
  static_assert(sizeof(tfp_alignment) == sizeof(AlignOut), "one layout");
  return align_core(e, qo, n, d_q, P, K, ids.data(), reinterpret_cast<tfp_alignment*>(al), s, false);
}

// Keys to rows for named clips, as fill_candidates; the alignments of the rows kept move with them.
void fill_neighbours(tfp_engine* e, const std::vector<unsigned long long>& keys, const std::vector<AlignOut>& al, int32_t n,
                     int32_t K, tfp_candidate* out, tfp_alignment* align, int32_t* counts) {
  std::vector<int32_t> cnt((size_t)std::max(n, 1));
  fill_candidates(e, keys, n, K, out, cnt.data());
  if (align) {
    memset(align, 0, sizeof(tfp_alignment) * (size_t)n * K);
    for (int32_t i = 0; i < n; i++) {
      int32_t w = 0;
      for (int32_t r = 0; r < K && keys[(size_t)i * K + r]; r++) {
        if (clip_of_key(e, keys[(size_t)i * K + r]) < 0) continue;  // (fill_candidates skipped it too)
        const AlignOut& a = al[(size_t)i * K + r];
        align[(size_t)i * K + w++] = tfp_alignment{a.aligned_count, a.offset, a.first_frame, a.last_frame};
      }
    }
  }
  std::copy(cnt.begin(), cnt.begin() + n, counts);
}

// The body of tfp_index_neighbours over resolved clip ids. Shaped like slide_core: the vote form at the
// tolerances whose key bitsets hold a live index delta's columns, else (and for a key outside the vote
// range) the general form over the merged index.
int neighbours_core(tfp_engine* e, const std::vector<int32_t>& ids, const tfp_search_params* P, const int32_t* scopes,
                    int32_t K, std::vector<unsigned long long>& keys, std::vector<AlignOut>* al, hipStream_t s) {
  const int32_t n = (int32_t)ids.size();
  int rc = rebuild(e);  // synchronous on e->stream
  if (rc) return rc;
  const SearchConsts sc = search_consts(P);
  keys.assign((size_t)n * K, 0ull);
  if (al) al->assign((size_t)n * K, AlignOut{0, 0, 0, 0});
  int64_t frames = 0;
  for (const int32_t id : ids) frames += e->clips[id].nrows;
  if (sc.coefs == 1 && delta_tol_ok(sc.tole)) {
    if (e->ncols <= 0 || e->nrows + e->delta.rows <= 0) {  // no row that can match: no neighbour, nothing launched
      e->n_nbr_vote++;
      e->n_nbr_frames += frames;
      return TFP_OK;
    }
    if ((rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_key_bits(e, s)) || (rc = ensure_scope_table(e, s)) ||
        (rc = ensure_neighbour_cols(e, s)))
      return rc;
    // named clips in batches of <= 256 MB of partial keys (and of the launch grid's second dimension), as rank_vote
    const int32_t nb = rank_vote_blocks(e->ncols);
    int64_t chunk = (int64_t)(256ll << 20) / ((int64_t)sizeof(unsigned long long) * nb * K);
    chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(chunk, 65535 / K), n));
    bool bad = false;
    for (int64_t i0 = 0; i0 < n && !bad; i0 += chunk) {
      const int32_t m = (int32_t)std::min<int64_t>(chunk, n - i0);
      if ((rc = neighbour_vote(e, ids.data() + i0, scopes ? scopes + i0 : nullptr, m, sc, K, keys.data() + i0 * K,
                               al ? al->data() + i0 * K : nullptr, &bad, s)))
        return rc;
    }
    if (!bad) {
      e->n_nbr_vote++;
      e->n_nbr_frames += frames;
      for (const unsigned long long k : keys) e->n_nbr_pairs += al && k != 0;
      return TFP_OK;
    }
    keys.assign((size_t)n * K, 0ull);
    if (al) al->assign((size_t)n * K, AlignOut{0, 0, 0, 0});
  }
  if ((rc = consolidate(e))) return rc;  // (the clips' staged rows may move: descriptors are built after it)
  std::vector<int32_t> any;
  if (!scopes) any.assign((size_t)n, kScopeAny);
  const int32_t* sv = scopes ? scopes : any.data();
  // named clips in batches of <= 256 MB of gathered frame values (and of the launch grid's second dimension)
  const int64_t cap_frames = (int64_t)(256ll << 20) / (2 * sizeof(double));
  for (int32_t i0 = 0; i0 < n;) {
    int32_t i1 = i0;
    int64_t nf = 0;
    while (i1 < n && i1 - i0 < 65535 && (i1 == i0 || nf + e->clips[ids[i1]].nrows <= cap_frames)) nf += e->clips[ids[i1++]].nrows;
    const int32_t m = i1 - i0;
    int64_t total, longest;
    std::vector<NeighbourClip> nc;
    neighbour_clips(e, ids.data() + i0, sv + i0, m, false, nc, &total, &longest);
    std::vector<int64_t> qo((size_t)m + 1, 0);
    for (int32_t i = 0; i < m; i++) qo[i + 1] = qo[i] + nc[i].nrows;
    if ((rc = upload(e, e->nbr_clips, nc.data(), sizeof(NeighbourClip) * nc.size(), s))) return rc;
    HIPCHK(e, e->nbr_q.reserve(2 * sizeof(double) * (size_t)(total + 1)));
    HIPCHK(e, launch_neighbour_gather(e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), e->nbr_clips.as<NeighbourClip>(), m,
                                      longest, e->nbr_q.as<double>(), s));
    if ((rc = neighbour_general(e, qo, m, e->nbr_q.as<double>(), P, sv + i0, ids.data() + i0, K, keys.data() + (size_t)i0 * K,
                                al ? al->data() + (size_t)i0 * K : nullptr, s)))
      return rc;
    HIPCHK(e, hipStreamSynchronize(s));  // (an empty index returns before any wait: nc is released here)
    i0 = i1;
  }
  e->n_nbr_general++;
  e->n_nbr_frames += frames;
  for (const unsigned long long k : keys) e->n_nbr_pairs += al && k != 0;
  return TFP_OK;
}

int neighbour_args(tfp_engine* e, int32_t n, const void* ptrs, const tfp_search_params* P, const int32_t* scopes, int32_t k,
                   const void* out, const void* counts) {
  if (n < 0 || (n && (!ptrs || !out || !counts))) return fail(e, TFP_E_ARG, "neighbours: bad clip count or NULL array");
  int rc = check_k(e, "neighbours", k);
  if (rc || (rc = check_params(e, "neighbours", P))) return rc;
  return check_scopes(e, "neighbours", scopes, n, "clip");
}

}  // namespace

int tfp_index_neighbours(tfp_engine* e, int32_t nclips, const char* const* uuids, const tfp_search_params* P,
                         const int32_t* scopes, int32_t k, tfp_candidate* out, tfp_alignment* align, int32_t* counts,
                         int32_t* frame_counts) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  int rc = neighbour_args(e, nclips, uuids, P, scopes, k, out, counts);
  if (rc) return rc;
  std::vector<int32_t> ids((size_t)nclips);
  for (int32_t i = 0; i < nclips; i++) {  // all or nothing: every name resolved before anything is written
    if (!uuids[i]) return fail(e, TFP_E_ARG, "neighbours: uuid %d is NULL", i);
    const auto it = e->by_uuid.find(uuids[i]);
    if (it == e->by_uuid.end()) return fail(e, TFP_E_NOENT, "uuid %s not indexed", uuids[i]);
    ids[i] = it->second;
  }
  if (!nclips) return TFP_OK;
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<unsigned long long> keys;
  std::vector<AlignOut> al;
  if ((rc = neighbours_core(e, ids, P, scopes, k, keys, align ? &al : nullptr, e->stream))) return rc;
  fill_neighbours(e, keys, al, nclips, k, out, align, counts);
  for (int32_t i = 0; frame_counts && i < nclips; i++) frame_counts[i] = (int32_t)e->clips[ids[i]].nrows;
  return TFP_OK;
}

int tfp_neighbour_stats(tfp_engine* e, int64_t* vote_batches, int64_t* general_batches, int64_t* pairs_aligned,
                        int64_t* frames_read) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (vote_batches) *vote_batches = e->n_nbr_vote;
  if (general_batches) *general_batches = e->n_nbr_general;
  if (pairs_aligned) *pairs_aligned = e->n_nbr_pairs;
  if (frames_read) *frames_read = e->n_nbr_frames;
  return TFP_OK;
}

// A device group's steps (tfp_group_index_neighbours). _frames: the frame values of this engine's named
// clips (the gather kernel), clip i at out[foff[i]]. _of_frames: the rows of host frames over this
// engine's clips with self_ids[i] (-1: the clip lies on another shard) deleted, general form's body.
int tfp_internal_neighbour_rows(tfp_engine* e, int32_t nclips, const char* const* uuids, int64_t* nrows) {
  if (!e || nclips < 0 || (nclips && (!uuids || !nrows))) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  for (int32_t i = 0; i < nclips; i++) {
    const auto it = e->by_uuid.find(uuids[i]);
    if (it == e->by_uuid.end()) return fail(e, TFP_E_NOENT, "uuid %s not indexed", uuids[i]);
    nrows[i] = e->clips[it->second].nrows;
  }
  return TFP_OK;
}

int tfp_internal_neighbour_frames(tfp_engine* e, int32_t nclips, const char* const* uuids, const int64_t* foff,
                                  tfp_frame* out) {
  if (!e || nclips < 0 || (nclips && (!uuids || !foff || !out))) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  std::vector<int32_t> ids((size_t)nclips);
  for (int32_t i = 0; i < nclips; i++) {
    const auto it = e->by_uuid.find(uuids[i]);
    if (it == e->by_uuid.end()) return fail(e, TFP_E_NOENT, "uuid %s not indexed", uuids[i]);
    ids[i] = it->second;
  }
  if (!nclips) return TFP_OK;
  HIPCHK(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  int64_t total, longest;
  std::vector<NeighbourClip> nc;
  neighbour_clips(e, ids.data(), nullptr, nclips, false, nc, &total, &longest);
  if (!total) return TFP_OK;
  int rc = upload(e, e->nbr_clips, nc.data(), sizeof(NeighbourClip) * nc.size(), s);
  if (rc) return rc;
  HIPCHK(e, e->nbr_q.reserve(2 * sizeof(double) * (size_t)(total + 1)));
  for (int32_t i0 = 0; i0 < nclips; i0 += 65535)
    HIPCHK(e, launch_neighbour_gather(e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), e->nbr_clips.as<NeighbourClip>() + i0,
                                      std::min(65535, nclips - i0), longest, e->nbr_q.as<double>(), s));
  std::vector<double> q(2 * (size_t)total);
  HIPCHK(e, hipMemcpyAsync(q.data(), e->nbr_q.p, sizeof(double) * q.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));
  for (int32_t i = 0; i < nclips; i++)
    for (int64_t j = 0; j < nc[i].nrows; j++) {
      tfp_frame& f = out[foff[i] + j];
      memset(&f, 0, sizeof f);
      f.frame_idx = (int32_t)j;
      f.q1 = q[2 * (size_t)(nc[i].box0 + j)];
      f.q2 = q[2 * (size_t)(nc[i].box0 + j) + 1];
    }
  return TFP_OK;
}

int tfp_internal_neighbours_of_frames(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                                      const tfp_search_params* P, const int32_t* scopes, const int32_t* self_ids, int32_t k,
                                      tfp_candidate* out, int32_t* counts) {
  if (!e || !qoff || nq < 0 || !out || !counts || !scopes) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  int rc = check_k(e, "neighbours", k);
  if (rc || (rc = check_params(e, "neighbours", P))) return rc;
  if (!nq) return TFP_OK;
  const std::vector<int64_t> qo = relative_offsets(qoff, nq);
  HIPCHK(e, hipSetDevice(e->device));
  if ((rc = upload_frames(e, frames, qoff, nq))) return rc;
  std::vector<unsigned long long> keys((size_t)nq * k, 0ull);
  if ((rc = neighbour_general(e, qo, nq, e->q.as<double>(), P, scopes, self_ids, k, keys.data(), nullptr, e->stream))) return rc;
  fill_candidates(e, keys, nq, k, out, counts);
  e->n_nbr_general++;
  for (int32_t i = 0; self_ids && i < nq; i++)  // a clip's stored rows are read on its own shard: counted there, once
    if (self_ids[i] >= 0) e->n_nbr_frames += qo[i + 1] - qo[i];
  return TFP_OK;
}

int tfp_internal_neighbour_align(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq,
                                 const tfp_search_params* P, const int32_t* clip_ids, int32_t k, tfp_alignment* out) {
  if (!e || !qoff || nq < 0 || !out || (nq && !clip_ids)) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  int rc = check_k(e, "neighbours", k);
  if (rc || (rc = check_params(e, "neighbours", P)) || !nq) return rc;
  const std::vector<int64_t> qo = relative_offsets(qoff, nq);
  HIPCHK(e, hipSetDevice(e->device));
  if ((rc = upload_frames(e, frames, qoff, nq)) ||
      (rc = align_core(e, qo, nq, e->q.as<double>(), P, k, clip_ids, out, e->stream, false)))
    return rc;
  for (size_t p = 0; p < (size_t)nq * k; p++) e->n_nbr_pairs += clip_ids[p] >= 0;
  return TFP_OK;
}

// ---- match census (tfp_census.hpp): fp_handler.c:367-374's rows counted by count(*) ---------
static_assert(kCensusLdsBins >= 2, "bin 0 is the host's");

int64_t tfp_census_at_least(const int32_t* hist_row, int32_t nbins, int32_t count) {
  if (!hist_row) return 0;
  int64_t n = 0;
  for (int32_t c = count <= 0 ? 0 : count; c < nbins; c++) n += hist_row[c];
  return n;
}

namespace {
// The match census over a query source (tfp_census_*_batch).
int census_search(tfp_engine* e, QuerySrc src, int32_t nq, const tfp_search_params* P, const int32_t* scopes, int32_t nbins,
                  int32_t* hist, int32_t* need_bins) {
  std::vector<int32_t> sv;
  int rc = census_args(e, P, nq, scopes, need_bins, sv);
  if (rc || (rc = src.check_offsets(e, nq))) return rc;
  const std::vector<int64_t> fo = src.fo(nq);
  if ((rc = src.check_data(e, fo[nq])) || (rc = census_bins(e, fo.data(), nq, nbins, hist, need_bins)) || !nq) return rc;
  const double* d_q;
  // the core runs, hence the index is built, even without a frame: bin 0 needs the scopes' populations
  if ((rc = src.materialise(e, nq, fo, P, &d_q))) return rc;
  rc = census_core(e, fo.data(), nq, d_q, P, sv.data(), nbins, hist, e->stream);
  const int waited = src.settle(e);  // (after a failed core too, unlike the other forms)
  return waited ? waited : rc;
}
}  // namespace

int tfp_census_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nq, const tfp_search_params* P,
                     const int32_t* scopes, int32_t nbins, int32_t* hist, int32_t* need_bins) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return census_search(e, QuerySrc{frames, qoff, 0, false}, nq, P, scopes, nbins, hist, need_bins);
}

int tfp_census_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                         const tfp_search_params* P, const int32_t* scopes, int32_t nbins, int32_t* hist,
                         int32_t* need_bins) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return census_search(e, QuerySrc{pcm, offsets, sr, true}, nq, P, scopes, nbins, hist, need_bins);
}

int tfp_census_stats(tfp_engine* e, int64_t* vote_batches, int64_t* general_batches) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (vote_batches) *vote_batches = e->n_census_vote;
  if (general_batches) *general_batches = e->n_census_general;
  return TFP_OK;
}

// ---- sliding search (tfp_slide.hpp): fp_handler.c:367-374 for every window of a recording ----
static_assert(kSlideRun == TFP_SLIDE_RUN, "tfp_slide.hpp and the public header agree");

int64_t tfp_sliding_windows(int64_t nframes, int32_t window, int32_t hop) { return plan_windows(nframes, window, hop); }

namespace {
// Sliding search over a query source (tfp_search_sliding_*_batch); aligned: with each row's alignment
// (tfp_search_sliding_aligned_*_batch), which leaves the recordings' boxes in e->align_boxes.
int search_sliding(tfp_engine* e, QuerySrc src, int32_t nrec, const tfp_search_params* P, int32_t window, int32_t hop,
                   const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts, bool aligned, tfp_alignment* align,
                   int64_t cap_windows, int64_t* nwindows, const std::vector<int64_t>* checked_fo = nullptr) {
  int rc = checked_fo ? TFP_OK : src.check_offsets(e, nrec);  // (before the other arguments, unlike the ranked forms)
  if (rc) return rc;
  // (nrec < 0: no offset is read, slide_args rejects the count; checked_fo: the occurrence search's, not worked out twice)
  const std::vector<int64_t>& fo = checked_fo ? *checked_fo : src.fo(nrec);
  std::vector<int64_t> woff;
  if ((rc = slide_args(e, P, window, hop, k, nrec, scopes, fo, out, counts, cap_windows, nwindows, woff))) return rc;
  const int32_t nw = (int32_t)woff[nrec];
  if (!nw) return TFP_OK;  // no full window: nothing is fingerprinted or launched
  if (aligned) {  // (asked only once a window exists)
    if (!align) return fail(e, TFP_E_ARG, "sliding aligned search: NULL output");
    if ((rc = slide_align_limits(e, window))) return rc;
  }
  std::vector<unsigned long long> keys;
  const double* d_q;
  if ((rc = src.check_data(e, fo[nrec])) || (rc = src.materialise(e, nrec, fo, P, &d_q)) ||
      (rc = slide_core(e, fo, nrec, d_q, P, window, hop, scopes, k, woff, keys, e->stream)) || (rc = src.settle(e)))
    return rc;
  fill_candidates(e, keys, nw, k, out, counts);
  if (!aligned) return TFP_OK;
  return slide_align_core(e, fo, nrec, d_q, P, window, hop, k, woff, candidate_ids(out, counts, nw, k).data(), align,
                          e->stream);
}
}  // namespace

int tfp_search_sliding_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nrec,
                             const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes, int32_t k,
                             tfp_candidate* out, int32_t* counts, int64_t cap_windows, int64_t* nwindows) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_sliding(e, QuerySrc{frames, qoff, 0, false}, nrec, P, window, hop, scopes, k, out, counts, false, nullptr,
                        cap_windows, nwindows);
}

int tfp_search_sliding_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nrec, int32_t sr,
                                 const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes, int32_t k,
                                 tfp_candidate* out, int32_t* counts, int64_t cap_windows, int64_t* nwindows) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_sliding(e, QuerySrc{pcm, offsets, sr, true}, nrec, P, window, hop, scopes, k, out, counts, false, nullptr,
                        cap_windows, nwindows);
}

int tfp_slide_stats(tfp_engine* e, int64_t* vote_batches, int64_t* general_batches, int64_t* windows) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (vote_batches) *vote_batches = e->n_slide_vote;
  if (general_batches) *general_batches = e->n_slide_general;
  if (windows) *windows = e->n_slide_windows;
  return TFP_OK;
}

// ---- sliding aligned search (tfp_slide_align.hpp): fp_handler.c:287-351 per window frame against
// the rows of each window's clips ----
int tfp_align_sliding_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nrec,
                            const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* clip_ids, int32_t k,
                            tfp_alignment* out, int64_t cap_windows, int64_t* nwindows) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  QuerySrc src{frames, qoff, 0, false};
  int rc = src.check_offsets(e, nrec);
  if (rc) return rc;
  std::vector<int64_t> fo = src.fo(nrec), woff;
  if ((rc = slide_args(e, P, window, hop, k, nrec, nullptr, fo, out, clip_ids, cap_windows, nwindows, woff)) ||
      (rc = slide_align_limits(e, window)))
    return rc;
  if (!woff[nrec]) return TFP_OK;  // no full window: nothing is launched
  const double* d_q;
  if ((rc = src.check_data(e, fo[nrec])) || (rc = src.materialise(e, nrec, fo, P, &d_q))) return rc;
  return slide_align_core(e, fo, nrec, d_q, P, window, hop, k, woff, clip_ids, out, e->stream);
}

int tfp_search_sliding_aligned_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nrec,
                                     const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes,
                                     int32_t k, tfp_candidate* out, int32_t* counts, tfp_alignment* align,
                                     int64_t cap_windows, int64_t* nwindows) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_sliding(e, QuerySrc{frames, qoff, 0, false}, nrec, P, window, hop, scopes, k, out, counts, true, align,
                        cap_windows, nwindows);
}

int tfp_search_sliding_aligned_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nrec, int32_t sr,
                                         const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes,
                                         int32_t k, tfp_candidate* out, int32_t* counts, tfp_alignment* align,
                                         int64_t cap_windows, int64_t* nwindows) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_sliding(e, QuerySrc{pcm, offsets, sr, true}, nrec, P, window, hop, scopes, k, out, counts, true, align,
                        cap_windows, nwindows);
}

int tfp_slide_align_stats(tfp_engine* e, int64_t* batches, int64_t* slid_entries, int64_t* direct_entries) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (batches) *batches = e->n_sa_batches;
  if (slid_entries) *slid_entries = e->n_sa_slid;
  if (direct_entries) *direct_entries = e->n_sa_direct;
  return TFP_OK;
}

// ---- diagonal trace and occurrence search (tfp_trace.hpp): fp_handler.c:287-351 along one diagonal
// of a recording against a clip's rows ----
int tfp_trace_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nrec, const tfp_search_params* P,
                    const tfp_trace_req* reqs, int64_t nreqs, int32_t max_gap, tfp_trace* out) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (nrec < 0 || nreqs < 0 || (nreqs && (!reqs || !out))) return fail(e, TFP_E_ARG, "trace: bad count or NULL array");
  if (max_gap < 0) return fail(e, TFP_E_ARG, "trace: max_gap = %d", max_gap);
  QuerySrc src{frames, qoff, 0, false};
  int rc = check_params(e, "trace", P);
  if (rc || (rc = src.check_offsets(e, nrec))) return rc;
  for (int64_t i = 0; i < nreqs; i++)
    if (reqs[i].recording < 0 || reqs[i].recording >= nrec)
      return fail(e, TFP_E_ARG, "trace: recording %d of request %lld", reqs[i].recording, (long long)i);
  if (!nreqs) return TFP_OK;
  const std::vector<int64_t> fo = src.fo(nrec);
  if (fo[nrec] > INT32_MAX) return fail(e, TFP_E_CAPACITY, "trace: %lld frames", (long long)fo[nrec]);
  if ((rc = src.check_data(e, fo[nrec]))) return rc;
  return trace_core(
      e, fo, reqs, nreqs, max_gap, P,
      [&]() -> int {  // the recordings' frame values and their boxes, once a request needs them
        const double* d_q;
        if (int rc = src.materialise(e, nrec, fo, P, &d_q)) return rc;
        HIPCHK(e, e->align_boxes.reserve(sizeof(FrameBox) * (fo[nrec] + 1)));
        HIPCHK(e, launch_prep_boxes(d_q, fo[nrec], search_consts(P), e->align_boxes.as<FrameBox>(), nullptr, 0,
                                    e->stream));
        return TFP_OK;
      },
      out, e->stream);
}

namespace {
// The sliding aligned search's own buffers for nw windows (0 when the count is out of range: the
// search then reports it).
struct OccurRows {
  std::vector<tfp_candidate> cand;
  std::vector<int32_t> counts;
  std::vector<tfp_alignment> align;
  int64_t cap;
  OccurRows(int64_t nw, int32_t k) : cap(nw >= 0 && nw <= INT32_MAX ? nw : 0) {
    cand.resize((size_t)cap * k + 1);
    counts.resize((size_t)cap + 1);
    align.resize((size_t)cap * k + 1);
  }
};

// Occurrence search over a query source (tfp_search_occurrences_*_batch): the sliding aligned search into
// its own rows, then their occurrences.
int search_occurrences(tfp_engine* e, QuerySrc src, int32_t nrec, const tfp_search_params* P, int32_t window, int32_t hop,
                       const int32_t* scopes, int32_t k, int32_t max_gap, int32_t min_hits, tfp_occurrence* out, int64_t cap,
                       int64_t* nocc) {
  if (!nocc) return fail(e, TFP_E_ARG, "occurrence search: NULL noccurrences");
  if (max_gap < 0 || min_hits < 1) return fail(e, TFP_E_ARG, "occurrence search: max_gap = %d, min_hits = %d", max_gap, min_hits);
  int rc = check_k(e, "occurrence search", k);  // (the sliding aligned search checks the rest)
  if (rc || (rc = src.check_offsets(e, nrec))) return rc;
  const std::vector<int64_t> fo = src.fo(nrec);
  OccurRows rows(window_offsets(fo, nrec, window, hop)[std::max(nrec, 0)], k);
  int64_t got = 0;
  if ((rc = search_sliding(e, src, nrec, P, window, hop, scopes, k, rows.cand.data(), rows.counts.data(), true,
                           rows.align.data(), rows.cap, &got, &fo)))
    return rc;
  *nocc = 0;
  if (!got) return TFP_OK;  // no full window: no occurrence
  // (the frame boxes are still in e->align_boxes wherever a row came back)
  return occur_core(e, fo, nrec, P, window, hop, k, rows.cand.data(), rows.counts.data(), rows.align.data(), max_gap,
                    min_hits, out, cap, nocc, e->stream);
}
}  // namespace

int tfp_search_occurrences_batch(tfp_engine* e, const tfp_frame* frames, const int64_t* qoff, int32_t nrec,
                                 const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes, int32_t k,
                                 int32_t max_gap, int32_t min_hits, tfp_occurrence* out, int64_t cap, int64_t* nocc) {
  if (!e || !qoff) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_occurrences(e, QuerySrc{frames, qoff, 0, false}, nrec, P, window, hop, scopes, k, max_gap, min_hits, out, cap,
                            nocc);
}

int tfp_search_occurrences_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nrec, int32_t sr,
                                     const tfp_search_params* P, int32_t window, int32_t hop, const int32_t* scopes,
                                     int32_t k, int32_t max_gap, int32_t min_hits, tfp_occurrence* out, int64_t cap,
                                     int64_t* nocc) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  return search_occurrences(e, QuerySrc{pcm, offsets, sr, true}, nrec, P, window, hop, scopes, k, max_gap, min_hits, out,
                            cap, nocc);
}

int tfp_trace_stats(tfp_engine* e, int64_t* batches, int64_t* traces) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (batches) *batches = e->n_trace_batches;
  if (traces) *traces = e->n_traces;
  return TFP_OK;
}

namespace {
// One search over host samples, the queries given as (pointer, samples); no coalescing.
int search_gather_impl(tfp_engine* e, const void* const* ptrs, const int64_t* lens, int32_t nq, bool f32, int32_t sr,
                       const tfp_search_params* P, tfp_result* out, const G711Src* g711 = nullptr,
                       const RateSrc* rate = nullptr, const MixSrc* mix = nullptr, const AnySrc* any = nullptr) {
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<int64_t> foff(nq + 1, 0);
  for (int32_t i = 0; i < nq; i++) foff[i + 1] = foff[i] + tfp_frame_count(lens[i]);
  for (int32_t i = 0; e->fail_query_len >= 0 && i < nq; i++)  // (test knob: a query that fails on the device)
    if (lens[i] == e->fail_query_len)
      return fail(e, TFP_E_NOMEM, "hipMalloc for query %d of %d (%lld samples): out of memory (TFP_TEST_FAIL_QUERY_SAMPLES)", i,
                  nq, (long long)lens[i]);
  std::vector<unsigned long long> keys(nq, 0ull);
  if (valid_params(P) && nq && foff[nq] > 0) {
    int64_t nf;
    int rc = fingerprint_host(e, ptrs, lens, f32, nq, sr, &nf, nullptr, P->coefs == 2, g711, rate, mix, any);
    if (rc) return rc;
    if ((rc = search_core(e, foff.data(), nq, e->db.as<double>(), P, keys, nullptr, e->stream))) return rc;
    e->stage_pending = false;  // search_core waited for e->stream (keys on the host)
  }
  fill_results(e, keys, foff.data(), nq, out);
  return TFP_OK;
}

// Argument checks, then the call alone (large batches, TFP_COALESCE=0) or through the coalescer.
int search_gather_entry(tfp_engine* e, const void* const* ptrs, const int64_t* lens, int32_t nq, bool f32, int32_t sr,
                        const tfp_search_params* P, tfp_result* out) {
  if (!e || nq < 0 || !out || (nq && (!ptrs || !lens))) return TFP_E_ARG;
  for (int32_t i = 0; i < nq; i++)
    if (lens[i] < 0 || (lens[i] && !ptrs[i])) return fail(e, TFP_E_ARG, "bad query %d", i);
  if (!e->coalesce || nq == 0 || nq > Coalescer::kMaxCallQueries)
    return search_gather_impl(e, ptrs, lens, nq, f32, sr, P, out);
  SearchReq r;
  r.ptrs.assign(ptrs, ptrs + nq);
  r.lens.assign(lens, lens + nq);
  r.f32 = f32;
  r.sr = sr;
  if (P) r.P = *P;
  else r.P.coefs = 0;  // (invalid: NULL results, fp_handler.c:247-250)
  r.out = out;
  const int rc = e->coal.submit(&r, [e](std::vector<SearchReq*>& batch) {
    exec_batch(
        batch,
        [e](const void* const* p, const int64_t* l, int32_t n, bool f, int32_t rate, const tfp_search_params* q,
            tfp_result* o) { return search_gather_impl(e, p, l, n, f, rate, q, o); },
        [e] { return std::string(tfp_engine_last_error(e)); });
  });
  if (rc) e->err.note(e, r.err.c_str());  // (the leader ran it: the message into this caller's slot)
  return rc;
}

int search_samples_impl(tfp_engine* e, const void* pcm, bool f32, const int64_t* offsets, int32_t nq, int32_t sr,
                        const tfp_search_params* P, tfp_result* out) {
  if (!e || !offsets || nq < 0 || !out) return TFP_E_ARG;
  if (int rc = check_monotone(e, offsets, nq, true)) return rc;
  if (!pcm && nq && offsets[nq] > offsets[0]) return fail(e, TFP_E_ARG, "samples are NULL");
  std::vector<const void*> ptrs;
  std::vector<int64_t> lens;
  split_offsets(pcm, f32 ? sizeof(float) : sizeof(int16_t), offsets, nq, &ptrs, &lens);
  return search_gather_entry(e, ptrs.data(), lens.data(), nq, f32, sr, P, out);
}
}  // namespace

int tfp_search_pcm_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t sr,
                         const tfp_search_params* P, tfp_result* out) {
  return search_samples_impl(e, pcm, false, offsets, nq, sr, P, out);
}

int tfp_search_f32_batch(tfp_engine* e, const float* x, const int64_t* offsets, int32_t nq, int32_t sr,
                         const tfp_search_params* P, tfp_result* out) {
  return search_samples_impl(e, x, true, offsets, nq, sr, P, out);
}

// (also tfp_internal.hpp: a device group's per-shard call) Not coalesced: the coalescer gathers
// callers' queries by pointer for the in-place read of int16 buffers; codes are expanded from one
// flat array, and gathering several callers' arrays into one would add a host copy per call.
int tfp_internal_search_g711(tfp_engine* e, const uint8_t* codes, const int64_t* offsets, int32_t nq, int32_t law,
                             int32_t sr, const tfp_search_params* P, tfp_result* out) {
  if (!e || !offsets || nq < 0 || !out) return TFP_E_ARG;
  if (!g711_law_ok(law)) return fail(e, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  if (int rc = check_monotone(e, offsets, nq, true)) return rc;
  if (!codes && nq && offsets[nq] > offsets[0]) return fail(e, TFP_E_ARG, "codes are NULL");
  std::vector<int64_t> lens(nq);
  for (int32_t i = 0; i < nq; i++) lens[i] = offsets[i + 1] - offsets[i];
  const G711Src g{nq ? codes + offsets[0] : codes, law};
  return search_gather_impl(e, nullptr, lens.data(), nq, false, sr, P, out, &g);
}

// (tfp_internal.hpp) codes already on this engine's device into int16 there, on `stream`: a device
// group's query-sharded batch expands each shard's share in front of tfp_fingerprint_device.
int tfp_internal_g711_expand_device(tfp_engine* e, const uint8_t* d_codes, int64_t n, int32_t law, int16_t* d_pcm,
                                    void* stream) {
  if (!e || n < 0 || !g711_law_ok(law)) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  if (!n) return TFP_OK;
  HIPCHK(e, launch_g711_expand(d_codes, n, law, d_pcm, (hipStream_t)stream));
  e->n_g711_expand++;
  e->n_g711_codes += n;
  return TFP_OK;
}

int tfp_search_g711_batch(tfp_engine* e, const uint8_t* codes, const int64_t* offsets, int32_t nq, int32_t law, int32_t sr,
                          const tfp_search_params* P, tfp_result* out) {
  return tfp_internal_search_g711(e, codes, offsets, nq, law, sr, P, out);
}

// ---- rate-normalised ingest: the forms over int16 at another rate (tfp_resample.hpp) -------
// Equal rates are the plain forms (no table, no launch), entered as their own callers enter them: before
// the engine's lock is taken, since tfp_search_pcm_batch may wait in the coalescer for a leader that
// needs that lock. The converting forms are not coalesced, as the G.711 forms.
int tfp_fingerprint_rate_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nclips, int32_t rate_in,
                               int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!e) return TFP_E_ARG;
  if (rate_in < 1 || rate_out < 1) return fail(e, TFP_E_ARG, "bad sample rate %d", rate_in < 1 ? rate_in : rate_out);
  if (rate_in == rate_out) return tfp_fingerprint_batch(e, pcm, offsets, nclips, rate_out, out, cap, nframes);
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!offsets || nclips < 0 || !nframes || (!pcm && nclips && offsets[nclips] > offsets[0]))
    return fail(e, TFP_E_ARG, "bad arguments");
  RateSrc rs;
  std::vector<int64_t> out_off;
  if (int rc = rate_source(e, pcm, offsets, nclips, rate_in, rate_out, &rs, &out_off)) return rc;
  const int64_t need = sample_frame_offsets(out_off.data(), nclips)[nclips];
  *nframes = need;
  if (need > 0 && (!out || cap < need)) return fail(e, TFP_E_CAPACITY, "need %lld frames", (long long)need);
  if (need == 0) return TFP_OK;
  std::vector<int64_t> lens(nclips), foff;
  for (int32_t c = 0; c < nclips; c++) lens[c] = out_off[c + 1] - out_off[c];
  int64_t nf;
  if (int rc = fingerprint_host(e, nullptr, lens.data(), false, nclips, rate_out, &nf, &foff, true, nullptr, &rs)) return rc;
  return copy_frames_out(e, nf, foff, out);
}

int tfp_search_rate_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t rate_in,
                          int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!e) return TFP_E_ARG;
  if (rate_in < 1 || rate_out < 1) return fail(e, TFP_E_ARG, "bad sample rate %d", rate_in < 1 ? rate_in : rate_out);
  if (rate_in == rate_out) return tfp_search_pcm_batch(e, pcm, offsets, nq, rate_out, P, out);  // (no lock held: coalesced)
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!offsets || nq < 0 || !out) return TFP_E_ARG;
  RateSrc rs;
  std::vector<int64_t> out_off;
  if (int rc = rate_source(e, pcm, offsets, nq, rate_in, rate_out, &rs, &out_off)) return rc;
  if (!pcm && nq && offsets[nq] > offsets[0]) return fail(e, TFP_E_ARG, "samples are NULL");
  std::vector<int64_t> lens(nq);
  for (int32_t i = 0; i < nq; i++) lens[i] = out_off[i + 1] - out_off[i];
  return search_gather_impl(e, nullptr, lens.data(), nq, false, rate_out, P, out, nullptr, &rs);
}

int tfp_search_scoped_rate_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t rate_in,
                                 int32_t rate_out, const tfp_search_params* P, const int32_t* scopes, int32_t k,
                                 tfp_candidate* out, int32_t* counts, int32_t* frame_counts) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (rate_in < 1 || rate_out < 1) return fail(e, TFP_E_ARG, "bad sample rate %d", rate_in < 1 ? rate_in : rate_out);
  // the cheap arguments first, in search_ranked's order: an argument error does no device work
  if (nq < 0 || !out || !counts) return fail(e, TFP_E_ARG, "ranked search: bad query count or NULL output");
  if (int rc0 = check_k(e, "ranked search", k)) return rc0;
  if (int rc0 = check_params(e, "ranked search", P)) return rc0;
  if (nq && !scopes) return fail(e, TFP_E_ARG, "scoped search: scopes is NULL");
  if (int rc0 = check_scopes(e, "scoped search", scopes, nq, "query")) return rc0;
  RateSrc rs;
  std::vector<int64_t> out_off;
  int rc;
  if (rate_in == rate_out) {
    if ((rc = check_monotone(e, offsets, nq, true))) return rc;
    out_off = relative_offsets(offsets, nq);
    rc = search_ranked(e, QuerySrc{pcm, offsets, rate_out, true}, nq, P, k, out, counts, nullptr, true, scopes);
  } else {
    if ((rc = rate_source(e, pcm, offsets, nq, rate_in, rate_out, &rs, &out_off))) return rc;
    QuerySrc src{rs.pcm, out_off.data(), rate_out, true};
    src.rate = &rs;
    rc = search_ranked(e, src, nq, P, k, out, counts, nullptr, true, scopes);
  }
  if (rc) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) frame_counts[i] = (int32_t)tfp_frame_count(out_off[i + 1] - out_off[i]);
  return TFP_OK;
}

int tfp_resample_stats(tfp_engine* e, int64_t* launches, int64_t* samples_in, int64_t* samples_out) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (launches) *launches = e->n_rs_launch;
  if (samples_in) *samples_in = e->n_rs_in;
  if (samples_out) *samples_out = e->n_rs_out;
  return TFP_OK;
}

// ---- rate-normalised ingest of multichannel int16 (tfp_resample.hpp, "the multichannel form") ----
namespace {
// The mix source of a batch of `channels` > 1 interleaved channels: checks the pair and the offsets (in
// frames), takes the pair's table onto the device (none at equal rates: the downmix alone), and gives
// the clips' offsets at rate_out (out_off[0] = 0).
int mix_source(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t n, int32_t channels, int32_t rate_in,
               int32_t rate_out, MixSrc* ms, std::vector<int64_t>* out_off) {
  if (int rc = check_monotone(e, offsets, n, true)) return rc;
  ResamplePlan P;
  bool bad = false;
  if (!resample_plan(rate_in, rate_out, &P, &bad))
    return fail(e, TFP_E_ARG, "unsupported rate ratio %d -> %d", rate_in, rate_out);
  ms->tab = nullptr;
  ms->d_taps = nullptr;
  if (rate_in != rate_out) {
    const tfp_engine::RsTable* tab;
    if (int rc = ensure_rs_table(e, P, rate_in, rate_out, &tab)) return rc;
    ms->tab = tab->host.get();
    ms->d_taps = tab->dev.as<int16_t>();
  }
  ms->channels = channels;
  ms->pcm = pcm && n > 0 ? pcm + offsets[0] * channels : pcm;
  ms->in_off.assign((size_t)std::max(n, 0) + 1, 0);
  out_off->assign((size_t)std::max(n, 0) + 1, 0);
  for (int32_t c = 0; c < n; c++) {
    const int64_t len = offsets[c + 1] - offsets[c], no = rate_in == rate_out ? len : resample_count(P, len);
    if (no < 0 || len > INT64_MAX / (2 * channels) - ms->in_off[c])
      return fail(e, TFP_E_ARG, "clip %d: %lld frames past the index range", c, (long long)len);
    ms->in_off[c + 1] = ms->in_off[c] + len;
    (*out_off)[c + 1] = (*out_off)[c] + no;
  }
  return TFP_OK;
}

// The checks every mix form makes first: the channel count, then the rates, as the rate forms word them.
int check_mix(tfp_engine* e, int32_t channels, int32_t rate_in, int32_t rate_out) {
  if (channels < 1 || channels > TFP_MIX_CHANNELS_MAX) return fail(e, TFP_E_ARG, "unsupported channel count %d", channels);
  if (rate_in < 1 || rate_out < 1) return fail(e, TFP_E_ARG, "bad sample rate %d", rate_in < 1 ? rate_in : rate_out);
  return TFP_OK;
}
}  // namespace

// One channel is the rate form itself (hence, at equal rates, the plain form), entered before the
// engine's lock is taken, as the rate forms enter the plain ones. Not coalesced.
int tfp_fingerprint_mix_rate_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                                   int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                   int64_t* nframes) {
  if (!e) return TFP_E_ARG;
  if (channels == 1) return tfp_fingerprint_rate_batch(e, pcm, offsets, nclips, rate_in, rate_out, out, cap, nframes);
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (int rc = check_mix(e, channels, rate_in, rate_out)) return rc;
  if (!offsets || nclips < 0 || !nframes || (!pcm && nclips && offsets[nclips] > offsets[0]))
    return fail(e, TFP_E_ARG, "bad arguments");
  MixSrc ms;
  std::vector<int64_t> out_off;
  if (int rc = mix_source(e, pcm, offsets, nclips, channels, rate_in, rate_out, &ms, &out_off)) return rc;
  const int64_t need = sample_frame_offsets(out_off.data(), nclips)[nclips];
  *nframes = need;
  if (need > 0 && (!out || cap < need)) return fail(e, TFP_E_CAPACITY, "need %lld frames", (long long)need);
  if (need == 0) return TFP_OK;
  std::vector<int64_t> lens(nclips), foff;
  for (int32_t c = 0; c < nclips; c++) lens[c] = out_off[c + 1] - out_off[c];
  int64_t nf;
  if (int rc = fingerprint_host(e, nullptr, lens.data(), false, nclips, rate_out, &nf, &foff, true, nullptr, nullptr, &ms))
    return rc;
  return copy_frames_out(e, nf, foff, out);
}

int tfp_search_mix_rate_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t channels,
                              int32_t rate_in, int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!e) return TFP_E_ARG;
  if (channels == 1) return tfp_search_rate_batch(e, pcm, offsets, nq, rate_in, rate_out, P, out);
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (int rc = check_mix(e, channels, rate_in, rate_out)) return rc;
  if (!offsets || nq < 0 || !out) return TFP_E_ARG;
  MixSrc ms;
  std::vector<int64_t> out_off;
  if (int rc = mix_source(e, pcm, offsets, nq, channels, rate_in, rate_out, &ms, &out_off)) return rc;
  if (!pcm && nq && offsets[nq] > offsets[0]) return fail(e, TFP_E_ARG, "samples are NULL");
  std::vector<int64_t> lens(nq);
  for (int32_t i = 0; i < nq; i++) lens[i] = out_off[i + 1] - out_off[i];
  return search_gather_impl(e, nullptr, lens.data(), nq, false, rate_out, P, out, nullptr, nullptr, &ms);
}

int tfp_search_scoped_mix_rate_batch(tfp_engine* e, const int16_t* pcm, const int64_t* offsets, int32_t nq, int32_t channels,
                                     int32_t rate_in, int32_t rate_out, const tfp_search_params* P, const int32_t* scopes,
                                     int32_t k, tfp_candidate* out, int32_t* counts, int32_t* frame_counts) {
  if (!e || !offsets) return TFP_E_ARG;
  if (channels == 1)
    return tfp_search_scoped_rate_batch(e, pcm, offsets, nq, rate_in, rate_out, P, scopes, k, out, counts, frame_counts);
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (int rc0 = check_mix(e, channels, rate_in, rate_out)) return rc0;
  // the cheap arguments first, in search_ranked's order: an argument error does no device work
  if (nq < 0 || !out || !counts) return fail(e, TFP_E_ARG, "ranked search: bad query count or NULL output");
  if (int rc0 = check_k(e, "ranked search", k)) return rc0;
  if (int rc0 = check_params(e, "ranked search", P)) return rc0;
  if (nq && !scopes) return fail(e, TFP_E_ARG, "scoped search: scopes is NULL");
  if (int rc0 = check_scopes(e, "scoped search", scopes, nq, "query")) return rc0;
  MixSrc ms;
  std::vector<int64_t> out_off;
  if (int rc = mix_source(e, pcm, offsets, nq, channels, rate_in, rate_out, &ms, &out_off)) return rc;
  QuerySrc src{ms.pcm, out_off.data(), rate_out, true};
  src.mix = &ms;
  if (int rc = search_ranked(e, src, nq, P, k, out, counts, nullptr, true, scopes)) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) frame_counts[i] = (int32_t)tfp_frame_count(out_off[i + 1] - out_off[i]);
  return TFP_OK;
}

int tfp_resample_mix_stats(tfp_engine* e, int64_t* launches, int64_t* frames_in, int64_t* samples_out,
                           int64_t* staged_launches) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (launches) *launches = e->n_mix_launch;
  if (frames_in) *frames_in = e->n_mix_in;
  if (samples_out) *samples_out = e->n_mix_out;
  if (staged_launches) *staged_launches = e->n_mix_staged;
  return TFP_OK;
}

// ---- rate-normalised ingest of 24/32-bit and float audio (tfp_resample.hpp, "the wide form") ----
namespace {
// The source of a batch of interleaved int32 Q31 frames: mix_source's checks, table and offsets, the range
// the wide accumulator needs of the pair (A C < 2^30), and the frames in place of the int16 samples.
int wide_source(tfp_engine* e, const int32_t* q31, const int64_t* offsets, int32_t n, int32_t channels, int32_t rate_in,
                int32_t rate_out, MixSrc* ms, std::vector<int64_t>* out_off) {
  if (int rc = mix_source(e, nullptr, offsets, n, channels, rate_in, rate_out, ms, out_off)) return rc;
  if (ms->tab && !resample_wide_in_range(*ms->tab, channels))
    return fail(e, TFP_E_ARG, "unsupported rate ratio %d -> %d for %d wide channels", rate_in, rate_out, channels);
  if (ms->in_off[std::max(n, 0)] > INT64_MAX / (4 * (int64_t)channels))
    return fail(e, TFP_E_ARG, "%lld frames past the index range", (long long)ms->in_off[std::max(n, 0)]);
  ms->q31 = q31 && n > 0 ? q31 + offsets[0] * channels : q31;
  return TFP_OK;
}
}  // namespace

// The twins of the mix forms over int32 Q31 frames. One channel is a form of its own here (the samples are
// not the rate forms' int16), and so are equal rates (a rounding and a clamp). Not coalesced.
int tfp_fingerprint_wide_rate_batch(tfp_engine* e, const int32_t* q31, const int64_t* offsets, int32_t nclips,
                                    int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                    int64_t* nframes) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (int rc = check_mix(e, channels, rate_in, rate_out)) return rc;
  if (!offsets || nclips < 0 || !nframes || (!q31 && nclips && offsets[nclips] > offsets[0]))
    return fail(e, TFP_E_ARG, "bad arguments");
  HIPCHK(e, hipSetDevice(e->device));
  MixSrc ms;
  std::vector<int64_t> out_off;
  if (int rc = wide_source(e, q31, offsets, nclips, channels, rate_in, rate_out, &ms, &out_off)) return rc;
  const int64_t need = sample_frame_offsets(out_off.data(), nclips)[nclips];
  *nframes = need;
  if (need > 0 && (!out || cap < need)) return fail(e, TFP_E_CAPACITY, "need %lld frames", (long long)need);
  if (need == 0) return TFP_OK;
  std::vector<int64_t> lens(nclips), foff;
  for (int32_t c = 0; c < nclips; c++) lens[c] = out_off[c + 1] - out_off[c];
  int64_t nf;
  if (int rc = fingerprint_host(e, nullptr, lens.data(), false, nclips, rate_out, &nf, &foff, true, nullptr, nullptr, &ms))
    return rc;
  return copy_frames_out(e, nf, foff, out);
}

int tfp_search_wide_rate_batch(tfp_engine* e, const int32_t* q31, const int64_t* offsets, int32_t nq, int32_t channels,
                               int32_t rate_in, int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (int rc = check_mix(e, channels, rate_in, rate_out)) return rc;
  if (!offsets || nq < 0 || !out) return TFP_E_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  MixSrc ms;
  std::vector<int64_t> out_off;
  if (int rc = wide_source(e, q31, offsets, nq, channels, rate_in, rate_out, &ms, &out_off)) return rc;
  if (!q31 && nq && offsets[nq] > offsets[0]) return fail(e, TFP_E_ARG, "samples are NULL");
  std::vector<int64_t> lens(nq);
  for (int32_t i = 0; i < nq; i++) lens[i] = out_off[i + 1] - out_off[i];
  return search_gather_impl(e, nullptr, lens.data(), nq, false, rate_out, P, out, nullptr, nullptr, &ms);
}

int tfp_search_scoped_wide_rate_batch(tfp_engine* e, const int32_t* q31, const int64_t* offsets, int32_t nq, int32_t channels,
                                      int32_t rate_in, int32_t rate_out, const tfp_search_params* P, const int32_t* scopes,
                                      int32_t k, tfp_candidate* out, int32_t* counts, int32_t* frame_counts) {
  if (!e || !offsets) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (int rc0 = check_mix(e, channels, rate_in, rate_out)) return rc0;
  // the cheap arguments first, in search_ranked's order: an argument error does no device work
  if (nq < 0 || !out || !counts) return fail(e, TFP_E_ARG, "ranked search: bad query count or NULL output");
  if (int rc0 = check_k(e, "ranked search", k)) return rc0;
  if (int rc0 = check_params(e, "ranked search", P)) return rc0;
  if (nq && !scopes) return fail(e, TFP_E_ARG, "scoped search: scopes is NULL");
  if (int rc0 = check_scopes(e, "scoped search", scopes, nq, "query")) return rc0;
  HIPCHK(e, hipSetDevice(e->device));
  MixSrc ms;
  std::vector<int64_t> out_off;
  if (int rc = wide_source(e, q31, offsets, nq, channels, rate_in, rate_out, &ms, &out_off)) return rc;
  QuerySrc src{ms.q31, out_off.data(), rate_out, true};
  src.mix = &ms;
  if (int rc = search_ranked(e, src, nq, P, k, out, counts, nullptr, true, scopes)) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) frame_counts[i] = (int32_t)tfp_frame_count(out_off[i + 1] - out_off[i]);
  return TFP_OK;
}

int tfp_resample_wide_stats(tfp_engine* e, int64_t* launches, int64_t* frames_in, int64_t* samples_out,
                            int64_t* staged_launches) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (launches) *launches = e->n_wide_launch;
  if (frames_in) *frames_in = e->n_wide_in;
  if (samples_out) *samples_out = e->n_wide_out;
  if (staged_launches) *staged_launches = e->n_wide_staged;
  return TFP_OK;
}

// ---- mixed batches: clips of any rate, channel count and sample kind (tfp_resample_any.hpp) ----
namespace {
// The source of a mixed batch: any_prepare's rules (nothing touches the device before they pass), then the
// call's plans' tables laid end to end on the device, kept from the last call while the plans are the same.
int any_source(tfp_engine* e, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t n, int32_t rate_out,
               AnyBatch* B, AnySrc* as) {
  std::string err;
  if (!any_prepare(clips, n, nbytes, rate_out, resample_table, B, &err)) return fail(e, TFP_E_ARG, "%s", err.c_str());
  if (!data && B->in_off[(size_t)n] > 0) return fail(e, TFP_E_ARG, "samples are NULL");
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<std::pair<int32_t, int32_t>> key;
  for (const AnyPlanDev& p : B->plans) key.emplace_back(p.P.M, p.P.L);
  if (!key.empty() && key != e->any_taps_key) {
    std::vector<int16_t> all((size_t)B->taps_total);
    for (size_t i = 0; i < B->plans.size(); i++)
      std::copy(B->tables[i]->taps.begin(), B->tables[i]->taps.end(), all.begin() + B->plans[i].taps_off);
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (no launch of an earlier call reads the old tables any more)
    e->any_taps_key.clear();
    if (int rc = upload(e, e->any_taps, all.data(), sizeof(int16_t) * all.size())) return rc;
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (all is released on return)
    e->any_taps_key = key;
  }
  as->data = data;
  as->nbytes = nbytes;
  as->B = B;
  as->d_taps = key.empty() ? nullptr : e->any_taps.as<int16_t>();
  return TFP_OK;
}
}  // namespace

int tfp_fingerprint_any_batch(tfp_engine* e, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nclips,
                              int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!nframes) return fail(e, TFP_E_ARG, "bad arguments");
  AnyBatch B;
  AnySrc as;
  if (int rc = any_source(e, data, nbytes, clips, nclips, rate_out, &B, &as)) return rc;
  const int64_t need = sample_frame_offsets(B.out_off.data(), nclips)[nclips];
  *nframes = need;
  if (need > 0 && (!out || cap < need)) return fail(e, TFP_E_CAPACITY, "need %lld frames", (long long)need);
  if (need == 0) return TFP_OK;
  std::vector<int64_t> lens(nclips), foff;
  for (int32_t c = 0; c < nclips; c++) lens[c] = B.clips[c].n_out;
  int64_t nf;
  if (int rc = fingerprint_host(e, nullptr, lens.data(), false, nclips, rate_out, &nf, &foff, true, nullptr, nullptr, nullptr, &as))
    return rc;
  return copy_frames_out(e, nf, foff, out);
}

int tfp_search_any_batch(tfp_engine* e, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nq,
                         int32_t rate_out, const tfp_search_params* P, tfp_result* out) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!out) return fail(e, TFP_E_ARG, "bad arguments");
  AnyBatch B;
  AnySrc as;
  if (int rc = any_source(e, data, nbytes, clips, nq, rate_out, &B, &as)) return rc;
  std::vector<int64_t> lens(nq);
  for (int32_t i = 0; i < nq; i++) lens[i] = B.clips[i].n_out;
  return search_gather_impl(e, nullptr, lens.data(), nq, false, rate_out, P, out, nullptr, nullptr, nullptr, &as);
}

int tfp_search_scoped_any_batch(tfp_engine* e, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nq,
                                int32_t rate_out, const tfp_search_params* P, const int32_t* scopes, int32_t k,
                                tfp_candidate* out, int32_t* counts, int32_t* frame_counts) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  // the cheap arguments first, in search_ranked's order: an argument error does no device work
  if (nq < 0 || !out || !counts) return fail(e, TFP_E_ARG, "ranked search: bad query count or NULL output");
  if (int rc0 = check_k(e, "ranked search", k)) return rc0;
  if (int rc0 = check_params(e, "ranked search", P)) return rc0;
  if (nq && !scopes) return fail(e, TFP_E_ARG, "scoped search: scopes is NULL");
  if (int rc0 = check_scopes(e, "scoped search", scopes, nq, "query")) return rc0;
  AnyBatch B;
  AnySrc as;
  if (int rc = any_source(e, data, nbytes, clips, nq, rate_out, &B, &as)) return rc;
  QuerySrc src{data, B.out_off.data(), rate_out, true};
  src.any = &as;
  if (int rc = search_ranked(e, src, nq, P, k, out, counts, nullptr, true, scopes)) return rc;
  for (int32_t i = 0; frame_counts && i < nq; i++) frame_counts[i] = (int32_t)tfp_frame_count(B.clips[i].n_out);
  return TFP_OK;
}

int tfp_resample_any_stats(tfp_engine* e, int64_t* launches, int64_t* clips, int64_t* frames_in, int64_t* samples_out,
                           int64_t* tiles_staged, int64_t* tiles_global, int64_t* tiles_plain) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (launches) *launches = e->n_any_launch;
  if (clips) *clips = e->n_any_clips;
  if (frames_in) *frames_in = e->n_any_in;
  if (samples_out) *samples_out = e->n_any_out;
  if (tiles_staged) *tiles_staged = e->n_any_staged;
  if (tiles_global) *tiles_global = e->n_any_global;
  if (tiles_plain) *tiles_plain = e->n_any_plain;
  return TFP_OK;
}

int tfp_search_pcm_gather(tfp_engine* e, const int16_t* const* pcms, const int64_t* nsamples, int32_t nq, int32_t sr,
                          const tfp_search_params* P, tfp_result* out) {
  return search_gather_entry(e, reinterpret_cast<const void* const*>(pcms), nsamples, nq, false, sr, P, out);
}

int tfp_sweep_stats(tfp_engine* e, int64_t* bins, int64_t* library, int64_t* redone, int64_t* crowd_bins) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (bins) *bins = e->n_sweep_bins;
  if (library) *library = e->n_sweep_lib;
  if (redone) *redone = e->n_sweep_redo;
  if (crowd_bins) *crowd_bins = e->n_sweep_crowd;
  return TFP_OK;
}

int tfp_search_path_stats(tfp_engine* e, int64_t* small, int64_t* vote_class, int64_t* vote_gemm, int64_t* vote_redone,
                          int64_t* general) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (small) *small = e->n_path_small;
  if (vote_class) *vote_class = e->n_path_class;
  if (vote_gemm) *vote_gemm = e->n_path_gemm;
  if (vote_redone) *vote_redone = e->n_path_redone;
  if (general) *general = e->n_path_general;
  return TFP_OK;
}

int tfp_index_cache_stats(tfp_engine* e, int64_t* cache_builds, int64_t* cache_hits, int64_t* from_order,
                          int64_t* order_builds, int64_t* order_merges, int64_t* delta_cache_builds,
                          int64_t* delta_sweeps) {
  if (!e) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (cache_builds) *cache_builds = e->tc.n_builds;
  if (cache_hits) *cache_hits = e->tc.n_hits;
  if (from_order) *from_order = e->tc.n_from_order;
  if (order_builds) *order_builds = e->order.n_builds;
  if (order_merges) *order_merges = e->order.n_merges;
  if (delta_cache_builds) *delta_cache_builds = e->tc.n_delta_builds;
  if (delta_sweeps) *delta_sweeps = e->tc.n_delta_sweeps;
  return TFP_OK;
}

int64_t tfp_internal_delta_main_keys(tfp_engine* e) { return e ? e->n_delta_main_keys : 0; }
const char* tfp_internal_engine_own_error(tfp_engine* e) { return e ? e->err.own() : nullptr; }
void tfp_internal_engine_clear_error(tfp_engine* e) {
  if (e) e->err.clear_own();
}

int tfp_search_coalesce_stats(tfp_engine* e, int64_t* calls, int64_t* batches) {
  if (!e) return TFP_E_ARG;
  e->coal.stats(calls, batches);
  return TFP_OK;
}

// (internal, tfp_internal.hpp) the device group's per-shard search: already coalesced by the group
int tfp_internal_search_gather(tfp_engine* e, const void* const* ptrs, const int64_t* lens, int32_t nq, bool f32,
                               int32_t sr, const tfp_search_params* P, tfp_result* out) {
  if (!e || nq < 0 || !out || (nq && (!ptrs || !lens))) return TFP_E_ARG;
  return search_gather_impl(e, ptrs, lens, nq, f32, sr, P, out);
}

int tfp_search_device(tfp_engine* e, const tfp_plan* p, const int16_t* d_pcm, const tfp_search_params* P,
                      uint64_t* d_keys, void* stream) {
  if (!e || !p || !d_keys || !valid_params(P)) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  NullStreamOrder order(e, stream);
  if (!order.ok()) return fail(e, TFP_E_HIP, "ordering after the null stream failed");
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  const DspTables* T;
  bool fx = false;
  int rc = ensure_tables(e, p->sample_rate, &T, &fx);
  if (rc) return rc;
  HIPCHK(e, e->micro.reserve(sizeof(int32_t) * 2 * (p->nframes + 1)));
  HIPCHK(e, e->db.reserve(sizeof(double) * 2 * (p->nframes + 1)));
  HIPCHK(e, launch_fingerprint(e->fpcfg, T, fx && !p->long_clip, p->tile_frames, d_pcm, p->d_soff.as<int64_t>(), p->d_soff.as<int64_t>() + 1,
                               p->d_foff.as<int64_t>(), p->d_toff.as<int32_t>(),
                               p->d_tclip.as<int32_t>(), p->ntiles, p->nframes, e->micro.as<int32_t>(),
                               e->db.as<double>(), s, P->coefs == 2 ? e->logfix : LogFix{}, &e->fpstats));
  std::vector<unsigned long long> keys;
  return search_core(e, p->foff.data(), p->nclips, e->db.as<double>(), P, keys,
                     reinterpret_cast<unsigned long long*>(d_keys), s);
}

int tfp_search_q_device(tfp_engine* e, const double* d_q, const int64_t* qoff, int32_t nq, const tfp_search_params* P,
                        uint64_t* d_keys, void* stream) {
  if (!e || !qoff || nq < 0 || !d_keys || !valid_params(P) || (!d_q && nq && qoff[nq] > qoff[0])) return TFP_E_ARG;
  for (int32_t i = 0; i < nq; i++)
    if (qoff[i + 1] < qoff[i]) return fail(e, TFP_E_ARG, "query offsets not monotone");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  NullStreamOrder order(e, stream);
  if (!order.ok()) return fail(e, TFP_E_HIP, "ordering after the null stream failed");
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  std::vector<unsigned long long> keys;
  return search_core(e, qoff, nq, d_q ? d_q + 2 * qoff[0] : d_q, P, keys, reinterpret_cast<unsigned long long*>(d_keys),
                     s);
}

// ---- streams ------------------------------------------------------------------------------

struct tfp_stream {
  tfp_engine* eng = nullptr;
  int32_t nch = 0, sr = 0;
  int64_t W = 0;                 // window samples
  int64_t wpos = 0;              // ring position of the oldest sample of every window
  std::vector<int64_t> filled;   // samples of history per channel (saturates at W)
  DevBuf ring;
  HostBuf stage_h;               // this tick's samples + window layout: mapped, coherent pinned memory
  void* stage_host = nullptr;    // the allocation stage_dev was taken for
  char* stage_dev = nullptr;     // its device address: the kernels read it in place (no upload)
  bool stage_pending = false;    // stage_h may still be read by the last tick's kernels
};

// ring[c][2W]: every sample is written at p and p + W, so the last W samples of a channel are
// always the contiguous run ring[c][wpos .. wpos + W).
__global__ void stream_scatter_kernel(const int16_t* __restrict__ tick, int32_t T, int64_t W, int64_t wpos,
                                      int32_t nch, int16_t* __restrict__ ring) {
  const int64_t n = (int64_t)nch * T;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i / T, t = i % T;
    int64_t p = wpos + t;
    if (p >= W) p -= W;
    const int16_t v = tick[i];
    ring[c * 2 * W + p] = v;
    ring[c * 2 * W + p + W] = v;
  }
}

int tfp_stream_create(tfp_engine* e, int32_t nch, int32_t sr, int64_t W, tfp_stream** out) {
  if (!e || nch <= 0 || W <= 0 || !out) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  const DspTables* T;
  int rc = ensure_tables(e, sr, &T);
  if (rc) return rc;
  tfp_stream* st = new tfp_stream();
  st->eng = e;
  st->nch = nch;
  st->sr = sr;
  st->W = W;
  st->filled.assign(nch, 0);
  if (st->ring.reserve(sizeof(int16_t) * 2 * W * nch) != hipSuccess) {
    delete st;
    return fail(e, TFP_E_NOMEM, "stream ring of %lld bytes", (long long)(4 * W * nch));
  }
  (void)hipMemsetAsync(st->ring.p, 0, sizeof(int16_t) * 2 * W * nch, e->stream);
  *out = st;
  return TFP_OK;
}

void tfp_stream_destroy(tfp_stream* st) {
  if (!st) return;
  {
    std::lock_guard<std::recursive_mutex> lk(st->eng->mu);
    (void)hipSetDevice(st->eng->device);
    (void)hipStreamSynchronize(st->eng->stream);  // the last tick's kernels may still read stage_h
  }
  delete st;
}

int tfp_stream_reset(tfp_stream* st, int32_t ch) {
  if (!st || ch >= st->nch) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(st->eng->mu);
  if (ch < 0) std::fill(st->filled.begin(), st->filled.end(), 0);
  else st->filled[ch] = 0;
  return TFP_OK;
}

// The windows ring[c][wpos .. wpos + W) of the channels `act`, staged for one fingerprint launch:
// the tile choice and, in the stream's mapped pinned buffer (read in place by the kernels), room
// for pcm_bytes of a tick's samples followed by the windows' layout (sbeg, send, foff, toff, tclip).
struct StreamWindows {
  const DspTables* tables = nullptr;
  bool fx = false;
  int32_t tile = 0, ntiles = 0;
  int64_t nframes = 0;
  char* h = nullptr;        // the staging buffer (host view): the tick's samples go to its start
  const char* d = nullptr;  // ... and its device view
  size_t o_sb = 0, o_se = 0, o_fo = 0, o_to = 0, o_tc = 0;  // byte offsets of the layout arrays
};

// Stages the layout of the windows of `act` (in that order, window i's frames at [i F, (i + 1) F))
// at ring position wpos. An upload and its hand-off to the first kernel cost ~16 us a tick, hence
// the mapped buffer; the previous launch's kernels must be done reading it. Caller holds e->mu.
static int stream_stage_windows(tfp_stream* st, size_t pcm_bytes, const std::vector<int32_t>& act, int64_t wpos,
                                StreamWindows* w, std::vector<int64_t>& fov) {
  tfp_engine* e = st->eng;
  int rc;
  if ((rc = ensure_tables(e, st->sr, &w->tables, &w->fx))) return rc;
  const int32_t na = (int32_t)act.size();
  const int64_t F = tfp_frame_count(st->W);
  w->tile = fp_tile_frames(e->fpcfg, w->fx, false, false);
  const int32_t tiles = (int32_t)((F + w->tile - 1) / w->tile);
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_pcm = al(pcm_bytes), b_sb = al(sizeof(int64_t) * na), b_fo = al(sizeof(int64_t) * (na + 1)),
               b_to = al(sizeof(int32_t) * (na + 1)), b_tc = al(sizeof(int32_t) * (size_t)na * tiles);
  const size_t total = b_pcm + 2 * b_sb + b_fo + b_to + b_tc;
  if (st->stage_pending) HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, st->stage_h.reserve(total, hipHostMallocMapped | hipHostMallocCoherent));
  if (st->stage_h.p != st->stage_host) {
    HIPCHK(e, hipHostGetDevicePointer(reinterpret_cast<void**>(&st->stage_dev), st->stage_h.p, 0));
    st->stage_host = st->stage_h.p;
  }
  w->h = st->stage_h.as<char>();
  w->d = st->stage_dev;
  w->o_sb = b_pcm;
  w->o_se = w->o_sb + b_sb;
  w->o_fo = w->o_se + b_sb;
  w->o_to = w->o_fo + b_fo;
  w->o_tc = w->o_to + b_to;
  int64_t* sb = reinterpret_cast<int64_t*>(w->h + w->o_sb);
  int64_t* se = reinterpret_cast<int64_t*>(w->h + w->o_se);
  int64_t* fo = reinterpret_cast<int64_t*>(w->h + w->o_fo);
  int32_t* to = reinterpret_cast<int32_t*>(w->h + w->o_to);
  int32_t* tc = reinterpret_cast<int32_t*>(w->h + w->o_tc);
  for (int32_t i = 0; i < na; i++) {
    sb[i] = (int64_t)act[i] * 2 * st->W + wpos;
    se[i] = sb[i] + st->W;
    fo[i] = (int64_t)i * F;
    to[i] = i * tiles;
    for (int32_t t = 0; t < tiles; t++) tc[(size_t)i * tiles + t] = i;
  }
  fo[na] = (int64_t)na * F;
  to[na] = na * tiles;
  w->ntiles = to[na];
  w->nframes = fo[na];
  st->stage_pending = true;
  fov.assign(fo, fo + na + 1);  // (the pinned buffer is rewritten by the next staging)
  return TFP_OK;
}

// Fingerprints the staged windows in place in the ring: micro-units into the engine's buffer, frame
// values into d_db (nullptr: the engine's buffer), corrected by lf (LogFix{}: truncation-exact only).
static int stream_fingerprint_windows(tfp_stream* st, const StreamWindows& w, double* d_db, const LogFix& lf) {
  tfp_engine* e = st->eng;
  if (!w.ntiles) return TFP_OK;
  HIPCHK(e, e->micro.reserve(sizeof(int32_t) * 2 * (w.nframes + 1)));
  if (!d_db) HIPCHK(e, e->db.reserve(sizeof(double) * 2 * (w.nframes + 1)));
  HIPCHK(e, launch_fingerprint(e->fpcfg, w.tables, w.fx, w.tile, st->ring.as<int16_t>(),
                               reinterpret_cast<const int64_t*>(w.d + w.o_sb),
                               reinterpret_cast<const int64_t*>(w.d + w.o_se),
                               reinterpret_cast<const int64_t*>(w.d + w.o_fo),
                               reinterpret_cast<const int32_t*>(w.d + w.o_to),
                               reinterpret_cast<const int32_t*>(w.d + w.o_tc), w.ntiles, w.nframes,
                               e->micro.as<int32_t>(), d_db ? d_db : e->db.as<double>(), e->stream, lf, &e->fpstats));
  return TFP_OK;
}

// One tick into a stream: the samples into the ring, then (match) the windows that are full after
// it fingerprinted into d_db (frame values, 2 doubles per frame; nullptr: the engine's buffer) at
// window i's frames [i F, (i + 1) F). act = their channels, in channel order. Caller holds e->mu.
// law < 0: pcm is int16[nch][T]; else G.711 codes uint8[nch][T] of that law, expanded by the scatter
// itself on their way into the ring (the ring is int16 either way; no extra pass or launch).
static int stream_tick(tfp_stream* st, const void* pcm, int32_t law, int32_t T, const tfp_search_params* P, double* d_db,
                       int64_t cap_frames, std::vector<int32_t>& act, int64_t* F_out, std::vector<int64_t>& fov) {
  const bool match = P && valid_params(P);
  tfp_engine* e = st->eng;
  HIPCHK(e, hipSetDevice(e->device));
  int rc;
  // Windows to match after this tick: the channels whose history is full once it is in.
  const int64_t wpos = (st->wpos + T) % st->W;
  act.clear();
  if (match)
    for (int32_t c = 0; c < st->nch; c++)
      if (std::min<int64_t>(st->W, st->filled[c] + T) >= st->W) act.push_back(c);
  const int32_t na = (int32_t)act.size();
  const int64_t F = tfp_frame_count(st->W);
  *F_out = F;
  if (d_db && (int64_t)na * F > cap_frames) return fail(e, TFP_E_ARG, "stream tick: %d windows of %lld frames past %lld", na,
                                                        (long long)F, (long long)cap_frames);
  // One mapped pinned buffer per tick: the tick's samples, then the windows' layout.
  const size_t pcm_bytes = (law < 0 ? sizeof(int16_t) : sizeof(uint8_t)) * (size_t)st->nch * T;
  StreamWindows w;
  if ((rc = stream_stage_windows(st, pcm_bytes, act, wpos, &w, fov))) return rc;
  memcpy(w.h, pcm, pcm_bytes);
  if (law < 0) {
    hipLaunchKernelGGL(stream_scatter_kernel, dim3(1024), dim3(256), 0, e->stream, reinterpret_cast<const int16_t*>(w.d), T,
                       st->W, st->wpos, st->nch, st->ring.as<int16_t>());
    HIPCHK(e, hipGetLastError());
  } else {
    HIPCHK(e, launch_stream_scatter_g711(reinterpret_cast<const uint8_t*>(w.d), T, st->W, st->wpos, st->nch, law,
                                         st->ring.as<int16_t>(), e->stream));
    e->n_g711_stream++;
    e->n_g711_codes += (int64_t)st->nch * T;
  }
  st->wpos = wpos;
  for (auto& f : st->filled) f = std::min<int64_t>(st->W, f + T);
  if (!na) return TFP_OK;
  return stream_fingerprint_windows(st, w, d_db, P->coefs == 2 ? e->logfix : LogFix{});
}

// tfp_stream_push (law < 0, int16 samples) and tfp_stream_push_g711 (codes of that law).
static int stream_push_impl(tfp_stream* st, const void* pcm, int32_t law, int32_t T, const tfp_search_params* P,
                            tfp_result* out) {
  if (!st || !pcm || T <= 0 || T > st->W || (P && !out)) return TFP_E_ARG;
  tfp_engine* e = st->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const bool match = P && valid_params(P);  // fp_handler.c:247-250: bad params -> NULL results
  std::vector<int32_t> act;
  std::vector<int64_t> fov;
  int64_t F = 0;
  int rc = stream_tick(st, pcm, law, T, P, nullptr, 0, act, &F, fov);
  if (rc) return rc;
  if (!P) return TFP_OK;
  for (int32_t c = 0; c < st->nch; c++) {
    memset(&out[c], 0, sizeof out[c]);
    out[c].clip_id = -1;
  }
  const int32_t na = (int32_t)act.size();
  if (!match || !na) return TFP_OK;  // full windows only
  std::vector<unsigned long long> keys;
  if ((rc = search_core(e, fov.data(), na, e->db.as<double>(), P, keys, nullptr, e->stream))) return rc;
  st->stage_pending = false;  // search_core waited for e->stream
  std::vector<tfp_result> res(na);
  fill_results(e, keys, fov.data(), na, res.data());
  for (int32_t i = 0; i < na; i++) out[act[i]] = res[i];
  return TFP_OK;
}

int tfp_stream_push(tfp_stream* st, const int16_t* pcm, int32_t T, const tfp_search_params* P, tfp_result* out) {
  return stream_push_impl(st, pcm, -1, T, P, out);
}

int tfp_stream_push_g711(tfp_stream* st, const uint8_t* codes, int32_t T, int32_t law, const tfp_search_params* P,
                         tfp_result* out) {
  if (!st) return TFP_E_ARG;
  if (!g711_law_ok(law)) return fail(st->eng, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  return stream_push_impl(st, codes, law, T, P, out);
}

int tfp_internal_stream_fp(tfp_stream* st, const void* pcm, int32_t law, int32_t T, const tfp_search_params* P, double* d_db,
                           int64_t cap_frames, int32_t* act, int32_t* nact, int64_t* frames_per_window) {
  const bool match = P && valid_params(P);
  if (!st || !pcm || T <= 0 || T > st->W || !nact || !frames_per_window || (match && (!d_db || !act)) ||
      (law >= 0 && !g711_law_ok(law)))
    return TFP_E_ARG;
  tfp_engine* e = st->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  std::vector<int32_t> a;
  std::vector<int64_t> fov;
  int rc = stream_tick(st, pcm, law, T, P, d_db, cap_frames, a, frames_per_window, fov);
  if (rc) return rc;
  HIPCHK(e, hipStreamSynchronize(e->stream));  // the values are read by other devices' streams next
  st->stage_pending = false;
  *nact = (int32_t)a.size();
  if (match) std::copy(a.begin(), a.end(), act);
  return TFP_OK;
}

int tfp_stream_window_frames(tfp_stream* st, int32_t ch, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!st || ch < 0 || ch >= st->nch || !nframes) return TFP_E_ARG;
  tfp_engine* e = st->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  *nframes = 0;
  if (st->filled[ch] < st->W) return TFP_OK;  // no full window yet
  const int64_t F = tfp_frame_count(st->W);
  *nframes = F;
  if (!out || cap < F) return fail(e, TFP_E_ARG, "stream window: %lld frames past %lld", (long long)F, (long long)cap);
  HIPCHK(e, hipSetDevice(e->device));
  // the window where it lies in the ring, by stream_tick's own staging and launch (exact q values)
  const std::vector<int32_t> act(1, ch);
  std::vector<int64_t> fov;
  StreamWindows w;
  int rc = stream_stage_windows(st, 0, act, st->wpos, &w, fov);
  if (rc) return rc;
  if ((rc = stream_fingerprint_windows(st, w, nullptr, e->logfix))) return rc;
  if ((rc = copy_frames_out(e, F, fov, out))) return rc;
  st->stage_pending = false;  // copy_frames_out waited for e->stream
  return TFP_OK;
}

// ---- live calls (tfp_live.hpp) -------------------------------------------------------------

struct tfp_live {
  tfp_engine* eng = nullptr;
  int32_t nch = 0, sr = 0;
  int64_t max_samples = 0, Fmax = 0;  // Fmax: frames of a full history
  std::vector<int64_t> samples;       // per channel: samples since its last reset
  std::vector<int64_t> added;         // ... and final frames its count row holds
  DevBuf hist, q, counts, bad, dstage, part, keys, gq, gfoff;
  int64_t count_cols = 0;             // the row width counts is laid out for (live_count_cols), 0: none yet
  HostBuf stage_h, keys_pin;          // a push's tick + descriptors; the rows' keys and the bad flag read back
  hipEvent_t stage_ev = nullptr;      // the upload of stage_h
  bool stage_pending = false;
  // what the count table was built for: any index update, the resolved tolerance, both ignore thresholds
  bool stamp_valid = false;
  uint64_t stamp_version = 0;
  SearchConsts stamp_sc{};
  int64_t n_incremental = 0, n_general = 0, n_rebuilds = 0, n_fp_frames = 0, n_added = 0;
  // a verdict's candidate table and the columns' staged rows it was built from; cand_builds: the
  // engine's scope-table build it follows (-1: none yet)
  DevBuf cand, cand_rows;
  int64_t cand_builds = -1;
  // the trailing window (tfp_live_window): a second count table in the layout of counts, allocated by the
  // first window call; per channel the final frames [wbeg, wend) its row holds (empty: the row is zero);
  // a stamp of its own, counts' fields plus the window length
  DevBuf wcounts, wbad;
  int64_t wcount_cols = 0;
  std::vector<int64_t> wbeg, wend;
  bool wstamp_valid = false;
  uint64_t wstamp_version = 0;
  SearchConsts wstamp_sc{};
  int64_t wstamp_window = 0;
  int64_t n_wslid = 0, n_wgeneral = 0, n_wrebuilds = 0, n_wadded = 0, n_wremoved = 0, n_wrestarted = 0;
  // the aligned window (tfp_live_window_aligned), allocated by its first call and grown as needed: the
  // rows' columns, the window frames' boxes [nchannels][stride], the pairs, launch_align's partial
  // keys, and the results ([keys][bad flag][AlignOut], one read-back into wa_pin); the longest live
  // clip's row count, per index version
  DevBuf wa_cols, wa_boxes, wa_pairs, wa_part, wa_res, wa_wchan;
  HostBuf wa_pin;
  bool wa_nmax_valid = false;
  uint64_t wa_nmax_version = 0;
  int64_t wa_nmax = 0;
  int64_t n_wa_inplace = 0, n_wa_general = 0, n_wa_pairs = 0;
  // the carried traces (tfp_live_occurrences): per channel its list of tracks, track i's summary in
  // slot c * kLiveTracksMax + i of tr_segs (allocated by the first occurrence call); a stamp of its
  // own, counts' fields plus coefs and max_gap
  struct Track {
    int32_t clip = -1;
    std::string uuid;       // the clip's, checked with the id (tfp_index_clear starts the ids again)
    int32_t s = 0, windows = 0;
    int64_t done = 0;       // the stored summary covers the final frames [lo, done) of the span
    bool stored = false;    // the slot holds that summary (else the next step restarts it)
    bool last_tail = false; // `last` has a tail frame's hit joined in
    TraceOut last{0, 0, 0, 0, 0, 0};
  };
  std::vector<std::vector<Track>> tracks;
  DevBuf tr_segs, tr_desc, tr_out;
  HostBuf tr_pin;
  bool tr_stamp_valid = false;
  uint64_t tr_stamp_version = 0;
  SearchConsts tr_stamp_sc{};
  int32_t tr_stamp_gap = 0;
  int64_t n_occ_calls = 0, n_tr_added = 0, n_tr_dropped = 0, n_tr_frames = 0, n_tr_retraces = 0;
  // a rate object (tfp_live_create_rate, tfp_live_rate.hpp): the ticks arrive at rate_in and are converted
  // into hist; `samples` is then the settled count. Per channel the input samples since its last reset and
  // the carry side its next push reads; carry: int16 [2][nch][ntaps - 1] (never cleared: a sample below
  // index 0 is never read from it)
  bool rated = false;
  int32_t rate_in = 0, rs_tile = 0;
  ResamplePlan rs_plan{};
  const int16_t* rs_taps = nullptr;  // the engine's device table of the pair (kept for its lifetime)
  std::vector<int64_t> in_samples;
  std::vector<int32_t> parity;
  DevBuf carry;
  int64_t n_rt_launch = 0, n_rt_in = 0, n_rt_out = 0;  // tfp_live_rate_stats
  ~tfp_live() {
    if (stage_ev) (void)hipEventDestroy(stage_ev);
  }
};

int tfp_live_create(tfp_engine* e, int32_t nch, int32_t sr, int64_t max_samples, tfp_live** out) {
  return tfp_live_create_rate(e, nch, sr, sr, max_samples, out);
}

int tfp_live_create_rate(tfp_engine* e, int32_t nch, int32_t rate_in, int32_t sr, int64_t max_samples, tfp_live** out) {
  if (!e || !out) return TFP_E_ARG;
  *out = nullptr;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  ResamplePlan rs_plan{};
  if (rate_in != sr) {
    if (rate_in < 1 || sr < 1) return fail(e, TFP_E_ARG, "bad sample rate %d", rate_in < 1 ? rate_in : sr);
    bool bad = false;
    if (!resample_plan(rate_in, sr, &rs_plan, &bad) || !live_rate_supported(rs_plan))
      return fail(e, TFP_E_ARG, "unsupported rate ratio %d -> %d", rate_in, sr);
  }
  if (nch <= 0 || nch > 65535) return fail(e, TFP_E_ARG, "live calls: %d channels outside [1, 65535]", nch);
  if (!live_capacity_ok(max_samples))
    return fail(e, TFP_E_ARG, "live calls: max_samples %lld outside [1, %lld]", (long long)max_samples,
                (long long)kLiveMaxSamples);
  HIPCHK(e, hipSetDevice(e->device));
  const DspTables* T;
  int rc = ensure_tables(e, sr, &T);
  if (rc) return rc;
  std::unique_ptr<tfp_live> lv(new tfp_live());
  lv->eng = e;
  lv->nch = nch;
  lv->sr = sr;
  lv->max_samples = max_samples;
  lv->Fmax = live_frames(max_samples);
  lv->samples.assign(nch, 0);
  lv->added.assign(nch, 0);
  lv->wbeg.assign(nch, 0);
  lv->wend.assign(nch, 0);
  lv->tracks.assign(nch, {});
  if (rate_in != sr) {
    const tfp_engine::RsTable* tab;
    if ((rc = ensure_rs_table(e, rs_plan, rate_in, sr, &tab))) return rc;
    lv->rated = true;
    lv->rate_in = rate_in;
    lv->rs_plan = rs_plan;
    lv->rs_tile = live_rate_tile(rs_plan);
    lv->rs_taps = tab->dev.as<int16_t>();
    lv->in_samples.assign(nch, 0);
    lv->parity.assign(nch, 0);
    if (lv->carry.reserve(sizeof(int16_t) * 2 * (size_t)nch * (rs_plan.ntaps - 1)) != hipSuccess)
      return fail(e, TFP_E_NOMEM, "live calls: the carried input of %d channels", nch);
  }
  // (neither needs clearing: a push reads only samples and frame values that a push has written)
  if (lv->hist.reserve(sizeof(int16_t) * (size_t)nch * max_samples) != hipSuccess ||
      lv->q.reserve(sizeof(double) * 2 * (size_t)nch * lv->Fmax) != hipSuccess ||
      lv->bad.reserve(sizeof(int32_t)) != hipSuccess)
    return fail(e, TFP_E_NOMEM, "live calls: %d channels of %lld samples", nch, (long long)max_samples);
  HIPCHK(e, hipMemsetAsync(lv->bad.p, 0, sizeof(int32_t), e->stream));
  HIPCHK(e, hipEventCreateWithFlags(&lv->stage_ev, hipEventDisableTiming));
  *out = lv.release();
  return TFP_OK;
}

void tfp_live_destroy(tfp_live* lv) {
  if (!lv) return;
  {
    std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
    (void)hipSetDevice(lv->eng->device);
    (void)hipStreamSynchronize(lv->eng->stream);  // the last push's kernels and copies
  }
  delete lv;
}

int tfp_live_reset(tfp_live* lv, int32_t ch) {
  if (!lv || ch >= lv->nch) return TFP_E_ARG;
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  const int32_t c0 = ch < 0 ? 0 : ch, c1 = ch < 0 ? lv->nch : ch + 1;
  if (lv->count_cols)  // a new call starts with an empty count row
    HIPCHK(e, hipMemsetAsync(lv->counts.as<uint16_t>() + (size_t)c0 * lv->count_cols, 0,
                             sizeof(uint16_t) * (size_t)(c1 - c0) * lv->count_cols, e->stream));
  if (lv->wcount_cols)  // ... and with an empty window row
    HIPCHK(e, hipMemsetAsync(lv->wcounts.as<uint16_t>() + (size_t)c0 * lv->wcount_cols, 0,
                             sizeof(uint16_t) * (size_t)(c1 - c0) * lv->wcount_cols, e->stream));
  for (int32_t c = c0; c < c1; c++) {
    lv->samples[c] = lv->added[c] = 0;
    if (lv->rated) lv->in_samples[c] = 0;  // (the carry stays: a sample below index 0 is never read from it)
    lv->n_wremoved += lv->wend[c] - lv->wbeg[c];
    lv->wbeg[c] = lv->wend[c] = 0;
    lv->tracks[c].clear();  // a new call starts with an empty log
  }
  return TFP_OK;
}

int tfp_live_samples(tfp_live* lv, int32_t ch, int64_t* nsamples) {
  if (!lv || ch < 0 || ch >= lv->nch || !nsamples) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  *nsamples = lv->samples[ch];
  return TFP_OK;
}

int tfp_live_input_samples(tfp_live* lv, int32_t ch, int64_t* nsamples) {
  if (!lv || ch < 0 || ch >= lv->nch || !nsamples) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  *nsamples = lv->rated ? lv->in_samples[ch] : lv->samples[ch];
  return TFP_OK;
}

int tfp_live_rate_info(tfp_live* lv, int32_t* rate_in, int64_t* lag_in) {
  if (!lv) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  if (rate_in) *rate_in = lv->rated ? lv->rate_in : lv->sr;
  if (lag_in) *lag_in = lv->rated ? live_rate_lag(lv->rs_plan) : 0;
  return TFP_OK;
}

int tfp_live_rate_stats(tfp_live* lv, int64_t* launches, int64_t* samples_in, int64_t* samples_out) {
  if (!lv) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  if (launches) *launches = lv->n_rt_launch;
  if (samples_in) *samples_in = lv->n_rt_in;
  if (samples_out) *samples_out = lv->n_rt_out;
  return TFP_OK;
}

int tfp_live_stats(tfp_live* lv, int64_t* incremental_pushes, int64_t* general_pushes, int64_t* rebuilds,
                   int64_t* frames_fingerprinted, int64_t* frames_added) {
  if (!lv) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  if (incremental_pushes) *incremental_pushes = lv->n_incremental;
  if (general_pushes) *general_pushes = lv->n_general;
  if (rebuilds) *rebuilds = lv->n_rebuilds;
  if (frames_fingerprinted) *frames_fingerprinted = lv->n_fp_frames;
  if (frames_added) *frames_added = lv->n_added;
  return TFP_OK;
}

namespace {

bool live_stamp_holds(const tfp_live* lv, const SearchConsts& sc) {
  const SearchConsts& t = lv->stamp_sc;
  return lv->stamp_valid && lv->stamp_version == lv->eng->index_version && t.tole == sc.tole && t.has_low == sc.has_low &&
         t.has_high == sc.has_high && (!sc.has_low || t.thr_low == sc.thr_low) && (!sc.has_high || t.thr_high == sc.thr_high);
}

// The exact fallback: every channel's frames so far, the tail included, as one query of the scoped
// search core (which merges a live index delta where its form needs that). Caller holds e->mu and
// waits for the stream.
// window > 0 (tfp_live_window): each channel's trailing window [first, F) of them instead.
int live_general(tfp_live* lv, const tfp_search_params* P, const int32_t* scopes, int32_t K,
                 std::vector<unsigned long long>& keys, int64_t window = 0) {
  tfp_engine* e = lv->eng;
  const int32_t nch = lv->nch;
  std::vector<int64_t> foff(2 * (size_t)nch + 1, 0);  // the offsets, then the channels' first frames
  int64_t max_n = 0;
  for (int32_t c = 0; c < nch; c++) {
    const int64_t F = live_frames(lv->samples[c]), first = window > 0 && F > window ? F - window : 0;
    foff[c + 1] = foff[c] + (F - first);
    foff[nch + 1 + c] = first;
    max_n = std::max(max_n, F - first);
  }
  keys.assign((size_t)nch * K, 0ull);
  if (!foff[nch]) return TFP_OK;
  int rc = upload(e, lv->gfoff, foff.data(), sizeof(int64_t) * foff.size());
  if (rc) return rc;
  HIPCHK(e, lv->gq.reserve(sizeof(double) * 2 * (size_t)(foff[nch] + 1)));
  HIPCHK(e, launch_live_gather(lv->q.as<double>(), lv->Fmax, lv->gfoff.as<int64_t>(), lv->gfoff.as<int64_t>() + nch + 1, nch,
                               max_n, lv->gq.as<double>(), e->stream));
  return rank_core(e, foff.data(), nch, lv->gq.as<double>(), P, K, scopes, keys, e->stream);
}

// The verdict's candidate table (launch_live_candidates) for the current index and scopes: rebuilt
// when the scope table was (an index update or a scope change), else it stands. Caller holds e->mu and
// has run ensure_scope_table.
int ensure_live_candidates(tfp_live* lv, hipStream_t s) {
  tfp_engine* e = lv->eng;
  if (lv->cand_builds == e->n_scope_builds) return TFP_OK;
  const int32_t Cp = scope_table_cols(e->ncols);
  std::vector<LiveColRows> rows((size_t)std::max(Cp, 1), LiveColRows{0, 0});
  auto put = [&](size_t col, int32_t clip) {
    if (clip >= 0 && e->clips[clip].alive) rows[col] = LiveColRows{e->clips[clip].off, e->clips[clip].nrows};
  };
  for (size_t c = 0; c < e->col_clip.size(); c++) put(c, e->col_clip[c]);
  for (size_t j = 0; j < e->delta.clip.size(); j++) put((size_t)e->delta.col0 + j, e->delta.clip[j]);
  HIPCHK(e, lv->cand_rows.reserve(sizeof(LiveColRows) * rows.size()));
  HIPCHK(e, lv->cand.reserve(sizeof(int32_t) * rows.size()));
  HIPCHK(e, hipMemcpyAsync(lv->cand_rows.p, rows.data(), sizeof(LiveColRows) * rows.size(), hipMemcpyHostToDevice, s));
  HIPCHK(e, launch_live_candidates(e->st_m1.as<int32_t>(), lv->cand_rows.as<LiveColRows>(), e->scope_table.as<int32_t>(),
                                   e->ncols, lv->cand.as<int32_t>(), s));
  HIPCHK(e, hipStreamSynchronize(s));  // (rows is released on return)
  lv->cand_builds = e->n_scope_builds;
  return TFP_OK;
}

// What tfp_live_verdict asks of the shared body instead of a push's rows: per channel the planned
// length in, the two greatest candidate keys of launch_live_verdict out (0: none), and whether a key
// lay outside the vote range (the keys are then zeroed: nothing can be said).
struct LiveVerdictReq {
  const int64_t* total;
  unsigned long long* keys;  // [nch * 2]
  bool bad;
};

// The body of every live call. A push: tick[nch][T] is int16 (law < 0) or G.711 codes of that law
// (uint8), the only difference between tfp_live_push and tfp_live_push_g711. A verdict (vd set):
// no tick, T = 0, every channel idle; the count rows are brought up to date as a searching push of
// no samples does, and launch_live_verdict takes launch_live_select's place.
// What a verdict skips, each by the guard an idle push already takes: the tick's copy (0 bytes), the
// scatter (nch * T = 0), the fingerprint plan, launch and store (no channel has new samples, na = 0),
// the sample counters (n_new = 0). What it runs: the index and stamp checks, the candidate table, the
// one upload of descriptors (chan for the adds' bookkeeping, adds, its own LiveVerdictChan), the
// rebuild memsets and launch_live_add where frames are owed, launch_live_verdict, the read-back.
// K is the rows per channel read back: the caller's k for a push, 2 (leader, rival) for a verdict.
int live_step(tfp_live* lv, const void* pcm, int32_t law, int32_t T, const int32_t* nsamples, const tfp_search_params* P,
              const int32_t* scopes, int32_t K, tfp_candidate* out, int32_t* counts, int32_t* frame_counts,
              LiveVerdictReq* vd) {
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const int32_t nch = lv->nch;
  if (!vd && (!pcm || T <= 0)) return fail(e, TFP_E_ARG, "live push: NULL samples or tick_samples %d", T);
  if (P && !vd) {
    if (!out || !counts) return fail(e, TFP_E_ARG, "live push: NULL output");
    if (K < 1 || K > TFP_RANK_MAX) return fail(e, TFP_E_ARG, "live push: k = %d outside [1, %d]", K, TFP_RANK_MAX);
    for (int32_t c = 0; scopes && c < nch; c++)
      if (scopes[c] < TFP_SCOPE_ANY) return fail(e, TFP_E_ARG, "live push: scope %d of channel %d", scopes[c], c);
  }
  for (int32_t c = 0; nsamples && c < nch; c++)
    if (nsamples[c] < 0 || nsamples[c] > T)
      return fail(e, TFP_E_ARG, "live push: nsamples[%d] = %d outside [0, %d]", c, nsamples[c], T);
  // A rate object's push (tfp_live_rate.hpp): the tick is at rate_in, and what enters the history is each
  // channel's newly settled samples; from the descriptors on it is the plain push of those.
  const bool rate = lv->rated && !vd;
  std::vector<LiveRateChan> rchan(rate ? nch : 0);
  for (int32_t c = 0; c < nch; c++) {  // all or nothing: no channel has taken a sample yet
    const int32_t n_in = nsamples ? nsamples[c] : T;
    int64_t s_new = lv->samples[c] + n_in;
    if (rate) {
      LiveRateStep st;
      if (!live_rate_step(lv->rs_plan, lv->in_samples[c], n_in, &st))
        return fail(e, TFP_E_ARG, "live push: channel %d past the index range", c);
      s_new = st.n_old + st.n_new;  // (st.n_old = lv->samples[c])
      if (s_new <= lv->max_samples)
        rchan[c] = LiveRateChan{lv->in_samples[c], st.n_old, n_in, (int32_t)st.n_new, lv->parity[c], 0};
    }
    if (s_new > lv->max_samples)
      return fail(e, TFP_E_CAPACITY, "live push: channel %d past %lld samples", c, (long long)lv->max_samples);
  }
  std::vector<int32_t> rs_toff(1, 0), rs_tclip;
  int32_t rs_ntiles = 0, rs_max_new = 0;
  if (rate) {
    rs_ntiles = live_rate_tiles(rchan.data(), nch, lv->rs_tile, &rs_toff, &rs_tclip);
    for (const LiveRateChan& r : rchan) rs_max_new = std::max(rs_max_new, r.n_new);
  }
  if (rs_tclip.empty()) rs_tclip.push_back(0);  // (staged like the other tables: never an empty copy)
  HIPCHK(e, hipSetDevice(e->device));
  hipStream_t s = e->stream;
  int rc;
  const bool match = P && valid_params(P);  // fp_handler.c:247-250: bad params -> empty rows
  // The index and the table's stamp first: a failure here leaves the call uningested.
  SearchConsts sc{};
  bool vote = false, rebuild_table = false;
  if (match) {
    if ((rc = rebuild(e))) return rc;
    sc = search_consts(P);
    if (sc.coefs == 1) {
      if (!e->delta.clip.empty() && !delta_tol_ok(sc.tole) && (rc = consolidate(e))) return rc;
      if (e->ncols > 0 && e->nrows + e->delta.rows > 0) {
        if ((rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_key_bits(e, s)) || (rc = ensure_scope_table(e, s))) return rc;
        if (vd && (rc = ensure_live_candidates(lv, s))) return rc;
        vote = true;
        rebuild_table = !live_stamp_holds(lv, sc);
      }
    }
  }
  const int32_t C = e->ncols;
  const int64_t Cpad = vote ? live_count_cols(C) : 0;
  // The push's plan: per channel its descriptor; per channel with new samples one clip to
  // fingerprint and one copy of its kept frames; per channel with newly final frames one add.
  std::vector<LiveChan> chan(nch);
  std::vector<int32_t> act;
  std::vector<LivePlan> plans;
  std::vector<LiveVerdictChan> vchan(vd ? nch : 0);
  for (int32_t c = 0; vd && c < nch; c++) {
    vchan[c].tail = live_tail_frame(lv->samples[c]);
    vchan[c].scope = scopes ? scopes[c] : TFP_SCOPE_ANY;
    vchan[c].complete = lv->samples[c] == vd->total[c] ? 1 : 0;
  }
  for (int32_t c = 0; c < nch; c++) {
    const int32_t n = rate ? rchan[c].n_new : nsamples ? nsamples[c] : T;
    chan[c].s_old = lv->samples[c];
    chan[c].n_new = n;
    chan[c].scope = scopes ? scopes[c] : TFP_SCOPE_ANY;
    chan[c].tail = live_tail_frame(lv->samples[c] + n);
    if (n > 0) {
      act.push_back(c);
      plans.push_back(live_plan(lv->samples[c], n));
    }
  }
  const int32_t na = (int32_t)act.size();
  const DspTables* tables = nullptr;
  bool fx = false;
  if ((rc = ensure_tables(e, lv->sr, &tables, &fx))) return rc;
  int64_t nf16 = 0, max_frames = 0;
  for (const LivePlan& p : plans) {
    nf16 += (p.clip_frames + 15) / 16;
    max_frames = std::max(max_frames, p.clip_frames);
  }
  // 4-frame wave tiles for a small batch (fingerprint_host's rule) and for a tick's worth per channel
  const bool small = fx && (nf16 <= 256 || max_frames <= 4);
  const int32_t tile = fp_tile_frames(e->fpcfg, fx, false, small);
  std::vector<int64_t> sbeg(std::max(na, 1)), send(std::max(na, 1)), foff(na + 1, 0);
  std::vector<int32_t> toff(na + 1, 0), tclip;
  std::vector<LiveCopy> copies(std::max(na, 1));
  for (int32_t i = 0; i < na; i++) {
    const LivePlan& p = plans[i];
    sbeg[i] = (int64_t)act[i] * lv->max_samples + p.clip_beg;
    send[i] = (int64_t)act[i] * lv->max_samples + p.s_new;
    foff[i + 1] = foff[i] + p.clip_frames;
    toff[i + 1] = toff[i] + (int32_t)((p.clip_frames + tile - 1) / tile);
    copies[i] = LiveCopy{foff[i] + p.drop, (int64_t)act[i] * lv->Fmax + p.f0, p.keep};
  }
  tclip.assign(std::max<int32_t>(toff[na], 1), 0);
  for (int32_t i = 0; i < na; i++)
    for (int32_t t = toff[i]; t < toff[i + 1]; t++) tclip[t] = i;
  std::vector<LiveAdd> adds;
  int64_t add_frames = 0;
  if (vote)
    for (int32_t c = 0; c < nch; c++) {
      const int64_t from = rebuild_table ? 0 : lv->added[c], to = live_final_frames(lv->samples[c] + chan[c].n_new);
      if (to > from) {
        adds.push_back(LiveAdd{c, (int32_t)from, (int32_t)to, 0});
        add_frames += to - from;
      }
    }
  // One pinned buffer, one upload: the tick, then the descriptors.
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t tick_bytes = (law < 0 ? sizeof(int16_t) : sizeof(uint8_t)) * (size_t)nch * T;  // (a verdict: none)
  const size_t b_pcm = al(tick_bytes), b_chan = al(sizeof(LiveChan) * nch),
               b_sb = al(sizeof(int64_t) * sbeg.size()), b_fo = al(sizeof(int64_t) * foff.size()),
               b_to = al(sizeof(int32_t) * toff.size()), b_tc = al(sizeof(int32_t) * tclip.size()),
               b_cp = al(sizeof(LiveCopy) * copies.size()), b_add = al(sizeof(LiveAdd) * std::max<size_t>(adds.size(), 1)),
               b_vch = al(sizeof(LiveVerdictChan) * vchan.size()), b_rch = al(sizeof(LiveRateChan) * rchan.size()),
               b_rto = al(sizeof(int32_t) * rs_toff.size());
  const size_t o_chan = b_pcm, o_sb = o_chan + b_chan, o_se = o_sb + b_sb, o_fo = o_se + b_sb, o_to = o_fo + b_fo,
               o_tc = o_to + b_to, o_cp = o_tc + b_tc, o_add = o_cp + b_cp, o_vch = o_add + b_add, o_rch = o_vch + b_vch,
               o_rto = o_rch + b_rch, o_rtc = o_rto + b_rto, total = o_rtc + al(sizeof(int32_t) * rs_tclip.size());
  if (lv->stage_pending) HIPCHK(e, hipEventSynchronize(lv->stage_ev));  // the last push's upload has read stage_h
  lv->stage_pending = false;
  HIPCHK(e, lv->stage_h.reserve(total));
  HIPCHK(e, lv->dstage.reserve(total));
  char* h = lv->stage_h.as<char>();
  if (tick_bytes) memcpy(h, pcm, tick_bytes);
  if (vd) memcpy(h + o_vch, vchan.data(), sizeof(LiveVerdictChan) * nch);
  memcpy(h + o_chan, chan.data(), sizeof(LiveChan) * nch);
  memcpy(h + o_sb, sbeg.data(), sizeof(int64_t) * sbeg.size());
  memcpy(h + o_se, send.data(), sizeof(int64_t) * send.size());
  memcpy(h + o_fo, foff.data(), sizeof(int64_t) * foff.size());
  memcpy(h + o_to, toff.data(), sizeof(int32_t) * toff.size());
  memcpy(h + o_tc, tclip.data(), sizeof(int32_t) * tclip.size());
  memcpy(h + o_cp, copies.data(), sizeof(LiveCopy) * copies.size());
  if (!adds.empty()) memcpy(h + o_add, adds.data(), sizeof(LiveAdd) * adds.size());
  if (rate) {
    memcpy(h + o_rch, rchan.data(), sizeof(LiveRateChan) * rchan.size());
    memcpy(h + o_rto, rs_toff.data(), sizeof(int32_t) * rs_toff.size());
    memcpy(h + o_rtc, rs_tclip.data(), sizeof(int32_t) * rs_tclip.size());
  }
  const int64_t nf = foff[na];
  HIPCHK(e, e->micro.reserve(sizeof(int32_t) * 2 * (nf + 1)));
  HIPCHK(e, e->db.reserve(sizeof(double) * 2 * (nf + 1)));
  if (rebuild_table) HIPCHK(e, lv->counts.reserve(sizeof(uint16_t) * (size_t)nch * Cpad));
  if (vd) K = 2;  // the leader and the rival
  const size_t nkeys = P ? (size_t)nch * K : 0;
  if (vote) {
    HIPCHK(e, lv->part.reserve(sizeof(unsigned long long) * (size_t)nch * rank_vote_blocks(C) * K));
    HIPCHK(e, lv->keys.reserve(sizeof(unsigned long long) * nkeys));
    HIPCHK(e, lv->keys_pin.reserve(sizeof(unsigned long long) * (nkeys + 1)));
  }
  // From here on the call ingests.
  HIPCHK(e, hipMemcpyAsync(lv->dstage.p, h, total, hipMemcpyHostToDevice, s));
  HIPCHK(e, hipEventRecord(lv->stage_ev, s));
  lv->stage_pending = true;
  const char* d = lv->dstage.as<char>();
  const LiveChan* d_chan = reinterpret_cast<const LiveChan*>(d + o_chan);
  // 1: scatter (codes are expanded on their way into the int16 history: everything after is one path)
  if (rate) {
    // ... a rate object: the one launch that converts the tick into the history and moves the carry on
    int32_t nmove = 0;
    int64_t n_in_all = 0, n_out_all = 0;
    for (const LiveRateChan& r : rchan) nmove += r.n_in > 0, n_in_all += r.n_in, n_out_all += r.n_new;
    HIPCHK(e, launch_live_rate(lv->rs_plan, lv->rs_taps, d, law, T, reinterpret_cast<const LiveRateChan*>(d + o_rch), nch,
                               reinterpret_cast<const int32_t*>(d + o_rto), reinterpret_cast<const int32_t*>(d + o_rtc),
                               rs_ntiles, nmove, rs_max_new, lv->carry.as<int16_t>(), lv->max_samples,
                               lv->hist.as<int16_t>(), s));
    for (int32_t c = 0; c < nch; c++) {
      lv->in_samples[c] += rchan[c].n_in;
      if (rchan[c].n_in > 0) lv->parity[c] ^= 1;
    }
    if (rs_ntiles + nmove > 0) lv->n_rt_launch++;
    lv->n_rt_in += n_in_all;
    lv->n_rt_out += n_out_all;
    if (law >= 0) {
      e->n_g711_stream++;
      e->n_g711_codes += n_in_all;
    }
  } else if (law < 0) {
    HIPCHK(e, launch_live_scatter(reinterpret_cast<const int16_t*>(d), T, d_chan, nch, lv->max_samples, lv->hist.as<int16_t>(), s));
  } else {
    HIPCHK(e, launch_live_scatter_g711(reinterpret_cast<const uint8_t*>(d), T, d_chan, nch, law, lv->max_samples,
                                       lv->hist.as<int16_t>(), s));
    e->n_g711_stream++;
    for (int32_t c = 0; c < nch; c++) e->n_g711_codes += chan[c].n_new;
  }
  // 2: fingerprint only what changed (exact frame values: the kept history serves coefs = 2 as well,
  // and a coefs = 1 key is their truncation either way), then the kept frames into the history
  if (na) {
    HIPCHK(e, launch_fingerprint(e->fpcfg, tables, fx, tile, lv->hist.as<int16_t>(), reinterpret_cast<const int64_t*>(d + o_sb),
                                 reinterpret_cast<const int64_t*>(d + o_se), reinterpret_cast<const int64_t*>(d + o_fo),
                                 reinterpret_cast<const int32_t*>(d + o_to), reinterpret_cast<const int32_t*>(d + o_tc),
                                 toff[na], nf, e->micro.as<int32_t>(), e->db.as<double>(), s, e->logfix, &e->fpstats));
    int64_t max_keep = 0;
    for (const LivePlan& p : plans) max_keep = std::max(max_keep, p.keep);
    HIPCHK(e, launch_live_store(e->db.as<double>(), reinterpret_cast<const LiveCopy*>(d + o_cp), na, max_keep,
                                lv->q.as<double>(), s));
  }
  for (int32_t c = 0; c < nch; c++) lv->samples[c] += chan[c].n_new;
  lv->n_fp_frames += nf;
  if (!P) return TFP_OK;
  if (vd) {
    std::fill(vd->keys, vd->keys + nkeys, 0ull);
    vd->bad = false;
    if (!vote) return TFP_OK;  // an empty index: no candidate
  } else {
    memset(out, 0, sizeof(tfp_candidate) * nkeys);
    for (int32_t c = 0; c < nch; c++) {
      counts[c] = 0;
      if (frame_counts) frame_counts[c] = (int32_t)live_frames(lv->samples[c]);
    }
  }
  if (!match) return TFP_OK;
  std::vector<unsigned long long> keys(nkeys, 0ull);
  if (sc.coefs == 1 && !vote) {  // an empty index: no row
    lv->n_incremental++;
    return TFP_OK;
  }
  if (vote) {
    // 3: add the newly final frames (after a stamp mismatch: all of them, into a zeroed table)
    if (rebuild_table) {
      HIPCHK(e, hipMemsetAsync(lv->counts.p, 0, sizeof(uint16_t) * (size_t)nch * Cpad, s));
      HIPCHK(e, hipMemsetAsync(lv->bad.p, 0, sizeof(int32_t), s));
      std::fill(lv->added.begin(), lv->added.end(), 0);
      lv->count_cols = Cpad;
      lv->stamp_valid = true;
      lv->stamp_version = e->index_version;
      lv->stamp_sc = sc;
      lv->n_rebuilds++;
    }
    const uint32_t* d_bits = e->tc.ranges.active().key_bits.as<uint32_t>();
    HIPCHK(e, launch_live_add(lv->q.as<double>(), lv->Fmax, reinterpret_cast<const LiveAdd*>(d + o_add), (int32_t)adds.size(),
                              sc, d_bits, C, lv->counts.as<uint16_t>(), lv->bad.as<int32_t>(), s));
    for (const LiveAdd& a : adds) lv->added[a.ch] = a.fend;
    lv->n_added += add_frames;
    // 4: select (a verdict: its own selection over the candidate table)
    if (vd)
      HIPCHK(e, launch_live_verdict(lv->q.as<double>(), lv->Fmax, reinterpret_cast<const LiveVerdictChan*>(d + o_vch), nch, sc,
                                    d_bits, C, lv->counts.as<uint16_t>(), e->tiekey.as<int32_t>(), lv->cand.as<int32_t>(),
                                    lv->part.as<unsigned long long>(), lv->keys.as<unsigned long long>(),
                                    lv->bad.as<int32_t>(), s));
    else
      HIPCHK(e, launch_live_select(lv->q.as<double>(), lv->Fmax, d_chan, nch, sc, d_bits, C, lv->counts.as<uint16_t>(),
                                   e->tiekey.as<int32_t>(), e->scope_table.as<int32_t>(), K,
                                   lv->part.as<unsigned long long>(), lv->keys.as<unsigned long long>(), lv->bad.as<int32_t>(), s));
    unsigned long long* hk = lv->keys_pin.as<unsigned long long>();
    HIPCHK(e, hipMemcpyAsync(hk, lv->keys.p, sizeof(unsigned long long) * nkeys, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(hk + nkeys, lv->bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    lv->stage_pending = false;
    // A frame's key is trunc(10 log10|c|) of a finite DCT coefficient of int16 samples, or 0 where
    // the value is not finite (frame_key): |key| <= 459 (kKeyOffset), so no int16 input reaches an
    // out-of-range key. The route stays: the table then holds frames it could not add, so it is
    // dropped, and this and every later push of such a call take the general form.
    if (!(uint32_t)hk[nkeys]) {
      if (vd) {
        std::copy(hk, hk + nkeys, vd->keys);
        return TFP_OK;
      }
      std::copy(hk, hk + nkeys, keys.begin());
      fill_candidates(e, keys, nch, K, out, counts);
      lv->n_incremental++;
      return TFP_OK;
    }
    lv->stamp_valid = false;
    if (vd) {  // nothing can be said of counts the table could not take
      vd->bad = true;
      return TFP_OK;
    }
  }
  std::vector<int32_t> any;
  if (!scopes) any.assign(nch, TFP_SCOPE_ANY);
  if ((rc = live_general(lv, P, scopes ? scopes : any.data(), K, keys))) return rc;
  HIPCHK(e, hipStreamSynchronize(s));  // (live_general returns before any wait when no channel has a frame)
  lv->stage_pending = false;
  fill_candidates(e, keys, nch, K, out, counts);
  lv->n_general++;
  return TFP_OK;
}

// A verdict's arguments (tiresias_fp.h): nothing is written and nothing brought up to date on failure.
int live_verdict_args(tfp_live* lv, const int64_t* total, const tfp_search_params* P, const int32_t* scopes) {
  char msg[160];
  if (!live_verdict_args_ok(total, P ? &P->coefs : nullptr, scopes, lv->samples.data(), lv->nch, lv->max_samples, msg, sizeof msg))
    return fail(lv->eng, TFP_E_ARG, "%s", msg);
  return TFP_OK;
}

bool live_wstamp_holds(const tfp_live* lv, const SearchConsts& sc, int64_t window) {
  const SearchConsts& t = lv->wstamp_sc;
  return lv->wstamp_valid && lv->wstamp_version == lv->eng->index_version && lv->wstamp_window == window &&
         t.tole == sc.tole && t.has_low == sc.has_low && t.has_high == sc.has_high &&
         (!sc.has_low || t.thr_low == sc.thr_low) && (!sc.has_high || t.thr_high == sc.thr_high);
}

// What tfp_live_window_aligned asks of the window call's body besides the keys: out[c * K + r] = the
// alignment of row r of channel c with the channel's window (zeros where the key is 0).
struct LiveAlignReq {
  std::vector<AlignOut> out;
};

// An aligned window call's sizes: per channel its window, the boxes' stride (the longest window), the
// bands of the longest live clip against it, and the pairs per launch_align chunk.
struct LiveAlignPlan {
  std::vector<LiveWinChan> wchan;
  int64_t stride = 0, max_bands = 0, chunk = 1;
};

int live_align_plan(tfp_live* lv, int32_t K, int64_t window, LiveAlignPlan& ap) {
  tfp_engine* e = lv->eng;
  const int32_t nch = lv->nch;
  if (!lv->wa_nmax_valid || lv->wa_nmax_version != e->index_version) {  // (the caller has run rebuild)
    lv->wa_nmax = 0;
    for (const Clip& c : e->clips)
      if (c.alive) lv->wa_nmax = std::max(lv->wa_nmax, c.nrows);
    lv->wa_nmax_version = e->index_version;
    lv->wa_nmax_valid = true;
  }
  ap.wchan.resize(nch);
  ap.stride = 0;
  for (int32_t c = 0; c < nch; c++) {
    const int64_t F = live_frames(lv->samples[c]), first = F > window ? F - window : 0;
    ap.wchan[c] = LiveWinChan{(int32_t)first, (int32_t)(F - first)};
    ap.stride = std::max(ap.stride, F - first);
  }
  if (ap.stride + lv->wa_nmax > (int64_t(1) << 31))  // align_core's limit
    return fail(e, TFP_E_CAPACITY, "live window: %lld frames against %lld rows", (long long)ap.stride, (long long)lv->wa_nmax);
  ap.max_bands = align_bands(ap.stride, lv->wa_nmax);
  const int64_t npairs = (int64_t)nch * K;
  // pairs in chunks of <= 256 MB of partial keys (and of the launch grid's second dimension), as align_core
  ap.chunk = std::max<int64_t>(1, std::min<int64_t>({(int64_t(1) << 25) / std::max<int64_t>(ap.max_bands, 1), kAlignMaxPairs, npairs}));
  HIPCHK(e, lv->wa_cols.reserve(sizeof(int32_t) * (size_t)npairs));
  HIPCHK(e, lv->wa_boxes.reserve(sizeof(FrameBox) * (size_t)(nch * ap.stride + 1)));
  HIPCHK(e, lv->wa_pairs.reserve(sizeof(AlignPair) * (size_t)npairs));
  HIPCHK(e, lv->wa_part.reserve(sizeof(unsigned long long) * (size_t)(ap.chunk * std::max<int64_t>(ap.max_bands, 1))));
  const size_t rbytes = (sizeof(unsigned long long) + sizeof(AlignOut)) * (size_t)npairs + 8;
  HIPCHK(e, lv->wa_res.reserve(rbytes));
  HIPCHK(e, lv->wa_pin.reserve(rbytes));
  return TFP_OK;
}

// The window frames' boxes from the kept frame values in place, then launch_align over the nch * K
// pairs at wa_pairs, into d_out. Queued on s, no wait. The engine's tfp_align_stats is not moved.
int live_align_launch(tfp_live* lv, const SearchConsts& sc, const LiveAlignPlan& ap, const LiveWinChan* d_wchan, int32_t K,
                      AlignOut* d_out, hipStream_t s) {
  tfp_engine* e = lv->eng;
  const int64_t npairs = (int64_t)lv->nch * K;
  HIPCHK(e, launch_live_window_boxes(lv->q.as<double>(), lv->Fmax, d_wchan, lv->nch, ap.stride, sc, lv->wa_boxes.as<FrameBox>(), s));
  for (int64_t p0 = 0; p0 < npairs; p0 += ap.chunk) {
    const int32_t n = (int32_t)std::min<int64_t>(ap.chunk, npairs - p0);
    HIPCHK(e, launch_align(lv->wa_pairs.as<AlignPair>() + p0, n, ap.max_bands, lv->wa_boxes.as<FrameBox>(), e->st_m1.as<int32_t>(),
                           e->st_m2.as<int32_t>(), sc.coefs == 2, lv->wa_part.as<unsigned long long>(), d_out + p0, s));
  }
  return TFP_OK;
}

// The general form's alignments: the rows came back from the scoped search core (keys, on the host), so
// the pairs are built here from the clips' staging rows, uploaded with the channels' windows, and
// aligned as the in-place form's are. Caller holds e->mu; returns after waiting for the stream.
int live_align_general(tfp_live* lv, const SearchConsts& sc, int32_t K, int64_t window,
                       const std::vector<unsigned long long>& keys, LiveAlignReq* al) {
  tfp_engine* e = lv->eng;
  hipStream_t s = e->stream;
  const int32_t nch = lv->nch;
  const size_t npairs = (size_t)nch * K;
  LiveAlignPlan ap;
  int rc = live_align_plan(lv, K, window, ap);
  if (rc) return rc;
  std::vector<AlignPair> pairs(npairs, AlignPair{0, 0, 0, 0});
  for (size_t p = 0; p < npairs; p++) {
    if (!keys[p]) continue;
    const int32_t clip = clip_of_col(e, col_of_key(e, (int32_t)(uint32_t)(keys[p] & 0xffffffffu)));
    if (clip < 0) return fail(e, TFP_E_HIP, "live window: tie-break key %u names no clip", (unsigned)(keys[p] & 0xffffffffu));
    const Clip& c = e->clips[clip];
    const LiveWinChan& w = ap.wchan[p / K];
    if (c.nrows > 0 && w.F > 0) pairs[p] = AlignPair{c.off, (int64_t)(p / K) * ap.stride, (int32_t)c.nrows, w.F};
  }
  if ((rc = upload(e, lv->wa_pairs, pairs.data(), sizeof(AlignPair) * npairs)) ||
      (rc = upload(e, lv->wa_wchan, ap.wchan.data(), sizeof(LiveWinChan) * nch)))
    return rc;
  AlignOut* d_out = reinterpret_cast<AlignOut*>(lv->wa_res.as<char>());
  if ((rc = live_align_launch(lv, sc, ap, lv->wa_wchan.as<LiveWinChan>(), K, d_out, s))) return rc;
  HIPCHK(e, hipMemcpyAsync(lv->wa_pin.p, d_out, sizeof(AlignOut) * npairs, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));  // (pairs and ap.wchan are released on return)
  al->out.assign(lv->wa_pin.as<AlignOut>(), lv->wa_pin.as<AlignOut>() + npairs);
  return TFP_OK;
}

// The body of tfp_live_window: nothing is ingested and no frame fingerprinted. coefs = 1 over an index
// with rows: the window table's stamp is checked (a mismatch zeroes the table and empties every range),
// each channel's row is planned (live_window_plan) and the rows that owe frames go to the slide
// kernel in one launch; the push's selection then reads the window table, with the tail's bit added
// as a push adds it. One upload (descriptors), one read-back (keys and the bad flag), one wait.
// coefs = 2, and a key outside the vote range (which drops the table), gather each channel's window of
// kept frame values for the scoped search core. keys: nch * K, zeroed where there is no row.
// al (tfp_live_window_aligned): the rows' alignments as well. Served from the table, the select's keys
// stay on the device: their columns, the window's boxes and the pairs are built there and launch_align
// follows on the stream, so the call still has one upload, one read-back (keys, flag and alignments)
// and one wait. The general form aligns after its rows have come back (live_align_general).
int live_window_step(tfp_live* lv, const tfp_search_params* P, const int32_t* scopes, int32_t K, int64_t window,
                     std::vector<unsigned long long>& keys, LiveAlignReq* al = nullptr) {
  tfp_engine* e = lv->eng;
  const int32_t nch = lv->nch;
  hipStream_t s = e->stream;
  int rc;
  if ((rc = rebuild(e))) return rc;
  const SearchConsts sc = search_consts(P);
  bool vote = false;
  if (sc.coefs == 1) {
    if (!e->delta.clip.empty() && !delta_tol_ok(sc.tole) && (rc = consolidate(e))) return rc;
    if (e->ncols > 0 && e->nrows + e->delta.rows > 0) {
      if ((rc = ensure_ranges(e, sc.tole, s)) || (rc = ensure_key_bits(e, s)) || (rc = ensure_scope_table(e, s))) return rc;
      if (al && (rc = ensure_live_candidates(lv, s))) return rc;  // the columns' staged rows (LiveColRows)
      vote = true;
    }
  }
  keys.assign((size_t)nch * K, 0ull);
  if (al) al->out.assign((size_t)nch * K, AlignOut{0, 0, 0, 0});
  if (sc.coefs == 1 && !vote) {  // an empty index: no row
    lv->n_wslid++;
    if (al) lv->n_wa_inplace++;
    return TFP_OK;
  }
  if (vote) {
    const int32_t C = e->ncols;
    const int64_t Cpad = live_count_cols(C);
    const bool holds = live_wstamp_holds(lv, sc, window);
    std::vector<LiveChan> chan(nch);
    std::vector<LiveSlide> slides;
    std::vector<LiveWindowPlan> plans(nch);
    for (int32_t c = 0; c < nch; c++) {
      chan[c] = LiveChan{lv->samples[c], live_tail_frame(lv->samples[c]), 0, scopes ? scopes[c] : TFP_SCOPE_ANY};
      const LiveWindowPlan& p = plans[c] = live_window_plan(lv->samples[c], window, holds, lv->wbeg[c], lv->wend[c]);
      if (p.owes)
        slides.push_back(LiveSlide{c, (int32_t)p.sub_beg, (int32_t)p.sub_end, (int32_t)p.add_beg, (int32_t)p.add_end, p.restart, 0, 0});
    }
    LiveAlignPlan ap;
    if (al && (rc = live_align_plan(lv, K, window, ap))) return rc;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_chan = up(sizeof(LiveChan) * nch), o_wchan = b_chan + up(sizeof(LiveSlide) * std::max<size_t>(slides.size(), 1)),
                 total = o_wchan + (al ? up(sizeof(LiveWinChan) * nch) : 0);
    const size_t nkeys = (size_t)nch * K;
    if (lv->stage_pending) HIPCHK(e, hipEventSynchronize(lv->stage_ev));  // the last call's upload has read stage_h
    lv->stage_pending = false;
    HIPCHK(e, lv->stage_h.reserve(total));
    HIPCHK(e, lv->dstage.reserve(total));
    HIPCHK(e, lv->part.reserve(sizeof(unsigned long long) * (size_t)nch * rank_vote_blocks(C) * K));
    HIPCHK(e, lv->keys.reserve(sizeof(unsigned long long) * nkeys));
    HIPCHK(e, lv->keys_pin.reserve(sizeof(unsigned long long) * (nkeys + 1)));
    if (!holds) {
      HIPCHK(e, lv->wcounts.reserve(sizeof(uint16_t) * (size_t)nch * Cpad));
      HIPCHK(e, lv->wbad.reserve(sizeof(int32_t)));
    }
    char* h = lv->stage_h.as<char>();
    memcpy(h, chan.data(), sizeof(LiveChan) * nch);
    if (!slides.empty()) memcpy(h + b_chan, slides.data(), sizeof(LiveSlide) * slides.size());
    if (al) memcpy(h + o_wchan, ap.wchan.data(), sizeof(LiveWinChan) * nch);
    HIPCHK(e, hipMemcpyAsync(lv->dstage.p, h, total, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipEventRecord(lv->stage_ev, s));
    lv->stage_pending = true;
    if (!holds) {  // every row restarts: the table is zeroed, every range is empty
      HIPCHK(e, hipMemsetAsync(lv->wcounts.p, 0, sizeof(uint16_t) * (size_t)nch * Cpad, s));
      HIPCHK(e, hipMemsetAsync(lv->wbad.p, 0, sizeof(int32_t), s));
      for (int32_t c = 0; c < nch; c++) {
        lv->n_wremoved += lv->wend[c] - lv->wbeg[c];
        lv->wbeg[c] = lv->wend[c] = 0;
      }
      lv->wcount_cols = Cpad;
      lv->wstamp_valid = true;
      lv->wstamp_version = e->index_version;
      lv->wstamp_sc = sc;
      lv->wstamp_window = window;
      lv->n_wrebuilds++;
    }
    const char* d = lv->dstage.as<char>();
    const uint32_t* d_bits = e->tc.ranges.active().key_bits.as<uint32_t>();
    HIPCHK(e, launch_live_slide(lv->q.as<double>(), lv->Fmax, reinterpret_cast<const LiveSlide*>(d + b_chan), (int32_t)slides.size(),
                                sc, d_bits, C, lv->wcounts.as<uint16_t>(), lv->wbad.as<int32_t>(), s));
    for (int32_t c = 0; c < nch; c++) {
      const LiveWindowPlan& p = plans[c];
      lv->n_wadded += p.add_end - p.add_beg;
      lv->n_wremoved += (p.sub_end - p.sub_beg) + p.dropped;
      if (p.owes && p.restart) lv->n_wrestarted++;
      lv->wbeg[c] = p.a;
      lv->wend[c] = p.b;
    }
    // (aligned: the keys go where the one read-back takes them from, [keys][bad flag][AlignOut])
    unsigned long long* d_keys = al ? lv->wa_res.as<unsigned long long>() : lv->keys.as<unsigned long long>();
    HIPCHK(e, launch_live_select(lv->q.as<double>(), lv->Fmax, reinterpret_cast<const LiveChan*>(d), nch, sc, d_bits, C,
                                 lv->wcounts.as<uint16_t>(), e->tiekey.as<int32_t>(), e->scope_table.as<int32_t>(), K,
                                 lv->part.as<unsigned long long>(), d_keys, lv->wbad.as<int32_t>(), s));
    unsigned long long* hk = lv->keys_pin.as<unsigned long long>();
    if (al) {
      const LiveWinChan* d_wchan = reinterpret_cast<const LiveWinChan*>(d + o_wchan);
      int32_t* d_flag = reinterpret_cast<int32_t*>(d_keys + nkeys);
      AlignOut* d_out = reinterpret_cast<AlignOut*>(d_keys + nkeys + 1);
      HIPCHK(e, hipMemsetAsync(lv->wa_cols.p, 0xff, sizeof(int32_t) * nkeys, s));  // -1: no column
      HIPCHK(e, launch_live_key_cols(d_keys, reinterpret_cast<const LiveChan*>(d), nch, K, e->tiekey.as<int32_t>(),
                                     e->scope_table.as<int32_t>(), lv->cand_rows.as<LiveColRows>(), C, lv->wa_cols.as<int32_t>(), s));
      HIPCHK(e, launch_live_pairs(d_keys, lv->wa_cols.as<int32_t>(), lv->cand_rows.as<LiveColRows>(), C, d_wchan, nch, K, ap.stride,
                                  lv->wbad.as<int32_t>(), lv->wa_pairs.as<AlignPair>(), d_flag, s));
      if ((rc = live_align_launch(lv, sc, ap, d_wchan, K, d_out, s))) return rc;
      hk = lv->wa_pin.as<unsigned long long>();
      HIPCHK(e, hipMemcpyAsync(hk, d_keys, (sizeof(unsigned long long) + sizeof(AlignOut)) * nkeys + 8, hipMemcpyDeviceToHost, s));
    } else {
      HIPCHK(e, hipMemcpyAsync(hk, lv->keys.p, sizeof(unsigned long long) * nkeys, hipMemcpyDeviceToHost, s));
      HIPCHK(e, hipMemcpyAsync(hk + nkeys, lv->wbad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    lv->stage_pending = false;
    if (!(uint32_t)hk[nkeys]) {
      std::copy(hk, hk + nkeys, keys.begin());
      lv->n_wslid++;
      if (al) {
        // (counted before the check below: the table has moved, so the stats name the call it was)
        lv->n_wa_inplace++;
        for (size_t p = 0; p < nkeys; p++) lv->n_wa_pairs += keys[p] != 0;
        const AlignOut* ho = reinterpret_cast<const AlignOut*>(hk + nkeys + 1);
        for (size_t p = 0; p < nkeys; p++) {
          if (!keys[p]) continue;
          // a row has a frame that hits one of its clip's rows, so its best diagonal holds a hit
          if (ho[p].aligned_count <= 0)
            return fail(e, TFP_E_HIP, "live window: no staged rows found for tie-break key %u", (unsigned)(keys[p] & 0xffffffffu));
          al->out[p] = ho[p];
        }
      }
      return TFP_OK;
    }
    lv->wstamp_valid = false;  // the table holds frames it could not add: dropped, as a push drops its own
  }
  std::vector<int32_t> any;
  if (!scopes) any.assign(nch, TFP_SCOPE_ANY);
  if ((rc = live_general(lv, P, scopes ? scopes : any.data(), K, keys, window))) return rc;
  HIPCHK(e, hipStreamSynchronize(s));  // (live_general returns before any wait when no channel has a frame)
  lv->stage_pending = false;
  lv->n_wgeneral++;
  if (al) {
    if ((rc = live_align_general(lv, sc, K, window, keys, al))) return rc;
    for (size_t p = 0; p < keys.size(); p++)
      if (!keys[p]) al->out[p] = AlignOut{0, 0, 0, 0};
      else lv->n_wa_pairs++;
    lv->n_wa_general++;
  }
  return TFP_OK;
}

}  // namespace

int tfp_live_push(tfp_live* lv, const int16_t* pcm, int32_t T, const int32_t* nsamples, const tfp_search_params* P,
                  const int32_t* scopes, int32_t K, tfp_candidate* out, int32_t* counts, int32_t* frame_counts) {
  if (!lv) return TFP_E_ARG;
  return live_step(lv, pcm, -1, T, nsamples, P, scopes, K, out, counts, frame_counts, nullptr);
}

int tfp_live_push_g711(tfp_live* lv, const uint8_t* codes, int32_t T, int32_t law, const int32_t* nsamples,
                       const tfp_search_params* P, const int32_t* scopes, int32_t K, tfp_candidate* out, int32_t* counts,
                       int32_t* frame_counts) {
  if (!lv) return TFP_E_ARG;
  if (!g711_law_ok(law)) return fail(lv->eng, TFP_E_ARG, "G.711 law %d is neither TFP_G711_ULAW nor TFP_G711_ALAW", law);
  return live_step(lv, codes, law, T, nsamples, P, scopes, K, out, counts, frame_counts, nullptr);
}

int tfp_internal_live_verdict_keys(tfp_live* lv, const int64_t* total, const tfp_search_params* P, const int32_t* scopes,
                                   unsigned long long* keys, int32_t* bad) {
  if (!lv || !keys || !bad) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  int rc = live_verdict_args(lv, total, P, scopes);
  if (rc) return rc;
  LiveVerdictReq vd{total, keys, false};
  if ((rc = live_step(lv, nullptr, -1, 0, nullptr, P, scopes, 2, nullptr, nullptr, nullptr, &vd))) return rc;
  *bad = vd.bad ? 1 : 0;
  return TFP_OK;
}

int tfp_live_verdict(tfp_live* lv, const int64_t* total, const tfp_search_params* P, const int32_t* scopes,
                     struct tfp_live_verdict* out) {
  if (!lv || !out) return TFP_E_ARG;
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const int32_t nch = lv->nch;
  std::vector<unsigned long long> keys((size_t)nch * 2, 0ull);
  int32_t bad = 0;
  const int rc = tfp_internal_live_verdict_keys(lv, total, P, scopes, keys.data(), &bad);
  if (rc) return rc;
  std::vector<struct tfp_live_verdict> res(nch);  // copied out on success: every failure leaves out untouched
  for (int32_t c = 0; c < nch; c++) {
    const LiveVerdictRule r = live_verdict_rule(bad ? 0ull : keys[2 * c], bad ? 0ull : keys[2 * c + 1], lv->samples[c], total[c]);
    struct tfp_live_verdict& v = res[c];
    memset(&v, 0, sizeof v);
    v.remaining = r.remaining;
    v.complete = r.complete;
    v.decided = r.decided;
    const unsigned long long side[2] = {r.leader, r.rival};  // (a rival's packed key may be 0: count 0, tie key 0)
    for (int i = 0; i < 2; i++) {
      if (!(i ? r.has_rival : r.has_leader)) continue;
      const int32_t clip = clip_of_col(e, col_of_key(e, (int32_t)(uint32_t)(side[i] & 0xffffffffu)));
      if (clip < 0) return fail(e, TFP_E_HIP, "live verdict: tie-break key %u names no clip", (unsigned)(side[i] & 0xffffffffu));
      tfp_candidate& cd = i ? v.rival : v.leader;
      cd.match_count = (int32_t)(side[i] >> 32);
      cd.clip_id = clip;
      snprintf(cd.uuid, sizeof cd.uuid, "%s", e->clips[clip].uuid.c_str());
      (i ? v.has_rival : v.has_leader) = 1;
    }
  }
  std::copy(res.begin(), res.end(), out);
  return TFP_OK;
}

namespace {
// tfp_live_window (align NULL, aligned false) and tfp_live_window_aligned: the same arguments, rows,
// counts and frame ranges; the aligned call also fills align[nch * K], zeros past counts[c].
int live_window_call(tfp_live* lv, const tfp_search_params* P, const int32_t* scopes, int32_t K, int32_t window,
                     tfp_candidate* out, tfp_alignment* align, bool aligned, int32_t* counts, int32_t* frame_counts,
                     int32_t* first_frames) {
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const int32_t nch = lv->nch;
  if (!P || !out || !counts || (aligned && !align)) return fail(e, TFP_E_ARG, "live window: NULL params or output");
  if (window < 1) return fail(e, TFP_E_ARG, "live window: window = %d frames", window);
  if (K < 1 || K > TFP_RANK_MAX) return fail(e, TFP_E_ARG, "live window: k = %d outside [1, %d]", K, TFP_RANK_MAX);
  for (int32_t c = 0; scopes && c < nch; c++)
    if (scopes[c] < TFP_SCOPE_ANY) return fail(e, TFP_E_ARG, "live window: scope %d of channel %d", scopes[c], c);
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<unsigned long long> keys((size_t)nch * K, 0ull);
  LiveAlignReq al;
  if (aligned) al.out.assign((size_t)nch * K, AlignOut{0, 0, 0, 0});
  if (valid_params(P)) {  // fp_handler.c:247-250: bad params -> empty rows
    const int rc = live_window_step(lv, P, scopes, K, window, keys, aligned ? &al : nullptr);
    if (rc) return rc;
  }
  fill_candidates(e, keys, nch, K, out, counts);
  if (aligned) {
    memset(align, 0, sizeof(tfp_alignment) * (size_t)nch * K);
    for (int32_t c = 0; c < nch; c++) {  // fill_candidates' walk: a key that names no clip has no row
      int32_t n = 0;
      for (int32_t r = 0; r < K && keys[(size_t)c * K + r]; r++) {
        if (clip_of_col(e, col_of_key(e, (int32_t)(uint32_t)(keys[(size_t)c * K + r] & 0xffffffffu))) < 0) continue;
        memcpy(&align[(size_t)c * K + n++], &al.out[(size_t)c * K + r], sizeof(tfp_alignment));
      }
    }
  }
  for (int32_t c = 0; c < nch; c++) {
    const int64_t F = live_frames(lv->samples[c]), first = F > window ? F - window : 0;
    if (frame_counts) frame_counts[c] = (int32_t)(F - first);
    if (first_frames) first_frames[c] = (int32_t)first;
  }
  return TFP_OK;
}
}  // namespace

int tfp_live_window(tfp_live* lv, const tfp_search_params* P, const int32_t* scopes, int32_t K, int32_t window,
                    tfp_candidate* out, int32_t* counts, int32_t* frame_counts, int32_t* first_frames) {
  if (!lv) return TFP_E_ARG;
  return live_window_call(lv, P, scopes, K, window, out, nullptr, false, counts, frame_counts, first_frames);
}

int tfp_live_window_aligned(tfp_live* lv, const tfp_search_params* P, const int32_t* scopes, int32_t K, int32_t window,
                            tfp_candidate* out, tfp_alignment* align, int32_t* counts, int32_t* frame_counts,
                            int32_t* first_frames) {
  if (!lv) return TFP_E_ARG;
  return live_window_call(lv, P, scopes, K, window, out, align, true, counts, frame_counts, first_frames);
}

int tfp_live_window_aligned_stats(tfp_live* lv, int64_t* inplace_calls, int64_t* general_calls, int64_t* pairs) {
  if (!lv) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  if (inplace_calls) *inplace_calls = lv->n_wa_inplace;
  if (general_calls) *general_calls = lv->n_wa_general;
  if (pairs) *pairs = lv->n_wa_pairs;
  return TFP_OK;
}

int32_t tfp_live_window_frames(int64_t window_ms, int32_t sample_rate) {
  const int64_t f = live_window_frames_of_ms(window_ms, sample_rate);
  return f > INT32_MAX ? INT32_MAX : (int32_t)f;
}

int tfp_live_frames(tfp_live* lv, int32_t ch, int64_t first, tfp_frame* out, int64_t cap, int64_t* nframes) {
  if (!lv || !nframes) return TFP_E_ARG;
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (ch < 0 || ch >= lv->nch) return fail(e, TFP_E_ARG, "live frames: channel %d outside [0, %d)", ch, lv->nch);
  const int64_t F = live_frames(lv->samples[ch]);
  if (first < 0 || first > F) return fail(e, TFP_E_ARG, "live frames: first = %lld outside [0, %lld]", (long long)first, (long long)F);
  const int64_t n = F - first;
  *nframes = n;
  if (cap < n) return fail(e, TFP_E_ARG, "live frames: cap %lld below the %lld frames asked for", (long long)cap, (long long)n);
  if (!n) return TFP_OK;
  if (!out) return fail(e, TFP_E_ARG, "live frames: NULL output");
  HIPCHK(e, hipSetDevice(e->device));
  std::vector<double> d(2 * (size_t)n);
  HIPCHK(e, hipMemcpyAsync(d.data(), lv->q.as<double>() + 2 * ((int64_t)ch * lv->Fmax + first), sizeof(double) * 2 * n,
                           hipMemcpyDeviceToHost, e->stream));
  HIPCHK(e, hipStreamSynchronize(e->stream));
  lv->stage_pending = false;
  for (int64_t f = 0; f < n; f++) {
    out[f].frame_idx = (int32_t)(first + f);
    out[f].m1 = micro_of_db(d[2 * f]);  // as stored (db_ctx_handler.c:479-481)
    out[f].m2 = micro_of_db(d[2 * f + 1]);
    out[f].reserved = 0;
    out[f].q1 = d[2 * f];
    out[f].q2 = d[2 * f + 1];
  }
  return TFP_OK;
}

int tfp_live_window_stats(tfp_live* lv, int64_t* slid_calls, int64_t* general_calls, int64_t* rebuilds, int64_t* frames_added,
                          int64_t* frames_removed, int64_t* rows_restarted) {
  if (!lv) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  if (slid_calls) *slid_calls = lv->n_wslid;
  if (general_calls) *general_calls = lv->n_wgeneral;
  if (rebuilds) *rebuilds = lv->n_wrebuilds;
  if (frames_added) *frames_added = lv->n_wadded;
  if (frames_removed) *frames_removed = lv->n_wremoved;
  if (rows_restarted) *rows_restarted = lv->n_wrestarted;
  return TFP_OK;
}

// ---- the carried traces of live calls (tfp_live_occurrences; tfp_live.hpp, tfp_live_trace.hip): the
// call in four steps, rows, offer, advance and select, each a function of its own: a device group runs
// the rows and the offer once on its merged rows, every shard advances its own clips' tracks, and the
// select runs on the union (tfp_group.cpp).
namespace {

static_assert(TFP_LIVE_TRACKS_MAX == kLiveTracksMax, "tfp_live.hpp and the public header agree");

struct LiveOccCand {
  int32_t ch, clip, s;
};

// Step 1: tfp_live_window_aligned's rows as candidates, channel ascending, row ascending: a row with
// aligned_count >= 1 names (clip, s = first - offset). Moves the window table and both window stats as
// that call does. Invalid params: no rows.
int live_occ_rows(tfp_live* lv, const tfp_search_params* P, const int32_t* scopes, int32_t K, int32_t window,
                  std::vector<LiveOccCand>& cands) {
  tfp_engine* e = lv->eng;
  cands.clear();
  if (!valid_params(P)) return TFP_OK;
  std::vector<unsigned long long> keys;
  LiveAlignReq al;
  const int rc = live_window_step(lv, P, scopes, K, window, keys, &al);
  if (rc) return rc;
  for (int32_t c = 0; c < lv->nch; c++) {
    const int64_t F = live_frames(lv->samples[c]), first = F > window ? F - window : 0;
    for (int32_t r = 0; r < K && keys[(size_t)c * K + r]; r++) {  // fill_candidates' walk
      const int32_t clip = clip_of_col(e, col_of_key(e, (int32_t)(uint32_t)(keys[(size_t)c * K + r] & 0xffffffffu)));
      if (clip < 0) continue;
      const AlignOut& a = al.out[(size_t)c * K + r];
      if (a.aligned_count >= 1) cands.push_back(LiveOccCand{c, clip, (int32_t)(first - a.offset)});
    }
  }
  return TFP_OK;
}

bool live_track_clip_ok(const tfp_engine* e, const tfp_live::Track& t) {
  return t.clip >= 0 && (size_t)t.clip < e->clips.size() && e->clips[t.clip].alive && e->clips[t.clip].uuid == t.uuid;
}

// A new track at the end of channel ch's list (the caller has checked the room and that it is new).
void live_occ_append(tfp_live* lv, int32_t ch, int32_t clip, int32_t s) {
  tfp_live::Track t;
  t.clip = clip;
  t.uuid = lv->eng->clips[clip].uuid;
  t.s = s;
  t.windows = 1;
  lv->tracks[ch].push_back(std::move(t));
  lv->n_tr_added++;
}

// Step 2: the offer rule over the candidates in order. dropped[c] (may be NULL) counts this call's.
void live_occ_offer(tfp_live* lv, const std::vector<LiveOccCand>& cands, int32_t max_tracks, int32_t* dropped) {
  for (const LiveOccCand& c : cands) {
    std::vector<tfp_live::Track>& list = lv->tracks[c.ch];
    auto it = std::find_if(list.begin(), list.end(), [&](const tfp_live::Track& t) { return t.clip == c.clip && t.s == c.s; });
    if (it != list.end()) {
      it->windows++;
    } else if ((int64_t)list.size() < max_tracks) {
      live_occ_append(lv, c.ch, c.clip, c.s);
    } else {
      lv->n_tr_dropped++;
      if (dropped) dropped[c.ch]++;
    }
  }
}

bool live_tr_stamp_holds(const tfp_live* lv, const SearchConsts& sc, int32_t max_gap) {
  const SearchConsts& t = lv->tr_stamp_sc;
  return lv->tr_stamp_valid && lv->tr_stamp_version == lv->eng->index_version && lv->tr_stamp_gap == max_gap &&
         t.coefs == sc.coefs && t.tole == sc.tole && t.has_low == sc.has_low && t.has_high == sc.has_high &&
         (!sc.has_low || t.thr_low == sc.thr_low) && (!sc.has_high || t.thr_high == sc.thr_high);
}

// Step 3: every track brought up to its channel's frames. Tracks of removed clips are deleted; a
// changed stamp restarts every summary from its lo. One upload (descriptors), one launch, one
// read-back; a track with nothing to fold and no tail in its span is answered from its last result.
// Caller holds e->mu and has run rebuild (step 1 does).
int live_occ_advance(tfp_live* lv, const tfp_search_params* P, int32_t max_gap) {
  tfp_engine* e = lv->eng;
  hipStream_t s = e->stream;
  const int32_t nch = lv->nch;
  const SearchConsts sc = search_consts(P);
  if (!live_tr_stamp_holds(lv, sc, max_gap)) {
    bool any = false;  // a call retraces when a summary it kept is started again
    for (int32_t c = 0; c < nch; c++)
      for (tfp_live::Track& t : lv->tracks[c]) any |= t.stored, t.stored = false;
    if (any) lv->n_tr_retraces++;
    lv->tr_stamp_valid = true;
    lv->tr_stamp_version = e->index_version;
    lv->tr_stamp_sc = sc;
    lv->tr_stamp_gap = max_gap;
  }
  for (int32_t c = 0; c < nch; c++) {  // (a clip's removal changes the index version: the stamp has restarted all)
    std::vector<tfp_live::Track>& list = lv->tracks[c];
    const size_t n0 = list.size();
    list.erase(std::remove_if(list.begin(), list.end(), [&](const tfp_live::Track& t) { return !live_track_clip_ok(e, t); }),
               list.end());
    if (list.size() != n0)  // the slots follow the list's positions: the channel's summaries start again
      for (tfp_live::Track& t : list) t.stored = false;
  }
  std::vector<LiveTrace> desc;
  std::vector<tfp_live::Track*> who;
  std::vector<int64_t> folds;
  for (int32_t c = 0; c < nch; c++) {
    const int64_t S = lv->samples[c], F = live_frames(S), Ff = S / 256, tail = live_tail_frame(S);
    for (size_t i = 0; i < lv->tracks[c].size(); i++) {
      tfp_live::Track& t = lv->tracks[c][i];
      const Clip& clip = e->clips[t.clip];
      int64_t lo, hi;
      trace_span(F, clip.nrows, t.s, &lo, &hi);
      const int32_t overlap = (int32_t)(hi > lo ? hi - lo : 0);
      const int64_t end = std::min<int64_t>(Ff, (int64_t)t.s + clip.nrows);
      if (!t.stored) t.done = lo;
      const int64_t beg = std::max(t.done, lo), nfold = end > beg ? end - beg : 0;
      const bool tail_in = tail >= 0 && tail >= lo && tail < (int64_t)t.s + clip.nrows;
      if (!nfold && !tail_in && (!t.stored || !t.last_tail)) {  // nothing new on this diagonal
        if (!t.stored) t.last = TraceOut{0, 0, 0, 0, 0, 0};
        t.last.overlap = overlap;
        t.last_tail = false;
        continue;
      }
      desc.push_back(LiveTrace{clip.off, (int32_t)clip.nrows, t.s, c, (int32_t)(c * kLiveTracksMax + (int32_t)i), (int32_t)beg,
                               (int32_t)(beg + nfold), tail_in ? (int32_t)tail : -1, t.stored ? 0 : 1, overlap, 0});
      who.push_back(&t);
      folds.push_back(nfold);
    }
  }
  if (desc.empty()) return TFP_OK;
  const size_t obytes = sizeof(TraceOut) * desc.size();
  HIPCHK(e, lv->tr_segs.reserve(sizeof(TraceSeg) * (size_t)nch * kLiveTracksMax));
  HIPCHK(e, lv->tr_out.reserve(obytes));
  HIPCHK(e, lv->tr_pin.reserve(obytes));
  int rc = upload(e, lv->tr_desc, desc.data(), sizeof(LiveTrace) * desc.size(), s);
  if (rc) return rc;
  lv->tr_stamp_valid = false;  // (until the results are back: a failure below leaves the slots unknown)
  HIPCHK(e, launch_live_trace(lv->tr_desc.as<LiveTrace>(), (int32_t)desc.size(), max_gap, lv->q.as<double>(), lv->Fmax, sc,
                              e->st_m1.as<int32_t>(), e->st_m2.as<int32_t>(), lv->tr_segs.as<TraceSeg>(),
                              lv->tr_out.as<TraceOut>(), s));
  HIPCHK(e, hipMemcpyAsync(lv->tr_pin.p, lv->tr_out.p, obytes, hipMemcpyDeviceToHost, s));
  HIPCHK(e, hipStreamSynchronize(s));  // (desc is released on return)
  lv->stage_pending = false;
  lv->tr_stamp_valid = true;
  const TraceOut* res = lv->tr_pin.as<TraceOut>();
  for (size_t i = 0; i < desc.size(); i++) {
    tfp_live::Track& t = *who[i];
    t.last = res[i];
    t.last_tail = desc[i].tail >= 0;
    t.stored = true;
    t.done = desc[i].end > desc[i].beg ? desc[i].end : t.done;
    lv->n_tr_frames += folds[i];
  }
  return TFP_OK;
}

}  // namespace

int tfp_live_occurrences(tfp_live* lv, const tfp_search_params* P, const int32_t* scopes, int32_t K, int32_t window,
                         int32_t max_gap, int32_t min_hits, int32_t max_tracks, tfp_occurrence* out, int64_t cap,
                         int64_t* nocc, int32_t* dropped) {
  if (!lv) return TFP_E_ARG;
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const int32_t nch = lv->nch;
  if (const char* bad = live_occ_args(P, scopes, nch, K, window, max_gap, min_hits, max_tracks, out, cap, nocc))
    return fail(e, TFP_E_ARG, "live occurrences: %s", bad);
  HIPCHK(e, hipSetDevice(e->device));
  if (dropped) memset(dropped, 0, sizeof(int32_t) * nch);
  *nocc = 0;
  lv->n_occ_calls++;
  if (!valid_params(P)) return TFP_OK;  // fp_handler.c:247-250: no rows, nothing offered, the lists stay
  std::vector<LiveOccCand> cands;
  int rc = live_occ_rows(lv, P, scopes, K, window, cands);
  if (rc) return rc;
  live_occ_offer(lv, cands, max_tracks, dropped);
  if ((rc = live_occ_advance(lv, P, max_gap))) return rc;
  std::vector<LiveOccTrack> tr;
  for (int32_t c = 0; c < nch; c++) {
    const int32_t scope = scopes ? scopes[c] : TFP_SCOPE_ANY;
    for (const tfp_live::Track& t : lv->tracks[c])  // (step 3 has deleted the tracks of removed clips)
      if (scope == TFP_SCOPE_ANY || e->clips[t.clip].scope == scope)
        tr.push_back(LiveOccTrack{c, t.clip, t.clip, t.s, t.windows, t.last, e->clips[t.clip].uuid.c_str()});
  }
  std::string err;
  if ((rc = live_occ_select(tr, min_hits, out, cap, nocc, &err))) return fail(e, rc, "%s", err.c_str());
  return TFP_OK;
}

int tfp_live_tracks(tfp_live* lv, int32_t ch, tfp_trace_req* reqs, tfp_trace* traces, int32_t* windows, int64_t cap,
                    int64_t* ntracks) {
  if (!lv || !ntracks) return TFP_E_ARG;
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (ch < 0 || ch >= lv->nch) return fail(e, TFP_E_ARG, "live tracks: channel %d outside [0, %d)", ch, lv->nch);
  const std::vector<tfp_live::Track>& list = lv->tracks[ch];
  *ntracks = (int64_t)list.size();
  if (cap < *ntracks)
    return fail(e, TFP_E_CAPACITY, "live tracks: %lld tracks, room for %lld", (long long)*ntracks, (long long)cap);
  for (size_t i = 0; i < list.size(); i++) {
    if (reqs) reqs[i] = tfp_trace_req{ch, list[i].clip, list[i].s, 0};
    if (traces) memcpy(&traces[i], &list[i].last, sizeof(tfp_trace));
    if (windows) windows[i] = list[i].windows;
  }
  return TFP_OK;
}

int tfp_live_occurrence_stats(tfp_live* lv, int64_t* calls, int64_t* tracks_added, int64_t* tracks_dropped,
                              int64_t* frames_traced, int64_t* retraces) {
  if (!lv) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(lv->eng->mu);
  if (calls) *calls = lv->n_occ_calls;
  if (tracks_added) *tracks_added = lv->n_tr_added;
  if (tracks_dropped) *tracks_dropped = lv->n_tr_dropped;
  if (frames_traced) *frames_traced = lv->n_tr_frames;
  if (retraces) *retraces = lv->n_tr_retraces;
  return TFP_OK;
}

// (tfp_internal.hpp) a device group's shard: the offer ran on the group's merged rows, so a track is
// appended as told, and the advance is asked for on its own.
int tfp_internal_live_occ_add(tfp_live* lv, int32_t ch, int32_t clip_id, int32_t s) {
  if (!lv || ch < 0 || ch >= lv->nch) return TFP_E_ARG;
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (clip_id < 0 || (size_t)clip_id >= e->clips.size() || !e->clips[clip_id].alive)
    return fail(e, TFP_E_NOENT, "live occurrences: clip id %d is not in the index", clip_id);
  if ((int64_t)lv->tracks[ch].size() >= kLiveTracksMax)
    return fail(e, TFP_E_CAPACITY, "live occurrences: channel %d holds %d tracks", ch, kLiveTracksMax);
  live_occ_append(lv, ch, clip_id, s);
  return TFP_OK;
}

int tfp_internal_live_occ_advance(tfp_live* lv, const tfp_search_params* P, int32_t max_gap) {
  if (!lv || !valid_params(P) || max_gap < 0) return TFP_E_ARG;
  tfp_engine* e = lv->eng;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  int rc = rebuild(e);
  if (rc) return rc;
  lv->n_occ_calls++;
  return live_occ_advance(lv, P, max_gap);
}

int tfp_synth_pcm(const tfp_synth_spec* specs, int32_t nclips, int64_t spc, int16_t* out) {
  if (nclips < 0 || spc < 0 || (nclips && (!specs || !out))) return TFP_E_ARG;
  for (int32_t c = 0; c < nclips; c++) {
    const SynthClip p = synth_clip(specs[c].seed, specs[c].clip);
    for (int64_t s = 0; s < spc; s++) out[(int64_t)c * spc + s] = synth_sample(p, specs[c].offset + s);
  }
  return TFP_OK;
}

int tfp_synth_pcm_device(tfp_engine* e, const tfp_synth_spec* specs, int32_t nclips, int64_t spc, int16_t* d_out,
                         void* stream) {
  if (!e || nclips < 0 || spc < 0 || (nclips && (!specs || !d_out))) return TFP_E_ARG;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIPCHK(e, hipSetDevice(e->device));
  NullStreamOrder order(e, stream);
  if (!order.ok()) return fail(e, TFP_E_HIP, "ordering after the null stream failed");
  hipStream_t s = stream ? (hipStream_t)stream : e->stream;
  static_assert(sizeof(tfp_synth_spec) == sizeof(SynthSpecDev), "spec layout");
  int rc = upload(e, e->specs, specs, sizeof(tfp_synth_spec) * nclips);
  if (rc) return rc;
  if (s != e->stream) HIPCHK(e, hipStreamSynchronize(e->stream));
  HIPCHK(e, launch_synth(e->specs.as<SynthSpecDev>(), nclips, spc, d_out, s));
  HIPCHK(e, hipStreamSynchronize(s));  // specs buffer is reused by the next call
  return TFP_OK;
}

int tfp_synchronize(tfp_engine* e, void* stream) {
  if (!e) return TFP_E_ARG;
  HIPCHK(e, hipSetDevice(e->device));
  HIPCHK(e, hipStreamSynchronize(stream ? (hipStream_t)stream : e->stream));
  return TFP_OK;
}

}  // extern "C"
