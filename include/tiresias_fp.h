/* tiresias_fp.h — C-ABI of the MI355X-native tiresias fingerprint engine.
 *
 * Drop-in boundary for the hot path of pchero/asterisk-tiresias (/root/reference):
 * the Asterisk-side C (application_handler.c, cli_handler.c, app_tiresias.c and the SQLite
 * catalog in db_ctx_handler.c) keeps working and calls these entry points from a thin
 * fp_handler.c shim. Plain C types only; memory is caller-allocated unless
 * stated; every int return is TFP_OK (0) or a negative TFP_E_* code, with the message in
 * tfp_engine_last_error(). All engine calls are thread-safe (serialised per engine).
 *
 * Reference interfaces replaced (file:line in /root/reference/src):
 *   tfp_fingerprint_pcm / _batch      create_audio_fingerprints      fp_handler.c:577-671
 *   tfp_index_add                     create_audio_fingerprint_info  fp_handler.c:538-575
 *                                     (+ the INSERT it issues        db_ctx_handler.c:413-556)
 *   tfp_index_remove                  fp_delete_audio_list_info's    fp_handler.c:146-157
 *                                     "delete from audio_fingerprint where audio_uuid=..."
 *   tfp_search / _batch / _pcm_batch  fp_search_fingerprint_info     fp_handler.c:207-408
 *                                     (declared in fp_handler.h:28-35)
 *   tfp_wav_decode / tfp_wav_read     new_aubio_source + aubio_source_do at the native rate
 *                                     fp_handler.c:37, :604, :633 (libaubio source_wavread)
 */
#ifndef TIRESIAS_FP_H
#define TIRESIAS_FP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFP_ABI_VERSION 1
#define TFP_HOP 256              /* DEF_AUBIO_HOPSIZE, fp_handler.c:33 */
#define TFP_WIN 512              /* DEF_AUBIO_BUFSIZE, fp_handler.c:34 */
#define TFP_DEFAULT_TOLERANCE 0.001 /* DEF_SEARCH_TOLERANCE, fp_handler.c:41 */
#define TFP_NULL_MICRO INT32_MIN /* a max1/max2 value the reference stores as SQL NULL */

enum {
  TFP_OK = 0,
  TFP_E_ARG = -1,       /* bad argument (NULL pointer, bad size, coefs out of range ...) */
  TFP_E_HIP = -2,       /* HIP runtime / kernel launch failure */
  TFP_E_NOMEM = -3,     /* device or host allocation failed */
  TFP_E_NOENT = -4,     /* uuid not in the index */
  TFP_E_CAPACITY = -5,  /* caller buffer too small (needed size returned through out param) */
  TFP_E_EXISTS = -6,    /* uuid already indexed */
  TFP_E_NODEV = -7,     /* no usable gfx950 device */
  TFP_E_FORMAT = -8     /* audio the engine cannot take exactly (tfp_wav_*) or a malformed file */
};

typedef struct tfp_engine tfp_engine;
typedef struct tfp_plan tfp_plan;

/* One fingerprint row = one 256-sample hop (reference JSON row {frame_idx, audio_uuid,
 * max1, max2}, fp_handler.c:645-652). m1/m2 are the values as STORED: printf("%f") of
 * 10*log10|c| in integer micro-units (db_ctx_handler.c:479-481); TFP_NULL_MICRO where the
 * reference stores NULL. q1/q2 are the unrounded doubles the search loop reads back
 * (fp_handler.c:290,321); -inf where the key is absent. */
typedef struct tfp_frame {
  int32_t frame_idx;
  int32_t m1;
  int32_t m2;
  int32_t reserved;
  double q1;
  double q2;
} tfp_frame;

/* fp_search_fingerprint_info arguments (fp_handler.h:28-35). coefs in [1,2]; tolerance < 0
 * selects TFP_DEFAULT_TOLERANCE; freq_ignore_* <= 0 disables the filter. */
typedef struct tfp_search_params {
  int32_t coefs;
  int32_t freq_ignore_low;
  int32_t freq_ignore_high;
  int32_t reserved;
  double tolerance;
} tfp_search_params;

/* Result of one search: the reference returns NULL (found = 0) or
 * {uuid,...,frame_count,match_count} (fp_handler.c:394-404). */
typedef struct tfp_result {
  int32_t found;
  int32_t match_count;   /* count(*) of the winning audio_uuid */
  int32_t frame_count;   /* all query frames, ignored ones included */
  int32_t clip_id;       /* engine clip id of the winner, -1 if none */
  char uuid[64];         /* winning audio_uuid, NUL-terminated ("" if none) */
} tfp_result;

/* ---- engine ------------------------------------------------------------------------ */
int tfp_abi_version(void);
int tfp_device_count(int32_t* count);
int tfp_engine_create(int32_t device, tfp_engine** out);
void tfp_engine_destroy(tfp_engine* eng); /* destroy the engine's streams first */
const char* tfp_engine_last_error(const tfp_engine* eng); /* eng == NULL: this thread's last
                                                          * engine-less error (tfp_wav_*). The calling
                                                          * thread's last failure on eng, else eng's
                                                          * latest; the pointer stays valid until this
                                                          * thread's next failing call or last_error
                                                          * read on the same handle */
int64_t tfp_frame_count(int64_t nsamples); /* ceil(n / 256) */

/* ---- host buffers the engine reads in place ------------------------------------------- */
/* Pinned, device-mapped host memory for PCM (new in round 2). Samples handed to a query search
 * (tfp_search_pcm_batch, tfp_search_pcm) or a small tfp_fingerprint_* call from inside such a
 * buffer are read by the GPU where they lie: the call skips copying them into the engine's
 * staging (a 5 s query is 80 KB, several microseconds of batch-1 latency). Any other caller memory
 * works as before. Thread-safe, usable with every engine; the buffer must stay allocated until
 * the call that reads it returns. The Asterisk shim reads WAV files straight into one.
 * tfp_host_alloc: TFP_E_ARG for bytes == 0 or out == NULL, TFP_E_NOMEM when allocation fails. */
int tfp_host_alloc(size_t bytes, void** out);
void tfp_host_free(void* p); /* NULL is a no-op; p must come from tfp_host_alloc */

/* ---- audio ingest: the aubio_source step of create_audio_fingerprints ------------------ */
/* RIFF/WAVE -> mono int16 PCM at the file's native rate (fp_handler.c:37 DEF_AUBIO_SAMPLERATE 0,
 * :604, :633). Accepts integer PCM (format 1, or EXTENSIBLE with the PCM subformat), mono,
 * 16-bit (samples as stored) or 8-bit ((u - 128) << 8: aubio's (u - 128) / 128 exactly). Other
 * audio has aubio values between int16 steps (multichannel mean, 24/32-bit, float) and returns
 * TFP_E_FORMAT. A data size of 0 or past the end of the bytes takes the whole samples present.
 * pcm == NULL (cap 0) only sets *nsamples / *sample_rate; cap < samples -> TFP_E_CAPACITY with
 * *nsamples set. Host-only (no GPU); errors via tfp_engine_last_error(NULL). */
int tfp_wav_decode(const void* bytes, int64_t nbytes, int16_t* pcm, int64_t cap, int64_t* nsamples,
                   int32_t* sample_rate);
int tfp_wav_read(const char* path, int16_t* pcm, int64_t cap, int64_t* nsamples, int32_t* sample_rate);
/* RIFF/WAVE -> the fp32 mono hop values aubio_source_do produces (fp_handler.c:604, :633), for
 * every file tfp_wav_decode refuses as well: 8/16/24/32-bit integer PCM and 32/64-bit float
 * (format 3, or EXTENSIBLE), any channel count. Per sample: unsigned 8-bit (u - 128) / 128,
 * signed w-bit x / 2^(w-1) (32-bit x rounded to float first, as libsndfile's normalised read),
 * float as stored, double rounded to float; per frame the channels are summed in fp32 in channel
 * order and divided by the channel count in fp32 (aubio 0.4.5 sndfile/wavread downmix). Feed
 * the result to tfp_fingerprint_f32_batch / tfp_search_f32_batch. Same size-query, capacity and
 * error conventions as tfp_wav_decode. Host-only. */
int tfp_wav_decode_f32(const void* bytes, int64_t nbytes, float* x, int64_t cap, int64_t* nsamples,
                       int32_t* sample_rate);
int tfp_wav_read_f32(const char* path, float* x, int64_t cap, int64_t* nsamples, int32_t* sample_rate);

/* ---- G.711 ingest: mu-law / A-law codes, one byte per sample (new) ----------------------- */
/* Telephony audio is G.711: a channel's native payload, Asterisk's .ulaw / .alaw prompt files, WAVs
 * with format tag 6 or 7. libsndfile, the backend of new_aubio_source (fp_handler.c:604), hands
 * aubio_source_do (fp_handler.c:633) exactly table[code] / 32768 for such a file, table being the
 * 16-bit expansion libsndfile, Asterisk and Python's audioop share. That is the value the int16
 * paths compute from the int16 table[code], so a fingerprint from codes equals the fingerprint of
 * the expanded int16 bit for bit, for all 256 codes of both laws: exact, no tolerance. The code
 * forms below move one byte per sample to the GPU and expand there, in front of the unchanged
 * fingerprint kernels. Any law other than these two is TFP_E_ARG everywhere. */
enum { TFP_G711_ULAW = 0, TFP_G711_ALAW = 1 };
/* codes[n] -> pcm[n], the expansion aubio_source reads (fp_handler.c:604, :633): mu-law range
 * +-32124 (0x7F and 0xFF both 0), A-law +-32256. n = 0 is TFP_OK; a NULL pointer with n > 0 or a
 * bad law is TFP_E_ARG. Host-only. The search forms without a code twin (ranked, scoped, census,
 * sliding, aligned, occurrences) take the output of this call through their pcm form. */
int tfp_g711_decode(const uint8_t* codes, int64_t n, int32_t law, int16_t* pcm);
/* RIFF/WAVE -> the codes as stored, for the files new_aubio_source opens through libsndfile
 * (fp_handler.c:604, :633): mono, 8-bit, format tag 6 (A-law) or 7 (mu-law), or EXTENSIBLE with
 * that sub-format; *law receives TFP_G711_ALAW / TFP_G711_ULAW. Everything else (PCM, float, more
 * than one channel, bits != 8, a block align that is not 1) is TFP_E_FORMAT with a reason. The
 * size query (codes == NULL, cap 0), TFP_E_CAPACITY, unpatched data sizes and truncated files as
 * tfp_wav_decode. tfp_wav_decode and tfp_wav_decode_f32 keep refusing tags 6 and 7. Host-only. */
int tfp_wav_decode_g711(const void* bytes, int64_t nbytes, uint8_t* codes, int64_t cap, int64_t* nsamples,
                        int32_t* sample_rate, int32_t* law);
int tfp_wav_read_g711(const char* path, uint8_t* codes, int64_t cap, int64_t* nsamples, int32_t* sample_rate,
                      int32_t* law);

/* ---- fingerprinting: create_audio_fingerprints (fp_handler.c:577-671) -------------- */
/* sample_rate, here and in every call below that takes one (the search-from-PCM forms, plans,
 * streams, live calls, groups): any rate >= 1 is taken, as aubio 0.4.5 takes it
 * (aubio_filterbank_set_triangle_bands only warns when bands pass Nyquist; their filters are then
 * empty and their log rows the constant log of the clamped 0). A rate <= 0 is refused with
 * TFP_E_ARG and "bad sample rate <rate>" in tfp_engine_last_error; nothing else about a rate is
 * refused (the filterbank schedule's own size limit is met by no rate). Tables are built per rate on
 * first use and kept for the engine's lifetime. Rates whose filterbank schedule has the 8 kHz shape
 * (7954..7959 and 7997..8020 Hz) run the 8 kHz kernels on their own tables, every other rate the
 * generic kernel; the frames are bit-exact either way. */
/* One clip of mono int16 PCM at its native rate (DEF_AUBIO_SAMPLERATE 0, :37). */
int tfp_fingerprint_pcm(tfp_engine* eng, const int16_t* pcm, int64_t nsamples, int32_t sample_rate,
                        tfp_frame* out, int64_t cap, int64_t* nframes);
/* Many clips: offsets[nclips+1] are sample offsets into pcm; frames are concatenated in
 * clip order (clip c starts at sum of tfp_frame_count of clips < c). */
int tfp_fingerprint_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                          int32_t sample_rate, tfp_frame* out, int64_t cap, int64_t* nframes);
/* The same over fp32 hop values (tfp_wav_decode_f32: multichannel, 24/32-bit or float audio):
 * aubio's x is taken as given instead of int16 / 32768. For int16-valued input (x = s / 32768)
 * the frames equal tfp_fingerprint_batch's on s. */
int tfp_fingerprint_f32_batch(tfp_engine* eng, const float* x, const int64_t* offsets, int32_t nclips,
                              int32_t sample_rate, tfp_frame* out, int64_t cap, int64_t* nframes);
/* The same over G.711 codes (aubio_source on a mu-law / A-law file, fp_handler.c:604, :633):
 * offsets[nclips+1] index into codes, the outputs are tfp_fingerprint_batch's. The frames equal
 * tfp_fingerprint_batch on tfp_g711_decode(codes) bit for bit. The codes are copied to the GPU (1 B
 * per sample), expanded there by one launch, and fingerprinted by the launch an int16 batch of the
 * same lengths takes (tfp_fingerprint_stats counts it alike). */
int tfp_fingerprint_g711_batch(tfp_engine* eng, const uint8_t* codes, const int64_t* offsets, int32_t nclips,
                               int32_t law, int32_t sample_rate, tfp_frame* out, int64_t cap, int64_t* nframes);
/* G.711 expansion on the GPU so far (aubio_source's table[code], fp_handler.c:604, :633): launches of
 * the batch expansion (fingerprint and search calls over codes; a group's query-sharded batches),
 * stream ticks whose scatter expanded codes, and the codes they took. Counted where the kernels are
 * issued. Any pointer may be NULL. */
int tfp_g711_stats(tfp_engine* eng, int64_t* expand_launches, int64_t* stream_launches, int64_t* codes);

/* Device-resident batches (inputs already in HBM; used by the benchmark and by callers that
 * keep PCM on the GPU). A plan uploads the clip layout once. d_micro receives 2 int32 per
 * frame (m1, m2), d_db 2 doubles per frame (q1, q2) or may be NULL.
 *
 * The stream contract of the five device forms (tfp_fingerprint_device, tfp_index_add_device,
 * tfp_search_device, tfp_search_q_device, tfp_synth_pcm_device; tests/test_gpu_stream_order.py):
 * - stream == NULL: the work runs on the engine's own, non-blocking stream, ordered after the work
 *   queued on the HIP null stream before the call and before the work queued on it after the call
 *   returns (the null stream is torch's default stream). Only the null stream is ordered: no other
 *   stream of the caller's is waited for.
 * - stream != NULL (a hipStream_t): every kernel and copy that reads the caller's device inputs
 *   or writes the caller's device outputs is queued on that stream, behind its earlier work. (The
 *   engine's own small uploads, the clip layout or the synth specs, go through its own stream and
 *   are waited for on the host before the launch that reads them.)
 * - tfp_fingerprint_device returns after its launch, without waiting: its outputs are ready to
 *   later work on the same stream (stream == NULL: on the null stream), or after tfp_synchronize.
 * - The other four wait on the host for the work they queued before they return (a
 *   tfp_index_add_device of no frames queues none): their outputs are complete on return.
 * Work on two streams that share one of HIP's hardware queues runs in submission order, whatever
 * the contract leaves unordered. */
int tfp_plan_create(tfp_engine* eng, const int64_t* offsets, int32_t nclips, int32_t sample_rate,
                    tfp_plan** out);
void tfp_plan_destroy(tfp_plan* plan);
int64_t tfp_plan_frames(const tfp_plan* plan);
int tfp_fingerprint_device(tfp_engine* eng, const tfp_plan* plan, const int16_t* d_pcm, int32_t* d_micro,
                           double* d_db, void* stream);
/* Fingerprint kernel launches so far, by kernel and from every entry point (host batches, plans,
 * the search-from-PCM forms, stream ticks and window read-outs): the small 8 kHz launch (4-frame
 * tiles, batches of few frames), the throughput 8 kHz launch, and the generic kernel over int16 and
 * over fp32 samples (other sample rates, fp32 input). Counted where the kernel is issued; a call
 * with no frames launches nothing. Any pointer may be NULL. */
int tfp_fingerprint_stats(tfp_engine* eng, int64_t* small8k, int64_t* throughput8k, int64_t* generic_i16,
                          int64_t* generic_f32);

/* ---- enrolled index: the audio_fingerprint table (fp_handler.c:713-753) ------------- */
/* Append one clip's rows (create_audio_fingerprint_info). m1/m2 in micro-units. */
int tfp_index_add(tfp_engine* eng, const char* uuid, const int32_t* m1, const int32_t* m2, int32_t nframes,
                  int32_t* clip_id);
/* Append nclips clips whose rows are already on the device: d_micro holds 2 int32 per frame
 * in the layout tfp_fingerprint_device writes, frame_offsets[nclips+1] on the host. */
int tfp_index_add_device(tfp_engine* eng, int32_t nclips, const char* const* uuids, const int64_t* frame_offsets,
                         const int32_t* d_micro, void* stream);
/* Append nclips clips from host rows (m1/m2 indexed by frame_offsets[0..nclips]); the bulk
 * form of tfp_index_add used to load an audio_recongition.db snapshot (fp_init ->
 * db_ctx_load_db_data, fp_handler.c:68-90, db_ctx_handler.c:750-772). All-or-nothing on
 * argument errors (bad/duplicate uuid). */
int tfp_index_add_batch(tfp_engine* eng, int32_t nclips, const char* const* uuids, const int64_t* frame_offsets,
                        const int32_t* m1, const int32_t* m2);
/* Read back one clip's stored rows in frame order (for the fp_term backup,
 * db_ctx_backup db_ctx_handler.c:673-717). *nframes always receives the row count;
 * TFP_E_CAPACITY if cap is smaller. */
int tfp_index_rows(tfp_engine* eng, const char* uuid, int32_t* m1, int32_t* m2, int64_t cap, int64_t* nframes);
int tfp_index_remove(tfp_engine* eng, const char* uuid);
int tfp_index_clear(tfp_engine* eng);
int tfp_index_stats(tfp_engine* eng, int64_t* nrows, int32_t* nclips);
/* Rebuild the sorted device index now (otherwise done lazily by the next search). After the first
 * build, adds and removals are merged into the sorted index in one pass over it (the added rows
 * alone are sorted), as the reference's INSERTs update its max1 B-tree (fp_handler.c:559-571,
 * :745-753); a full re-sort happens only for the first build, after many removals (staging
 * compaction) or when the new rows outnumber half the index. */
int tfp_index_commit(tfp_engine* eng);
/* How the index was brought up to date so far: full sorts and incremental merges (new in round 3;
 * either pointer may be NULL). */
int tfp_index_build_stats(tfp_engine* eng, int64_t* full_builds, int64_t* merges);
/* Index delta (new in round 4): up to 512 clips enrolled since the last merge are searched beside
 * the sorted index by the coefs = 1 paths (the dialplan's, application_handler.c:180) without a
 * merge: an enrolment then costs its own rows, as the reference's INSERT into its B-tree does
 * (fp_handler.c:559-571, :745-753). coefs = 2 searches (round 6) sweep the delta's own clip-set cache
 * beside the main one. The delta is merged when it outgrows that, when a clip of the sorted index is
 * removed, or before a search that reads the sorted rows (a coefs = 1 tolerance above 8, a coefs = 2
 * tolerance above 0.49, a row-scan fallback); results are unchanged either way. TFP_INDEX_DELTA=0 at engine
 * creation turns it off. Stats: delta updates so far and the clips in the delta now. */
int tfp_index_delta_stats(tfp_engine* eng, int64_t* delta_updates, int32_t* delta_clips);
/* The coefs = 2 clip-set caches (new in round 6): builds so far, searches served by a cached
 * tolerance (the active one or one of three others kept, least recently used out), builds made from
 * the clip order (tolerances up to 0.49: a filter, no sort), the clip order's full builds (one
 * radix sort per full index build, when first needed) and merges (carried through every index
 * merge), and the index delta's caches built and sweeps run over them (an enrolment followed by a
 * coefs = 2 search: the main caches stay, the delta's rows get their own). Any pointer may be NULL. */
int tfp_index_cache_stats(tfp_engine* eng, int64_t* cache_builds, int64_t* cache_hits, int64_t* from_order,
                          int64_t* order_builds, int64_t* order_merges, int64_t* delta_cache_builds,
                          int64_t* delta_sweeps);
/* The coefs = 2 sweep's frame sort per batch (new in round 6): batches whose hand-written bin sort
 * stood, batches sorted by the library sort (a first pass that could not take the bin sort, or the
 * redo), speculative passes redone (an overfull bin, a window width outside the packed key, a frame
 * for the row scan), and the crowd bins (one value: the silence floor) the bin sort copied unsorted.
 * Any pointer may be NULL. */
int tfp_sweep_stats(tfp_engine* eng, int64_t* bins, int64_t* library, int64_t* redone, int64_t* crowd_bins);
/* Which form served each plain-search batch so far (tfp_search*, the device forms, streams; not the
 * ranked, scoped, census or sliding forms, which have their own counters): the small vote (up to 8
 * queries of up to 2048 frames), the coefs = 1 vote by pattern classes and by the GEMM, votes the
 * host redid on the general path (a per-key count above 2048, a key outside the vote range), and
 * passes of the general path that produced the batch's results (every coefs = 2 batch, coefs = 1
 * queries of 16384 frames and more, the redone votes). Counted in the branch that wrote the
 * results. Any pointer may be NULL. */
int tfp_search_path_stats(tfp_engine* eng, int64_t* small, int64_t* vote_class, int64_t* vote_gemm,
                          int64_t* vote_redone, int64_t* general);
/* Multi-GPU sharding: override the tie-break key of each live clip (default: its rank among
 * this engine's uuids). keys[clip_id] must order like the uuids across all shards and be
 * distinct over live clips. A clip added after this call has no key: the next search (or
 * tfp_index_commit) fails with TFP_E_ARG until the keys are set again; nclip_ids = 0 clears
 * the override.
 *
 * The keys' contract (the same for tfp_index_update_tiebreak): the keys of live clips lie in
 * [0, INT32_MAX] (both ends included: a result is count << 32 | key with the key as its unsigned low
 * half, and every search form is exact over that whole range), they are distinct, and they order like
 * the uuids. A live clip with a negative key, or two live clips with one key, fail the next index
 * update (tfp_index_commit or a search) with TFP_E_ARG and a message that names the key, on the full
 * build and on the index delta's path alike. Keys given to clip ids that are not live (removed
 * clips) are ignored, whatever their value: a device group passes -1 for those. */
int tfp_index_set_tiebreak(tfp_engine* eng, const int32_t* keys, int32_t nclip_ids);
/* The override's keys of clip ids [first_clip_id, first_clip_id + n) only (new in round 6): a device
 * group gives each clip enrolled since the last update its key without re-sending every clip's
 * (first_clip_id <= the number of keys set so far). Keys of clips added since the last index update
 * cost the next update O(new clips); keys of older clips refresh every column's. */
int tfp_index_update_tiebreak(tfp_engine* eng, int32_t first_clip_id, const int32_t* keys, int32_t n);

/* ---- search: fp_search_fingerprint_info (fp_handler.c:207-408) ---------------------- */
int tfp_search(tfp_engine* eng, const tfp_frame* frames, int32_t nframes, const tfp_search_params* params,
               tfp_result* out);
/* qoffsets[nqueries+1] index into frames. */
int tfp_search_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                     const tfp_search_params* params, tfp_result* out);
/* PCM in, results out: fingerprints the queries on the GPU and searches without a host
 * round trip of the frames (fp_handler.c:275 + :287-374). */
int tfp_search_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                         int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
/* The same over fp32 hop values (tfp_wav_decode_f32). */
int tfp_search_f32_batch(tfp_engine* eng, const float* x, const int64_t* offsets, int32_t nqueries,
                         int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
/* The same over G.711 codes (fp_handler.c:604, :633 on a mu-law / A-law recording, then :275 +
 * :287-374): the results equal tfp_search_pcm_batch on tfp_g711_decode(codes). Not coalesced: the
 * coalescer gathers its callers' int16 buffers by pointer, and joining several callers' code arrays
 * would cost a host copy each, so a call runs serialised per engine like every other call. */
int tfp_search_g711_batch(tfp_engine* eng, const uint8_t* codes, const int64_t* offsets, int32_t nqueries,
                          int32_t law, int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
/* Queries in separate buffers (new in round 4): query i is the nsamples[i] int16 samples at pcms[i].
 * The results equal tfp_search_pcm_batch's over the same queries laid end to end. Samples inside
 * tfp_host_alloc buffers are read in place wherever they lie (one per channel recording, say).
 *
 * Concurrent callers (new in round 4). The reference runs one fp_search_fingerprint_info per channel
 * thread (application_handler.c:180) on one shared handle (fp_handler.c:1161-1169). Calls of
 * tfp_search_pcm_batch, tfp_search_f32_batch and tfp_search_pcm_gather with at most 16 queries each
 * are coalesced: a call made while another batch runs on the engine waits for it, then runs together
 * with every other waiting call of the same sample format, rate and search parameters as one batch
 * (<= 512 queries). A lone call runs at once. Each call gets exactly its own results.
 * TFP_COALESCE=0 in the environment at engine creation turns this off. tfp_search_coalesce_stats:
 * calls taken through the coalescer and the batches they ran as (either pointer may be NULL). */
int tfp_search_pcm_gather(tfp_engine* eng, const int16_t* const* pcms, const int64_t* nsamples, int32_t nqueries,
                          int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
int tfp_search_coalesce_stats(tfp_engine* eng, int64_t* calls, int64_t* batches);
/* Device form for benchmarks / sharded search: per query a 64-bit key
 * (match_count << 32 | tiebreak key), 0 = NOTFOUND, written to d_keys[nqueries] (device).
 * The maximum key over shards is the global winner (RCCL allreduce MAX). */
int tfp_search_device(tfp_engine* eng, const tfp_plan* plan, const int16_t* d_pcm,
                      const tfp_search_params* params, uint64_t* d_keys, void* stream);
/* The same from frame values already on the device: d_q holds 2 doubles per frame (q1, q2 as
 * tfp_fingerprint_device writes them to d_db), queries at frame offsets qoffsets[nqueries+1]
 * (host). Lets N ranks each fingerprint 1/N of a query batch, all-gather the frame values and
 * search their clip shard (the reference's per-frame SQL, fp_handler.c:287-374, on q1/q2). */
int tfp_search_q_device(tfp_engine* eng, const double* d_q, const int64_t* qoffsets, int32_t nqueries,
                        const tfp_search_params* params, uint64_t* d_keys, void* stream);
/* Map a tie-break key from tfp_search_device back to the uuid (this engine's clips only). */
int tfp_index_uuid_of_key(tfp_engine* eng, int32_t key, char* uuid, int32_t len);

/* ---- ranked search: the result query's first k rows (fp_handler.c:367-374) ------------ */
/* The reference's result query, "select *, count(*) from temp group by audio_uuid order by
 * count(*) DESC" (fp_handler.c:367-374), yields one row per clip that matched a frame; the
 * reference reads the first (:376-392). SQLite returns the rows by count descending, tied counts
 * by audio_uuid descending. These calls return the first k rows, so a caller sees the runner-up
 * and the winner's margin over it. out[q * k + r] is row r of query q; counts[q] = min(k, clips
 * with a non-zero count); entries past counts[q] are zeroed. Row 0 is what tfp_search_batch
 * returns for the same call. A query with no frames, or with every frame ignored, has counts[q] =
 * 0. k < 1, k > TFP_RANK_MAX or coefs outside [1,2] is TFP_E_ARG. Calls are not coalesced. */
#define TFP_RANK_MAX 32
typedef struct tfp_candidate {   /* one row of the reference's result set (fp_handler.c:367-374) */
  int32_t match_count;           /* count(*) of this audio_uuid, > 0 */
  int32_t clip_id;               /* engine clip id (group calls: the shard, as tfp_result) */
  char uuid[64];                 /* audio_uuid, NUL-terminated */
} tfp_candidate;
/* One query, fp_handler.c:367-374 read to row k; out[k], *count as counts[0]. */
int tfp_search_ranked(tfp_engine* eng, const tfp_frame* frames, int32_t nframes, const tfp_search_params* params,
                      int32_t k, tfp_candidate* out, int32_t* count);
/* fp_handler.c:367-374 per query; qoffsets[nqueries+1] index into frames, out[nqueries*k], counts[nqueries]. */
int tfp_search_ranked_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                            const tfp_search_params* params, int32_t k, tfp_candidate* out, int32_t* counts);
/* PCM in (fp_handler.c:275 + :287-374), rows out: the queries as tfp_search_pcm_batch takes them. */
int tfp_search_ranked_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                int32_t sample_rate, const tfp_search_params* params, int32_t k, tfp_candidate* out,
                                int32_t* counts);
/* Ranked batches served so far by the vote form (coefs = 1: the rows of fp_handler.c:367-374 counted
 * from the key bitsets) and by the general form (coefs = 2, or a frame value outside the key range:
 * counted over the sorted rows). Either pointer may be NULL. */
int tfp_rank_stats(tfp_engine* eng, int64_t* vote_batches, int64_t* general_batches);

/* ---- context-scoped search: the result query over one context's clips (new) ------------- */
/* Every search entry point of the reference takes a context, and its documentation promises a scoped
 * search: the application "attempts to detect the given channel's voice is in the list of the given
 * tiresias's context" (doc/dialplan_application.rst:11) and FOUND means found "from the context's
 * audio list" (doc/dialplan_application.rst:52-53). Its per-frame insert (fp_handler.c:308-314) has
 * no context predicate, so tfp_search_batch and every call above span all contexts, as the reference
 * does. The calls below run the search the documentation describes.
 *
 * A clip carries a scope, an int32 >= 0; a new clip has scope 0. The engine knows nothing of context
 * names: the caller maps them to scope ids. A scoped search of a query with scope s returns the first
 * k rows of the result query (fp_handler.c:367-374) when the per-frame insert (fp_handler.c:308-314)
 * also carries "and context = '<s>'", which is the unmodified SQL over a table holding scope s's
 * clips only: rows by count descending, tied counts by audio_uuid descending, clips with a non-zero
 * count only. The restriction is applied where the rows are selected on the GPU, not to the global
 * first k rows (a scope's best clip may lie below any global row). frame_count is unaffected. */
#define TFP_SCOPE_ANY (-1) /* a query's scope: every clip (equals tfp_search_ranked_batch row for row) */
/* Set the scopes of n clips (the context column of fp_handler.c:713-753, which fp_handler.c:308-314
 * never reads). All or nothing: an unknown uuid is TFP_E_NOENT, a negative scope TFP_E_ARG, and no
 * scope has changed then. A scope may be changed at any time; the next search sees it. It follows
 * the clip through every index update and goes away with tfp_index_remove and tfp_index_clear. */
int tfp_index_set_scope(tfp_engine* eng, int32_t n, const char* const* uuids, const int32_t* scopes);
/* A clip's scope read back (doc/dialplan_application.rst:52-53: which context's audio list holds it). */
int tfp_index_scope(tfp_engine* eng, const char* uuid, int32_t* scope);
/* fp_handler.c:367-374 per query over the clips of scopes[q] (fp_handler.c:308-314 with the context
 * predicate of doc/dialplan_application.rst:11): out, counts, the zeroing and the argument rules
 * exactly as tfp_search_ranked_batch; scopes[nqueries], each TFP_SCOPE_ANY or >= 0, below -1 is
 * TFP_E_ARG. A scope no live clip has gives counts[q] = 0. */
int tfp_search_scoped_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                            const tfp_search_params* params, const int32_t* scopes, int32_t k, tfp_candidate* out,
                            int32_t* counts);
/* PCM in (fp_handler.c:275 + :287-374 with the context predicate at :308-314), rows out (:367-374):
 * the queries as tfp_search_ranked_pcm_batch takes them (doc/dialplan_application.rst:11). */
int tfp_search_scoped_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                int32_t sample_rate, const tfp_search_params* params, const int32_t* scopes, int32_t k,
                                tfp_candidate* out, int32_t* counts);
/* Scoped batches served so far by the vote form and by the general form (as tfp_rank_stats: the rows
 * of fp_handler.c:367-374 under the predicate at :308-314, doc/dialplan_application.rst:11), and
 * builds of the per-column scope table on the device: one after each index update or scope change
 * that a scoped search follows, none per search. Any pointer may be NULL. */
int tfp_scope_stats(tfp_engine* eng, int64_t* vote_batches, int64_t* general_batches, int64_t* table_builds);

/* ---- match census: how every clip's count is distributed, per query (new) ---------------- */
/* Every search above returns the head of the result query (fp_handler.c:367-374): the winner, or up
 * to TFP_RANK_MAX rows. The census says how those rows stand against the rest of the catalog: per
 * query, the exact number of clips of the query's scope at each count(*), which is the reference's
 * own SQL one level up,
 *   select c, count(*) from (select count(*) c from temp group by audio_uuid) group by c
 * over the temp table of fp_handler.c:287-351 (with the context predicate of tfp_search_scoped_batch
 * at :308-314 for a scope >= 0). A clip's count is exactly the match_count tfp_search_scoped_batch
 * would report for it were k unbounded: the same coefs, tolerance < 0, ignore filters and NULL rules.
 *
 * hist[q * nbins + c], 1 <= c <= F_q (the query's frames): live clips of scope scopes[q] with count
 * c. hist[q * nbins + 0]: live clips of the scope with count 0, row-less clips included, removed
 * clips not (the scope's live clips minus the other bins). hist[q * nbins + c] = 0 for c > F_q. A
 * scope no live clip has, and an empty index, give an all-zero row. The application's ratio test
 * (application_handler.c:180-203) reads off it how many clips reach the winner's count, how many tie
 * with it and how many lie within a margin of it. Rows of index shards add up bin by bin. */
/* fp_handler.c:287-374 per query, counted by count(*) instead of read from the top. scopes[nqueries]
 * (TFP_SCOPE_ANY or >= 0), or NULL for TFP_SCOPE_ANY everywhere. *need_bins always receives
 * max_q F_q + 1; if nbins is below it the call returns TFP_E_CAPACITY and writes nothing else.
 * TFP_E_ARG: coefs outside [1,2], a scope below -1, non-monotone offsets, NULL need_bins. Calls are
 * not coalesced. */
int tfp_census_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                     const tfp_search_params* params, const int32_t* scopes, int32_t nbins, int32_t* hist,
                     int32_t* need_bins);
/* PCM in (fp_handler.c:275), census out (:287-374 counted by count(*)): the queries as
 * tfp_search_scoped_pcm_batch takes them; query q has tfp_frame_count(samples) frames. The frame
 * values stay on the device between the fingerprint and the census. */
int tfp_census_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries, int32_t sample_rate,
                         const tfp_search_params* params, const int32_t* scopes, int32_t nbins, int32_t* hist,
                         int32_t* need_bins);
/* Census batches served so far by the vote form (coefs = 1, every key in range: the counts of
 * fp_handler.c:367-374 from the key bitsets) and by the general form (every other batch, counted
 * over the sorted rows). Either pointer may be NULL. */
int tfp_census_stats(tfp_engine* eng, int64_t* vote_batches, int64_t* general_batches);
/* Clips with count(*) >= count in one census row (fp_handler.c:367-374: the rows down to that
 * count; with the winner's match_count, application_handler.c:180-203, the winner and its ties):
 * the sum of hist_row[c] for c >= count, bin 0 excluded unless count <= 0. Host-only. */
int64_t tfp_census_at_least(const int32_t* hist_row, int32_t nbins, int32_t count);

/* ---- sliding search: the ranked rows of every window of a long recording (new) ------------- */
/* The reference records a fixed `duration` ms (default 3000) and searches that one window
 * (application_handler.c:152-185, fp_handler.c:275-374). A caller with a whole call recording wants
 * to know whether, and when, an enrolled clip occurs in it. The calls below search every window of a
 * recording in one call: the recording is fingerprinted once, and the vote moves from one window to
 * the next (the hop frames that left are subtracted, the hop that entered added) instead of being
 * rebuilt, in exact integer arithmetic over the same key bitsets ranked search reads.
 *
 * Windows. A recording is the frames [qoffsets[r], qoffsets[r+1]) of frames, F_r of them. With
 * window >= 1 and hop >= 1, window w of recording r is the `window` consecutive frames from
 * qoffsets[r] + w * hop, and a recording of F frames has
 *     nwin(F) = F < window ? 0 : (F - window) / hop + 1
 * windows: trailing frames no full window covers are not searched. The windows of all recordings are
 * numbered in order: woff[0] = 0, woff[r+1] = woff[r] + nwin(F_r).
 *
 * Rows. For window j = woff[r] + w, out[j * k + i] and counts[j] are exactly what
 * tfp_search_scoped_batch returns for one query made of that window's frames with scope scopes[r]
 * (TFP_SCOPE_ANY: tfp_search_ranked_batch's rows): the first k rows of fp_handler.c:367-374 run over
 * those frames alone, by count descending, tied counts by audio_uuid descending, clips with a
 * non-zero count only; entries past counts[j] are zeroed; every window's frame_count is `window`.
 *
 * PCM form. Each recording is fingerprinted once, as one clip (fp_handler.c:275), and a window's rows
 * are those of the recording's own frame values, not of a fresh fingerprint of the cut-out samples:
 * the two differ only in each cut's frame 0, which would see zero history where the recording has
 * the previous hop (aubio_pvoc_do's sliding buffer, fp_handler.c:577-671). Window 0 of a recording
 * equals tfp_search_ranked_pcm_batch on its first window * 256 samples. */
#define TFP_SLIDE_RUN 32 /* consecutive windows of a recording one GPU block scores in turn */
/* nwin above for a recording of nframes frames (the window fp_handler.c:275-374 searches, moved by
 * hop); 0 for any non-positive argument. Host-only. */
int64_t tfp_sliding_windows(int64_t nframes, int32_t window, int32_t hop);
/* fp_handler.c:367-374 per window of each of nrecordings recordings (application_handler.c:152-185
 * moved along the recording). scopes[nrecordings], or NULL for TFP_SCOPE_ANY everywhere. *nwindows
 * always receives woff[nrecordings]; if that exceeds cap_windows (the rows out holds: out[cap_windows
 * * k], counts[cap_windows]) the call returns TFP_E_CAPACITY and writes nothing else. TFP_E_ARG:
 * window < 1, hop < 1, k outside [1, TFP_RANK_MAX], coefs outside [1,2], a scope below -1,
 * non-monotone offsets. No recordings, empty recordings and recordings shorter than window give no
 * window, and a call without a window or with an empty index launches nothing (an empty index: every
 * counts[j] = 0). Calls are not coalesced. */
int tfp_search_sliding_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nrecordings,
                             const tfp_search_params* params, int32_t window, int32_t hop, const int32_t* scopes,
                             int32_t k, tfp_candidate* out, int32_t* counts, int64_t cap_windows, int64_t* nwindows);
/* PCM in (fp_handler.c:275, each recording once), rows out per window (:287-374): the recordings as
 * tfp_search_ranked_pcm_batch takes its queries; a recording of n samples has tfp_frame_count(n)
 * frames. The frame values stay on the device between the fingerprint and the slide. */
int tfp_search_sliding_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nrecordings,
                                 int32_t sample_rate, const tfp_search_params* params, int32_t window, int32_t hop,
                                 const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                 int64_t cap_windows, int64_t* nwindows);
/* Sliding batches served so far by the vote form (coefs = 1, every key in range, tolerance in [0, 8]:
 * the rows of fp_handler.c:367-374 slid over the key bitsets) and by the general form (every other
 * batch: the windows laid end to end and counted over the sorted rows), and the windows they held.
 * Any pointer may be NULL. */
int tfp_slide_stats(tfp_engine* eng, int64_t* vote_batches, int64_t* general_batches, int64_t* windows);

/* ---- aligned search: where in the clip a candidate matches (new; no reference counterpart) --- */
/* The reference's count (fp_handler.c:287-374) says how many query frames found a row of the clip,
 * not where, nor whether the hits line up in time: the inserted rows carry frame_idx (:287-359
 * "select * from audio_fingerprint"), but the result query (:367-374) never reads it. A clip's
 * stored rows j = 0..N-1 are in frame order, so with the query's frames i = 0..F-1 and hit(i, j) =
 * "frame i runs its SQL and row j satisfies its predicate" (:287-351: max1, and max2 where the
 * clause is present, non-NULL and inside the frame's printed bounds), the histogram over the
 * diagonals hist[d] = #{(i, j) : hit(i, j), j - i = d}, d in [-(F-1), N-1], gives
 *   aligned_count = max over d of hist[d]           (the hits that agree on one time offset),
 *   offset        = the smallest d attaining it     (query frame i lies at clip frame i + offset;
 *                                                    negative: the recording starts before the clip),
 *   first_frame, last_frame = the least and greatest i with hit(i, i + offset).
 * All four are 0 when no row hits. For a row a ranked search returns, 1 <= aligned_count <=
 * match_count. Exact integers; coefs, tolerance < 0 and the ignore filters as in tfp_search_params.
 * The clip's rows are read as enrolled: no tfp_index_commit is needed. Calls are not coalesced. */
typedef struct tfp_alignment {
  int32_t aligned_count;
  int32_t offset;
  int32_t first_frame;
  int32_t last_frame;
} tfp_alignment;
/* Query q against clips clip_ids[q * k + r], r < k: out[q * k + r]. An id of -1 gives a zeroed row
 * (a ranked result's unused entries pass straight through); any other id out of range or of a
 * removed clip is TFP_E_NOENT. k < 1, k > TFP_RANK_MAX or coefs outside [1,2] is TFP_E_ARG. */
int tfp_align_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                    const tfp_search_params* params, const int32_t* clip_ids, int32_t k, tfp_alignment* out);
/* tfp_search_ranked_batch (fp_handler.c:367-374 read to row k: the same cand and counts) plus
 * align[q * k + r] for row r; entries past counts[q] are zeroed. */
int tfp_search_aligned_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                             const tfp_search_params* params, int32_t k, tfp_candidate* cand, tfp_alignment* align,
                             int32_t* counts);
/* tfp_search_ranked_pcm_batch (fp_handler.c:275 + :287-374) plus the rows' alignments; the frame
 * values stay on the device between the search and the alignment. */
int tfp_search_aligned_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                 int32_t sample_rate, const tfp_search_params* params, int32_t k, tfp_candidate* cand,
                                 tfp_alignment* align, int32_t* counts);
/* Batches that reached the alignment kernels so far and the (query, clip) pairs they named (the
 * frames of fp_handler.c:287-351 against the clips' rows). Either pointer may be NULL. */
int tfp_align_stats(tfp_engine* eng, int64_t* batches, int64_t* pairs);

/* ---- sliding aligned search: each window's rows with where the clip lies (new) -------------- */
/* Sliding search above says which clips win each window of a recording by the bag count of
 * fp_handler.c:367-374; aligned search says for one query and a clip on which time offset the hits
 * line up. The calls below do both for every window: window, hop, woff, the rows, counts and k are
 * tfp_search_sliding_batch's, and for window j = woff[r] + w and row i < counts[j], align[j * k + i]
 * is exactly the tfp_alignment tfp_align_batch returns for a query made of that window's `window`
 * frames alone and that row's clip (the per-frame predicate of fp_handler.c:287-351): aligned_count,
 * the smallest offset attaining it, first_frame and last_frame, all window-relative. Window frame x
 * lies at clip frame x + offset, and recording frame w * hop + x lies there too. Entries past
 * counts[j] are zeroed.
 *
 * Joining windows. w * hop - offset is the recording frame at which clip frame 0 lies. Where the
 * occurrence's diagonal is the only one of the window that attains aligned_count, the rows of one
 * occurrence of a clip share that value across windows, and a caller joins the windows with equal
 * (clip, w * hop - offset) into one occurrence, from recording frame w * hop + first_frame of its
 * first window to w * hop + last_frame of its last. Where a window fits the clip equally well in an
 * earlier place (offset is the smallest diagonal attaining the count), that window reports the
 * earlier place: short windows, a high tolerance, and audio whose max1 hardly moves (8 kHz speech
 * and noise span about 1 dB) make such ties common, so a caller takes the value most windows of a
 * stretch agree on, or lengthens the window (48 frames of a clip with varying level were unique in
 * the tests where 24 were not).
 *
 * Consecutive windows share all but hop frames: a clip's diagonal counts move from one window to the
 * next by subtracting the hop frames that left and adding the hop that entered, in exact integer
 * arithmetic over the predicate aligned search tests. The (window, row) entries are grouped by
 * (recording, clip) and cut into runs wherever two successive needed windows share no frame
 * ((w' - w) * hop >= window); a run with one entry, and every run when 2 * hop >= window (a slid step
 * tests 2 * hop * N boxes, a window from scratch window * N), is aligned from scratch (direct), the
 * rest slid. Both give the same integers. Calls are not coalesced. */
/* (The join itself, verified along each candidate's own diagonal over the whole recording, is
 * tfp_search_occurrences_batch below; tfp_trace_batch is its primitive.) */
/* The primitive (fp_handler.c:287-351 per window frame against the named clips' rows): window j of
 * the recordings (as tfp_search_sliding_batch numbers them) against clips clip_ids[j * k + i], i < k:
 * out[j * k + i]; clip_ids[nwindows * k] and out[nwindows * k]. An id of -1 gives a zeroed row; any
 * other id out of range or of a removed clip is TFP_E_NOENT. The argument and capacity rules are
 * tfp_search_sliding_batch's (cap_windows: the windows clip_ids and out hold): *nwindows is always
 * set, and on TFP_E_CAPACITY nothing else is written. TFP_E_CAPACITY also, before anything is
 * written, when window + N exceeds 2^31 or 32 * window + N nears 2^28 for the N rows of the longest
 * enrolled clip (the sizes one launch holds); in the group form a shard finds this after out and
 * counts are written. The clips' rows are read as enrolled: no tfp_index_commit is needed. */
int tfp_align_sliding_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nrecordings,
                            const tfp_search_params* params, int32_t window, int32_t hop, const int32_t* clip_ids,
                            int32_t k, tfp_alignment* out, int64_t cap_windows, int64_t* nwindows);
/* tfp_search_sliding_batch (fp_handler.c:367-374 per window: the same out, counts and *nwindows,
 * byte for byte) plus align[j * k + i] for row i of window j (align[cap_windows * k]). */
int tfp_search_sliding_aligned_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets,
                                     int32_t nrecordings, const tfp_search_params* params, int32_t window, int32_t hop,
                                     const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                     tfp_alignment* align, int64_t cap_windows, int64_t* nwindows);
/* tfp_search_sliding_pcm_batch (fp_handler.c:275 once per recording, :287-374 per window) plus the
 * rows' alignments. The frame values and their boxes stay on the device between the fingerprint, the
 * slide and the alignment. */
int tfp_search_sliding_aligned_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nrecordings,
                                         int32_t sample_rate, const tfp_search_params* params, int32_t window,
                                         int32_t hop, const int32_t* scopes, int32_t k, tfp_candidate* out,
                                         int32_t* counts, tfp_alignment* align, int64_t cap_windows, int64_t* nwindows);
/* Batches that reached the sliding alignment so far, and the (window, clip) entries they computed by
 * the slid form and by the direct form (the frames of fp_handler.c:287-351 against the clips' rows,
 * by the run rule above). An entry is counted where it is computed: a (window, clip) named twice in
 * clip_ids counts once (the second row is a copy), and a clip without rows, an id of -1 and a call
 * that launches nothing count nothing. Any pointer may be NULL. */
int tfp_slide_align_stats(tfp_engine* eng, int64_t* batches, int64_t* slid_entries, int64_t* direct_entries);

/* ---- occurrences: which enrolled clips play in a recording, from which frame to which (new) --- */
/* Sliding aligned search reports per window where its clips lie. A window that covers only the head
 * or tail of an occurrence has few hits on the true diagonal and is often won by another one, and
 * the smallest-diagonal tie rule of `offset` scatters spurious starts, so window rows alone give no
 * exact extent. The calls below verify a start along its own diagonal over the whole recording with
 * the per-frame predicate aligned search tests (fp_handler.c:287-351: hit(x, j) = recording frame x
 * runs its SQL and clip row j is non-NULL and inside the frame's printed bounds, max1, and max2 where
 * the clause is present). The clip's rows are read in frame order as enrolled: no tfp_index_commit is
 * needed. Exact integers. Calls are not coalesced.
 *
 * Trace. A recording of F frames, a clip of N rows and start = s, the recording frame at which clip
 * frame 0 lies (any int32: negative, or past the end). The diagonal covers the recording frames x in
 * [lo, hi), lo = max(0, s), hi = min(F, s + N), and overlap = max(0, hi - lo). Let x_1 < ... < x_h be
 * the frames of [lo, hi) with hit(x, x - s). A segment is a maximal run of them in which consecutive
 * hits are at most max_gap frames apart (x_{i+1} - x_i - 1 <= max_gap; max_gap = INT32_MAX: one
 * segment). The best segment has the most hits, among equals the smallest seg_first. seg_first and
 * seg_last are recording frames counted from the recording's first frame. With no hit every field but
 * overlap is 0. */
typedef struct tfp_trace_req {
  int32_t recording; /* index into qoffsets */
  int32_t clip_id;   /* engine clip id; -1: a zeroed row */
  int32_t start;     /* s */
  int32_t reserved;
} tfp_trace_req;
typedef struct tfp_trace {
  int32_t overlap;   /* frames of the recording the clip covers at this start */
  int32_t hits;      /* h */
  int32_t segments;
  int32_t seg_hits;  /* the best segment: its hits, first and last hitting frame */
  int32_t seg_first;
  int32_t seg_last;
} tfp_trace;
/* The primitive (fp_handler.c:287-351 per recording frame against the one clip row its diagonal
 * meets): out[i] = the trace of reqs[i] at max_gap. clip_id = -1 gives a zeroed row; any other id out
 * of range or of a removed clip is TFP_E_NOENT. TFP_E_ARG: a recording index outside [0, nrecordings),
 * max_gap < 0, coefs outside [1,2], non-monotone offsets; out is untouched then. A request with
 * overlap = 0 is answered on the host, and a call with nothing to trace launches nothing. */
int tfp_trace_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nrecordings,
                    const tfp_search_params* params, const tfp_trace_req* reqs, int64_t nreqs, int32_t max_gap,
                    tfp_trace* out);
/* Occurrences of a call with window, hop, scopes, k, max_gap >= 0 and min_hits >= 1:
 *  1. the rows of tfp_search_sliding_aligned_batch with the same arguments (fp_handler.c:367-374 per
 *     window, each row with its alignment);
 *  2. the candidates are the distinct (r, clip, s = w * hop - offset) over all rows, w being the
 *     window's index inside recording r; `windows` is the number of rows naming the candidate;
 *  3. each candidate is traced once at max_gap, and those with seg_hits < min_hits are dropped;
 *  4. within one (r, clip) the rest are visited by seg_hits descending, then windows descending, then
 *     s ascending, and one is kept unless its [seg_first, seg_last] meets the interval of one already
 *     kept (non-maximum suppression: the earlier-place ties and the partial diagonals around a real
 *     occurrence go);
 *  5. output order: recording ascending, first_frame ascending, hits descending, audio_uuid
 *     descending (the tie order of fp_handler.c:367-374). */
typedef struct tfp_occurrence {
  int32_t recording;
  int32_t clip_id;          /* engine clip id (group calls: the shard, as tfp_candidate) */
  int32_t clip_start_frame; /* s: the recording frame at which clip frame 0 lies */
  int32_t first_frame;      /* seg_first, seg_last of the candidate's trace */
  int32_t last_frame;
  int32_t hits;             /* seg_hits */
  int32_t diagonal_hits;    /* h, over the whole diagonal */
  int32_t overlap;
  int32_t windows;
  char uuid[64];            /* audio_uuid, NUL-terminated */
} tfp_occurrence;
/* fp_handler.c:367-374 per window, fp_handler.c:287-351 along each candidate's diagonal. The argument
 * rules are tfp_search_sliding_batch's, and min_hits < 1 or max_gap < 0 is TFP_E_ARG too.
 * *noccurrences is always set on TFP_OK and TFP_E_CAPACITY; if it exceeds cap (the entries out holds)
 * the call returns TFP_E_CAPACITY and writes nothing else. No recordings, recordings shorter than
 * window and an empty index give no occurrence and launch nothing. */
int tfp_search_occurrences_batch(tfp_engine* eng, const tfp_frame* frames, const int64_t* qoffsets, int32_t nrecordings,
                                 const tfp_search_params* params, int32_t window, int32_t hop, const int32_t* scopes,
                                 int32_t k, int32_t max_gap, int32_t min_hits, tfp_occurrence* out, int64_t cap,
                                 int64_t* noccurrences);
/* PCM in (fp_handler.c:275, each recording once; :287-374 per window; :287-351 per diagonal): the
 * recordings as tfp_search_sliding_pcm_batch takes them. The frame values and their boxes stay on the
 * device through the slide, the alignment and the trace. */
int tfp_search_occurrences_pcm_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nrecordings,
                                     int32_t sample_rate, const tfp_search_params* params, int32_t window, int32_t hop,
                                     const int32_t* scopes, int32_t k, int32_t max_gap, int32_t min_hits,
                                     tfp_occurrence* out, int64_t cap, int64_t* noccurrences);
/* Batches that launched the trace kernel so far and the requests it computed (the diagonals of
 * fp_handler.c:287-351; for an occurrence call its distinct candidates). A request answered on the
 * host (clip_id = -1, overlap = 0) counts nothing. Either pointer may be NULL. */
int tfp_trace_stats(tfp_engine* eng, int64_t* batches, int64_t* traces);

/* ---- live channels: rolling fingerprint + match (configs[4]) --------------------------
 * The dialplan app records `duration` ms of a channel to a WAV and searches it
 * (application_handler.c:152-185, record_voice :248-312). A stream keeps the most recent
 * window_samples of every channel on the GPU; after each tick (every channel's next
 * tick_samples, SLIN 20 ms = 160 samples at 8 kHz) the result of a channel whose history
 * holds a full window equals fp_search_fingerprint_info on a recording of exactly those
 * samples. Channels with less history report found = 0, frame_count = 0. */
typedef struct tfp_stream tfp_stream;
int tfp_stream_create(tfp_engine* eng, int32_t nchannels, int32_t sample_rate, int64_t window_samples,
                      tfp_stream** out);
void tfp_stream_destroy(tfp_stream* st); /* before tfp_engine_destroy of its engine */
/* A new call on `channel` (< 0: every channel): its history restarts empty. */
int tfp_stream_reset(tfp_stream* st, int32_t channel);
/* pcm[nchannels][tick_samples] (host); tick_samples <= window_samples. params NULL: only
 * ingest. out[nchannels] receives each channel's result when params != NULL. */
int tfp_stream_push(tfp_stream* st, const int16_t* pcm, int32_t tick_samples, const tfp_search_params* params,
                    tfp_result* out);
/* The same tick as G.711 codes[nchannels][tick_samples] (a channel's native payload; aubio_source's
 * table[code], fp_handler.c:604, :633): the codes are expanded on their way into the ring by the
 * launch that scatters them, so a tick has the launches of an int16 tick and half its bytes. The
 * ring is int16 either way: int16, mu-law and A-law ticks may follow one another in any order. */
int tfp_stream_push_g711(tfp_stream* st, const uint8_t* codes, int32_t tick_samples, int32_t law,
                         const tfp_search_params* params, tfp_result* out);
/* The frames of `channel`'s most recent window_samples, as tfp_fingerprint_pcm returns them for a
 * recording of exactly those samples (exact q values), fingerprinted where they lie in the stream's
 * ring by the launch a tick uses. *nframes = 0 (nothing written) while the channel's history is not
 * full. Changes nothing a later push or read-out sees. TFP_E_ARG for a channel outside
 * [0, nchannels) or cap below the window's frame count (*nframes then holds it). */
int tfp_stream_window_frames(tfp_stream* st, int32_t channel, tfp_frame* out, int64_t cap, int64_t* nframes);

/* ---- live calls: the scoped rows of each call so far, counts carried from push to push (new) ----
 * The dialplan application answers a channel, records `duration` ms of it from the start of the call
 * and asks which clip of its context the recording matches (application_handler.c:152-185,
 * record_voice :248-312; doc/dialplan_application.rst:11). A live object keeps every channel's
 * recording so far on the GPU, anchored at the start of the call: after a searching push the rows of
 * channel c are what tfp_search_scoped_pcm_batch returns for one query holding exactly the S_c samples
 * the channel has taken since its last reset (fp_handler.c:287-374 with the context predicate at
 * :308-314), with the same params, scope and k, row for row (match_count, uuid, clip_id), and
 * frame_counts[c] = tfp_frame_count(S_c); a channel with S_c = 0 has counts[c] = 0 and
 * frame_counts[c] = 0. This holds after every push, for every interleaving of pushes and resets,
 * across index updates and across changes of params or scope between pushes. So the caller can ask
 * after every 20 ms frame what the application asks once at the end, and stop recording as soon as
 * the winner's margin suffices.
 *
 * Frame f of a recording reads samples [256 (f - 1), 256 (f + 1)), so with S samples in, frames
 * [0, floor(S / 256)) never change again: a push fingerprints only the frames its samples complete
 * or touch, and for coefs = 1 adds each newly final frame's key bitset row to the channel's row of
 * per-clip counts; the rows are selected from those counts plus the provisional last frame's bit.
 * The counts are rebuilt from the kept frame values when the index, the resolved tolerance or an
 * ignore threshold has changed since they were built (a change of scope or k needs no rebuild).
 * coefs = 2 runs the scoped search over the kept frame values: exact, not incremental. Calls take the
 * engine's mutex, as the stream calls do, and are not coalesced. */
typedef struct tfp_live tfp_live;
/* max_samples: the longest call kept (record_voice's duration, application_handler.c:248-312),
 * 1 <= max_samples <= 65535 * 256 so that a count fits 16 bits; anything else is TFP_E_ARG. */
int tfp_live_create(tfp_engine* eng, int32_t nchannels, int32_t sample_rate, int64_t max_samples, tfp_live** out);
void tfp_live_destroy(tfp_live* lv); /* before tfp_engine_destroy of its engine */
/* A new call on `channel` (< 0: every channel) starts empty (application_handler.c:152-185: one
 * recording per tiresias_exec). */
int tfp_live_reset(tfp_live* lv, int32_t channel);
/* pcm[nchannels][tick_samples] (host): channel c takes its first nsamples[c] samples,
 * 0 <= nsamples[c] <= tick_samples, 0 = an idle channel; nsamples NULL = tick_samples for every
 * channel (record_voice's frame loop, application_handler.c:248-312). A push that would take any
 * channel past max_samples returns TFP_E_CAPACITY and ingests nothing, for any channel.
 * params NULL: ingest only, the out pointers are ignored. Else the search follows
 * (fp_handler.c:287-374 with the context predicate at :308-314): scopes[nchannels], each
 * TFP_SCOPE_ANY or >= 0 (NULL: TFP_SCOPE_ANY everywhere; below -1 is TFP_E_ARG); 1 <= k <=
 * TFP_RANK_MAX; out[nchannels * k] and counts[nchannels] as tfp_search_scoped_batch writes them,
 * entries past counts[c] zeroed; frame_counts[nchannels] may be NULL. Invalid params (coefs outside
 * [1, 2]) ingest and give empty rows, as tfp_stream_push does (fp_handler.c:247-250). */
int tfp_live_push(tfp_live* lv, const int16_t* pcm, int32_t tick_samples, const int32_t* nsamples,
                  const tfp_search_params* params, const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                  int32_t* frame_counts);
/* Samples `channel` has taken since its last reset (record_voice's running length,
 * application_handler.c:248-312). */
int tfp_live_samples(tfp_live* lv, int32_t channel, int64_t* nsamples);
/* Searching pushes served from the carried counts and by the general form (the rows of
 * fp_handler.c:367-374 either way), rebuilds of the count table, frames given to the fingerprint
 * kernels (the lead-in frames included) and final frames added to count rows (a rebuild adds every
 * final frame again). Any pointer may be NULL. */
int tfp_live_stats(tfp_live* lv, int64_t* incremental_pushes, int64_t* general_pushes, int64_t* rebuilds,
                   int64_t* frames_fingerprinted, int64_t* frames_added);
/* tfp_live_push over a channel's native G.711 payload: codes[nchannels][tick_samples], one byte per
 * sample, of law TFP_G711_ULAW or TFP_G711_ALAW (any other law is TFP_E_ARG, nothing ingested). The
 * codes cross to the GPU as bytes and the scatter expands them into the int16 history
 * (aubio_source's table[code], fp_handler.c:604, :633), so int16, mu-law and A-law pushes of one call
 * may follow one another in any order. Every other argument and rule is tfp_live_push's, the
 * all-or-nothing capacity check included. Rows, counts, frame counts and every later verdict equal
 * those of tfp_live_push on tfp_g711_decode(codes), bit for bit. tfp_g711_stats counts the scatter
 * among its stream_launches (a tick whose scatter expanded codes) and the samples taken among codes. */
int tfp_live_push_g711(tfp_live* lv, const uint8_t* codes, int32_t tick_samples, int32_t law, const int32_t* nsamples,
                       const tfp_search_params* params, const int32_t* scopes, int32_t k, tfp_candidate* out,
                       int32_t* counts, int32_t* frame_counts);

/* The early verdict: when the margin suffices. record_voice records a planned `duration`
 * (application_handler.c:163, :248-312), so with S_c samples of total_samples[c] in, the frames still
 * to come are known: F_tot - F_fin, F_tot = tfp_frame_count(total_samples[c]), F_fin = floor(S_c / 256).
 *
 * Per channel: the base count of a clip is its count over the final frames [0, F_fin) while
 * S_c < total_samples[c] (the provisional tail is left out: it can still change), and over every frame,
 * tail included, once S_c == total_samples[c] (`complete`; then it is tfp_live_push's count).
 * remaining = F_tot - F_fin, 0 when complete. The candidates are the enrolled, not removed clips of
 * the channel's scope that have at least one row with a non-NULL max1 (a clip without one can never
 * score), a base count of 0 included, ordered by (base count, tie-break key) as the rows are. The
 * leader is the greatest candidate if its base count is >= 1 (else there is neither leader nor
 * rival); the rival is the greatest other candidate. decided = complete, or has_leader and (no rival,
 * or (leader count, leader key) > (rival count + remaining, rival key)); keys are distinct.
 *
 * decided implies that row 0 of tfp_search_scoped_pcm_batch on any recording of total_samples[c]
 * samples that extends the S_c samples so far is the leader: the recording's frames [0, F_fin) are the
 * final frames, so every clip's count there is its base count plus at most one per remaining frame
 * and the leader's is at least its base count; every candidate but the leader is bounded by the
 * rival, and a clip that is no candidate never scores. The verdict holds for the index, the params and
 * the scope of the call that produced it.
 *
 * The call ingests nothing. It brings the count rows up to date exactly as a searching push of no
 * samples would (the same check of what the rows were built for, rebuild and adds; tfp_live_stats
 * counts the rebuild and the frames added, a verdict is not counted as a push), then one launch
 * selects the two greatest candidates per channel. total_samples[c] < S_c or > max_samples is
 * TFP_E_ARG naming the channel; params->coefs != 1 (the dialplan passes 1, application_handler.c:180)
 * or a scope below -1 is TFP_E_ARG; nothing is written then. scopes NULL: TFP_SCOPE_ANY everywhere.
 * An empty index gives no leader and decided = complete. Where a frame's key lies outside the vote
 * range every channel comes back with no leader and decided = complete, and the count rows are
 * dropped as a push drops them: a verdict that cannot be computed is undecided, never wrong.
 * (The struct has no typedef: C keeps struct tags apart from function names, a typedef would clash.) */
struct tfp_live_verdict {
  tfp_candidate leader;   /* zeroed when has_leader == 0; match_count = its base count */
  tfp_candidate rival;    /* zeroed when has_rival == 0;  match_count = its base count */
  int32_t has_leader, has_rival;
  int32_t remaining;      /* frames of the finished recording that are not final yet */
  int32_t complete;       /* S_c == total_samples[c] */
  int32_t decided;
};
/* out[nchannels]: every channel's verdict against its planned length (record_voice's duration,
 * application_handler.c:163, :248-312). */
int tfp_live_verdict(tfp_live* lv, const int64_t* total_samples, const tfp_search_params* params,
                     const int32_t* scopes, struct tfp_live_verdict* out /*[nchannels]*/);

/* The trailing window: the rows of the last `window` frames of each call. An announcement or a
 * greeting that begins after an unknown stretch of ringback is diluted by its lead-in for as long as
 * the recording stays anchored at the start of the call (application_handler.c:152-185, record_voice
 * :248-312); the window is that recording with its start moved along.
 *
 * Channel c has taken S samples since its last reset: F = tfp_frame_count(S), Ff = floor(S / 256), the
 * provisional tail is frame Ff when S % 256 != 0; first = max(0, F - window). The channel's window is
 * frames [first, F) of the call, the tail included. Its rows are what tfp_search_scoped_batch returns
 * for one query holding exactly the frame values of [first, F) as the live object keeps them
 * (tfp_live_frames; fp_handler.c:287-374 with the context predicate at :308-314), with the same
 * params, scope and k, row for row (match_count, uuid, clip_id); frame_counts[c] = F - first and
 * first_frames[c] = first. So while F <= window the rows are tfp_live_push's, and once F >= window
 * they are the last window of tfp_search_sliding_batch over the call's frames with that window and
 * hop = 1. This holds after every call, for every interleaving of pushes (int16 or G.711) and resets,
 * across index updates and across changes of params, scope, k or window between calls. A channel with
 * S = 0 gives no rows, frame_counts = 0 and first_frames = 0; an empty index gives no rows.
 *
 * The call ingests nothing and fingerprints nothing (a caller pushes, ingest only or searching, and
 * then asks). For coefs = 1 a second table of 16-bit counts, nchannels x the count row's columns,
 * allocated by the first window call, holds per channel the sum of the key bitset rows of the
 * window's final frames [first, Ff): a call subtracts the rows of the frames that left a channel's
 * window and adds those of the frames that became final, or starts the row again from zero where
 * that visits fewer frames, so it visits at most min(leaving + entering, Ff - first) frames per
 * channel; the rows are selected from those counts plus the tail's bit. The table is restarted when
 * the index, the resolved tolerance, an ignore threshold or `window` has changed since it was built
 * (a change of scope or k needs no restart). coefs = 2, and a frame key outside the vote range, run
 * the scoped search over each channel's window of kept frame values: exact, not incremental.
 *
 * 1 <= k <= TFP_RANK_MAX, window >= 1 (frames), scopes as tfp_live_push (NULL: TFP_SCOPE_ANY), params,
 * out[nchannels * k] and counts[nchannels] not NULL: anything else is TFP_E_ARG and nothing is
 * written. frame_counts and first_frames may be NULL. Invalid params (coefs outside [1, 2]) give empty
 * rows, as a push does (fp_handler.c:247-250). */
int tfp_live_window(tfp_live* lv, const tfp_search_params* params, const int32_t* scopes, int32_t k, int32_t window,
                    tfp_candidate* out, int32_t* counts, int32_t* frame_counts, int32_t* first_frames);
/* `window` for window_ms of audio at sample_rate (the unit record_voice's duration is given in,
 * application_handler.c:163): ceil(window_ms * sample_rate / 1000 / 256) frames, at least 1. Host-only. */
int32_t tfp_live_window_frames(int64_t window_ms, int32_t sample_rate);
/* The kept frame values of frames [first, F) of `channel`'s call so far, the provisional tail
 * included (exact q values, what a push and a window search read; fp_handler.c:290, :321), as
 * tfp_stream_window_frames reads out a stream's window. frame_idx is the frame's index in the call;
 * m1 / m2 are the values as they would be stored. Changes nothing a later call sees. TFP_E_ARG for a
 * channel outside [0, nchannels), first outside [0, F], or cap below F - first (*nframes then holds
 * it). */
int tfp_live_frames(tfp_live* lv, int32_t channel, int64_t first, tfp_frame* out, int64_t cap, int64_t* nframes);
/* Window calls served from the window table (a coefs = 1 call over an empty index counts here too,
 * though it builds no table and restarts nothing) and by the general form (the rows of
 * fp_handler.c:367-374 either way), restarts of the whole table (a changed stamp), frames whose bitset
 * rows the slide kernel added, frames that left rows (subtracted by the slide kernel, or dropped
 * unvisited where a row restarted, a channel was reset or the table restarted: frames_added -
 * frames_removed is what the rows hold), and rows restarted by a call. Any pointer may be NULL.
 * tfp_live_stats is not moved by window calls. */
int tfp_live_window_stats(tfp_live* lv, int64_t* slid_calls, int64_t* general_calls, int64_t* rebuilds,
                          int64_t* frames_added, int64_t* frames_removed, int64_t* rows_restarted);

/* The aligned trailing window: tfp_live_window's rows, each with where its clip lies in the window. The
 * rows say which clip a call is playing; a record loop (application_handler.c:152-185, record_voice
 * :248-312) also needs where in the clip the call is: a greeting of N frames that began after an
 * unknown stretch of ringback ends at call frame clip_start_frame + N, and aligned_count against
 * match_count tells a prompt heard once in order from the same frames scattered.
 *
 * out, counts, frame_counts and first_frames are byte for byte what tfp_live_window writes for the same
 * arguments; the argument rules, the empty index, a channel with S = 0 and invalid params are
 * tfp_live_window's too, and align == NULL is TFP_E_ARG with nothing written. For channel c and row
 * r < counts[c], align[c * k + r] is exactly the tfp_alignment tfp_align_batch returns for one query
 * holding the kept frame values of frames [first, F) of the call (as tfp_live_frames(c, first) reads
 * them out, the provisional tail included), the clip out[c * k + r].clip_id and the same params: the
 * per-frame predicate of fp_handler.c:287-351 applied to the clip's stored rows in frame order,
 * coefs = 2 testing max2 as tfp_align_batch does, for the rows of :367-374. Entries past counts[c] are
 * zeroed. All four fields are relative to the window: window frame x is call frame first + x and lies
 * at clip frame x + offset, so clip frame 0 lies at call frame
 *   clip_start_frame = first_frames[c] - offset
 * (negative when the clip began before the call, or was joined midway). offset is the smallest
 * diagonal attaining aligned_count, exactly as in the batch forms, and their warning holds: on a short
 * window, or a clip with repeating rows, several diagonals may attain the count, and the smallest need
 * not be the one the audio was cut from.
 *
 * This holds after every call, for any interleaving of int16 and G.711 pushes, resets, tfp_live_window
 * and tfp_live_window_aligned calls, across index updates (clips of the index delta, removed clips, a
 * merge between calls) and across changes of params, scope, k or window.
 *
 * The call ingests nothing and fingerprints nothing (tfp_fingerprint_stats and tfp_live_stats do not
 * move). It moves the window count table exactly as tfp_live_window with the same arguments would and
 * tfp_live_window_stats counts it as that window call, so the two may alternate on one table. Served
 * from the table (coefs = 1), the selected rows never leave the device before they are aligned: their
 * columns, the window frames' boxes (from the kept frame values in place) and one (rows, boxes) pair
 * per row are built there, the alignment kernels of tfp_align_batch follow on the stream, and one
 * read-back brings rows and alignments. coefs = 2, and a frame key outside the vote range, align after
 * the general form's rows have come back: exact, not the fast path. (The key route is defensive only:
 * a frame key is trunc(10 log10|c|) of a DCT coefficient of int16 samples, |key| <= 459 inside the vote
 * range of +-512, and a live object takes nothing but samples, so no input reaches it and no test
 * drives it.) The engine's tfp_align_stats is not moved; tfp_live_window_aligned_stats counts instead. */
int tfp_live_window_aligned(tfp_live* lv, const tfp_search_params* params, const int32_t* scopes, int32_t k,
                            int32_t window, tfp_candidate* out /*[nchannels * k]*/, tfp_alignment* align /*[nchannels * k]*/,
                            int32_t* counts, int32_t* frame_counts, int32_t* first_frames);
/* Aligned window calls whose rows came from the window table and whose pairs were built on the device
 * (a call over an empty index counts here with 0 pairs, as tfp_live_window_stats counts its own), calls
 * whose rows came from the general form (coefs = 2, a frame key outside the vote range; the rows of
 * fp_handler.c:367-374 either way), and the non-empty (channel, row) pairs given to the alignment
 * kernels (the per-frame predicate of fp_handler.c:287-351 along each pair's diagonals). Any pointer may
 * be NULL. */
int tfp_live_window_aligned_stats(tfp_live* lv, int64_t* inplace_calls, int64_t* general_calls, int64_t* pairs);

/* The log of a live call: which clips have played so far, from which call frame to which. The window
 * calls above describe the present moment; a monitored call (application_handler.c:152-185, record_voice
 * :248-312) needs the list tfp_search_occurrences_batch gives for a finished recording (greeting from
 * frame 40 to 310, ringback, the voicemail prompt from frame 520 and still playing), kept up to date at
 * O(new frames) per call instead of by reading every channel's frames back and searching the whole
 * call again at every tick.
 *
 * A live object keeps, per channel, a list of tracks (clip, s, windows), s being the call frame at which
 * clip frame 0 lies, each with a carried summary of its diagonal's hits (the per-frame predicate of
 * fp_handler.c:287-351, as tfp_trace_batch tests it). tfp_live_reset of a channel empties its list. One
 * call ingests nothing and fingerprints nothing (tfp_fingerprint_stats and tfp_live_stats do not move)
 * and does four steps in this order:
 *  1. rows: exactly what tfp_live_window_aligned(lv, params, scopes, k, window, ...) runs. The window
 *     count table, tfp_live_window_stats and tfp_live_window_aligned_stats move as that call moves
 *     them, so all three window calls may alternate on one table; coefs = 2 takes the general form.
 *  2. offer: for each channel c ascending and its rows r ascending, a row with aligned_count >= 1 names
 *     the candidate (clip, s = first_frames[c] - offset). A candidate already on the channel's list has
 *     its `windows` raised by one; otherwise it is appended with windows = 1 while the list holds fewer
 *     than max_tracks entries; otherwise dropped[c] goes up by one (dropped starts at 0 on every call).
 *     max_tracks below a list's length drops nothing and only stops additions.
 *  3. advance: every track of every channel is brought up to the call's current frames. Afterwards the
 *     tfp_trace of track (c, clip, s) is exactly what tfp_trace_batch returns for one recording holding
 *     tfp_live_frames(c, 0) (all F frames, the provisional tail included), the request {0, clip, s}, the
 *     same params and max_gap. The stored summary covers the final frames [0, floor(S / 256)) only (they
 *     never change); the tail's hit is joined into the answer and not into what is stored.
 *  4. occurrences: per channel the tracks whose clip is still enrolled, lies in scopes[c]
 *     (TFP_SCOPE_ANY: every clip) and has seg_hits >= min_hits are thinned per (channel, clip) by
 *     tfp_search_occurrences_batch's step 4 (seg_hits descending, windows descending, s ascending; one
 *     is kept unless its [seg_first, seg_last] meets the interval of one already kept) and written as
 *     tfp_occurrence entries with recording = channel, in that call's output order (channel ascending,
 *     first_frame ascending, hits descending, audio_uuid descending: the tie order of
 *     fp_handler.c:367-374). cap, *noccurrences and TFP_E_CAPACITY as tfp_search_occurrences_batch.
 *
 * The stored summaries are valid for a stamp: the index version, the resolved tolerance, the ignore
 * thresholds, coefs and max_gap. A call whose stamp differs from the last call's traces every track
 * again from the first frame of its span (one `retraces` count per such call that had a summary to
 * start again); the lists and `windows` are kept, and tracks whose clip has been removed are deleted
 * (a track names its clip by the engine's clip id, which index updates and merges keep, with the uuid
 * as a check). A change of scopes, k, window, min_hits or max_tracks needs no retrace.
 *
 * TFP_E_ARG with nothing written and no state moved: k outside [1, TFP_RANK_MAX], window < 1,
 * max_gap < 0, min_hits < 1, max_tracks outside [1, TFP_LIVE_TRACKS_MAX], a scope below TFP_SCOPE_ANY,
 * NULL params, out (with cap > 0) or noccurrences. scopes and dropped may be NULL. Invalid params (coefs
 * outside [1, 2]) give no rows as the window calls do (fp_handler.c:247-250): nothing is offered, the
 * lists stay as they are and no occurrence is written. An empty index and a channel with S = 0 offer
 * nothing. */
#define TFP_LIVE_TRACKS_MAX 64
int tfp_live_occurrences(tfp_live* lv, const tfp_search_params* params, const int32_t* scopes, int32_t k,
                         int32_t window, int32_t max_gap, int32_t min_hits, int32_t max_tracks, tfp_occurrence* out,
                         int64_t cap, int64_t* noccurrences, int32_t* dropped /*[nchannels], may be NULL*/);
/* `channel`'s list as of the last tfp_live_occurrences call, in list order (fp_handler.c:287-351 along
 * each track's diagonal): reqs[i] = {channel, clip_id, s}, traces[i] its trace, windows[i] its count;
 * any of the three may be NULL. *ntracks is always set; cap below it is TFP_E_CAPACITY and nothing else
 * is written. Changes nothing. */
int tfp_live_tracks(tfp_live* lv, int32_t channel, tfp_trace_req* reqs, tfp_trace* traces, int32_t* windows,
                    int64_t cap, int64_t* ntracks);
/* Occurrence calls so far, tracks appended and candidates dropped by the offer, the (track, final
 * frame) pairs folded into stored summaries (each a test of fp_handler.c:287-351; the tail and frames
 * outside a track's span are not counted), and calls that started kept summaries again. A track
 * appended at call frame Ff catches up over [lo, min(Ff, s + N)) once, then costs one pair per newly
 * final frame inside its span and nothing once s + N <= Ff: the work per call does not grow with the
 * call's age. Any pointer may be NULL. */
int tfp_live_occurrence_stats(tfp_live* lv, int64_t* calls, int64_t* tracks_added, int64_t* tracks_dropped,
                              int64_t* frames_traced, int64_t* retraces);

/* ---- catalog neighbours: which enrolled clips sound like a given clip (new) -------------- */
/* The reference deduplicates enrolments by MD5 alone (fp_handler.c:713-753), so the same prompt from
 * another encoder, or two prompts that share most of their keys, is found only when a search
 * (fp_handler.c:287-374) returns the wrong one. These calls ask the catalog itself.
 *
 * A stored row (m1, m2) used as a query frame has the frame values (double)m / 1e6 by IEEE division,
 * -inf where m is TFP_NULL_MICRO: the double SQLite reads back from the "%f" text of
 * fp_handler.c:559-571. The neighbours of clip a under (params, scope, k) are the first k rows of the
 * result query (fp_handler.c:367-374) for the recording whose fingerprints are a's stored rows, NULL
 * rows included as frames, restricted to scope as tfp_search_scoped_batch restricts it
 * (fp_handler.c:308-314 with the context predicate), with the row of a itself deleted. A clip need not
 * match itself (its own row lies in a frame's box only when the value's fraction is within the
 * tolerance), so this is "k + 1 rows minus self": self is dropped if it is among the first k + 1 rows,
 * else row k + 1 is. Each row carries the tfp_alignment tfp_align_batch gives those frames against
 * the row's clip. */
/* fp_handler.c:287-374 for each named clip's stored rows (fp_handler.c:713-753: the catalog's clips)
 * over the clips of scopes[i] (TFP_SCOPE_ANY or >= 0; scopes NULL: ANY everywhere; a scope the named
 * clip is not in is legal). out[i * k + r] is row r of clip i, align[i * k + r] its alignment (align
 * NULL: none computed), counts[i] the rows, frame_counts[i] (or NULL) the clip's stored rows; entries
 * past counts[i] are zeroed. k < 1, k > TFP_RANK_MAX, coefs outside [1,2] or a scope below -1 is
 * TFP_E_ARG; an unknown or removed uuid TFP_E_NOENT, nothing written then. A uuid may be named
 * twice; nclips = 0 is TFP_OK. No frame value is written and no row leaves the device on the vote
 * form (coefs = 1, keys inside the vote range). */
int tfp_index_neighbours(tfp_engine* eng, int32_t nclips, const char* const* uuids, const tfp_search_params* params,
                         const int32_t* scopes /* [nclips] or NULL */, int32_t k, tfp_candidate* out /* [nclips*k] */,
                         tfp_alignment* align /* [nclips*k] or NULL */, int32_t* counts /* [nclips] */,
                         int32_t* frame_counts /* [nclips] or NULL */);
/* Neighbour calls served so far by the vote form and by the general form (the rows of
 * fp_handler.c:287-374 over stored rows of fp_handler.c:713-753's clips), the rows aligned, and the
 * stored rows used as query frames. Any pointer may be NULL. */
int tfp_neighbour_stats(tfp_engine* eng, int64_t* vote_batches, int64_t* general_batches, int64_t* pairs_aligned,
                        int64_t* frames_read);

/* ---- device groups: the node's GPUs behind one index (new in round 3) -------------------
 * The module's enrolled DB sharded over one engine per listed device (the reference
 * has one SQLite DB, fp_handler.c:30): each clip lives on one engine (the one holding the fewest
 * rows when it is added) and is never split, since the per-frame GROUP BY audio_uuid of
 * fp_handler.c:353 is not additive over a split clip. Every search runs on all engines in parallel
 * (a worker thread per engine); the engines carry the group-wide uuid ranks as tie-break keys, so
 * the per-query key (match_count << 32 | rank) of each shard combines by an integer max into the
 * reference's winner (count(*) DESC, ties to the greatest audio_uuid, fp_handler.c:367-374).
 * Batches of >= 64 equal-length int16 queries per engine are query-sharded: each engine
 * fingerprints its share and the frame values are exchanged GPU to GPU (peer copies over xGMI);
 * smaller batches and stream ticks are fingerprinted by every engine, so the latency path has no
 * exchange. A device may be listed more than once (shards sharing a GPU). Results as the engine
 * calls, except tfp_result.clip_id = the index of the engine holding the winner. Thread-safe
 * (calls are serialised per group); errors through tfp_group_last_error. */
typedef struct tfp_group tfp_group;
int tfp_group_create(const int32_t* devices, int32_t ndevices, tfp_group** out);
void tfp_group_destroy(tfp_group* g); /* destroy its streams first */
int32_t tfp_group_size(const tfp_group* g);
/* Peer access among the group's distinct devices (new in round 6): ordered pairs of distinct
 * devices, how many of them hipDeviceCanAccessPeer allows, and for how many
 * hipDeviceEnablePeerAccess succeeded (or was already on). Any pointer may be NULL. */
int tfp_group_peer_stats(const tfp_group* g, int32_t* pairs, int32_t* can_access, int32_t* enabled);
/* The group's tie-break keys (new in round 6): respaces (every key re-spread and sent to every shard:
 * the first enrolment, a large batch, a gap exhausted), pushes of new clips' keys only, and the
 * shards' index delta updates that still re-sent every main column's key. An enrolment of a few
 * clips costs a push of their keys, not a pass over every clip. Any pointer may be NULL. */
int tfp_group_tiebreak_stats(tfp_group* g, int64_t* respaces, int64_t* partial_pushes, int64_t* shard_full_key_updates);
const char* tfp_group_last_error(const tfp_group* g);
tfp_engine* tfp_group_engine(tfp_group* g, int32_t shard); /* for stats; do not change its index */
int tfp_group_fingerprint_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                                int32_t sample_rate, tfp_frame* out, int64_t cap, int64_t* nframes);
int tfp_group_fingerprint_f32_batch(tfp_group* g, const float* x, const int64_t* offsets, int32_t nclips,
                                    int32_t sample_rate, tfp_frame* out, int64_t cap, int64_t* nframes);
int tfp_group_index_add(tfp_group* g, const char* uuid, const int32_t* m1, const int32_t* m2, int32_t nframes);
int tfp_group_index_add_batch(tfp_group* g, int32_t nclips, const char* const* uuids, const int64_t* frame_offsets,
                              const int32_t* m1, const int32_t* m2);
int tfp_group_index_remove(tfp_group* g, const char* uuid);
int tfp_group_index_clear(tfp_group* g);
int tfp_group_index_rows(tfp_group* g, const char* uuid, int32_t* m1, int32_t* m2, int64_t cap, int64_t* nframes);
int tfp_group_index_stats(tfp_group* g, int64_t* nrows, int32_t* nclips);
int tfp_group_index_commit(tfp_group* g);
int tfp_group_search_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                           const tfp_search_params* params, tfp_result* out);
int tfp_group_search_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                               int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
int tfp_group_search_f32_batch(tfp_group* g, const float* x, const int64_t* offsets, int32_t nqueries,
                               int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
/* Ranked search on a group (fp_handler.c:367-374 read to row k, as tfp_search_ranked_batch): every
 * shard returns its first k rows, and per query the greatest k of their global keys are kept, which
 * are the first k rows over all shards' clips. tfp_candidate.clip_id = the shard holding the clip.
 * A failing shard fails the call. */
int tfp_group_search_ranked_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                                  const tfp_search_params* params, int32_t k, tfp_candidate* out, int32_t* counts);
/* The same from PCM (fp_handler.c:275 + :287-374), every shard fingerprinting the batch. */
int tfp_group_search_ranked_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                      int32_t sample_rate, const tfp_search_params* params, int32_t k,
                                      tfp_candidate* out, int32_t* counts);
/* Scoped search on a group (fp_handler.c:308-314 with the context predicate, :367-374 read to row k;
 * doc/dialplan_application.rst:11, :52-53): a clip's scope is set on the shard that holds it (all or
 * nothing over the group), every shard returns its scoped first k rows, and they merge as
 * tfp_group_search_ranked_batch's do. */
int tfp_group_index_set_scope(tfp_group* g, int32_t n, const char* const* uuids, const int32_t* scopes);
int tfp_group_index_scope(tfp_group* g, const char* uuid, int32_t* scope);
int tfp_group_search_scoped_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                                  const tfp_search_params* params, const int32_t* scopes, int32_t k, tfp_candidate* out,
                                  int32_t* counts);
int tfp_group_search_scoped_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                      int32_t sample_rate, const tfp_search_params* params, const int32_t* scopes,
                                      int32_t k, tfp_candidate* out, int32_t* counts);
/* Catalog neighbours on a group (fp_handler.c:287-374 for the stored rows of fp_handler.c:713-753's
 * clips, as tfp_index_neighbours): the shard that holds a named clip produces its frame values, every
 * shard returns its first k rows for them (only the owner has a row to delete), the rows merge as
 * tfp_group_search_scoped_batch's do and each is aligned on the shard that holds its clip. The result
 * equals one engine over all the clips; clip_id is the shard. Arguments and rules as the engine call's.
 * tfp_neighbour_stats of a shard's engine (tfp_group_engine): every shard serves each group call once and
 * counts it as a general batch, whatever the parameters (the shards rank the owner's frame values, which
 * reach them as frames); frames_read is counted on the owner shard and pairs_aligned on the shard that
 * aligned the row, so their sums over the shards equal one engine's. */
int tfp_group_index_neighbours(tfp_group* g, int32_t nclips, const char* const* uuids, const tfp_search_params* params,
                               const int32_t* scopes, int32_t k, tfp_candidate* out, tfp_alignment* align, int32_t* counts,
                               int32_t* frame_counts);
/* Census on a group (fp_handler.c:287-374 counted by count(*), as tfp_census_batch): every shard
 * takes the census of its own clips and the rows are summed bin by bin, bin 0 included. A clip lies
 * on one shard, so the sum is exact. The arguments and rules as the engine calls'. */
int tfp_group_census_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                           const tfp_search_params* params, const int32_t* scopes, int32_t nbins, int32_t* hist,
                           int32_t* need_bins);
int tfp_group_census_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                               int32_t sample_rate, const tfp_search_params* params, const int32_t* scopes, int32_t nbins,
                               int32_t* hist, int32_t* need_bins);
/* Sliding search on a group (fp_handler.c:367-374 read to row k for every window,
 * application_handler.c:152-185 moved along the recording): every shard slides over every recording,
 * and per window the shards' rows merge as tfp_group_search_ranked_batch's do; clip_id is the shard;
 * scopes as tfp_group_search_scoped_batch. The other arguments and rules as the engine calls'. */
int tfp_group_search_sliding_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets, int32_t nrecordings,
                                   const tfp_search_params* params, int32_t window, int32_t hop, const int32_t* scopes,
                                   int32_t k, tfp_candidate* out, int32_t* counts, int64_t cap_windows, int64_t* nwindows);
int tfp_group_search_sliding_pcm_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nrecordings,
                                       int32_t sample_rate, const tfp_search_params* params, int32_t window, int32_t hop,
                                       const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                       int64_t cap_windows, int64_t* nwindows);
/* tfp_search_aligned_batch on a group (fp_handler.c:367-374 read to row k, then each kept row's
 * alignment): the ranked search as tfp_group_search_ranked_batch, then every kept candidate is
 * aligned on the shard that holds it (tfp_align_batch with its clip id there). cand as that call's. */
int tfp_group_search_aligned_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets, int32_t nqueries,
                                   const tfp_search_params* params, int32_t k, tfp_candidate* cand,
                                   tfp_alignment* align, int32_t* counts);
/* tfp_search_sliding_aligned_batch on a group (fp_handler.c:367-374 read to row k for every window,
 * then each kept row's alignment): the sliding search as tfp_group_search_sliding_batch, then every
 * kept row is aligned on the shard that holds its clip (tfp_align_sliding_batch with the shard-local
 * clip id, -1 for the other shards' rows), as tfp_group_search_aligned_batch does per query. */
int tfp_group_search_sliding_aligned_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets,
                                           int32_t nrecordings, const tfp_search_params* params, int32_t window,
                                           int32_t hop, const int32_t* scopes, int32_t k, tfp_candidate* out,
                                           int32_t* counts, tfp_alignment* align, int64_t cap_windows,
                                           int64_t* nwindows);
/* tfp_search_occurrences_batch on a group (fp_handler.c:367-374 per window, fp_handler.c:287-351 per
 * diagonal): the rows of tfp_group_search_sliding_aligned_batch, each candidate traced on the shard
 * that holds its clip (tfp_trace_batch with the shard-local clip id), the suppression per (recording,
 * audio_uuid) and the output order over all shards. clip_id is the shard. A failing shard fails the
 * call. */
int tfp_group_search_occurrences_batch(tfp_group* g, const tfp_frame* frames, const int64_t* qoffsets,
                                       int32_t nrecordings, const tfp_search_params* params, int32_t window, int32_t hop,
                                       const int32_t* scopes, int32_t k, int32_t max_gap, int32_t min_hits,
                                       tfp_occurrence* out, int64_t cap, int64_t* noccurrences);
/* tfp_search_pcm_gather and the coalescing of concurrent calls (as for one engine) on a group: the
 * channel threads' batch-1 searches through the shim run as shared batches on every GPU. */
int tfp_group_search_pcm_gather(tfp_group* g, const int16_t* const* pcms, const int64_t* nsamples, int32_t nqueries,
                                int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
int tfp_group_search_coalesce_stats(tfp_group* g, int64_t* calls, int64_t* batches);
/* Live channels on a group: every engine keeps every channel's window and matches it against its
 * clips each tick; out[nchannels] = the combined results (as tfp_stream_push). */
typedef struct tfp_group_stream tfp_group_stream;
int tfp_group_stream_create(tfp_group* g, int32_t nchannels, int32_t sample_rate, int64_t window_samples,
                            tfp_group_stream** out);
void tfp_group_stream_destroy(tfp_group_stream* st);
int tfp_group_stream_reset(tfp_group_stream* st, int32_t channel);
int tfp_group_stream_push(tfp_group_stream* st, const int16_t* pcm, int32_t tick_samples,
                          const tfp_search_params* params, tfp_result* out);
/* Live calls on a group (tfp_live_*; application_handler.c:152-185, :248-312): every shard keeps
 * every channel's call so far, as replicated group streams do, and returns its first k rows per push
 * over its own clips; the rows merge as tfp_group_search_scoped_batch's do (fp_handler.c:367-374 with
 * the context predicate at :308-314 over all shards). clip_id is the shard. A failing shard fails the
 * call; a capacity failure (TFP_E_CAPACITY) leaves every shard unchanged. */
typedef struct tfp_group_live tfp_group_live;
int tfp_group_live_create(tfp_group* g, int32_t nchannels, int32_t sample_rate, int64_t max_samples, tfp_group_live** out);
void tfp_group_live_destroy(tfp_group_live* lv);
int tfp_group_live_reset(tfp_group_live* lv, int32_t channel);
int tfp_group_live_push(tfp_group_live* lv, const int16_t* pcm, int32_t tick_samples, const int32_t* nsamples,
                        const tfp_search_params* params, const int32_t* scopes, int32_t k, tfp_candidate* out,
                        int32_t* counts, int32_t* frame_counts);
int tfp_group_live_samples(tfp_group_live* lv, int32_t channel, int64_t* nsamples);
/* tfp_live_stats of shard `shard`'s object (every shard serves every push, over its own clips'
 * columns of fp_handler.c:367-374's rows). */
int tfp_group_live_stats(tfp_group_live* lv, int32_t shard, int64_t* incremental_pushes, int64_t* general_pushes,
                         int64_t* rebuilds, int64_t* frames_fingerprinted, int64_t* frames_added);
/* tfp_live_push_g711 on a group: the codes go to every shard as bytes and each shard's scatter
 * expands them (aubio_source's table[code], fp_handler.c:604, :633). */
int tfp_group_live_push_g711(tfp_group_live* lv, const uint8_t* codes, int32_t tick_samples, int32_t law,
                             const int32_t* nsamples, const tfp_search_params* params, const int32_t* scopes, int32_t k,
                             tfp_candidate* out, int32_t* counts, int32_t* frame_counts);
/* tfp_live_verdict on a group (application_handler.c:163, :248-312): every shard selects its two
 * greatest candidates over its own clips under the group-wide tie-break keys; the top 2 of their union
 * (the top 2 of a union is the top 2 of the parts' top 2s) go through the rule once. clip_id is the
 * shard. Arguments and failures as tfp_live_verdict; a failing shard fails the call. */
int tfp_group_live_verdict(tfp_group_live* lv, const int64_t* total_samples, const tfp_search_params* params,
                           const int32_t* scopes, struct tfp_live_verdict* out /*[nchannels]*/);
/* tfp_live_window on a group (application_handler.c:152-185, :248-312 with the recording's start moved
 * along): every shard keeps every channel, so each answers from a window table of its own over its
 * own clips' columns, and the rows merge as tfp_group_live_push's do (fp_handler.c:367-374 with the
 * context predicate at :308-314 over all shards). clip_id is the shard. Arguments and failures as
 * tfp_live_window; a failing shard fails the call. tfp_group_live_frames reads shard 0's kept frame
 * values (every shard keeps the same); tfp_group_live_window_stats is shard `shard`'s
 * tfp_live_window_stats. */
int tfp_group_live_window(tfp_group_live* lv, const tfp_search_params* params, const int32_t* scopes, int32_t k,
                          int32_t window, tfp_candidate* out, int32_t* counts, int32_t* frame_counts, int32_t* first_frames);
int tfp_group_live_frames(tfp_group_live* lv, int32_t channel, int64_t first, tfp_frame* out, int64_t cap, int64_t* nframes);
int tfp_group_live_window_stats(tfp_group_live* lv, int32_t shard, int64_t* slid_calls, int64_t* general_calls,
                                int64_t* rebuilds, int64_t* frames_added, int64_t* frames_removed, int64_t* rows_restarted);
/* tfp_live_window_aligned on a group (application_handler.c:152-185, :248-312; the per-frame predicate of
 * fp_handler.c:287-351 for the rows of :367-374): every shard runs its own tfp_live_window_aligned over
 * its own clips, the rows merge exactly as tfp_group_live_window's do, and each kept row carries the
 * alignment its shard computed (every shard keeps the same frame values, so it is the single
 * engine's). clip_id is the shard. Arguments and failures as tfp_live_window_aligned; a failing shard
 * fails the call. tfp_group_live_window_aligned_stats is shard `shard`'s tfp_live_window_aligned_stats. */
int tfp_group_live_window_aligned(tfp_group_live* lv, const tfp_search_params* params, const int32_t* scopes, int32_t k,
                                  int32_t window, tfp_candidate* out, tfp_alignment* align, int32_t* counts,
                                  int32_t* frame_counts, int32_t* first_frames);
int tfp_group_live_window_aligned_stats(tfp_group_live* lv, int32_t shard, int64_t* inplace_calls, int64_t* general_calls,
                                        int64_t* pairs);
/* tfp_live_occurrences on a group (application_handler.c:152-185, :248-312; fp_handler.c:287-351 along
 * each track's diagonal for the rows of :367-374): step 1 is tfp_group_live_window_aligned's merged rows,
 * the offer rule runs once on them (max_tracks bounds a channel's list over all shards together), every
 * shard carries and advances the traces of its own clips' tracks (every shard keeps the same frame
 * values, so they are the single engine's), and step 4 runs on the union: the entries, dropped and the
 * lists equal the single engine's. clip_id is the shard. Arguments and failures as
 * tfp_live_occurrences; a failing shard fails the call, and may leave it partly done: the window tables
 * moved, candidates offered and `windows` raised, but no track advanced. Nothing is lost: a track that
 * was appended and not advanced starts from its lo at the next call, which brings every trace up to
 * date. tfp_group_live_tracks is the merged list, with
 * reqs[i].clip_id = the shard and reqs[i].reserved = that shard's clip id.
 * tfp_group_live_occurrence_stats is shard `shard`'s tfp_live_occurrence_stats (its own tracks, frames and
 * retraces), except tracks_dropped: the group's offer drops, so that count is the group's. */
int tfp_group_live_occurrences(tfp_group_live* lv, const tfp_search_params* params, const int32_t* scopes, int32_t k,
                               int32_t window, int32_t max_gap, int32_t min_hits, int32_t max_tracks, tfp_occurrence* out,
                               int64_t cap, int64_t* noccurrences, int32_t* dropped);
int tfp_group_live_tracks(tfp_group_live* lv, int32_t channel, tfp_trace_req* reqs, tfp_trace* traces, int32_t* windows,
                          int64_t cap, int64_t* ntracks);
int tfp_group_live_occurrence_stats(tfp_group_live* lv, int32_t shard, int64_t* calls, int64_t* tracks_added,
                                    int64_t* tracks_dropped, int64_t* frames_traced, int64_t* retraces);
/* G.711 codes on a group (aubio_source's table[code], fp_handler.c:604, :633; as the engine calls):
 * a fingerprint batch's clips are expanded by the shard that fingerprints them; a search batch is
 * expanded by every shard, or, where an int16 batch would be query-sharded, each shard expands and
 * fingerprints its share and the frame values are exchanged as for int16; a stream tick's codes go
 * to the shards as bytes and each shard's scatter expands them. Not coalesced. */
int tfp_group_fingerprint_g711_batch(tfp_group* g, const uint8_t* codes, const int64_t* offsets, int32_t nclips,
                                     int32_t law, int32_t sample_rate, tfp_frame* out, int64_t cap, int64_t* nframes);
int tfp_group_search_g711_batch(tfp_group* g, const uint8_t* codes, const int64_t* offsets, int32_t nqueries,
                                int32_t law, int32_t sample_rate, const tfp_search_params* params, tfp_result* out);
int tfp_group_stream_push_g711(tfp_group_stream* st, const uint8_t* codes, int32_t tick_samples, int32_t law,
                               const tfp_search_params* params, tfp_result* out);

/* ---- rate-normalised ingest: int16 PCM of one rate at the index's rate (new) ------------- */
/* A fingerprint is comparable only with fingerprints taken at the same sample rate: the window is 512
 * samples and the filterbank is built per rate, and the reference takes every file at its native rate
 * (fp_handler.c:37 DEF_AUBIO_SAMPLERATE 0). These forms bring int16 audio of rate_in to rate_out with
 * one converter, defined in integers alone, so that the GPU and the host agree bit for bit:
 *   g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g, D = max(L, M), Z = 24
 *   n_out = ceil(n_in L / M)
 *   y[n] = clamp((sum_k h[p][k] x[i0 + k] + 16384) >> 15, -32768, 32767), i0 = n M div L, p = n M mod L,
 *          k = k_lo .. k_lo + ntaps - 1, x = 0 outside the clip's own samples, the sum exact (64-bit)
 *   k_lo = -(Z D div L), ntaps = ceil(Z D / L) - k_lo + 1; h[p][k] is int16 Q15, from
 *   h(u) = 0.9 sinc(0.9 u) I0(8 sqrt(1 - (u / Z)^2)) / I0(8) at u = (k L - p) / D (|u| < Z, else 0), each
 *   phase divided by its sum, times 32768, rounded, and 32768 - sum added to its largest tap: every
 *   phase sums to exactly 32768, so a constant stays that constant away from a clip's ends.
 * A rate <= 0 is TFP_E_ARG with "bad sample rate"; a pair with L * ntaps above 2^20 is TFP_E_ARG with
 * "unsupported rate ratio". rate_in == rate_out runs no filter: the rate forms are then the plain forms.
 * Not covered: tfp_stream_push (the ring), fp32 input. A live object takes its ticks at another rate
 * through tfp_live_create_rate (the last section of this header). Interleaved multichannel int16 has
 * forms of its own (tfp_fingerprint_mix_rate_batch), and so have 24/32-bit and float files, as int32
 * Q31 frames (tfp_fingerprint_wide_rate_batch): the two sections after tfp_synchronize. No claim of
 * equality with any other resampler is made. */
/* n_out for nsamples at rate_in; 0 for nsamples <= 0, -1 for a bad or unsupported pair. Host-only. */
int64_t tfp_resample_count(int64_t nsamples, int32_t rate_in, int32_t rate_out);
/* The pair's table taps[L][ntaps] and its shape (any of L, M, k_lo, ntaps may be NULL). taps == NULL
 * (cap 0) only sets the shape; cap < L * ntaps -> TFP_E_CAPACITY with the shape set, as tfp_wav_decode.
 * Host-only; errors via tfp_engine_last_error(NULL). */
int tfp_resample_taps(int32_t rate_in, int32_t rate_out, int32_t* L, int32_t* M, int32_t* k_lo, int32_t* ntaps,
                      int16_t* taps, int64_t cap);
/* One clip on the host: the map the GPU forms compute, sample for sample. out == NULL (cap 0) only sets
 * *nout = tfp_resample_count; cap < *nout -> TFP_E_CAPACITY with *nout set. Equal rates copy. Host-only.
 * The search forms without a rate twin (ranked, census, sliding, aligned, occurrences) take the output
 * of this call through their pcm form at rate_out. */
int tfp_resample_pcm(const int16_t* pcm, int64_t nsamples, int32_t rate_in, int32_t rate_out, int16_t* out, int64_t cap,
                     int64_t* nout);
/* tfp_fingerprint_batch over clips of rate_in: offsets[nclips+1] index into pcm, the frames equal
 * tfp_fingerprint_batch at rate_out over each clip's tfp_resample_pcm, bit for bit. The samples are
 * copied to the GPU as they are, converted there by one launch (each clip on its own: a clip's edge
 * never sees its neighbour), and fingerprinted by the launch an int16 batch of the output lengths at
 * rate_out takes (tfp_fingerprint_stats counts it alike). */
int tfp_fingerprint_rate_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                               int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes);
/* The results equal tfp_search_pcm_batch at rate_out on each query's tfp_resample_pcm. Not coalesced. */
int tfp_search_rate_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                          int32_t rate_in, int32_t rate_out, const tfp_search_params* params, tfp_result* out);
/* The rows equal tfp_search_scoped_pcm_batch at rate_out on each query's tfp_resample_pcm (the
 * dialplan's context search of a call heard at another rate). frame_counts[nqueries] (may be NULL)
 * receives each query's frame count at rate_out, which the caller's sample counts do not tell. */
int tfp_search_scoped_rate_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                 int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                                 const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                 int32_t* frame_counts);
/* Rate conversion on the GPU so far: launches, the samples they read and the samples they wrote.
 * Counted where the kernel is issued (a batch without an output sample launches nothing). Any pointer
 * may be NULL. */
int tfp_resample_stats(tfp_engine* eng, int64_t* launches, int64_t* samples_in, int64_t* samples_out);
/* The same on a group, equal to the engine forms: a fingerprint batch's clips are converted by the
 * shard that fingerprints them (cut by their frames at rate_out); a search batch is converted and
 * fingerprinted by every shard, and the shards' results are combined as the pcm forms' are. */
int tfp_group_fingerprint_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                                     int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes);
int tfp_group_search_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                int32_t rate_in, int32_t rate_out, const tfp_search_params* params, tfp_result* out);
int tfp_group_search_scoped_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                       int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                                       const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                       int32_t* frame_counts);

/* ---- deterministic synthetic PCM (benchmark / test data; identical host and device) -- */
/* One spec per clip: samples s of clip = synth(seed, clip, offset + s). */
typedef struct tfp_synth_spec {
  uint64_t seed;
  int64_t clip;
  int64_t offset;
} tfp_synth_spec;
int tfp_synth_pcm(const tfp_synth_spec* specs, int32_t nclips, int64_t samples_per_clip, int16_t* out);
int tfp_synth_pcm_device(tfp_engine* eng, const tfp_synth_spec* specs, int32_t nclips, int64_t samples_per_clip,
                         int16_t* d_out, void* stream);

/* ---- misc --------------------------------------------------------------------------- */
int tfp_synchronize(tfp_engine* eng, void* stream);

/* ---- mixed batches: clips of any rate, channel count and sample kind in one call (new) ------------ */
/* The three rate-normalised families below take ONE (rate_in, channels, sample kind) for a whole batch. A
 * prompt directory is mixed: 8 kHz .ulaw files, 16-bit mono WAVs at 8 and 16 kHz, 44.1/48 kHz stereo
 * masters of 16 and 24 bits. These forms take such a batch as it is: every clip carries its own rate,
 * channel count and kind, the whole call is converted to rate_out by ONE launch, and the unchanged
 * fingerprint kernels run behind it.
 * Nothing new is defined. A clip's int16 output is, by decree, the existing host map of its own class:
 *   TFP_AUDIO_S16, 1 channel     tfp_resample_pcm
 *   TFP_AUDIO_S16, C >= 2        tfp_resample_mix_pcm
 *   TFP_AUDIO_Q31                tfp_resample_wide_pcm        (int32 Q31, any C)
 *   TFP_AUDIO_ULAW / _ALAW       tfp_g711_decode, then tfp_resample_pcm
 * bit for bit, equal rates included (a copy, the integer mean, the Q31 mean, the expansion), and
 * tfp_resample_any_pcm is that dispatch on the host. The frames / results / rows of the engine forms equal
 * the pcm forms at rate_out over each clip's tfp_resample_any_pcm.
 * data is read-only and clips may overlap in it or name the same bytes. offset counts BYTES.
 * Argument rules, all TFP_E_ARG and all-or-nothing (nothing is launched or written; the message names the
 * first offending clip as "clip i: ..."): a rate <= 0 ("bad sample rate"); a pair the table builder refuses,
 * a Q31 clip with A C >= 2^30, or G.711 codes at a reduction past the int16 staging limit, about 29 to 1
 * ("unsupported rate ratio"); channels outside 1 .. TFP_MIX_CHANNELS_MAX; a G.711 kind with channels != 1;
 * an unknown kind; reserved != 0; an offset that is negative or no multiple of the sample size; nframes <
 * 0; a clip reaching past nbytes; more than TFP_ANY_RATES_MAX distinct rate_in values.
 * Out of scope: float-to-Q31 and packed 24-bit samples on the device (tfp_wav_decode_interleaved_q31 does
 * both on the host), taps in LDS, live pushes and tfp_stream_push of anything but mono int16 and G.711, a
 * query-sharded group search (every shard converts a search batch), coalescing. */
enum { TFP_AUDIO_S16 = 0, TFP_AUDIO_Q31 = 1, TFP_AUDIO_ULAW = 2, TFP_AUDIO_ALAW = 3 };
#define TFP_ANY_RATES_MAX 64       /* distinct rate_in values in one call */
typedef struct tfp_audio_clip {
  int64_t offset;    /* BYTES into `data`; a multiple of the sample size (2, 4, 1, 1) */
  int64_t nframes;   /* frames of `channels` interleaved samples; 0 is a clip without frames */
  int32_t rate_in;
  int32_t channels;  /* 1 .. TFP_MIX_CHANNELS_MAX; G.711 kinds: 1 only */
  int32_t kind;
  int32_t reserved;  /* 0 */
} tfp_audio_clip;
/* One clip on the host: the dispatch to the four host maps above, sample for sample what the GPU forms
 * compute. clip->offset is applied to data; the clip's extent is the caller's to guarantee here (there is
 * no nbytes). The size query (out == NULL, cap 0) and TFP_E_CAPACITY as tfp_resample_pcm. Host-only. */
int tfp_resample_any_pcm(const void* data, const tfp_audio_clip* clip, int32_t rate_out, int16_t* out, int64_t cap,
                         int64_t* nout);
/* The argument rules above on their own, without an engine: TFP_OK, or TFP_E_ARG with the message the
 * engine forms give (tfp_engine_last_error(NULL)). nout, if not NULL, receives nclips output lengths at
 * rate_out. Host-only; builds the pairs' tables (cached per process). */
int tfp_audio_clips_check(const tfp_audio_clip* clips, int32_t nclips, int64_t nbytes, int32_t rate_out, int64_t* nout);
/* The twins of the *_rate_batch forms, (data, nbytes, clips, nclips) in place of (pcm, offsets, nclips,
 * rate_in): output conventions are theirs (frame_counts[i] = frames of query i at rate_out). The bytes are
 * copied to the GPU as they are, in one copy, and converted there by one launch whatever the number of
 * classes; no launch when no clip has output. Not coalesced. */
int tfp_fingerprint_any_batch(tfp_engine* eng, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nclips,
                              int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes);
int tfp_search_any_batch(tfp_engine* eng, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nqueries,
                         int32_t rate_out, const tfp_search_params* params, tfp_result* out);
int tfp_search_scoped_any_batch(tfp_engine* eng, const void* data, int64_t nbytes, const tfp_audio_clip* clips,
                                int32_t nqueries, int32_t rate_out, const tfp_search_params* params, const int32_t* scopes,
                                int32_t k, tfp_candidate* out, int32_t* counts, int32_t* frame_counts);
/* The mixed kernel's launches so far, the clips and frames they read, the samples they wrote, and their
 * tiles of 1,024 outputs by form: staged in LDS under the clip's class's own limit, read per tap in global
 * memory past it, or plain (equal rates: no filter). Counted where the kernel is issued. A mixed call
 * moves none of tfp_resample_stats, tfp_resample_mix_stats, tfp_resample_wide_stats or tfp_g711_stats.
 * Any pointer may be NULL. */
int tfp_resample_any_stats(tfp_engine* eng, int64_t* launches, int64_t* clips, int64_t* frames_in, int64_t* samples_out,
                           int64_t* tiles_staged, int64_t* tiles_global, int64_t* tiles_plain);
/* The same on a group. A fingerprint batch is cut by its frames at rate_out as the rate twins cut theirs,
 * and each shard is handed only the byte range its clips span; every shard converts a search batch. */
int tfp_group_fingerprint_any_batch(tfp_group* g, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nclips,
                                    int32_t rate_out, tfp_frame* out, int64_t cap, int64_t* nframes);
int tfp_group_search_any_batch(tfp_group* g, const void* data, int64_t nbytes, const tfp_audio_clip* clips, int32_t nqueries,
                               int32_t rate_out, const tfp_search_params* params, tfp_result* out);
int tfp_group_search_scoped_any_batch(tfp_group* g, const void* data, int64_t nbytes, const tfp_audio_clip* clips,
                                      int32_t nqueries, int32_t rate_out, const tfp_search_params* params,
                                      const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                      int32_t* frame_counts);

/* ---- rate-normalised ingest of 24/32-bit and float audio: Q31 forms on the GPU (new) ------------ */
/* A prompt master out of a DAW or a studio is a 24-bit, 32-bit or float WAV at 44.1 or 48 kHz, usually
 * stereo. These forms take such audio without an outside requantisation to int16, which would be a
 * second definition. Wide samples are int32 Q31: value v in [-1, 1) is stored as v 2^31. Frames are
 * interleaved, q[i * C + c] with 1 <= C <= TFP_MIX_CHANNELS_MAX; clip lengths and offsets[] count FRAMES.
 * L, M, k_lo, ntaps, h[p][k] and n_out are exactly those of the pair's table (tfp_resample_taps,
 * tfp_resample_count of the frame count); no new table is built. The converter is linear, so widening
 * the samples changes only the accumulator's range and the final rounding:
 *   S[i] = sum_c q[i][c]                        (exact, |S| <= 2^36; 0 outside the clip's own frames)
 *   acc  = sum_k h[p][k] S[i0 + k]              (exact, 64-bit; i0 = n M div L, p = n M mod L)
 *   y[n] = clamp(floor((acc + 2^30 C) / (2^31 C)), -32768, 32767)
 * The division is a floor, not a truncation: q = (acc + 2^30 C) >> 31, then a 32-bit floor division by C.
 * rate_in == rate_out runs no filter: y[i] = clamp(floor((S[i] + 2^15 C) / (2^16 C))); the clamp is
 * needed there, since Q31 full scale rounds to 32768.
 * Consistency: for int16 frames x, the wide form on x << 16 is tfp_resample_mix_pcm of x bit for bit
 * (acc_wide = 2^16 acc), and for C = 1 it is tfp_resample_pcm. Host and GPU agree bit for bit.
 * Range: with A = max_p sum_k |h[p][k]| of the pair's table, |acc| <= 2^31 C A. A wide call with
 * A C >= 2^30 is TFP_E_ARG with "unsupported rate ratio"; below that acc stays under 2^61 and q fits
 * int32. The largest A over the pairs tests/test_resample_wide_host.py lists is 70,210 (7999 -> 8001,
 * about 2.14 * 32768), so A C stays below 2^22 at C = 32 and no supported pair met so far is refused.
 * Sample to Q31 happens on the host only (tfp_wav_decode_interleaved_q31, tfp_q31_from_f32 / _f64):
 * unsigned 8-bit (u - 128) << 24, signed 16-bit << 16, signed 24-bit << 8, signed 32-bit as stored,
 * float32 clamp(nearbyintf(x * 2^31f)) and float64 the same in double, ties to even (the product is exact:
 * a power-of-two scale), clamped to [-2^31, 2^31 - 1] so that +1.0 becomes 2^31 - 1, NaN 0, +-inf clamped.
 * It is not done on the GPU: denormal handling there would be a second definition.
 * Like the int16 mix form this is a new definition and NOT aubio's fp32 value (fp_handler.c:604, :633):
 * a file at the index's own rate should keep using tfp_wav_decode_f32 and the f32 forms.
 * Refusals and messages are those of the mix forms ("unsupported channel count", "bad sample rate",
 * "unsupported rate ratio"), plus the range refusal above. An argument error writes nothing to the outputs.
 * Not covered: live pushes and tfp_stream_push of wide samples, the compiled shim, per-clip channel
 * counts inside one call (tfp_fingerprint_any_batch, "mixed batches" above, takes those), packed 24-bit samples
 * on the device, float-to-Q31 on the device. */
/* RIFF/WAVE -> interleaved int32 Q31: integer PCM of 8, 16, 24 or 32 bits (format 1) and float of 32 or
 * 64 bits (format 3), or EXTENSIBLE with either subformat, 1 to TFP_MIX_CHANNELS_MAX channels. G.711 and
 * more channels are TFP_E_FORMAT with a reason. *nframes receives the whole frames present (a trailing
 * partial frame is dropped); cap counts samples, nframes * channels of them are written. Chunk skipping,
 * unpatched and truncated data sizes, the size query (q31 == NULL, cap 0) and TFP_E_CAPACITY (with
 * *nframes / *channels set) as tfp_wav_decode_interleaved. Host-only. */
int tfp_wav_decode_interleaved_q31(const void* bytes, int64_t nbytes, int32_t* q31, int64_t cap, int64_t* nframes,
                                   int32_t* channels, int32_t* sample_rate);
int tfp_wav_read_interleaved_q31(const char* path, int32_t* q31, int64_t cap, int64_t* nframes, int32_t* channels,
                                 int32_t* sample_rate);
/* The float maps above, n samples from src to dst (which may not overlap). Host-only. */
int tfp_q31_from_f32(const float* src, int64_t n, int32_t* dst);
int tfp_q31_from_f64(const double* src, int64_t n, int32_t* dst);
/* One clip on the host: the map the GPU forms compute, sample for sample. The size query and
 * TFP_E_CAPACITY as tfp_resample_mix_pcm (*nout = tfp_resample_count(nframes), or nframes at equal rates). */
int tfp_resample_wide_pcm(const int32_t* q31, int64_t nframes, int32_t channels, int32_t rate_in, int32_t rate_out,
                          int16_t* out, int64_t cap, int64_t* nout);
/* The twins of the mix forms over Q31 frames: the frames / results / rows equal the pcm forms at rate_out
 * over each clip's tfp_resample_wide_pcm, bit for bit. The int32 frames are copied to the GPU as they are
 * and converted there by one launch (each clip on its own); the fingerprint launch is the one an int16
 * batch of the output lengths takes. channels == 1 and equal rates are forms of this launch too (the
 * samples are not the rate forms' int16): equal rates round and clamp only. Not coalesced. */
int tfp_fingerprint_wide_rate_batch(tfp_engine* eng, const int32_t* q31, const int64_t* offsets, int32_t nclips,
                                    int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                    int64_t* nframes);
int tfp_search_wide_rate_batch(tfp_engine* eng, const int32_t* q31, const int64_t* offsets, int32_t nqueries,
                               int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                               tfp_result* out);
int tfp_search_scoped_wide_rate_batch(tfp_engine* eng, const int32_t* q31, const int64_t* offsets, int32_t nqueries,
                                      int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                                      const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                      int32_t* frame_counts);
/* The wide kernel's launches so far, the frames they read, the samples they wrote, and how many of the
 * launches staged in LDS (one channel: up to 15,360 int32 samples per tile; several: up to 7,680 int64
 * sums; equal rates always) rather than reading global memory per tap. Counted where the kernel is
 * issued; tfp_resample_stats and tfp_resample_mix_stats do not count these. Any pointer may be NULL. */
int tfp_resample_wide_stats(tfp_engine* eng, int64_t* launches, int64_t* frames_in, int64_t* samples_out,
                            int64_t* staged_launches);
/* The same on a group, split and combined exactly as the mix twins. */
int tfp_group_fingerprint_wide_rate_batch(tfp_group* g, const int32_t* q31, const int64_t* offsets, int32_t nclips,
                                          int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                          int64_t* nframes);
int tfp_group_search_wide_rate_batch(tfp_group* g, const int32_t* q31, const int64_t* offsets, int32_t nqueries,
                                     int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                                     tfp_result* out);
int tfp_group_search_scoped_wide_rate_batch(tfp_group* g, const int32_t* q31, const int64_t* offsets, int32_t nqueries,
                                            int32_t channels, int32_t rate_in, int32_t rate_out,
                                            const tfp_search_params* params, const int32_t* scopes, int32_t k,
                                            tfp_candidate* out, int32_t* counts, int32_t* frame_counts);

/* ---- rate-normalised ingest of multichannel int16: downmix and convert on the GPU (new) -------- */
/* The files the rate forms were built for are seldom mono: a prompt master is 44.1 or 48 kHz stereo, a
 * MixMonitor recording is two-channel. These forms take interleaved int16 frames of C channels
 * (1 <= C <= TFP_MIX_CHANNELS_MAX; frame i, channel c at pcm[i * C + c]) at rate_in to mono int16 at
 * rate_out. Clip lengths and offsets[] count FRAMES, not samples. L, M, k_lo, ntaps, h[p][k] and n_out
 * are exactly those of the pair's table above (tfp_resample_taps, tfp_resample_count of the frame
 * count); no new table is built. The converter is linear and exact, so the exact sum over channels
 * commutes with the exact sum over taps:
 *   S[i] = sum_c x[i][c]                        (exact; 0 outside the clip's own frames)
 *   acc  = sum_k h[p][k] S[i0 + k]              (exact, 64-bit; i0 = n M div L, p = n M mod L)
 *   y[n] = clamp(floor((acc + 16384 C) / (32768 C)), -32768, 32767)
 * The division is a floor, not a truncation. One exact sum, one rounding, one clamp: host and GPU agree
 * bit for bit, and C = 1 is tfp_resample_pcm bit for bit. A product h S needs more than 32 bits from
 * C = 3 on; |acc| stays below 2^37 for C <= 32. rate_in == rate_out runs no filter: n_out = n_in and
 * y[i] = floor((2 S[i] + C) / (2 C)), the integer mean rounded half up (an identity tap of 32768 does
 * not fit the int16 table, so this is a case of its own).
 * This is a new definition and NOT aubio's fp32 channel mean (fp_handler.c:604, :633), which lies
 * between int16 steps. It exists for the rate change: a file at the index's own rate should keep using
 * tfp_wav_decode_f32 and the f32 forms, which reproduce the reference.
 * channels < 1 or > TFP_MIX_CHANNELS_MAX is TFP_E_ARG with "unsupported channel count"; a bad rate and
 * an unsupported pair are refused as the rate forms refuse them. An argument error writes nothing to
 * the outputs.
 * Not covered: live pushes and tfp_stream_push with more than one channel, the compiled shim,
 * per-clip channel counts inside one call (tfp_fingerprint_any_batch takes those).
 * 24/32-bit and float input is not taken by these int16 forms:
 * it goes through the Q31 forms of the section before this one (tfp_fingerprint_wide_rate_batch). */
#define TFP_MIX_CHANNELS_MAX 32
/* RIFF/WAVE -> the interleaved int16 samples as stored: integer PCM (format 1, or EXTENSIBLE with the
 * PCM subformat), 8-bit ((u - 128) << 8) or 16-bit, 1 to TFP_MIX_CHANNELS_MAX channels. 24/32-bit,
 * float, G.711 and more channels are TFP_E_FORMAT with a reason. *nframes receives the whole frames
 * present (a trailing partial frame is dropped); cap counts samples, nframes * channels of them are
 * written. Chunk skipping, unpatched and truncated data sizes, the size query (pcm == NULL, cap 0) and
 * TFP_E_CAPACITY (with *nframes / *channels set) as tfp_wav_decode. Host-only. */
int tfp_wav_decode_interleaved(const void* bytes, int64_t nbytes, int16_t* pcm, int64_t cap, int64_t* nframes,
                               int32_t* channels, int32_t* sample_rate);
int tfp_wav_read_interleaved(const char* path, int16_t* pcm, int64_t cap, int64_t* nframes, int32_t* channels,
                             int32_t* sample_rate);
/* One clip on the host: the map the GPU forms compute, sample for sample. The size query and
 * TFP_E_CAPACITY as tfp_resample_pcm (*nout = tfp_resample_count(nframes), or nframes at equal rates). */
int tfp_resample_mix_pcm(const int16_t* pcm, int64_t nframes, int32_t channels, int32_t rate_in, int32_t rate_out,
                         int16_t* out, int64_t cap, int64_t* nout);
/* The twins of tfp_fingerprint_rate_batch, tfp_search_rate_batch and tfp_search_scoped_rate_batch with
 * `channels` added and offsets in frames: the frames / results / rows equal the pcm forms at rate_out
 * over each clip's tfp_resample_mix_pcm, bit for bit. The interleaved samples are copied to the GPU as
 * they are and downmixed and converted there by one launch (each clip on its own); the fingerprint
 * launch is the one an int16 batch of the output lengths takes (tfp_fingerprint_stats counts it alike).
 * channels == 1 IS the rate form (counted by tfp_resample_stats); at equal rates it is the plain form.
 * Equal rates with channels > 1 run the downmix alone. Not coalesced. */
int tfp_fingerprint_mix_rate_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                                   int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                   int64_t* nframes);
int tfp_search_mix_rate_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                              int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                              tfp_result* out);
int tfp_search_scoped_mix_rate_batch(tfp_engine* eng, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                     int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                                     const int32_t* scopes, int32_t k, tfp_candidate* out, int32_t* counts,
                                     int32_t* frame_counts);
/* The multichannel kernel's launches so far, the frames they read, the samples they wrote, and how many
 * of the launches ran the form that stages channel sums in LDS (the others read global memory per tap:
 * a pair whose tile spans more than 15,360 frames). Counted where the kernel is issued; tfp_resample_stats
 * keeps its meaning and does not count these. Any pointer may be NULL. */
int tfp_resample_mix_stats(tfp_engine* eng, int64_t* launches, int64_t* frames_in, int64_t* samples_out,
                           int64_t* staged_launches);
/* The same on a group, split and combined exactly as the rate twins: fingerprint clips are cut by their
 * frames at rate_out, a search batch is converted on every shard. */
int tfp_group_fingerprint_mix_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nclips,
                                         int32_t channels, int32_t rate_in, int32_t rate_out, tfp_frame* out, int64_t cap,
                                         int64_t* nframes);
int tfp_group_search_mix_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                    int32_t channels, int32_t rate_in, int32_t rate_out, const tfp_search_params* params,
                                    tfp_result* out);
int tfp_group_search_scoped_mix_rate_batch(tfp_group* g, const int16_t* pcm, const int64_t* offsets, int32_t nqueries,
                                           int32_t channels, int32_t rate_in, int32_t rate_out,
                                           const tfp_search_params* params, const int32_t* scopes, int32_t k,
                                           tfp_candidate* out, int32_t* counts, int32_t* frame_counts);

/* ---- live calls at another rate: each push converted to the index's rate on the GPU (new) -------- */
/* An Asterisk channel is often not at the index's rate (slin16 from G.722, slin48 from Opus, an 8 kHz
 * G.711 leg against a catalog enrolled at 16 kHz), and record_voice hands over its frames as they arrive
 * (application_handler.c:248-312; the reference takes every file at its native rate, fp_handler.c:37).
 * A rate object is a live object whose ticks arrive at rate_in: every push is converted by the converter
 * of "rate-normalised ingest" (L, M, k_lo, ntaps, k_hi = k_lo + ntaps - 1; output n reads the input
 * samples i0 + k_lo .. i0 + k_hi, i0 = n M div L) on its way into the int16 history, and everything
 * behind the history is unchanged. With S_in input samples taken by a channel since its last reset:
 *   settled  output n is settled once i0 + k_hi <= S_in - 1. N(S_in) = tfp_resample_count(S_in - k_hi)
 *            outputs are settled, 0 while S_in <= k_hi, and the channel's history is exactly the first
 *            N(S_in) samples of tfp_resample_pcm of its S_in input samples, hence of every continuation
 *            of the call: a settled sample never changes.
 *   lag      k_hi input samples: 48 at 16000 -> 8000, 144 at 48000 -> 8000, 24 at 8000 -> 16000,
 *            133 at 44100 -> 8000; 3 ms in every case.
 *   carry    the last ntaps - 1 input samples per channel are kept on the GPU between pushes; samples
 *            before the call's start are zeros, as the batch definition has them.
 *   flush    after k_hi zero samples N = tfp_resample_count(S_in) over the call's own samples and the
 *            history equals tfp_resample_pcm of the call, its last outputs included (zero flush).
 * By contract a rate object is a plain live object that has been pushed each tick's newly settled
 * samples: rows, frame counts, tfp_live_samples (the settled count), a verdict's total_samples, window
 * frames and occurrence frames are all in index-rate terms. One input rate per object: a caller with
 * legs at several rates keeps one object per rate. */
/* tfp_live_create with an input rate (record_voice's channel format, application_handler.c:248-312;
 * fp_handler.c:37). max_samples is in samples at sample_rate, range as tfp_live_create. rate_in < 1 is
 * TFP_E_ARG "bad sample rate"; a pair whose table passes 2^20 entries, or whose filter alone
 * (ntaps + ceil(M / L) + 1 samples) passes the 30,720 samples a workgroup stages, is TFP_E_ARG
 * "unsupported rate ratio". rate_in == sample_rate gives a plain object (no filter, no carry, lag 0).
 * On a rate object tfp_live_push and tfp_live_push_g711 take the tick at rate_in (int16, mu-law and
 * A-law pushes of one call may alternate: the carry is int16); a push that would take any channel's
 * settled count past max_samples is TFP_E_CAPACITY and ingests nothing (no carry or input count moves);
 * tfp_live_reset restarts the channel's input count. */
int tfp_live_create_rate(tfp_engine* eng, int32_t nchannels, int32_t rate_in, int32_t sample_rate, int64_t max_samples,
                         tfp_live** out);
/* Input samples `channel` has taken since its last reset (record_voice's running length at the
 * channel's own rate, application_handler.c:248-312); on a plain object tfp_live_samples. */
int tfp_live_input_samples(tfp_live* lv, int32_t channel, int64_t* nsamples);
/* The object's input rate and its lag k_hi in input samples (fp_handler.c:37: the rate the audio came
 * at); a plain object: its sample rate and 0. Pushing lag_in zeros to a channel at the end of its call
 * settles every output. Either pointer may be NULL. */
int tfp_live_rate_info(tfp_live* lv, int32_t* rate_in, int64_t* lag_in);
/* Conversion launches of this object's pushes, the input samples they took and the samples they settled
 * (the per-tick conversion of record_voice's frames, application_handler.c:248-312). Apart from
 * tfp_resample_stats, whose meaning stays. Any pointer may be NULL. */
int tfp_live_rate_stats(tfp_live* lv, int64_t* launches, int64_t* samples_in, int64_t* samples_out);
/* The same on a group (application_handler.c:248-312; fp_handler.c:37): every shard keeps every channel,
 * so the shards are created with the rate and pushed the same tick; the capacity check, made before any
 * shard is told, uses the same arithmetic over the group's own input counts. tfp_group_live_rate_stats is
 * shard `shard`'s tfp_live_rate_stats. */
int tfp_group_live_create_rate(tfp_group* g, int32_t nchannels, int32_t rate_in, int32_t sample_rate, int64_t max_samples,
                               tfp_group_live** out);
int tfp_group_live_input_samples(tfp_group_live* lv, int32_t channel, int64_t* nsamples);
int tfp_group_live_rate_info(tfp_group_live* lv, int32_t* rate_in, int64_t* lag_in);
int tfp_group_live_rate_stats(tfp_group_live* lv, int32_t shard, int64_t* launches, int64_t* samples_in,
                              int64_t* samples_out);

#ifdef __cplusplus
}
#endif
#endif
