/* fp_handler_tfp.h — the engine facade of the module (src/fp_handler.h:13-38, unchanged
 * signatures) as built from shim/fp_handler_tfp.c (hot half) + shim/fp_catalog.c (catalog half),
 * plus what the MI355X engine adds for the module's callers. */
#ifndef FP_HANDLER_TFP_H
#define FP_HANDLER_TFP_H

#include <stdbool.h>
#include <stdint.h>

struct ast_json;

/* src/fp_handler.h:13-38 */
bool fp_init(void);
bool fp_term(void);
bool fp_create_context_list_info(const char* name, const char* directory, bool replace);
bool fp_delete_context_list_info(const char* name);
struct ast_json* fp_get_context_lists_all(void);
struct ast_json* fp_get_context_list_info(const char* name);
struct ast_json* fp_get_audio_lists_all(void);
struct ast_json* fp_get_audio_lists_by_contextname(const char* name);
bool fp_craete_audio_list_info(const char* context, const char* filename);
bool fp_delete_audio_list_info(const char* uuid);
struct ast_json* fp_search_fingerprint_info(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high);
char* fp_generate_uuid(void);
char* fp_create_hash(const char* filename);

/* New: fp_craete_audio_list_info over a list of files of one context, as app_tiresias.c's
 * create_new_audio_info (:365-424) calls it file by file for its directory scan. ok[i] (ok may be
 * NULL) receives what fp_craete_audio_list_info(context, filenames[i]) would return. Returns the
 * number of files newly enrolled, or -1 for bad arguments. */
int fp_create_audio_list_infos(const char* context, const char* const* filenames, int count, bool* ok);

/* New: the GPUs the module's engines run on (tfp_group: the enrolled clips sharded over them,
 * every search on all of them), before fp_init — e.g. from a "devices" option of tiresias.conf:
 * "0-7", "0,2,5", or "" / NULL for every visible GPU (the default). */
void fp_set_gpu_devices(const char* list);

/* New: the index rate, before fp_init like fp_set_gpu_devices, e.g. from an "index_rate" option of
 * tiresias.conf. 0, the default, keeps every file at its native rate, as the reference does, and then
 * nothing changes. With a rate set (8000 for a telephony deployment), a file of another rate, of any
 * channel count (1 to 32) and kind (8/16/24/32-bit integer, float, G.711), is brought to it, so a prompt
 * enrolled from a 44.1 kHz stereo master matches the same prompt heard on an 8 kHz call:
 *  - fp_create_audio_list_infos collects such files into one mixed bucket, flushed by one
 *    tfp_group_fingerprint_any_batch (converted on the GPU, one launch per shard);
 *  - fp_craete_audio_list_info and every file search read such a file as the same map computed on the
 *    host (tfp_resample_any_pcm; bit-equal to the GPU's), at the index rate;
 *  - a file no reader takes, or at an unsupported rate ratio, is refused with the engine's message in the
 *    log, before any catalog row is written;
 *  - files at the index rate keep their paths (fp32 for multichannel included), and fp_live_open and
 *    fp_channel_* are unchanged: a call is opened at its own rate. */
void fp_set_index_rate(int rate);

/* New: how the channel threads' fp_search_fingerprint_info calls ran. Concurrent calls are
 * coalesced into shared GPU batches (tfp_group_search_pcm_batch, include/tiresias_fp.h): *calls
 * searches went through the coalescer as *batches batches. false before fp_init. */
bool fp_get_search_stats(int64_t* calls, int64_t* batches);

/* New: ranked search. fp_search_fingerprint_info returns the first row of its result query
 * (src/fp_handler.c:367-374: count(*) descending, tied counts by audio_uuid descending); this
 * returns the first max_results rows (at most 32) as a JSON array of the same objects, each with
 * frame_count and match_count, in rank order: element 0 is fp_search_fingerprint_info's answer,
 * element 1 the runner-up a dialplan compares it with. Empty array: NOTFOUND. NULL: bad arguments
 * or an unreadable file. A row whose audio_list entry is missing is skipped. */
struct ast_json* fp_search_fingerprint_candidates(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int max_results);

/* New: context-scoped search. fp_search_fingerprint_info and the calls above span every context, as
 * the reference's per-frame SQL does (src/fp_handler.c:308-314 has no context predicate) although
 * its documentation promises a search "from the context's audio list"
 * (doc/dialplan_application.rst:11, :52-53). This returns fp_search_fingerprint_candidates' array
 * over the clips enrolled in `context` alone: the first max_results rows of src/fp_handler.c:367-374
 * with "and context = '<context>'" in the insert, selected on the GPU among that context's clips
 * (not filtered out of the global rows). Empty array: NOTFOUND, also for a context without clips. */
struct ast_json* fp_search_fingerprint_in_context(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int max_results);

/* New: match census. The result query (src/fp_handler.c:367-374) lists one row per clip with a
 * non-zero count; every call above reads its head, and none says how the head stands against the
 * rest of the catalog, which on 8 kHz audio (max1 spans about 1 dB) is the missing half of the
 * application's decision (src/application_handler.c:180-203): a count of 80/94 that three clips reach
 * is not one that 4,000 clips reach. This returns, for the clips enrolled in `context` (a scope, as for
 * fp_search_fingerprint_in_context), a JSON object: "winner" (that call's first object, or null),
 * "frame_count", "population" (the context's clips), "clips_at_or_above" (clips whose count reaches
 * the winner's, the winner included), "clips_tied" (count equal to the winner's, the winner included)
 * and "histogram" ([[count, clips], ...]: the exact number of clips at each count, non-zero bins only,
 * counts descending, so count 0 comes last). NULL: bad arguments or an unreadable file. */
struct ast_json* fp_search_fingerprint_census(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high);

/* New: sliding search. The reference records a fixed duration and searches that one window
 * (src/application_handler.c:152-185, src/fp_handler.c:275-374). This searches every full window of
 * window_frames frames (256 samples each), hop_frames apart, of a longer recording, fingerprinting it
 * once: a JSON array of {"frame": <the window's first frame>, "rows": <fp_search_fingerprint_candidates'
 * array for that window's frames, frame_count = window_frames>} in time order, so a caller reads
 * whether, and when, an enrolled clip occurs in the recording. in_context: every window searches the
 * clips enrolled in `context` alone, as fp_search_fingerprint_in_context. Empty array: the recording
 * is shorter than one window. NULL: bad arguments or an unreadable file. */
struct ast_json* fp_search_fingerprint_timeline(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int window_frames,
		const int hop_frames, const int max_results, const bool in_context);

/* New: aligned search. fp_search_fingerprint_candidates' array (src/fp_handler.c:367-374 read to
 * row max_results), each element with four more integers saying where in the clip the recording
 * lies: "aligned_count" (the matching frames that agree on one time offset, <= match_count),
 * "offset" (query frame i lies at clip frame i + offset; 256 samples per frame; negative: the
 * recording starts before the clip), "first_frame" and "last_frame" (the first and last query frame
 * on that offset). A dialplan reads how far into an announcement the call is from offset, and
 * tells twenty frames in order from twenty scattered coincidences by aligned_count. */
struct ast_json* fp_search_fingerprint_aligned(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int max_results);

/* New: sliding aligned search. fp_search_fingerprint_timeline's array (src/fp_handler.c:367-374 per
 * window), each row with where in the clip its window lies: "aligned_count", "offset", "first_frame"
 * and "last_frame" as fp_search_fingerprint_aligned words them, window-relative (window frame x lies at
 * clip frame x + offset), and "clip_start_frame" = frame - offset, the recording frame at which clip
 * frame 0 lies. clip_start_frame is equal across the windows of one occurrence of a clip wherever the
 * occurrence's offset is the only one attaining the window's aligned_count, so a caller joins the
 * windows into "the announcement runs from recording frame A to B, from clip frame C on". A window
 * that fits the clip equally well in an earlier place reports the earlier one (the smallest offset
 * wins): join on the value most windows of a stretch agree on, and prefer windows of 48 frames or
 * more, since max1 of 8 kHz audio spans about 1 dB and short windows tie often.
 * The file is fingerprinted once and every row aligned on the GPU that holds its clip. NULL and the
 * empty array as for the timeline call. */
struct ast_json* fp_search_fingerprint_timeline_aligned(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int window_frames,
		const int hop_frames, const int max_results, const bool in_context);

/* New: occurrence search. Which clips of `context` play in the recording, and from which frame to
 * which: the join the timeline call above leaves to its caller, done by the engines. Every candidate
 * (clip, clip_start_frame) named by the first k rows (src/fp_handler.c:367-374) of a window is verified
 * along its own diagonal over the whole recording with the per-frame predicate of
 * src/fp_handler.c:287-351; hits at most max_gap frames apart form a segment, a candidate's best segment
 * needs min_hits hits, and overlapping candidates of one clip are thinned to the best. A JSON array, by
 * "first_frame", of the clips' audio_list rows with "frame_count" (the recording's frames),
 * "match_count" (= "hits"), "clip_start_frame", "first_frame", "last_frame" (recording frames), "hits", "diagonal_hits", "overlap"
 * and "windows". The context is a scope, as for fp_search_fingerprint_in_context. NULL for bad
 * arguments; the empty array where nothing plays or the recording is shorter than a window. */
struct ast_json* fp_search_fingerprint_occurrences(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int window_frames,
		const int hop_frames, const int k, const int max_gap, const int min_hits);

/* New: a live channel, for the dialplan application's record loop (application_handler.c:152-185,
 * record_voice :248-312) without the /tmp WAV round trip. Open one per call with max_ms >= the
 * recording's duration, push every voice frame's SLIN samples as it is read (160 per 20 ms frame
 * at 8 kHz), then fp_channel_search: the same result as fp_search_fingerprint_info on a WAV of
 * the samples pushed since open / reset (of the last max_ms of them, if more were pushed). The
 * samples stay in engine-mapped memory, read by the GPU in place; concurrent channels' searches run
 * as shared batches. A channel is used by one thread at a time. */
typedef struct fp_channel fp_channel;
fp_channel* fp_channel_open(int sample_rate, int max_ms);
bool fp_channel_push(fp_channel* ch, const int16_t* slin, int nsamples);
/* New: the same for a channel whose native format is G.711 (160 payload bytes per 20 ms frame):
 * law is TFP_G711_ULAW or TFP_G711_ALAW. The codes are expanded into the channel's SLIN buffer
 * (tfp_g711_decode: the int16 aubio_source reads a mu-law / A-law file as, fp_handler.c:604, :633),
 * so the search equals fp_channel_push of the expanded samples. SLIN and G.711 pushes may mix. */
bool fp_channel_push_g711(fp_channel* ch, const uint8_t* payload, int nsamples, int law);
void fp_channel_reset(fp_channel* ch);
struct ast_json* fp_channel_search(fp_channel* ch, const char* context, const int coefs, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high);
void fp_channel_close(fp_channel* ch);

/* New: live calls, for a record loop that wants the application's answer as early as it is certain
 * (application_handler.c:152-185 with the planned duration of :163; record_voice :248-312). One object
 * holds nchannels calls on the GPUs from their first sample; the thread that gathers the channels'
 * 20 ms frames into one tick pushes it, and asks for the verdicts when it likes. Open after fp_init
 * with max_ms >= the longest duration; close before fp_term.
 * fp_live_push: slin[nchannels][tick_samples], channel c takes its first nsamples[c] samples
 * (NULL: the whole tick; 0: the channel delivered nothing). fp_live_push_g711: the same over the
 * channels' native payload, one byte per sample, law TFP_G711_ULAW or TFP_G711_ALAW, expanded on the
 * GPU (aubio_source's table[code], fp_handler.c:604, :633); SLIN and G.711 ticks may mix. Both only
 * ingest. A tick that would take any channel past max_ms is refused for every channel.
 * fp_live_verdict: contexts[nchannels] and duration_ms[nchannels] (the planned recording of each
 * call, >= what it has taken so far); a JSON array with one object per channel holding "decided",
 * "complete" (0 / 1), "remaining" (frames of the finished recording that can still change a count)
 * and "rival_match_count" (the best other clip's count so far, -1: the context has no other clip
 * that can match), and, when a clip leads, the fields of fp_search_fingerprint_info (uuid, name,
 * context, hash, "match_count": its count over the frames that are final, every frame once complete;
 * "frame_count": the frames so far). decided = 1 with a leader: fp_search_fingerprint_in_context on
 * the finished recording will return this clip first, whatever audio follows; decided = 1 without:
 * the call is complete and nothing matched. The context maps to a scope as for
 * fp_search_fingerprint_in_context; coefs is 1, as the dialplan passes it (application_handler.c:180).
 * NULL: bad arguments (a duration below what the channel has taken among them).
 * fp_live_window: for a clip that begins after an unknown lead-in (ringback, early media), the search
 * of the last window_ms of each call instead of the whole recording so far. contexts[nchannels]; a
 * JSON array with one object per channel: "first_frame" and "frame_count" (the window is frames
 * [first_frame, first_frame + frame_count) of the call, ceil(window_ms * rate / 1000 / 256) frames
 * once the call is that long, at least 1, the unfinished last frame included) and "rows", the first
 * k results of fp_search_fingerprint_in_context on exactly those frames, each with the fields of
 * fp_search_fingerprint_info (uuid, name, context, hash, match_count, frame_count). It ingests
 * nothing: push, then ask. coefs is 1. NULL: bad arguments (window_ms <= 0 or k < 1 among them).
 * fp_live_window_aligned: fp_live_window's JSON, each row additionally with where its clip lies in the
 * window (the per-frame predicate of src/fp_handler.c:287-351 along the clip's stored rows):
 * "aligned_count", "offset", "first_frame" and "last_frame" (window frames: window frame x is call
 * frame first_frame(channel) + x and lies at clip frame x + offset) and "clip_start_frame" = the
 * channel's first_frame - offset, the call frame at which clip frame 0 lies: a greeting of N frames
 * ends at call frame clip_start_frame + N. The field names are the sliding aligned timeline's. NULL on
 * bad arguments, as fp_live_window.
 * fp_live_occurrences: the log of each call so far (tfp_group_live_occurrences; src/fp_handler.c:287-351
 * along each candidate's diagonal, for the rows of :367-374): a JSON array with one array per channel, by
 * "first_frame"; each entry has the clip's catalog fields (uuid, name, context, hash) and
 * "clip_start_frame" (the call frame at which clip frame 0 lies), "first_frame", "last_frame", "hits"
 * (the best run of hits along the clip's diagonal: its first and last call frame and its hits),
 * "diagonal_hits", "overlap" and "windows". Each call offers the rows of fp_live_window_aligned for
 * window_ms to the channel's list of candidates and brings every candidate's trace up to the call's
 * frames, so ask after each tick or each few ticks. window_ms converts to frames as fp_live_window's;
 * max_gap_ms (the silence a run may bridge) the same way, 0 ms being 0 frames; min_hits >= 1. NULL: bad
 * arguments (window_ms <= 0, max_gap_ms < 0, min_hits < 1 or k < 1 among them).
 * fp_live_reset: a new call on `channel` (< 0: on every channel). */
typedef struct fp_live fp_live;
/* New: catalog neighbours, which enrolled audios sound like each other at a set of search parameters. The
 * MD5 dedup of fp_craete_audio_list_info (src/fp_handler.c:479-530) catches a byte-identical file and
 * nothing else. fp_get_audio_list_neighbours returns a JSON array with one object per audio of the context
 * (fp_get_audio_lists_by_contextname's rows, in their order; an audio without fingerprint rows is left out):
 * its catalog fields, frame_count (its stored rows) and neighbours, the first k rows (at most 32) of the
 * search of src/fp_handler.c:287-374 for the audio's own stored rows over the same context's audios, its
 * own row deleted. Each row is the audio's catalog object with match_count, aligned_count, offset,
 * first_frame and last_frame. One tfp_group_index_neighbours call per 512 audios.
 * fp_get_audio_neighbours is that object for one audio, over the audios of every context. NULL: bad
 * arguments (a NULL context or uuid, coefs outside [1,2], k < 1), an unknown uuid, or a failed search. */
struct ast_json* fp_get_audio_list_neighbours(const char* context, const int coefs, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k);
struct ast_json* fp_get_audio_neighbours(const char* uuid, const int coefs, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k);
/* The tfp_group_index_neighbours calls the two entries above have made so far. false before fp_init. */
bool fp_get_neighbour_stats(int64_t* calls);

fp_live* fp_live_open(int nchannels, int sample_rate, int max_ms);
bool fp_live_push(fp_live* lv, const int16_t* slin, int tick_samples, const int32_t* nsamples);
bool fp_live_push_g711(fp_live* lv, const uint8_t* payload, int tick_samples, int law, const int32_t* nsamples);
struct ast_json* fp_live_verdict(fp_live* lv, const char* const* contexts, const int* duration_ms, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high);
struct ast_json* fp_live_window(fp_live* lv, const char* const* contexts, const int window_ms, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k);
struct ast_json* fp_live_window_aligned(fp_live* lv, const char* const* contexts, const int window_ms, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k);
struct ast_json* fp_live_occurrences(fp_live* lv, const char* const* contexts, const int window_ms, const int max_gap_ms,
		const int min_hits, const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int k);
void fp_live_reset(fp_live* lv, int channel);
void fp_live_close(fp_live* lv);

#endif
