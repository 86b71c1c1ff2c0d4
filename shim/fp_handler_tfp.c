/* fp_handler_tfp.c — the hot half of the reference's engine facade (src/fp_handler.h:13-38) on
 * the MI355X engines (include/tiresias_fp.h): a device group over the node's GPUs, the enrolled
 * clips sharded over them. Built into app_tiresias.so with shim/fp_catalog.c (the catalog half:
 * the reference's SQLite tables and backup) in place of the reference's fp_handler.c and
 * db_ctx_handler.c.
 *
 *   fp_init / fp_term                fp_handler.c:68-108   + the GPU engines and their index
 *   fp_craete_audio_list_info        fp_handler.c:161-197  (sic "craete": the reference's name)
 *   fp_delete_audio_list_info        fp_handler.c:115-159  + tfp_group_index_remove
 *   fp_search_fingerprint_info       fp_handler.c:207-408
 *
 * Conventions kept: false / NULL plus ast_log on errors; the search returns NULL both for
 * NOTFOUND and for errors (application_handler.c:180-191 maps both to TIRSTATUS=NOTFOUND);
 * a file already enrolled in the context is a success (fp_handler.c:181-185); the result is
 * {uuid, name, context, hash, frame_count, match_count}, owned by the caller (ast_json_unref).
 * Every tfp_group_* call is serialised per group, so the channel threads need no lock here. */
#include "asterisk.h"

#include <ctype.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asterisk/json.h"
#include "asterisk/logger.h"
#include "asterisk/utils.h"

#include "fp_catalog.h"
#include "fp_handler_tfp.h"
#include "tiresias_fp.h"

static tfp_group* g_tfp = NULL; /* the module's engines: one per configured GPU (fp_set_gpu_devices) */
static char g_devices[256] = ""; /* "" : every visible GPU */
static void pcm_pool_drain(void);

/* fp_set_gpu_devices: "0,2,5", "0-7", or "" / NULL for every visible GPU (a device may repeat) */
void fp_set_gpu_devices(const char* list)
{
	snprintf(g_devices, sizeof(g_devices), "%s", list ? list : "");
}

/* fp_set_index_rate: the rate every enrolled and searched file is brought to (before fp_init, e.g. from
 * an "index_rate" option of tiresias.conf). 0, the default: every file at its native rate, as the
 * reference (DEF_AUBIO_SAMPLERATE 0); then nothing below differs from a shim without the setting. */
static int32_t g_index_rate = 0;
void fp_set_index_rate(int rate)
{
	g_index_rate = rate > 0 ? rate : 0;
}

static bool create_group(void)
{
	int32_t dev[64], n = 0, count = 0, a, b;
	const char* p = g_devices;
	char* end;

	if(tfp_device_count(&count) != TFP_OK || count <= 0) {
		return false;
	}
	while(*p != '\0' && n < 64) {
		if(*p == ',' || *p == ' ') {
			p++;
			continue;
		}
		a = (int32_t)strtol(p, &end, 10);
		if(end == p) {
			return false;
		}
		b = a;
		if(*end == '-') {
			p = end + 1;
			b = (int32_t)strtol(p, &end, 10);
			if(end == p) {
				return false;
			}
		}
		for(; a <= b && n < 64; a++) {
			dev[n++] = a;
		}
		p = end;
	}
	if(n == 0) {
		for(a = 0; a < count && a < 64; a++) {
			dev[n++] = a;
		}
	}
	return tfp_group_create(dev, n, &g_tfp) == TFP_OK;
}

/* Context name -> scope id of its clips in the engines (tfp_group_index_set_scope): ids from 1 in
 * order of first enrolment, so scope 0 (a new clip's) belongs to no context. Rebuilt at fp_init from
 * audio_list's context column. An unknown context maps to an id no clip has. */
static struct {
	char** name;
	int32_t n, cap;
} g_ctx;
static pthread_mutex_t g_ctx_lock = PTHREAD_MUTEX_INITIALIZER;

static int32_t scope_of_context(const char* context, bool create)
{
	int32_t i, id = -1;

	pthread_mutex_lock(&g_ctx_lock);
	for(i = 0; i < g_ctx.n; i++) {
		if(strcmp(g_ctx.name[i], context) == 0) {
			id = i + 1;
			break;
		}
	}
	if(id < 0 && create == false) {
		id = g_ctx.n + 1; /* no clip has it */
	}
	else if(id < 0) {
		if(g_ctx.n == g_ctx.cap) {
			const int32_t cap = g_ctx.cap ? 2 * g_ctx.cap : 16;
			char** grown = ast_realloc(g_ctx.name, sizeof(char*) * cap);
			if(grown != NULL) {
				g_ctx.name = grown;
				g_ctx.cap = cap;
			}
		}
		if(g_ctx.n < g_ctx.cap && (g_ctx.name[g_ctx.n] = ast_malloc(strlen(context) + 1)) != NULL) {
			strcpy(g_ctx.name[g_ctx.n], context);
			id = ++g_ctx.n;
		}
	}
	pthread_mutex_unlock(&g_ctx_lock);
	return id; /* -1: out of memory */
}

static void scopes_reset(void)
{
	int32_t i;

	pthread_mutex_lock(&g_ctx_lock);
	for(i = 0; i < g_ctx.n; i++) {
		ast_free(g_ctx.name[i]);
	}
	ast_free(g_ctx.name);
	g_ctx.name = NULL;
	g_ctx.n = g_ctx.cap = 0;
	pthread_mutex_unlock(&g_ctx_lock);
}

/* n clips of one context into its scope; false when the engines refuse (the caller undoes the enrolment) */
static bool set_scopes(const char* context, const char* const* uuids, int32_t n)
{
	int32_t i, id, *sc;
	bool ret;

	if(n <= 0) {
		return true;
	}
	id = scope_of_context(context, true);
	sc = ast_malloc(sizeof(int32_t) * n);
	if(id < 0 || sc == NULL) {
		ast_free(sc);
		return false;
	}
	for(i = 0; i < n; i++) {
		sc[i] = id;
	}
	ret = tfp_group_index_set_scope(g_tfp, n, uuids, sc) == TFP_OK;
	if(ret == false) {
		ast_log(LOG_ERROR, "Could not set the context of %d clips: %s\n", n, tfp_group_last_error(g_tfp));
	}
	ast_free(sc);
	return ret;
}

/* fp_init: the loaded clips' scopes from audio_list's context column (clips without a catalog row
 * stay in scope 0: no context finds them, as no fp_search result can name them) */
static bool load_scopes(const fpc_rows* rows)
{
	int32_t c, n = 0, *sc;
	const char** uu;
	bool ret = true;

	if(rows->nclips <= 0) {
		return true;
	}
	sc = ast_malloc(sizeof(int32_t) * rows->nclips);
	uu = ast_malloc(sizeof(char*) * rows->nclips);
	if(sc == NULL || uu == NULL) {
		ast_free(sc);
		ast_free(uu);
		return false;
	}
	for(c = 0; c < rows->nclips && ret == true; c++) {
		struct ast_json* j = fpc_get_audio_list_info(rows->uuids[c]);
		const char* ctx = j ? ast_json_string_get(ast_json_object_get(j, "context")) : NULL;
		if(ctx != NULL) {
			sc[n] = scope_of_context(ctx, true);
			uu[n] = rows->uuids[c];
			ret = sc[n++] >= 0;
		}
		if(j != NULL) {
			ast_json_unref(j);
		}
	}
	ret = ret && (n == 0 || tfp_group_index_set_scope(g_tfp, n, uu, sc) == TFP_OK);
	ast_free(sc);
	ast_free(uu);
	return ret;
}

/* Every shard serves each tfp_group_index_neighbours call once, so shard 0's batches are the calls. */
bool fp_get_neighbour_stats(int64_t* calls)
{
	int64_t vote = 0, general = 0;

	if(g_tfp == NULL || calls == NULL ||
			tfp_neighbour_stats(tfp_group_engine(g_tfp, 0), &vote, &general, NULL, NULL) != TFP_OK) {
		return false;
	}
	*calls = vote + general;
	return true;
}

bool fp_get_search_stats(int64_t* calls, int64_t* batches)
{
	return g_tfp != NULL && tfp_group_search_coalesce_stats(g_tfp, calls, batches) == TFP_OK;
}

/* fp_init (fp_handler.c:68-90): the catalog (init_database + the backup's tables), the engine, and
 * the GPU index from the restored audio_fingerprint table in one tfp_group_index_add_batch. A failure
 * closes whatever was opened, without writing the backup. */
bool fp_init(void)
{
	fpc_rows rows;

	scopes_reset();
	if(fpc_db_init() == false) {
		ast_log(LOG_ERROR, "Could not initiate database.\n");
		return false;
	}
	if(create_group() == false) {
		ast_log(LOG_ERROR, "Could not create the MI355X fingerprint engines. devices[%s]\n", g_devices);
		g_tfp = NULL;
		fpc_db_close();
		return false;
	}
	if(fpc_load_fingerprints(&rows) == false) {
		ast_log(LOG_ERROR, "Could not load the database data.\n");
		tfp_group_destroy(g_tfp);
		g_tfp = NULL;
		fpc_db_close();
		return false;
	}
	if((rows.nclips > 0 && tfp_group_index_add_batch(g_tfp, rows.nclips, (const char* const*)rows.uuids,
			rows.frame_offsets, rows.m1, rows.m2) != TFP_OK) || load_scopes(&rows) == false ||
			tfp_group_index_commit(g_tfp) != TFP_OK) {
		ast_log(LOG_ERROR, "Could not load the fingerprint index: %s\n", tfp_group_last_error(g_tfp));
		fpc_rows_free(&rows);
		tfp_group_destroy(g_tfp);
		g_tfp = NULL;
		fpc_db_close();
		return false;
	}
	fpc_rows_free(&rows);
	return true;
}

/* fp_term (fp_handler.c:92-108): the backup (the rows were written to audio_fingerprint at
 * enrolment), then the engine */
bool fp_term(void)
{
	bool ret = fpc_db_term();
	pcm_pool_drain();
	tfp_group_destroy(g_tfp);
	g_tfp = NULL;
	scopes_reset();
	if(ret == false) {
		ast_log(LOG_ERROR, "Could not write database.\n");
	}
	return ret;
}

/* int16 sample buffers in engine-mapped host memory (tfp_host_alloc), which the engine reads in
 * place instead of copying into its staging. Pooled: pinning memory costs more than the copy it
 * saves. The channel threads search concurrently, so the pool is locked. */
#define PCM_POOL 32
static struct {
	int16_t* p;
	int64_t cap;
} g_pool[PCM_POOL];
static int g_npool = 0;
static pthread_mutex_t g_pool_lock = PTHREAD_MUTEX_INITIALIZER;

static int16_t* pcm_get(int64_t n, int64_t* cap)
{
	int i, best = -1;
	void* p = NULL;

	pthread_mutex_lock(&g_pool_lock);
	for(i = 0; i < g_npool; i++) {
		if(g_pool[i].cap >= n && (best < 0 || g_pool[i].cap < g_pool[best].cap)) {
			best = i;
		}
	}
	if(best >= 0) {
		int16_t* q = g_pool[best].p;
		*cap = g_pool[best].cap;
		g_pool[best] = g_pool[--g_npool];
		pthread_mutex_unlock(&g_pool_lock);
		return q;
	}
	pthread_mutex_unlock(&g_pool_lock);
	*cap = n < 80000 ? 80000 : n; /* at least 10 s at 8 kHz */
	if(tfp_host_alloc(sizeof(int16_t) * (size_t)*cap, &p) != TFP_OK) {
		*cap = 0;
		return NULL;
	}
	return (int16_t*)p;
}

static void pcm_put(int16_t* p, int64_t cap)
{
	if(p == NULL) {
		return;
	}
	pthread_mutex_lock(&g_pool_lock);
	if(g_npool < PCM_POOL) {
		g_pool[g_npool].p = p;
		g_pool[g_npool].cap = cap;
		g_npool++;
		p = NULL;
	}
	pthread_mutex_unlock(&g_pool_lock);
	tfp_host_free(p); /* pool full (NULL: kept) */
}

static void pcm_pool_drain(void)
{
	pthread_mutex_lock(&g_pool_lock);
	while(g_npool > 0) {
		g_npool--;
		tfp_host_free(g_pool[g_npool].p);
	}
	pthread_mutex_unlock(&g_pool_lock);
}

/* New behaviour (aubio cannot open these, so the reference skips them): a headerless Asterisk
 * sound file is told by its extension, G.711 codes, mono at 8 kHz: .ulaw / .ul / .mu are mu-law,
 * .alaw / .al are A-law. The law, or -1 for every other name. */
static int raw_g711_law(const char* filename)
{
	static const struct { const char* ext; int law; } known[] = {
		{"ulaw", TFP_G711_ULAW}, {"ul", TFP_G711_ULAW}, {"mu", TFP_G711_ULAW}, {"alaw", TFP_G711_ALAW}, {"al", TFP_G711_ALAW}};
	const char* dot = filename ? strrchr(filename, '.') : NULL;
	size_t k, i;

	if(dot == NULL || strchr(dot, '/') != NULL) {
		return -1;
	}
	for(k = 0; k < sizeof(known) / sizeof(known[0]); k++) {
		for(i = 0; known[k].ext[i] != '\0' && tolower((unsigned char)dot[1 + i]) == known[k].ext[i]; i++) {
		}
		if(known[k].ext[i] == '\0' && dot[1 + i] == '\0') {
			return known[k].law;
		}
	}
	return -1;
}

/* The G.711 codes of a file as stored, with tfp_wav_read_g711's conventions (codes == NULL: the
 * size query): a headerless file by its extension (raw_g711_law), else a mu-law / A-law WAV. */
static int read_g711(const char* filename, uint8_t* codes, int64_t cap, int64_t* ns, int32_t* sr, int32_t* law)
{
	const int raw = raw_g711_law(filename);
	FILE* fp;
	long size;
	size_t got;

	if(raw < 0) {
		return tfp_wav_read_g711(filename, codes, cap, ns, sr, law);
	}
	fp = fopen(filename, "rb");
	if(fp == NULL) {
		return TFP_E_NOENT;
	}
	if(fseek(fp, 0, SEEK_END) != 0 || (size = ftell(fp)) < 0) {
		fclose(fp);
		return TFP_E_NOENT;
	}
	*ns = size;
	*sr = 8000;
	*law = raw;
	if(codes == NULL || cap < size) {
		fclose(fp);
		return codes == NULL ? TFP_OK : TFP_E_CAPACITY;
	}
	rewind(fp);
	got = fread(codes, 1, (size_t)size, fp);
	fclose(fp);
	return got == (size_t)size ? TFP_OK : TFP_E_NOENT;
}

/* With an index rate: a file as a clip of a mixed batch (include/tiresias_fp.h, "mixed batches"), by the
 * reader of its kind, in read_audio's order: 8/16-bit integer PCM of 1 to 32 channels as interleaved int16
 * (tfp_wav_read_interleaved), G.711 codes as they are (read_g711), 24/32-bit integer and float as
 * interleaved int32 Q31 (tfp_wav_read_interleaved_q31). dst == NULL: the size query, which fills *clip
 * (offset 0) and *nbytes; else the samples into dst[*nbytes]. A file no reader takes is the last reader's
 * error, its reason in tfp_engine_last_error(NULL). */
static int read_any(const char* filename, void* dst, tfp_audio_clip* clip, int64_t* nbytes)
{
	const bool raw = raw_g711_law(filename) >= 0;
	int64_t ns = 0;
	int32_t sr = 0, law = -1, ch = 1;
	int rc;

	if(dst != NULL) {
		const int64_t cap = clip->nframes * clip->channels;
		if(clip->kind == TFP_AUDIO_S16) {
			rc = tfp_wav_read_interleaved(filename, dst, cap, &ns, &ch, &sr);
		}
		else if(clip->kind == TFP_AUDIO_Q31) {
			rc = tfp_wav_read_interleaved_q31(filename, dst, cap, &ns, &ch, &sr);
		}
		else {
			rc = read_g711(filename, dst, cap, &ns, &sr, &law);
		}
		return (rc == TFP_OK && (ns != clip->nframes || sr != clip->rate_in || ch != clip->channels)) ? TFP_E_FORMAT : rc;
	}
	memset(clip, 0, sizeof(*clip));
	if(!raw && (rc = tfp_wav_read_interleaved(filename, NULL, 0, &ns, &ch, &sr)) == TFP_OK) {
		clip->kind = TFP_AUDIO_S16;
		*nbytes = ns * ch * 2;
	}
	else if((rc = read_g711(filename, NULL, 0, &ns, &sr, &law)) == TFP_OK) {
		clip->kind = law == TFP_G711_ALAW ? TFP_AUDIO_ALAW : TFP_AUDIO_ULAW;
		ch = 1;
		*nbytes = ns;
	}
	else if(!raw && (rc = tfp_wav_read_interleaved_q31(filename, NULL, 0, &ns, &ch, &sr)) == TFP_OK) {
		clip->kind = TFP_AUDIO_Q31;
		*nbytes = ns * ch * 4;
	}
	else {
		return rc;
	}
	clip->nframes = ns;
	clip->rate_in = sr;
	clip->channels = ch;
	return TFP_OK;
}

/* With an index rate: whether a file is of another rate (*other) and, if so, whether the mixed call takes
 * it: the engine's own argument rules on its clip (tfp_audio_clips_check: an unsupported ratio, a Q31 pair
 * out of range), with *nout its length at the index rate. Run before a catalog row is written, so a file
 * that is refused leaves none. false: unreadable or refused, logged with the engine's message. */
static bool probe_any(const char* filename, bool* other, tfp_audio_clip* clip, int64_t* nbytes, int64_t* nout)
{
	*other = false;
	if(g_index_rate <= 0) {
		return true;
	}
	if(read_any(filename, NULL, clip, nbytes) != TFP_OK) {
		return true; /* (no mixed reader takes it: the native-rate readers decide, as without the setting) */
	}
	if(clip->rate_in == g_index_rate) {
		return true;
	}
	*other = true;
	if(tfp_audio_clips_check(clip, 1, *nbytes, g_index_rate, nout) != TFP_OK) {
		ast_log(LOG_WARNING, "Could not take %s at the index rate %d: %s\n", filename, (int)g_index_rate, tfp_engine_last_error(NULL));
		return false;
	}
	return true;
}

/* aubio_source (fp_handler.c:37,604,633): a file's mono hop values at its own rate — int16 PCM for
 * 8/16-bit mono (every Asterisk recording; in a pooled pcm_get buffer of *cap samples), then the
 * int16 expansion of G.711 codes (a mu-law / A-law WAV, or a headerless file; tfp_g711_decode on
 * the host: file searches are not hot), else (TFP_E_FORMAT) the fp32 values (multichannel mean,
 * 24/32-bit, float). Exactly one of *pcm / *x is set; release with pcm_put(*pcm, *cap) and
 * ast_free(*x). With an index rate (fp_set_index_rate) a file of another rate comes back as the int16 PCM
 * of the mixed call's host map (tfp_resample_any_pcm: what the enrolment's GPU launch computes, bit for
 * bit) with *sr the index rate; the conversion runs on the host, since file searches and single-file
 * enrolments are not hot. */
static int read_audio(const char* filename, int16_t** pcm, int64_t* cap, float** x, int64_t* ns, int32_t* sr)
{
	const bool raw = raw_g711_law(filename) >= 0;
	int32_t law = -1;
	int rc;
	bool other = false;
	tfp_audio_clip clip;
	int64_t nbytes = 0, nout = 0;

	*pcm = NULL;
	*cap = 0;
	*x = NULL;
	if(probe_any(filename, &other, &clip, &nbytes, &nout) == false) {
		return -1;
	}
	if(other) {
		void* bytes = ast_malloc(nbytes ? (size_t)nbytes : 1);
		*pcm = pcm_get(nout ? nout : 1, cap);
		rc = (bytes && *pcm) ? read_any(filename, bytes, &clip, &nbytes) : TFP_E_NOMEM;
		if(rc == TFP_OK) {
			rc = tfp_resample_any_pcm(bytes, &clip, g_index_rate, *pcm, *cap, ns);
		}
		ast_free(bytes);
		if(rc != TFP_OK) {
			ast_log(LOG_WARNING, "Could not read %s: %s\n", filename, tfp_engine_last_error(NULL));
			pcm_put(*pcm, *cap);
			*pcm = NULL;
			return -1;
		}
		*sr = g_index_rate;
		return 0;
	}
	rc = raw ? TFP_E_FORMAT : tfp_wav_read(filename, NULL, 0, ns, sr);
	if(rc == TFP_OK) {
		*pcm = pcm_get(*ns ? *ns : 1, cap);
		rc = *pcm ? tfp_wav_read(filename, *pcm, *cap, ns, sr) : TFP_E_NOMEM;
	}
	else if(rc == TFP_E_FORMAT && (rc = read_g711(filename, NULL, 0, ns, sr, &law)) == TFP_OK) {
		uint8_t* codes = ast_malloc(*ns ? (size_t)*ns : 1);
		*pcm = pcm_get(*ns ? *ns : 1, cap);
		rc = (codes && *pcm) ? read_g711(filename, codes, *ns, ns, sr, &law) : TFP_E_NOMEM;
		if(rc == TFP_OK) {
			rc = tfp_g711_decode(codes, *ns, law, *pcm);
		}
		ast_free(codes);
	}
	else if(!raw && rc == TFP_E_FORMAT && (rc = tfp_wav_read_f32(filename, NULL, 0, ns, sr)) == TFP_OK) {
		*x = ast_malloc(sizeof(float) * (*ns ? *ns : 1));
		rc = *x ? tfp_wav_read_f32(filename, *x, *ns, ns, sr) : TFP_E_NOMEM;
	}
	if(rc != TFP_OK) {
		ast_log(LOG_WARNING, "Could not read %s: %s\n", filename, tfp_engine_last_error(NULL));
		pcm_put(*pcm, *cap);
		ast_free(*x);
		*pcm = NULL;
		*x = NULL;
		return -1;
	}
	return 0;
}

/* create_audio_fingerprint_info (fp_handler.c:538-575): the file's frames on the GPU, into the
 * index and into audio_fingerprint. */
static bool create_audio_fingerprint_info(const char* context, const char* filename, const char* uuid)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, n, i, off[2];
	int32_t sr, *m1, *m2;
	tfp_frame* rows;
	int rc;
	bool ret;

	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return false;
	}
	n = tfp_frame_count(ns);
	rows = ast_calloc(n ? n : 1, sizeof(tfp_frame));
	m1 = ast_malloc(sizeof(int32_t) * (n ? n : 1));
	m2 = ast_malloc(sizeof(int32_t) * (n ? n : 1));
	if(rows == NULL || m1 == NULL || m2 == NULL) {
		pcm_put(pcm, cap); ast_free(x); ast_free(rows); ast_free(m1); ast_free(m2);
		return false;
	}
	off[0] = 0;
	off[1] = ns;
	rc = pcm ? tfp_group_fingerprint_batch(g_tfp, pcm, off, 1, sr, rows, n, &n)
	         : tfp_group_fingerprint_f32_batch(g_tfp, x, off, 1, sr, rows, n, &n);
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not fingerprint %s: %s\n", filename, tfp_group_last_error(g_tfp));
		ast_free(rows); ast_free(m1); ast_free(m2);
		return false;
	}
	for(i = 0; i < n; i++) {
		m1[i] = rows[i].m1;
		m2[i] = rows[i].m2;
	}
	ret = fpc_store_fingerprints(context, uuid, m1, m2, n);
	if(ret == true && tfp_group_index_add(g_tfp, uuid, m1, m2, (int32_t)n) != TFP_OK) {
		ast_log(LOG_ERROR, "Could not index %s: %s\n", filename, tfp_group_last_error(g_tfp));
		ret = false;
	}
	else if(ret == true && set_scopes(context, &uuid, 1) == false) {
		tfp_group_index_remove(g_tfp, uuid); /* undone as a failed index add: the caller drops the catalog rows */
		ret = false;
	}
	ast_free(rows);
	ast_free(m1);
	ast_free(m2);
	return ret;
}

bool fp_delete_audio_list_info(const char* uuid)
{
	if(uuid == NULL) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return false;
	}
	if(fpc_delete_audio_list_info(uuid) == false) {
		return false;
	}
	if(tfp_group_index_remove(g_tfp, uuid) != TFP_OK) {
		ast_log(LOG_NOTICE, "Audio %s was not in the GPU index.\n", uuid);
	}
	return true;
}

bool fp_craete_audio_list_info(const char* context, const char* filename)
{
	int ret;
	char* uuid;

	if((context == NULL) || (filename == NULL)) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return false;
	}
	if(g_index_rate > 0) { /* a file the index rate refuses leaves no catalog row */
		bool other;
		tfp_audio_clip clip;
		int64_t nbytes = 0, nout = 0;
		if(probe_any(filename, &other, &clip, &nbytes, &nout) == false) {
			return false;
		}
	}
	uuid = fp_generate_uuid();
	if(uuid == NULL) {
		return false;
	}
	ret = fpc_create_audio_list_info(context, filename, uuid);
	if(ret < 0) {
		ast_log(LOG_WARNING, "Could not create audio_list info. context[%s], filename[%s]\n", context, filename);
		ast_free(uuid);
		return false;
	}
	else if(ret == 0) {
		ast_log(LOG_VERBOSE, "The given audio file is already exist in the list. context[%s], filename[%s]\n",
				context, filename);
		ast_free(uuid);
		return true;
	}
	if(create_audio_fingerprint_info(context, filename, uuid) == false) {
		ast_log(LOG_NOTICE, "Could not create audio fingerprint info.\n");
		/* (the reference passes the filename here, fp_handler.c:192, so its clean-up never
		 * matches; the shim removes the row it created) */
		fpc_delete_audio_list_info(uuid);
		ast_free(uuid);
		return false;
	}
	ast_free(uuid);
	return true;
}

/* ---- batched enrolment: app_tiresias.c:365-424's directory scan onto the GPU ----------------
 * The reference calls fp_craete_audio_list_info once per file of a context's directory (scandir,
 * alphasort). fp_create_audio_list_infos takes the whole list: the catalog rows are written in
 * the same order with the same per-context MD5 dedup (a file repeated within the list counts as
 * already enrolled), and the audio of all new files is fingerprinted by one tfp_group_fingerprint_batch
 * (per sample rate and sample kind, and per ENROL_BATCH_SAMPLES) and indexed by one
 * tfp_group_index_add_batch, instead of a GPU round trip per file. The kinds: int16 PCM, fp32 hop
 * values, and G.711 codes of one law (a directory of .ulaw prompts is one
 * tfp_group_fingerprint_g711_batch per flush: the codes go to the GPU as they are). */
/* With an index rate (fp_set_index_rate) every file of another rate goes into one more bucket, ENROL_ANY,
 * whatever its rate, channel count and kind: its samples as read_any hands them out, a tfp_audio_clip per
 * file, and off[] the clips' running lengths at the index rate, so the batch bound and the frame counts
 * below are in output samples. It is flushed by one tfp_group_fingerprint_any_batch (one conversion launch
 * per shard). Files at the index rate keep the buckets above, fp32 for multichannel included. */
enum { ENROL_I16 = 0, ENROL_F32 = 1, ENROL_G711 = 2, ENROL_ANY = 3 };
#define ENROL_GROUPS 6
#define ENROL_BATCH_SAMPLES ((int64_t)1 << 27) /* 256 MB of int16 per batch */

typedef struct {
	int32_t sr;
	int kind;          /* ENROL_* */
	int32_t law;       /* ENROL_G711: TFP_G711_ULAW / TFP_G711_ALAW */
	int n, cap;
	int* file;         /* index into the caller's list */
	char** uuid;
	int64_t* off;      /* [n + 1] sample offsets */
	int64_t scap;      /* samples allocated */
	void* x;           /* int16 PCM, fp32 hop values or uint8 G.711 codes; ENROL_ANY: the mixed call's bytes */
	tfp_audio_clip* clips; /* ENROL_ANY: [n], offsets into x */
	int64_t nbytes;        /* ENROL_ANY: bytes of x in use (scap counts bytes) */
} enrol_group;

static void group_reset(enrol_group* g)
{
	int i;
	for(i = 0; i < g->n; i++) {
		ast_free(g->uuid[i]);
	}
	g->n = 0;
	g->nbytes = 0;
	if(g->off) {
		g->off[0] = 0;
	}
}

static void group_free(enrol_group* g)
{
	group_reset(g);
	ast_free(g->file);
	ast_free(g->uuid);
	ast_free(g->off);
	ast_free(g->x);
	ast_free(g->clips);
	memset(g, 0, sizeof(*g));
}

/* fingerprint, store and index one group; returns the clips enrolled */
static int group_flush(const char* context, enrol_group* g, bool* ok)
{
	int64_t nf = 0, got = 0, i;
	int c, kept = 0, done = 0;
	tfp_frame* rows = NULL;
	int32_t *m1 = NULL, *m2 = NULL;
	int64_t* foff = NULL;
	const char** uu = NULL;
	int rc;

	if(g->n == 0) {
		return 0;
	}
	for(c = 0; c < g->n; c++) {
		nf += tfp_frame_count(g->off[c + 1] - g->off[c]);
	}
	rows = ast_calloc(nf ? nf : 1, sizeof(tfp_frame));
	m1 = ast_malloc(sizeof(int32_t) * (nf ? nf : 1));
	m2 = ast_malloc(sizeof(int32_t) * (nf ? nf : 1));
	foff = ast_malloc(sizeof(int64_t) * (g->n + 1));
	uu = ast_malloc(sizeof(char*) * g->n);
	rc = TFP_E_NOMEM;
	if(rows && m1 && m2 && foff && uu) {
		rc = g->kind == ENROL_F32 ? tfp_group_fingerprint_f32_batch(g_tfp, (const float*)g->x, g->off, g->n, g->sr, rows, nf, &got)
		   : g->kind == ENROL_G711 ? tfp_group_fingerprint_g711_batch(g_tfp, (const uint8_t*)g->x, g->off, g->n, g->law, g->sr, rows, nf, &got)
		   : g->kind == ENROL_ANY ? tfp_group_fingerprint_any_batch(g_tfp, g->x, g->nbytes, g->clips, g->n, g->sr, rows, nf, &got)
		   : tfp_group_fingerprint_batch(g_tfp, (const int16_t*)g->x, g->off, g->n, g->sr, rows, nf, &got);
	}
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not fingerprint %d files: %s\n", g->n, tfp_group_last_error(g_tfp));
	}
	else {
		/* the audio_fingerprint rows of each clip; a clip whose rows could not be stored is dropped */
		int64_t src = 0;
		foff[0] = 0;
		for(c = 0; c < g->n; c++) {
			const int64_t n = tfp_frame_count(g->off[c + 1] - g->off[c]);
			int32_t* a = m1 + foff[kept];
			int32_t* b = m2 + foff[kept];
			for(i = 0; i < n; i++) {
				a[i] = rows[src + i].m1;
				b[i] = rows[src + i].m2;
			}
			src += n;
			if(fpc_store_fingerprints(context, g->uuid[c], a, b, n) == false) {
				ast_log(LOG_NOTICE, "Could not create audio fingerprint info.\n");
				fpc_delete_audio_list_info(g->uuid[c]);
				continue;
			}
			uu[kept] = g->uuid[c];
			foff[kept + 1] = foff[kept] + n;
			g->file[kept] = g->file[c];
			kept++;
		}
		if(tfp_group_index_add_batch(g_tfp, kept, (const char* const*)uu, foff, m1, m2) != TFP_OK) {
			ast_log(LOG_ERROR, "Could not index %d files: %s\n", kept, tfp_group_last_error(g_tfp));
			for(c = 0; c < kept; c++) {
				fpc_delete_audio_list_info(uu[c]);
			}
		}
		else if(set_scopes(context, (const char* const*)uu, kept) == false) {
			for(c = 0; c < kept; c++) { /* undone as a failed index add */
				tfp_group_index_remove(g_tfp, uu[c]);
				fpc_delete_audio_list_info(uu[c]);
			}
		}
		else {
			for(c = 0; c < kept; c++) {
				if(ok) {
					ok[g->file[c]] = true;
				}
			}
			done = kept;
		}
	}
	if(rc != TFP_OK) {
		for(c = 0; c < g->n; c++) {
			fpc_delete_audio_list_info(g->uuid[c]);
		}
	}
	ast_free(rows);
	ast_free(m1);
	ast_free(m2);
	ast_free(foff);
	ast_free(uu);
	group_reset(g);
	return done;
}

/* appends file f's audio (ns samples at rate sr) to g; false on allocation or read errors */
static bool group_add(enrol_group* g, int f, const char* filename, char* uuid, int64_t ns)
{
	const size_t ss = g->kind == ENROL_F32 ? sizeof(float) : g->kind == ENROL_G711 ? sizeof(uint8_t) : sizeof(int16_t);
	const int64_t at = g->off[g->n];
	int64_t got = 0;
	int32_t sr = 0, law = g->law;
	int rc;
	if(g->n + 1 >= g->cap) {
		int nc = g->cap ? 2 * g->cap : 64;
		int* nf = ast_realloc(g->file, sizeof(int) * (size_t)nc);
		char** nu = nf ? ast_realloc(g->uuid, sizeof(char*) * (size_t)nc) : NULL;
		int64_t* no = nu ? ast_realloc(g->off, sizeof(int64_t) * ((size_t)nc + 1)) : NULL;
		if(nf) g->file = nf;
		if(nu) g->uuid = nu;
		if(no) g->off = no;
		if(no == NULL) {
			return false;
		}
		g->cap = nc;
	}
	if(at + ns + 1 > g->scap) {
		int64_t nc = g->scap ? g->scap : (int64_t)1 << 20;
		void* nx;
		while(nc < at + ns + 1) {
			nc *= 2;
		}
		nx = ast_realloc(g->x, ss * (size_t)nc);
		if(nx == NULL) {
			return false;
		}
		g->x = nx;
		g->scap = nc;
	}
	rc = g->kind == ENROL_F32 ? tfp_wav_read_f32(filename, (float*)g->x + at, ns, &got, &sr)
	   : g->kind == ENROL_G711 ? read_g711(filename, (uint8_t*)g->x + at, ns, &got, &sr, &law)
	   : tfp_wav_read(filename, (int16_t*)g->x + at, ns, &got, &sr);
	if(rc != TFP_OK || got != ns || sr != g->sr || law != g->law) {
		return false;
	}
	g->file[g->n] = f;
	g->uuid[g->n] = uuid;
	g->off[g->n + 1] = at + ns;
	g->n++;
	return true;
}

/* appends file f (clip, of nbytes bytes and nout samples at the index rate) to the mixed bucket g */
static bool group_add_any(enrol_group* g, int f, const char* filename, char* uuid, tfp_audio_clip clip, int64_t nbytes, int64_t nout)
{
	const int64_t at = (g->nbytes + 3) & ~(int64_t)3; /* every clip 4-byte aligned: a multiple of each sample size */
	if(g->n + 1 >= g->cap) {
		int nc = g->cap ? 2 * g->cap : 64;
		int* nf = ast_realloc(g->file, sizeof(int) * (size_t)nc);
		char** nu = nf ? ast_realloc(g->uuid, sizeof(char*) * (size_t)nc) : NULL;
		int64_t* no = nu ? ast_realloc(g->off, sizeof(int64_t) * ((size_t)nc + 1)) : NULL;
		tfp_audio_clip* ncl = no ? ast_realloc(g->clips, sizeof(tfp_audio_clip) * (size_t)nc) : NULL;
		if(nf) g->file = nf;
		if(nu) g->uuid = nu;
		if(no) g->off = no;
		if(ncl) g->clips = ncl;
		if(ncl == NULL) {
			return false;
		}
		g->cap = nc;
	}
	if(at + nbytes + 1 > g->scap) {
		int64_t nc = g->scap ? g->scap : (int64_t)1 << 20;
		void* nx;
		while(nc < at + nbytes + 1) {
			nc *= 2;
		}
		nx = ast_realloc(g->x, (size_t)nc);
		if(nx == NULL) {
			return false;
		}
		g->x = nx;
		g->scap = nc;
	}
	memset((char*)g->x + g->nbytes, 0, (size_t)(at - g->nbytes));
	if(read_any(filename, (char*)g->x + at, &clip, &nbytes) != TFP_OK) {
		return false;
	}
	clip.offset = at;
	g->clips[g->n] = clip;
	g->file[g->n] = f;
	g->uuid[g->n] = uuid;
	g->off[g->n + 1] = g->off[g->n] + nout;
	g->nbytes = at + nbytes;
	g->n++;
	return true;
}

int fp_create_audio_list_infos(const char* context, const char* const* filenames, int count, bool* ok)
{
	enrol_group groups[ENROL_GROUPS];
	int i, k, enrolled = 0;
	/* a file repeated within the list: its first copy's uuid (created in this call) and index;
	 * the repeat reports the first copy's final result, known only after the flushes */
	char** made = NULL;
	int* dup_of = NULL;
	bool* res = NULL;

	if((context == NULL) || (filenames == NULL) || (count < 0)) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return -1;
	}
	made = ast_calloc(count ? count : 1, sizeof(char*));
	dup_of = ast_calloc(count ? count : 1, sizeof(int));
	res = ast_calloc(count ? count : 1, sizeof(bool));
	if(made == NULL || dup_of == NULL || res == NULL) {
		ast_free(made);
		ast_free(dup_of);
		ast_free(res);
		return -1;
	}
	for(i = 0; i < count; i++) {
		dup_of[i] = -1;
	}
	memset(groups, 0, sizeof(groups));
	for(i = 0; i < count; i++) {
		const char* f = filenames[i];
		char* uuid;
		int ret;
		int64_t ns = 0;
		int32_t sr = 0, law = -1;
		int kind = ENROL_I16;
		enrol_group* g = NULL;

		char existing[64] = "";
		bool other = false;
		tfp_audio_clip clip;
		int64_t nbytes = 0, nout = 0;

		if(f == NULL) {
			continue;
		}
		if(probe_any(f, &other, &clip, &nbytes, &nout) == false) {
			continue; /* refused at the index rate, before any catalog row */
		}
		uuid = fp_generate_uuid();
		if(uuid == NULL) {
			continue;
		}
		ret = fpc_create_audio_list_info_ex(context, f, uuid, existing, sizeof(existing));
		if(ret < 0) {
			ast_log(LOG_WARNING, "Could not create audio_list info. context[%s], filename[%s]\n", context, f);
			ast_free(uuid);
			continue;
		}
		if(ret == 0) {
			ast_log(LOG_VERBOSE, "The given audio file is already exist in the list. context[%s], filename[%s]\n",
					context, f);
			ast_free(uuid);
			res[i] = true;
			for(k = 0; k < i; k++) {
				if(made[k] != NULL && strcmp(made[k], existing) == 0) {
					dup_of[i] = k;
					break;
				}
			}
			continue;
		}
		made[i] = ast_malloc(strlen(uuid) + 1);
		if(made[i] != NULL) {
			memcpy(made[i], uuid, strlen(uuid) + 1);
		}
		if(other) { /* of another rate than the index's: the one mixed bucket */
			kind = ENROL_ANY;
			sr = g_index_rate;
			ns = nout;
		}
		/* aubio_source at the native rate: int16 PCM, then G.711 codes, else the fp32 hop values
		 * (read_audio's order; a headerless G.711 file is nothing else) */
		else if(raw_g711_law(f) >= 0 || tfp_wav_read(f, NULL, 0, &ns, &sr) != TFP_OK) {
			if(read_g711(f, NULL, 0, &ns, &sr, &law) == TFP_OK) {
				kind = ENROL_G711;
			}
			else if(raw_g711_law(f) < 0 && tfp_wav_read_f32(f, NULL, 0, &ns, &sr) == TFP_OK) {
				kind = ENROL_F32;
				law = -1;
			}
			else {
				ast_log(LOG_WARNING, "Could not read %s: %s\n", f, tfp_engine_last_error(NULL));
				ast_log(LOG_NOTICE, "Could not create audio fingerprint info.\n");
				fpc_delete_audio_list_info(uuid);
				ast_free(uuid);
				continue;
			}
		}
		for(k = 0; k < ENROL_GROUPS; k++) {
			if(groups[k].off != NULL && groups[k].sr == sr && groups[k].kind == kind && groups[k].law == law) {
				g = &groups[k];
				break;
			}
		}
		if(g == NULL) {
			for(k = 0; k < ENROL_GROUPS && groups[k].off != NULL; k++) {
			}
			if(k == ENROL_GROUPS) { /* many formats in one scan: flush them all */
				for(k = 0; k < ENROL_GROUPS; k++) {
					enrolled += group_flush(context, &groups[k], res);
					group_free(&groups[k]);
				}
				k = 0;
			}
			g = &groups[k];
			g->sr = sr;
			g->kind = kind;
			g->law = law;
			g->off = ast_calloc(1, sizeof(int64_t));
			if(g->off == NULL) {
				fpc_delete_audio_list_info(uuid);
				ast_free(uuid);
				continue;
			}
		}
		if(g->n > 0 && g->off[g->n] + ns > ENROL_BATCH_SAMPLES) {
			enrolled += group_flush(context, g, res);
		}
		if((other ? group_add_any(g, i, f, uuid, clip, nbytes, nout) : group_add(g, i, f, uuid, ns)) == false) {
			ast_log(LOG_WARNING, "Could not read %s: %s\n", f, tfp_engine_last_error(NULL));
			fpc_delete_audio_list_info(uuid);
			ast_free(uuid);
		}
	}
	for(k = 0; k < ENROL_GROUPS; k++) {
		enrolled += group_flush(context, &groups[k], res);
		group_free(&groups[k]);
	}
	for(i = 0; i < count; i++) {
		if(dup_of[i] >= 0) {
			res[i] = res[dup_of[i]];
		}
		if(ok) {
			ok[i] = res[i];
		}
		ast_free(made[i]);
	}
	ast_free(made);
	ast_free(dup_of);
	ast_free(res);
	return enrolled;
}

/* fp_handler.c:386-407: the winner's audio_list row + frame_count + match_count; NULL for NOTFOUND */
static struct ast_json* search_result(const tfp_result* r)
{
	struct ast_json* j_res;

	if(r->found == 0) {
		return NULL; /* no row in the temp table: NOTFOUND (fp_handler.c:367-382) */
	}
	j_res = fpc_get_audio_list_info(r->uuid); /* fp_handler.c:394-401 */
	if(j_res == NULL) {
		ast_log(LOG_ERROR, "Could not get audio list info. uuid[%s]\n", r->uuid);
		return NULL;
	}
	ast_json_object_set(j_res, "frame_count", ast_json_integer_create(r->frame_count));
	ast_json_object_set(j_res, "match_count", ast_json_integer_create(r->match_count));
	return j_res;
}

static bool search_params(tfp_search_params* p, const char* context, const int coefs, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high)
{
	if(context == NULL) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return false;
	}
	if((coefs < 1) || (coefs > 2)) { /* fp_handler.c:247-250 */
		ast_log(LOG_WARNING, "Wrong coefs count. coefs[%d]\n", coefs);
		return false;
	}
	memset(p, 0, sizeof(*p));
	p->coefs = coefs;
	p->tolerance = tolerance; /* < 0: the default 0.001 (fp_handler.c:252-256) */
	p->freq_ignore_low = freq_ignore_low;
	p->freq_ignore_high = freq_ignore_high;
	return true;
}

struct ast_json* fp_search_fingerprint_info(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, off[2];
	int32_t sr;
	int rc;
	tfp_search_params p;
	tfp_result r;

	if(filename == NULL) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return NULL;
	}
	off[0] = 0;
	off[1] = ns;
	/* concurrent channel threads' calls run as shared GPU batches (tfp_group's coalescer) */
	rc = pcm ? tfp_group_search_pcm_batch(g_tfp, pcm, off, 1, sr, &p, &r)
	         : tfp_group_search_f32_batch(g_tfp, x, off, 1, sr, &p, &r);
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not search %s: %s\n", filename, tfp_group_last_error(g_tfp));
		return NULL;
	}
	return search_result(&r);
}

/* New: the first max_results rows of the result query fp_search_fingerprint_info reads one row of
 * ("select *, count(*) from temp group by audio_uuid order by count(*) DESC", fp_handler.c:367-374),
 * as a JSON array of that call's result objects in rank order (tfp_group_search_ranked_pcm_batch).
 * NULL where fp_search_fingerprint_info returns NULL before the query; an empty array for NOTFOUND. */
static struct ast_json* search_candidates(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int max_results,
		const bool in_context)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, off[2], nf = 0;
	int32_t sr, count = 0, scope = TFP_SCOPE_ANY;
	int rc, k, i;
	tfp_search_params p;
	tfp_candidate cand[TFP_RANK_MAX];
	tfp_result r;
	struct ast_json* j_res;
	struct ast_json* j_tmp;

	if((filename == NULL) || (max_results < 1)) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return NULL;
	}
	k = max_results > TFP_RANK_MAX ? TFP_RANK_MAX : max_results;
	off[0] = 0;
	off[1] = ns;
	nf = tfp_frame_count(ns); /* ast_json_array_size(j_fprints), fp_handler.c:286 */
	if(in_context == true) {
		scope = scope_of_context(context, false);
	}
	if(pcm != NULL) {
		rc = in_context ? tfp_group_search_scoped_pcm_batch(g_tfp, pcm, off, 1, sr, &p, &scope, k, cand, &count)
		                : tfp_group_search_ranked_pcm_batch(g_tfp, pcm, off, 1, sr, &p, k, cand, &count);
	}
	else {
		/* audio tfp_wav_decode refuses (fp32 hop values): its frames, then the frames form */
		tfp_frame* fr = ast_calloc(nf > 0 ? nf : 1, sizeof(*fr));
		int64_t qoff[2] = {0, 0};
		rc = fr ? tfp_group_fingerprint_f32_batch(g_tfp, x, off, 1, sr, fr, nf, &qoff[1]) : TFP_E_NOMEM;
		if(rc == TFP_OK) {
			rc = in_context ? tfp_group_search_scoped_batch(g_tfp, fr, qoff, 1, &p, &scope, k, cand, &count)
			                : tfp_group_search_ranked_batch(g_tfp, fr, qoff, 1, &p, k, cand, &count);
		}
		ast_free(fr);
	}
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not search %s: %s\n", filename, tfp_group_last_error(g_tfp));
		return NULL;
	}
	j_res = ast_json_array_create();
	for(i = 0; i < count; i++) {
		memset(&r, 0, sizeof(r));
		r.found = 1;
		r.match_count = cand[i].match_count;
		r.frame_count = (int32_t)nf;
		snprintf(r.uuid, sizeof(r.uuid), "%s", cand[i].uuid);
		j_tmp = search_result(&r); /* a row whose audio_list entry is missing is skipped */
		if(j_tmp != NULL) {
			ast_json_array_append(j_res, j_tmp);
		}
	}
	return j_res;
}

struct ast_json* fp_search_fingerprint_candidates(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int max_results)
{
	return search_candidates(context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high, max_results, false);
}

/* New: fp_search_fingerprint_candidates over the clips enrolled in `context` alone: the search the
 * reference documents ("from the context's audio list", doc/dialplan_application.rst:11, :52-53)
 * and its per-frame SQL (fp_handler.c:308-314, no context predicate) does not run. The rows are the
 * first max_results of fp_handler.c:367-374 with "and context = '<context>'" in that insert
 * (tfp_group_search_scoped_pcm_batch); a context without clips gives the empty array. */
struct ast_json* fp_search_fingerprint_in_context(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int max_results)
{
	return search_candidates(context, filename, coefs, tolerance, freq_ignore_low, freq_ignore_high, max_results, true);
}

/* New: the match census. fp_search_fingerprint_in_context's winner with how it stands against every
 * other clip of `context`: the result query (fp_handler.c:367-374) lists one row per clip with a
 * non-zero count, and the census is those rows counted by count(*) ("select c, count(*) from (select
 * count(*) c from temp group by audio_uuid) group by c", tfp_group_census_pcm_batch), which the
 * application's ratio test (application_handler.c:180-203) cannot see from the first row. A JSON
 * object: "winner" (fp_search_fingerprint_in_context's first object, or null), "frame_count",
 * "population" (the context's clips), "clips_at_or_above" (clips whose count reaches the winner's,
 * the winner included), "clips_tied" (count equal to the winner's) and "histogram" ([[count, clips],
 * ...], non-zero bins only, counts descending, count 0 last). NULL for bad arguments or a failed call. */
struct ast_json* fp_search_fingerprint_census(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, off[2], nf = 0;
	int32_t sr, count = 0, scope, nbins, need = 0, c, top = 0;
	int32_t* hist;
	int rc;
	tfp_search_params p;
	tfp_candidate cand;
	tfp_result r;
	struct ast_json* j_res;
	struct ast_json* j_hist;
	struct ast_json* j_tmp;

	if(filename == NULL) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return NULL;
	}
	off[0] = 0;
	off[1] = ns;
	nf = tfp_frame_count(ns); /* ast_json_array_size(j_fprints), fp_handler.c:286 */
	nbins = (int32_t)nf + 1;
	hist = ast_calloc(nbins, sizeof(*hist));
	scope = scope_of_context(context, false);
	if(hist == NULL) {
		rc = TFP_E_NOMEM;
	}
	else if(pcm != NULL) {
		rc = tfp_group_search_scoped_pcm_batch(g_tfp, pcm, off, 1, sr, &p, &scope, 1, &cand, &count);
		if(rc == TFP_OK) {
			rc = tfp_group_census_pcm_batch(g_tfp, pcm, off, 1, sr, &p, &scope, nbins, hist, &need);
		}
	}
	else {
		/* audio tfp_wav_decode refuses (fp32 hop values): its frames, then the frames forms */
		tfp_frame* fr = ast_calloc(nf > 0 ? nf : 1, sizeof(*fr));
		int64_t qoff[2] = {0, 0};
		rc = fr ? tfp_group_fingerprint_f32_batch(g_tfp, x, off, 1, sr, fr, nf, &qoff[1]) : TFP_E_NOMEM;
		if(rc == TFP_OK) {
			rc = tfp_group_search_scoped_batch(g_tfp, fr, qoff, 1, &p, &scope, 1, &cand, &count);
		}
		if(rc == TFP_OK) {
			rc = tfp_group_census_batch(g_tfp, fr, qoff, 1, &p, &scope, nbins, hist, &need);
		}
		ast_free(fr);
	}
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not take the census of %s: %s\n", filename, tfp_group_last_error(g_tfp));
		ast_free(hist);
		return NULL;
	}
	j_res = ast_json_object_create();
	j_tmp = NULL;
	if(count > 0) {
		memset(&r, 0, sizeof(r));
		r.found = 1;
		r.match_count = top = cand.match_count;
		r.frame_count = (int32_t)nf;
		snprintf(r.uuid, sizeof(r.uuid), "%s", cand.uuid);
		j_tmp = search_result(&r); /* NULL: the row's audio_list entry is missing */
	}
	ast_json_object_set(j_res, "winner", j_tmp ? j_tmp : ast_json_null());
	ast_json_object_set(j_res, "frame_count", ast_json_integer_create(nf));
	ast_json_object_set(j_res, "population", ast_json_integer_create(tfp_census_at_least(hist, nbins, 0)));
	ast_json_object_set(j_res, "clips_at_or_above", ast_json_integer_create(top > 0 ? tfp_census_at_least(hist, nbins, top) : 0));
	ast_json_object_set(j_res, "clips_tied", ast_json_integer_create(top > 0 ? hist[top] : 0));
	j_hist = ast_json_array_create();
	for(c = nbins - 1; c >= 0; c--) {
		if(hist[c] == 0) {
			continue;
		}
		j_tmp = ast_json_array_create();
		ast_json_array_append(j_tmp, ast_json_integer_create(c));
		ast_json_array_append(j_tmp, ast_json_integer_create(hist[c]));
		ast_json_array_append(j_hist, j_tmp);
	}
	ast_json_object_set(j_res, "histogram", j_hist);
	ast_free(hist);
	return j_res;
}

/* New: fp_search_fingerprint_candidates for every window of a long recording. The reference records
 * a fixed duration and searches that one window (application_handler.c:152-185, fp_handler.c:275-374);
 * this returns a JSON array with one object per full window of window_frames frames, hop_frames
 * apart: {"frame": w * hop_frames, "rows": [...]}, rows being the first max_results rows of
 * fp_handler.c:367-374 over that window's frames, each fp_search_fingerprint_candidates' object with
 * frame_count = window_frames. in_context restricts every window to the clips enrolled in `context`,
 * as fp_search_fingerprint_in_context does. The recording is fingerprinted once
 * (tfp_group_search_sliding_pcm_batch). NULL where the candidates call returns NULL; an empty array
 * for a recording shorter than one window. */
struct ast_json* fp_search_fingerprint_timeline(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int window_frames,
		const int hop_frames, const int max_results, const bool in_context)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, off[2], nf = 0, nw = 0, got = 0, w;
	int32_t sr, scope = TFP_SCOPE_ANY;
	int rc, k, i;
	tfp_search_params p;
	tfp_candidate* cand;
	int32_t* counts;
	tfp_result r;
	struct ast_json* j_res;
	struct ast_json* j_win;
	struct ast_json* j_rows;
	struct ast_json* j_tmp;

	if((filename == NULL) || (max_results < 1) || (window_frames < 1) || (hop_frames < 1)) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return NULL;
	}
	k = max_results > TFP_RANK_MAX ? TFP_RANK_MAX : max_results;
	off[0] = 0;
	off[1] = ns;
	nf = tfp_frame_count(ns); /* ast_json_array_size(j_fprints), fp_handler.c:286 */
	nw = tfp_sliding_windows(nf, window_frames, hop_frames);
	if(in_context == true) {
		scope = scope_of_context(context, false);
	}
	cand = ast_calloc((nw > 0 ? nw : 1) * k, sizeof(*cand));
	counts = ast_calloc(nw > 0 ? nw : 1, sizeof(*counts));
	if((cand == NULL) || (counts == NULL)) {
		rc = TFP_E_NOMEM;
	}
	else if(pcm != NULL) {
		rc = tfp_group_search_sliding_pcm_batch(g_tfp, pcm, off, 1, sr, &p, window_frames, hop_frames, &scope, k, cand,
				counts, nw, &got);
	}
	else {
		/* audio tfp_wav_decode refuses (fp32 hop values): its frames, then the frames form */
		tfp_frame* fr = ast_calloc(nf > 0 ? nf : 1, sizeof(*fr));
		int64_t qoff[2] = {0, 0};
		rc = fr ? tfp_group_fingerprint_f32_batch(g_tfp, x, off, 1, sr, fr, nf, &qoff[1]) : TFP_E_NOMEM;
		if(rc == TFP_OK) {
			rc = tfp_group_search_sliding_batch(g_tfp, fr, qoff, 1, &p, window_frames, hop_frames, &scope, k, cand,
					counts, nw, &got);
		}
		ast_free(fr);
	}
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not search %s: %s\n", filename, tfp_group_last_error(g_tfp));
		ast_free(cand);
		ast_free(counts);
		return NULL;
	}
	j_res = ast_json_array_create();
	for(w = 0; w < got; w++) {
		j_rows = ast_json_array_create();
		for(i = 0; i < counts[w]; i++) {
			memset(&r, 0, sizeof(r));
			r.found = 1;
			r.match_count = cand[w * k + i].match_count;
			r.frame_count = window_frames;
			snprintf(r.uuid, sizeof(r.uuid), "%s", cand[w * k + i].uuid);
			j_tmp = search_result(&r); /* a row whose audio_list entry is missing is skipped */
			if(j_tmp != NULL) {
				ast_json_array_append(j_rows, j_tmp);
			}
		}
		j_win = ast_json_object_create();
		ast_json_object_set(j_win, "frame", ast_json_integer_create(w * hop_frames));
		ast_json_object_set(j_win, "rows", j_rows);
		ast_json_array_append(j_res, j_win);
	}
	ast_free(cand);
	ast_free(counts);
	return j_res;
}

/* New: fp_search_fingerprint_candidates' array with where in each clip the recording lies: every
 * element also carries aligned_count, offset, first_frame and last_frame (tfp_alignment: the hits
 * that agree on one time offset, that offset in frames, and the first and last query frame on it).
 * The reference's result query (fp_handler.c:367-374) counts the frames that hit and never reads
 * the rows' frame_idx. The file's frames (tfp_group_fingerprint_batch / _f32_batch), then
 * tfp_group_search_aligned_batch. NULL and the empty array as for the candidates call. */
struct ast_json* fp_search_fingerprint_aligned(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int max_results)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, off[2], qoff[2] = {0, 0}, nf = 0;
	int32_t sr, count = 0;
	int rc, k, i;
	tfp_search_params p;
	tfp_candidate cand[TFP_RANK_MAX];
	tfp_alignment align[TFP_RANK_MAX];
	tfp_result r;
	tfp_frame* fr;
	struct ast_json* j_res;
	struct ast_json* j_tmp;

	if((filename == NULL) || (max_results < 1)) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return NULL;
	}
	k = max_results > TFP_RANK_MAX ? TFP_RANK_MAX : max_results;
	off[0] = 0;
	off[1] = ns;
	nf = tfp_frame_count(ns); /* ast_json_array_size(j_fprints), fp_handler.c:286 */
	fr = ast_calloc(nf > 0 ? nf : 1, sizeof(*fr));
	if(fr == NULL) {
		rc = TFP_E_NOMEM;
	}
	else if(pcm != NULL) {
		rc = tfp_group_fingerprint_batch(g_tfp, pcm, off, 1, sr, fr, nf, &qoff[1]);
	}
	else {
		rc = tfp_group_fingerprint_f32_batch(g_tfp, x, off, 1, sr, fr, nf, &qoff[1]);
	}
	if(rc == TFP_OK) {
		rc = tfp_group_search_aligned_batch(g_tfp, fr, qoff, 1, &p, k, cand, align, &count);
	}
	ast_free(fr);
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not search %s: %s\n", filename, tfp_group_last_error(g_tfp));
		return NULL;
	}
	j_res = ast_json_array_create();
	for(i = 0; i < count; i++) {
		memset(&r, 0, sizeof(r));
		r.found = 1;
		r.match_count = cand[i].match_count;
		r.frame_count = (int32_t)nf;
		snprintf(r.uuid, sizeof(r.uuid), "%s", cand[i].uuid);
		j_tmp = search_result(&r); /* a row whose audio_list entry is missing is skipped */
		if(j_tmp != NULL) {
			ast_json_object_set(j_tmp, "aligned_count", ast_json_integer_create(align[i].aligned_count));
			ast_json_object_set(j_tmp, "offset", ast_json_integer_create(align[i].offset));
			ast_json_object_set(j_tmp, "first_frame", ast_json_integer_create(align[i].first_frame));
			ast_json_object_set(j_tmp, "last_frame", ast_json_integer_create(align[i].last_frame));
			ast_json_array_append(j_res, j_tmp);
		}
	}
	return j_res;
}

/* New: fp_search_fingerprint_timeline's array with where in its clip each row's window lies: every
 * row also carries aligned_count, offset, first_frame and last_frame (tfp_alignment of the window's
 * frames alone with the row's clip, as fp_search_fingerprint_aligned words them) and
 * clip_start_frame = frame - offset, the recording frame at which clip frame 0 lies, equal across
 * the windows of one occurrence wherever its offset alone attains the window's aligned_count. The reference's result query (fp_handler.c:367-374) never reads the
 * rows' frame_idx. The file's frames once (tfp_group_fingerprint_batch / _f32_batch), then
 * tfp_group_search_sliding_aligned_batch. NULL and the empty array as for the timeline call. */
struct ast_json* fp_search_fingerprint_timeline_aligned(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int window_frames,
		const int hop_frames, const int max_results, const bool in_context)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, off[2], qoff[2] = {0, 0}, nf = 0, nw = 0, got = 0, w;
	int32_t sr, scope = TFP_SCOPE_ANY;
	int rc, k, i;
	tfp_search_params p;
	tfp_candidate* cand;
	tfp_alignment* align;
	int32_t* counts;
	tfp_frame* fr;
	tfp_result r;
	struct ast_json* j_res;
	struct ast_json* j_win;
	struct ast_json* j_rows;
	struct ast_json* j_tmp;

	if((filename == NULL) || (max_results < 1) || (window_frames < 1) || (hop_frames < 1)) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return NULL;
	}
	k = max_results > TFP_RANK_MAX ? TFP_RANK_MAX : max_results;
	off[0] = 0;
	off[1] = ns;
	nf = tfp_frame_count(ns); /* ast_json_array_size(j_fprints), fp_handler.c:286 */
	nw = tfp_sliding_windows(nf, window_frames, hop_frames);
	if(in_context == true) {
		scope = scope_of_context(context, false);
	}
	cand = ast_calloc((nw > 0 ? nw : 1) * k, sizeof(*cand));
	align = ast_calloc((nw > 0 ? nw : 1) * k, sizeof(*align));
	counts = ast_calloc(nw > 0 ? nw : 1, sizeof(*counts));
	fr = ast_calloc(nf > 0 ? nf : 1, sizeof(*fr));
	if((cand == NULL) || (align == NULL) || (counts == NULL) || (fr == NULL)) {
		rc = TFP_E_NOMEM;
	}
	else if(pcm != NULL) {
		rc = tfp_group_fingerprint_batch(g_tfp, pcm, off, 1, sr, fr, nf, &qoff[1]);
	}
	else {
		rc = tfp_group_fingerprint_f32_batch(g_tfp, x, off, 1, sr, fr, nf, &qoff[1]);
	}
	if(rc == TFP_OK) {
		rc = tfp_group_search_sliding_aligned_batch(g_tfp, fr, qoff, 1, &p, window_frames, hop_frames, &scope, k, cand,
				counts, align, nw, &got);
	}
	ast_free(fr);
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not search %s: %s\n", filename, tfp_group_last_error(g_tfp));
		ast_free(cand);
		ast_free(align);
		ast_free(counts);
		return NULL;
	}
	j_res = ast_json_array_create();
	for(w = 0; w < got; w++) {
		j_rows = ast_json_array_create();
		for(i = 0; i < counts[w]; i++) {
			const tfp_alignment* a = &align[w * k + i];
			memset(&r, 0, sizeof(r));
			r.found = 1;
			r.match_count = cand[w * k + i].match_count;
			r.frame_count = window_frames;
			snprintf(r.uuid, sizeof(r.uuid), "%s", cand[w * k + i].uuid);
			j_tmp = search_result(&r); /* a row whose audio_list entry is missing is skipped */
			if(j_tmp != NULL) {
				ast_json_object_set(j_tmp, "aligned_count", ast_json_integer_create(a->aligned_count));
				ast_json_object_set(j_tmp, "offset", ast_json_integer_create(a->offset));
				ast_json_object_set(j_tmp, "first_frame", ast_json_integer_create(a->first_frame));
				ast_json_object_set(j_tmp, "last_frame", ast_json_integer_create(a->last_frame));
				ast_json_object_set(j_tmp, "clip_start_frame", ast_json_integer_create(w * hop_frames - a->offset));
				ast_json_array_append(j_rows, j_tmp);
			}
		}
		j_win = ast_json_object_create();
		ast_json_object_set(j_win, "frame", ast_json_integer_create(w * hop_frames));
		ast_json_object_set(j_win, "rows", j_rows);
		ast_json_array_append(j_res, j_win);
	}
	ast_free(cand);
	ast_free(align);
	ast_free(counts);
	return j_res;
}

/* New: which clips of `context` play in the recording, and from which frame to which: the join of
 * fp_search_fingerprint_timeline_aligned's rows that call leaves to its caller, done by the engines
 * (tfp_group_search_occurrences_batch). The candidates (clip, clip_start_frame) of the first k rows
 * (src/fp_handler.c:367-374) of every window are each verified along their own diagonal over the whole
 * recording with the per-frame predicate of src/fp_handler.c:287-351, hits at most max_gap frames apart
 * forming a segment, and thinned by non-maximum suppression. A JSON array, by first_frame, of the clips'
 * audio_list rows with "frame_count" (the recording's frames), "match_count" and "hits" (those of the
 * segment), "clip_start_frame", "first_frame", "last_frame", "diagonal_hits", "overlap" and "windows". The context
 * is mapped to a scope as fp_search_fingerprint_in_context maps it. NULL for bad arguments or a failed
 * search; the empty array where nothing plays. */
struct ast_json* fp_search_fingerprint_occurrences(const char* context, const char* filename, const int coefs,
		const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int window_frames,
		const int hop_frames, const int k, const int max_gap, const int min_hits)
{
	int16_t* pcm;
	float* x;
	int64_t cap, ns, off[2], qoff[2] = {0, 0}, nf = 0, room = 64, got = 0, i;
	int32_t sr, scope;
	int rc, rows;
	tfp_search_params p;
	tfp_occurrence* occ = NULL;
	tfp_frame* fr;
	tfp_result r;
	struct ast_json* j_res;
	struct ast_json* j_tmp;

	if((filename == NULL) || (k < 1) || (window_frames < 1) || (hop_frames < 1) || (max_gap < 0) || (min_hits < 1)) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	if(read_audio(filename, &pcm, &cap, &x, &ns, &sr) != 0) {
		return NULL;
	}
	rows = k > TFP_RANK_MAX ? TFP_RANK_MAX : k;
	off[0] = 0;
	off[1] = ns;
	nf = tfp_frame_count(ns); /* ast_json_array_size(j_fprints), fp_handler.c:286 */
	scope = scope_of_context(context, false);
	fr = ast_calloc(nf > 0 ? nf : 1, sizeof(*fr));
	if(fr == NULL) {
		rc = TFP_E_NOMEM;
	}
	else if(pcm != NULL) {
		rc = tfp_group_fingerprint_batch(g_tfp, pcm, off, 1, sr, fr, nf, &qoff[1]);
	}
	else {
		rc = tfp_group_fingerprint_f32_batch(g_tfp, x, off, 1, sr, fr, nf, &qoff[1]);
	}
	while(rc == TFP_OK) { /* (a list longer than the room: once more with the room it names) */
		occ = ast_calloc(room, sizeof(*occ));
		if(occ == NULL) {
			rc = TFP_E_NOMEM;
			break;
		}
		rc = tfp_group_search_occurrences_batch(g_tfp, fr, qoff, 1, &p, window_frames, hop_frames, &scope, rows, max_gap,
				min_hits, occ, room, &got);
		if((rc != TFP_E_CAPACITY) || (got <= room)) {
			break;
		}
		ast_free(occ);
		occ = NULL;
		room = got;
		rc = TFP_OK;
	}
	ast_free(fr);
	pcm_put(pcm, cap);
	ast_free(x);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not search %s: %s\n", filename, tfp_group_last_error(g_tfp));
		ast_free(occ);
		return NULL;
	}
	j_res = ast_json_array_create();
	for(i = 0; i < got; i++) {
		memset(&r, 0, sizeof(r));
		r.found = 1;
		r.match_count = occ[i].hits;
		r.frame_count = (int32_t)nf;
		snprintf(r.uuid, sizeof(r.uuid), "%s", occ[i].uuid);
		j_tmp = search_result(&r); /* an occurrence whose audio_list entry is missing is skipped */
		if(j_tmp != NULL) {
			ast_json_object_set(j_tmp, "clip_start_frame", ast_json_integer_create(occ[i].clip_start_frame));
			ast_json_object_set(j_tmp, "first_frame", ast_json_integer_create(occ[i].first_frame));
			ast_json_object_set(j_tmp, "last_frame", ast_json_integer_create(occ[i].last_frame));
			ast_json_object_set(j_tmp, "hits", ast_json_integer_create(occ[i].hits));
			ast_json_object_set(j_tmp, "diagonal_hits", ast_json_integer_create(occ[i].diagonal_hits));
			ast_json_object_set(j_tmp, "overlap", ast_json_integer_create(occ[i].overlap));
			ast_json_object_set(j_tmp, "windows", ast_json_integer_create(occ[i].windows));
			ast_json_array_append(j_res, j_tmp);
		}
	}
	ast_free(occ);
	return j_res;
}

/* ---- live channels: the dialplan application's recording without the /tmp WAV -------------
 * application_handler.c:152-185 records `duration` ms of the channel's voice frames
 * (record_voice, :248-312) into /tmp/tiresias-UUID.wav and searches that file. A channel keeps the
 * same samples in engine-mapped host memory instead: every voice frame is pushed as it is read,
 * and the search reads the recording in place (tfp_group_search_pcm_gather, coalesced with the
 * other channels' searches). The ring keeps the last max_ms of audio (written twice, so the kept
 * samples are always one contiguous run); with max_ms >= the recording's length it holds exactly
 * what record_voice would have written. */
struct fp_channel {
	int32_t sr;
	int64_t cap;   /* samples kept */
	int64_t n;     /* samples pushed since open / reset */
	int64_t pos;   /* ring position of the next sample */
	int16_t* ring; /* 2 * cap samples, tfp_host_alloc */
};

fp_channel* fp_channel_open(int sample_rate, int max_ms)
{
	fp_channel* ch;
	void* p = NULL;

	if(sample_rate <= 0 || max_ms <= 0) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	ch = ast_calloc(1, sizeof(*ch));
	if(ch == NULL) {
		return NULL;
	}
	ch->sr = sample_rate;
	ch->cap = ((int64_t)sample_rate * max_ms + 999) / 1000;
	if(tfp_host_alloc(sizeof(int16_t) * 2 * (size_t)ch->cap, &p) != TFP_OK) {
		ast_free(ch);
		return NULL;
	}
	ch->ring = (int16_t*)p;
	return ch;
}

bool fp_channel_push(fp_channel* ch, const int16_t* slin, int nsamples)
{
	int64_t i;

	if(ch == NULL || nsamples < 0 || (nsamples > 0 && slin == NULL)) {
		return false;
	}
	for(i = 0; i < nsamples; i++) {
		ch->ring[ch->pos] = slin[i];
		ch->ring[ch->pos + ch->cap] = slin[i];
		if(++ch->pos == ch->cap) {
			ch->pos = 0;
		}
	}
	ch->n += nsamples;
	return true;
}

bool fp_channel_push_g711(fp_channel* ch, const uint8_t* payload, int nsamples, int law)
{
	int16_t slin[512];
	int at;

	if(ch == NULL || nsamples < 0 || (nsamples > 0 && payload == NULL) || (law != TFP_G711_ULAW && law != TFP_G711_ALAW)) {
		return false;
	}
	for(at = 0; at < nsamples; at += 512) {
		const int n = nsamples - at < 512 ? nsamples - at : 512;
		if(tfp_g711_decode(payload + at, n, law, slin) != TFP_OK || fp_channel_push(ch, slin, n) == false) {
			return false;
		}
	}
	return true;
}

void fp_channel_reset(fp_channel* ch)
{
	if(ch != NULL) {
		ch->n = 0;
		ch->pos = 0;
	}
}

struct ast_json* fp_channel_search(fp_channel* ch, const char* context, const int coefs, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high)
{
	tfp_search_params p;
	tfp_result r;
	const int16_t* q;
	int64_t len;
	int rc;

	if(ch == NULL) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	if(search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	/* the kept samples: [0, n) before the ring wraps, else the cap samples from pos */
	len = ch->n < ch->cap ? ch->n : ch->cap;
	q = ch->n < ch->cap ? ch->ring : ch->ring + ch->pos;
	rc = tfp_group_search_pcm_gather(g_tfp, &q, &len, 1, ch->sr, &p, &r);
	if(rc != TFP_OK) {
		ast_log(LOG_ERROR, "Could not search the channel's recording: %s\n", tfp_group_last_error(g_tfp));
		return NULL;
	}
	return search_result(&r);
}

void fp_channel_close(fp_channel* ch)
{
	if(ch != NULL) {
		tfp_host_free(ch->ring);
		ast_free(ch);
	}
}

/* ---- live calls: the record loop's ticks in, an exact early verdict out ---------------------
 * record_voice (application_handler.c:248-312) reads one voice frame per channel every 20 ms for a
 * planned `duration` (:163), and the application searches the recording in its context once it is
 * complete (:152-185). A live object takes the frames of all its channels tick by tick
 * (tfp_group_live_push / tfp_group_live_push_g711: the calls stay on the GPUs from their first
 * sample) and fp_live_verdict says per channel whether the search of the finished recording is
 * already settled (tfp_group_live_verdict). Used by one thread, the one that aggregates the tick. */
struct fp_live {
	tfp_group_live* lv;
	int32_t nch, sr;
};

static int64_t samples_of_ms(int32_t sr, int ms)
{
	return ((int64_t)sr * ms + 999) / 1000; /* as fp_channel_open sizes its recording */
}

fp_live* fp_live_open(int nchannels, int sample_rate, int max_ms)
{
	fp_live* lv;

	if(g_tfp == NULL || nchannels <= 0 || sample_rate <= 0 || max_ms <= 0) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	lv = ast_calloc(1, sizeof(*lv));
	if(lv == NULL) {
		return NULL;
	}
	lv->nch = nchannels;
	lv->sr = sample_rate;
	if(tfp_group_live_create(g_tfp, nchannels, sample_rate, samples_of_ms(sample_rate, max_ms), &lv->lv) != TFP_OK) {
		ast_log(LOG_ERROR, "Could not open %d live calls: %s\n", nchannels, tfp_group_last_error(g_tfp));
		ast_free(lv);
		return NULL;
	}
	return lv;
}

bool fp_live_push(fp_live* lv, const int16_t* slin, int tick_samples, const int32_t* nsamples)
{
	if(lv == NULL || slin == NULL || tick_samples <= 0) {
		return false;
	}
	if(tfp_group_live_push(lv->lv, slin, tick_samples, nsamples, NULL, NULL, 0, NULL, NULL, NULL) != TFP_OK) {
		ast_log(LOG_ERROR, "Could not push a tick: %s\n", tfp_group_last_error(g_tfp));
		return false;
	}
	return true;
}

bool fp_live_push_g711(fp_live* lv, const uint8_t* payload, int tick_samples, int law, const int32_t* nsamples)
{
	if(lv == NULL || payload == NULL || tick_samples <= 0 || (law != TFP_G711_ULAW && law != TFP_G711_ALAW)) {
		return false;
	}
	if(tfp_group_live_push_g711(lv->lv, payload, tick_samples, law, nsamples, NULL, NULL, 0, NULL, NULL, NULL) != TFP_OK) {
		ast_log(LOG_ERROR, "Could not push a tick: %s\n", tfp_group_last_error(g_tfp));
		return false;
	}
	return true;
}

struct ast_json* fp_live_verdict(fp_live* lv, const char* const* contexts, const int* duration_ms, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high)
{
	tfp_search_params p;
	struct tfp_live_verdict* v;
	int64_t* total;
	int32_t* scopes;
	int32_t c;
	int rc;
	struct ast_json* j_res = NULL;

	if(lv == NULL || contexts == NULL || duration_ms == NULL) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	for(c = 0; c < lv->nch; c++) {
		if(contexts[c] == NULL || duration_ms[c] <= 0) {
			ast_log(LOG_WARNING, "Wrong input parameter.\n");
			return NULL;
		}
	}
	/* coefs = 1: what the dialplan passes (application_handler.c:180), and what a verdict's counts are */
	if(search_params(&p, contexts[0], 1, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	v = ast_calloc(lv->nch, sizeof(*v));
	total = ast_calloc(lv->nch, sizeof(*total));
	scopes = ast_calloc(lv->nch, sizeof(*scopes));
	if(v != NULL && total != NULL && scopes != NULL) {
		for(c = 0; c < lv->nch; c++) {
			total[c] = samples_of_ms(lv->sr, duration_ms[c]);
			scopes[c] = scope_of_context(contexts[c], false); /* as fp_search_fingerprint_in_context maps it */
		}
		rc = tfp_group_live_verdict(lv->lv, total, &p, scopes, v);
		if(rc != TFP_OK) {
			ast_log(LOG_ERROR, "Could not take the calls' verdicts: %s\n", tfp_group_last_error(g_tfp));
		}
		else {
			j_res = ast_json_array_create();
		}
		for(c = 0; j_res != NULL && c < lv->nch; c++) {
			struct ast_json* j_tmp = NULL;
			int64_t ns = 0;
			if(v[c].has_leader != 0) {
				j_tmp = fpc_get_audio_list_info(v[c].leader.uuid); /* fp_handler.c:394-401 */
				if(j_tmp == NULL) {
					ast_log(LOG_ERROR, "Could not get audio list info. uuid[%s]\n", v[c].leader.uuid);
				}
			}
			if(j_tmp == NULL) {
				j_tmp = ast_json_object_create();
			}
			else {
				tfp_group_live_samples(lv->lv, c, &ns);
				ast_json_object_set(j_tmp, "frame_count", ast_json_integer_create(tfp_frame_count(ns)));
				ast_json_object_set(j_tmp, "match_count", ast_json_integer_create(v[c].leader.match_count));
			}
			ast_json_object_set(j_tmp, "decided", ast_json_integer_create(v[c].decided));
			ast_json_object_set(j_tmp, "complete", ast_json_integer_create(v[c].complete));
			ast_json_object_set(j_tmp, "remaining", ast_json_integer_create(v[c].remaining));
			ast_json_object_set(j_tmp, "rival_match_count",
					ast_json_integer_create(v[c].has_rival != 0 ? v[c].rival.match_count : -1));
			ast_json_array_append(j_res, j_tmp);
		}
	}
	ast_free(v);
	ast_free(total);
	ast_free(scopes);
	return j_res;
}

/* The calls' trailing windows (tfp_group_live_window): per channel the first k rows of the search of
 * the last window_ms of its call in its context, each with its catalog fields as fp_live_verdict
 * fills the leader's (fp_handler.c:394-401), beside the window's first frame and frame count. */
static struct ast_json* live_window_json(fp_live* lv, const char* const* contexts, const int window_ms, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k, const bool aligned)
{
	tfp_search_params p;
	tfp_candidate* cand;
	tfp_alignment* align;
	int32_t* scopes;
	int32_t* counts;
	int32_t* fc;
	int32_t* ff;
	int32_t c, i, kk;
	int rc;
	struct ast_json* j_res = NULL;

	if(lv == NULL || contexts == NULL || window_ms <= 0 || k < 1) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	for(c = 0; c < lv->nch; c++) {
		if(contexts[c] == NULL) {
			ast_log(LOG_WARNING, "Wrong input parameter.\n");
			return NULL;
		}
	}
	/* coefs = 1: what the dialplan passes (application_handler.c:180), and the form whose counts slide */
	if(search_params(&p, contexts[0], 1, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	kk = k > TFP_RANK_MAX ? TFP_RANK_MAX : k;
	cand = ast_calloc((size_t)lv->nch * kk, sizeof(*cand));
	align = ast_calloc((size_t)lv->nch * kk, sizeof(*align));
	scopes = ast_calloc(lv->nch, sizeof(*scopes));
	counts = ast_calloc(lv->nch, sizeof(*counts));
	fc = ast_calloc(lv->nch, sizeof(*fc));
	ff = ast_calloc(lv->nch, sizeof(*ff));
	if(cand != NULL && align != NULL && scopes != NULL && counts != NULL && fc != NULL && ff != NULL) {
		for(c = 0; c < lv->nch; c++) {
			scopes[c] = scope_of_context(contexts[c], false); /* as fp_search_fingerprint_in_context maps it */
		}
		if(aligned) {
			rc = tfp_group_live_window_aligned(lv->lv, &p, scopes, kk, tfp_live_window_frames(window_ms, lv->sr), cand, align,
					counts, fc, ff);
		}
		else {
			rc = tfp_group_live_window(lv->lv, &p, scopes, kk, tfp_live_window_frames(window_ms, lv->sr), cand, counts, fc, ff);
		}
		if(rc != TFP_OK) {
			ast_log(LOG_ERROR, "Could not search the calls' windows: %s\n", tfp_group_last_error(g_tfp));
		}
		else {
			j_res = ast_json_array_create();
		}
		for(c = 0; j_res != NULL && c < lv->nch; c++) {
			struct ast_json* j_ch = ast_json_object_create();
			struct ast_json* j_rows = ast_json_array_create();
			for(i = 0; i < counts[c]; i++) {
				tfp_result r;
				struct ast_json* j_tmp;
				memset(&r, 0, sizeof(r));
				r.found = 1;
				r.match_count = cand[(size_t)c * kk + i].match_count;
				r.frame_count = fc[c];
				snprintf(r.uuid, sizeof(r.uuid), "%s", cand[(size_t)c * kk + i].uuid);
				j_tmp = search_result(&r); /* a row whose audio_list entry is missing is skipped */
				if(j_tmp != NULL && aligned) {
					const tfp_alignment* a = &align[(size_t)c * kk + i];
					ast_json_object_set(j_tmp, "aligned_count", ast_json_integer_create(a->aligned_count));
					ast_json_object_set(j_tmp, "offset", ast_json_integer_create(a->offset));
					ast_json_object_set(j_tmp, "first_frame", ast_json_integer_create(a->first_frame));
					ast_json_object_set(j_tmp, "last_frame", ast_json_integer_create(a->last_frame));
					ast_json_object_set(j_tmp, "clip_start_frame", ast_json_integer_create(ff[c] - a->offset));
				}
				if(j_tmp != NULL) {
					ast_json_array_append(j_rows, j_tmp);
				}
			}
			ast_json_object_set(j_ch, "first_frame", ast_json_integer_create(ff[c]));
			ast_json_object_set(j_ch, "frame_count", ast_json_integer_create(fc[c]));
			ast_json_object_set(j_ch, "rows", j_rows);
			ast_json_array_append(j_res, j_ch);
		}
	}
	ast_free(cand);
	ast_free(align);
	ast_free(scopes);
	ast_free(counts);
	ast_free(fc);
	ast_free(ff);
	return j_res;
}

struct ast_json* fp_live_window(fp_live* lv, const char* const* contexts, const int window_ms, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k)
{
	return live_window_json(lv, contexts, window_ms, tolerance, freq_ignore_low, freq_ignore_high, k, false);
}

/* fp_live_window with where each row's clip lies in the window (tfp_group_live_window_aligned): the
 * per-frame predicate of fp_handler.c:287-351 along the clip's stored rows, for the rows of :367-374. */
struct ast_json* fp_live_window_aligned(fp_live* lv, const char* const* contexts, const int window_ms, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k)
{
	return live_window_json(lv, contexts, window_ms, tolerance, freq_ignore_low, freq_ignore_high, k, true);
}

/* The calls' logs (tfp_group_live_occurrences): per channel the clips of its context that have played so
 * far, each with its catalog fields (fp_handler.c:394-401) and where it lies in the call: the per-frame
 * predicate of fp_handler.c:287-351 along each candidate's diagonal, for the rows of :367-374 over the last
 * window_ms. One JSON array per channel, by first_frame. */
struct ast_json* fp_live_occurrences(fp_live* lv, const char* const* contexts, const int window_ms, const int max_gap_ms,
		const int min_hits, const double tolerance, const int freq_ignore_low, const int freq_ignore_high, const int k)
{
	tfp_search_params p;
	tfp_occurrence* occ;
	int32_t* scopes;
	int64_t n = 0, i, cap;
	int32_t c, kk;
	int rc;
	struct ast_json* j_res = NULL;

	if(lv == NULL || contexts == NULL || window_ms <= 0 || max_gap_ms < 0 || min_hits < 1 || k < 1) {
		ast_log(LOG_WARNING, "Wrong input parameter.\n");
		return NULL;
	}
	for(c = 0; c < lv->nch; c++) {
		if(contexts[c] == NULL) {
			ast_log(LOG_WARNING, "Wrong input parameter.\n");
			return NULL;
		}
	}
	/* coefs = 1: what the dialplan passes (application_handler.c:180), and the form whose counts slide */
	if(search_params(&p, contexts[0], 1, tolerance, freq_ignore_low, freq_ignore_high) == false) {
		return NULL;
	}
	kk = k > TFP_RANK_MAX ? TFP_RANK_MAX : k;
	cap = (int64_t)lv->nch * TFP_LIVE_TRACKS_MAX; /* every track an occurrence: the call never lacks room */
	occ = ast_calloc((size_t)cap, sizeof(*occ));
	scopes = ast_calloc(lv->nch, sizeof(*scopes));
	if(occ != NULL && scopes != NULL) {
		for(c = 0; c < lv->nch; c++) {
			scopes[c] = scope_of_context(contexts[c], false); /* as fp_search_fingerprint_in_context maps it */
		}
		/* max_gap_ms converts as window_ms does; 0 ms is 0 frames */
		rc = tfp_group_live_occurrences(lv->lv, &p, scopes, kk, tfp_live_window_frames(window_ms, lv->sr),
				max_gap_ms > 0 ? tfp_live_window_frames(max_gap_ms, lv->sr) : 0, min_hits, TFP_LIVE_TRACKS_MAX, occ, cap, &n, NULL);
		if(rc != TFP_OK) {
			ast_log(LOG_ERROR, "Could not list the calls' occurrences: %s\n", tfp_group_last_error(g_tfp));
		}
		else {
			j_res = ast_json_array_create();
		}
		for(c = 0; j_res != NULL && c < lv->nch; c++) {
			ast_json_array_append(j_res, ast_json_array_create());
		}
		for(i = 0; j_res != NULL && i < n; i++) {
			const tfp_occurrence* o = &occ[i];
			struct ast_json* j_tmp = fpc_get_audio_list_info(o->uuid); /* an entry whose audio_list row is missing is skipped */
			if(j_tmp == NULL) {
				ast_log(LOG_ERROR, "Could not get audio list info. uuid[%s]\n", o->uuid);
				continue;
			}
			ast_json_object_set(j_tmp, "clip_start_frame", ast_json_integer_create(o->clip_start_frame));
			ast_json_object_set(j_tmp, "first_frame", ast_json_integer_create(o->first_frame));
			ast_json_object_set(j_tmp, "last_frame", ast_json_integer_create(o->last_frame));
			ast_json_object_set(j_tmp, "hits", ast_json_integer_create(o->hits));
			ast_json_object_set(j_tmp, "diagonal_hits", ast_json_integer_create(o->diagonal_hits));
			ast_json_object_set(j_tmp, "overlap", ast_json_integer_create(o->overlap));
			ast_json_object_set(j_tmp, "windows", ast_json_integer_create(o->windows));
			ast_json_array_append(ast_json_array_get(j_res, (size_t)o->recording), j_tmp);
		}
	}
	ast_free(occ);
	ast_free(scopes);
	return j_res;
}

#define FP_NEIGHBOUR_FLUSH 512 /* audios per tfp_group_index_neighbours call */

/* The audios j_list[first, first + n) (catalog objects) that have fingerprint rows, each as a fresh catalog
 * object with frame_count and neighbours, appended to j_res: one tfp_group_index_neighbours call. */
static bool neighbours_flush(struct ast_json* j_list, size_t first, size_t n, int32_t scope, const tfp_search_params* p,
		int k, struct ast_json* j_res)
{
	const char** uu = ast_calloc(n, sizeof(*uu));
	int32_t* scopes = ast_calloc(n, sizeof(*scopes));
	int32_t* counts = ast_calloc(n, sizeof(*counts));
	int32_t* frames = ast_calloc(n, sizeof(*frames));
	tfp_candidate* cand = ast_calloc(n * k, sizeof(*cand));
	tfp_alignment* align = ast_calloc(n * k, sizeof(*align));
	int32_t m = 0, s, i, r;
	size_t a;
	bool ret = (uu != NULL) && (scopes != NULL) && (counts != NULL) && (frames != NULL) && (cand != NULL) && (align != NULL);

	for(a = first; ret && a < first + n; a++) {
		const char* uuid = ast_json_string_get(ast_json_object_get(ast_json_array_get(j_list, a), "uuid"));
		if(uuid != NULL && tfp_group_index_scope(g_tfp, uuid, &s) == TFP_OK) { /* else: a catalog row without fingerprint rows */
			uu[m] = uuid;
			scopes[m++] = scope;
		}
	}
	if(ret && m > 0 && tfp_group_index_neighbours(g_tfp, m, uu, p, scopes, k, cand, align, counts, frames) != TFP_OK) {
		ast_log(LOG_ERROR, "Could not get neighbours: %s\n", tfp_group_last_error(g_tfp));
		ret = false;
	}
	for(i = 0; ret && i < m; i++) {
		struct ast_json* j_audio = fpc_get_audio_list_info(uu[i]);
		struct ast_json* j_rows;
		if(j_audio == NULL) {
			continue;
		}
		j_rows = ast_json_array_create();
		for(r = 0; r < counts[i]; r++) {
			const tfp_candidate* c = &cand[(size_t)i * k + r];
			const tfp_alignment* al = &align[(size_t)i * k + r];
			struct ast_json* j_tmp = fpc_get_audio_list_info(c->uuid); /* a row whose audio_list entry is missing is skipped */
			if(j_tmp == NULL) {
				ast_log(LOG_ERROR, "Could not get audio list info. uuid[%s]\n", c->uuid);
				continue;
			}
			ast_json_object_set(j_tmp, "match_count", ast_json_integer_create(c->match_count));
			ast_json_object_set(j_tmp, "aligned_count", ast_json_integer_create(al->aligned_count));
			ast_json_object_set(j_tmp, "offset", ast_json_integer_create(al->offset));
			ast_json_object_set(j_tmp, "first_frame", ast_json_integer_create(al->first_frame));
			ast_json_object_set(j_tmp, "last_frame", ast_json_integer_create(al->last_frame));
			ast_json_array_append(j_rows, j_tmp);
		}
		ast_json_object_set(j_audio, "frame_count", ast_json_integer_create(frames[i]));
		ast_json_object_set(j_audio, "neighbours", j_rows);
		ast_json_array_append(j_res, j_audio);
	}
	ast_free(uu);
	ast_free(scopes);
	ast_free(counts);
	ast_free(frames);
	ast_free(cand);
	ast_free(align);
	return ret;
}

/* j_list (consumed): an array of catalog objects; the array of their neighbour objects, or NULL */
static struct ast_json* audio_neighbours(struct ast_json* j_list, int32_t scope, const tfp_search_params* p, const int k)
{
	const int kk = k > TFP_RANK_MAX ? TFP_RANK_MAX : k;
	struct ast_json* j_res;
	size_t n, a;

	if(j_list == NULL) {
		return NULL;
	}
	n = ast_json_array_size(j_list);
	j_res = ast_json_array_create();
	for(a = 0; j_res != NULL && a < n; a += FP_NEIGHBOUR_FLUSH) {
		if(neighbours_flush(j_list, a, n - a < FP_NEIGHBOUR_FLUSH ? n - a : FP_NEIGHBOUR_FLUSH, scope, p, kk, j_res) == false) {
			ast_json_unref(j_res);
			j_res = NULL;
		}
	}
	ast_json_unref(j_list);
	return j_res;
}

struct ast_json* fp_get_audio_list_neighbours(const char* context, const int coefs, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k)
{
	tfp_search_params p;

	if((k < 1) || (search_params(&p, context, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false)) {
		return NULL;
	}
	return audio_neighbours(fp_get_audio_lists_by_contextname(context), scope_of_context(context, false), &p, k);
}

struct ast_json* fp_get_audio_neighbours(const char* uuid, const int coefs, const double tolerance,
		const int freq_ignore_low, const int freq_ignore_high, const int k)
{
	tfp_search_params p;
	struct ast_json* j_list;
	struct ast_json* j_info;
	struct ast_json* j_res;
	struct ast_json* j_one = NULL;

	if((k < 1) || (search_params(&p, uuid, coefs, tolerance, freq_ignore_low, freq_ignore_high) == false)) {
		return NULL;
	}
	j_info = fpc_get_audio_list_info(uuid);
	if(j_info == NULL) {
		return NULL;
	}
	j_list = ast_json_array_create();
	ast_json_array_append(j_list, j_info);
	j_res = audio_neighbours(j_list, TFP_SCOPE_ANY, &p, k);
	if(j_res != NULL && ast_json_array_size(j_res) == 1) {
		/* the one object rebuilt on its own: j_res is freed with its elements below */
		struct ast_json* j_src = ast_json_array_get(j_res, 0);
		struct ast_json* j_rows = ast_json_object_get(j_src, "neighbours");
		struct ast_json* j_new = ast_json_array_create();
		size_t r;
		static const char* const keys[] = {"match_count", "aligned_count", "offset", "first_frame", "last_frame"};
		j_one = fpc_get_audio_list_info(uuid);
		for(r = 0; j_one != NULL && r < ast_json_array_size(j_rows); r++) {
			struct ast_json* j_row = ast_json_array_get(j_rows, r);
			struct ast_json* j_tmp = fpc_get_audio_list_info(ast_json_string_get(ast_json_object_get(j_row, "uuid")));
			size_t f;
			if(j_tmp == NULL) {
				continue;
			}
			for(f = 0; f < sizeof(keys) / sizeof(keys[0]); f++) {
				ast_json_object_set(j_tmp, keys[f], ast_json_integer_create(ast_json_integer_get(ast_json_object_get(j_row, keys[f]))));
			}
			ast_json_array_append(j_new, j_tmp);
		}
		if(j_one != NULL) {
			ast_json_object_set(j_one, "frame_count",
					ast_json_integer_create(ast_json_integer_get(ast_json_object_get(j_src, "frame_count"))));
			ast_json_object_set(j_one, "neighbours", j_new);
		}
		else {
			ast_json_unref(j_new);
		}
	}
	ast_json_unref(j_res);
	return j_one;
}

void fp_live_reset(fp_live* lv, int channel)
{
	if(lv != NULL && channel < lv->nch) {
		tfp_group_live_reset(lv->lv, channel);
	}
}

void fp_live_close(fp_live* lv)
{
	if(lv != NULL) {
		tfp_group_live_destroy(lv->lv);
		ast_free(lv);
	}
}
