/* TEST HARNESS (tests/test_gpu_live_occurrences_shim.py; not product code): the calls' logs through the
 * module's facade from C, on the Asterisk stubs of shim_harness.c (linked in with its main renamed), over a
 * group of three engines on device 0:
 *   shim_live_occurrences BACKUP_DB TOL K CODES0 CODES1 A1 A2 B1 B2 WINDOW_MS MAX_GAP_MS MIN_HITS EVERY
 * shim_live_window_harness.c's set-up and pushes; after every EVERY-th tick it asks fp_live_occurrences. One
 * JSON line: {"catalog": {...}, "asks": [{"tick": T, "log": [CH, CH]}...]}, CH = [{uuid, name, context, hash,
 * clip_start_frame, first_frame, last_frame, hits, diagonal_hits, overlap, windows}...]. */
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"
#include "tiresias_fp.h"

static void print_catalog(const char* ctx) {
  struct ast_json* arr = fp_get_audio_lists_by_contextname(ctx);
  size_t i, n = arr ? ast_json_array_size(arr) : 0;
  printf("\"%s\": [", ctx);
  for (i = 0; i < n; i++) {
    struct ast_json* j = ast_json_array_get(arr, i);
    printf("%s{\"uuid\": \"%s\", \"name\": \"%s\"}", i ? ", " : "", ast_json_string_get(ast_json_object_get(j, "uuid")),
           ast_json_string_get(ast_json_object_get(j, "name")));
  }
  printf("]");
  if (arr) ast_json_unref(arr);
}

static int print_log(struct ast_json* arr) {
  static const char* const seven[7] = {"clip_start_frame", "first_frame", "last_frame", "hits", "diagonal_hits", "overlap", "windows"};
  size_t c, i;
  int f;
  if (!arr || ast_json_array_size(arr) != 2) return 1;
  printf("[");
  for (c = 0; c < 2; c++) {
    struct ast_json* ch = ast_json_array_get(arr, c);
    if (!ch) return 1;
    printf("%s[", c ? ", " : "");
    for (i = 0; i < ast_json_array_size(ch); i++) {
      struct ast_json* j = ast_json_array_get(ch, i);
      printf("%s{\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"hash\": \"%s\"", i ? ", " : "",
             ast_json_string_get(ast_json_object_get(j, "uuid")), ast_json_string_get(ast_json_object_get(j, "name")),
             ast_json_string_get(ast_json_object_get(j, "context")), ast_json_string_get(ast_json_object_get(j, "hash")));
      for (f = 0; f < 7; f++) {
        struct ast_json* v = ast_json_object_get(j, seven[f]);
        if (!v) return 1;
        printf(", \"%s\": %d", seven[f], (int)ast_json_integer_get(v));
      }
      printf("}");
    }
    printf("]");
  }
  printf("]");
  ast_json_unref(arr);
  return 0;
}

int main(int argc, char** argv) {
  static const char* const ctx[2] = {"a", "b"};
  static const char* const no_ctx[2] = {"a", NULL};
  int k, tick = 0, c, printed = 0, window_ms, gap_ms, min_hits, every;
  double tol;
  bool ok[2];
  FILE* fp[2];
  uint8_t blk[2][160];
  int32_t n[2];
  fp_live* lv;
  if (argc != 14) return 2;
  tol = atof(argv[2]);
  k = atoi(argv[3]);
  window_ms = atoi(argv[10]);
  gap_ms = atoi(argv[11]);
  min_hits = atoi(argv[12]);
  every = atoi(argv[13]);
  if (every < 1) return 2;
  fpc_set_backup_path(argv[1]);
  fp_set_gpu_devices("0,0,0");
  if (!fp_init()) return 3;
  if (fp_create_audio_list_infos("a", (const char* const*)(argv + 6), 2, ok) != 2 || !ok[0] || !ok[1]) return 4;
  if (fp_create_audio_list_infos("b", (const char* const*)(argv + 8), 2, ok) != 2 || !ok[0] || !ok[1]) return 4;
  printf("{\"catalog\": {");
  print_catalog("a");
  printf(", ");
  print_catalog("b");
  printf("}, \"asks\": [");
  lv = fp_live_open(2, 8000, 2000);
  if (!lv) return 5;
  /* a NULL object, NULL contexts, a NULL context, no window, a negative gap, no hit and no row asked for are refused */
  if (fp_live_occurrences(NULL, ctx, 100, 0, 1, tol, -1, -1, k) || fp_live_occurrences(lv, NULL, 100, 0, 1, tol, -1, -1, k) ||
      fp_live_occurrences(lv, no_ctx, 100, 0, 1, tol, -1, -1, k) || fp_live_occurrences(lv, ctx, 0, 0, 1, tol, -1, -1, k) ||
      fp_live_occurrences(lv, ctx, 100, -1, 1, tol, -1, -1, k) || fp_live_occurrences(lv, ctx, 100, 0, 0, tol, -1, -1, k) ||
      fp_live_occurrences(lv, ctx, 100, 0, 1, tol, -1, -1, 0))
    return 7;
  fp[0] = fopen(argv[4], "rb");
  fp[1] = fopen(argv[5], "rb");
  if (!fp[0] || !fp[1]) return 6;
  for (;;) {
    for (c = 0; c < 2; c++) n[c] = (int32_t)fread(blk[c], 1, 160, fp[c]);
    if (n[0] == 0 && n[1] == 0) break;
    if (!fp_live_push_g711(lv, &blk[0][0], 160, TFP_G711_ULAW, n)) return 6;
    tick++;
    if (tick % every) continue;
    printf("%s{\"tick\": %d, \"log\": ", printed++ ? ", " : "", tick);
    if (print_log(fp_live_occurrences(lv, ctx, window_ms, gap_ms, min_hits, tol, -1, -1, k))) return 8;
    printf("}");
  }
  fclose(fp[0]);
  fclose(fp[1]);
  fp_live_close(lv);
  printf("]}\n");
  return fp_term() ? 0 : 5;
}
