/* TEST HARNESS (tests/test_gpu_live_window_aligned_shim.py; not product code): the calls' aligned trailing
 * windows through the module's facade from C, on the Asterisk stubs of shim_harness.c (linked in with its
 * main renamed), over a group of three engines on device 0:
 *   shim_live_window_aligned BACKUP_DB TOL K CODES0 CODES1 A1 A2 B1 B2 TICK:WINDOW_MS...
 * shim_live_window_harness.c's set-up and pushes; after tick TICK of each TICK:WINDOW_MS it asks
 * fp_live_window and then fp_live_window_aligned for WINDOW_MS. One JSON line:
 *   {"catalog": {...}, "asks": [{"tick": T, "window_ms": W, "plain": [CH, CH], "aligned": [CH, CH]}...]}
 * CH = {"first_frame", "frame_count", "rows": [{uuid, name, context, hash, match_count, frame_count}...]},
 * an aligned row with "aligned_count", "offset", "first_frame", "last_frame" and "clip_start_frame" too. */
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

static int print_windows(struct ast_json* arr, bool aligned) {
  static const char* const five[5] = {"aligned_count", "offset", "first_frame", "last_frame", "clip_start_frame"};
  size_t c, i;
  int f;
  if (!arr || ast_json_array_size(arr) != 2) return 1;
  printf("[");
  for (c = 0; c < 2; c++) {
    struct ast_json* ch = ast_json_array_get(arr, c);
    struct ast_json* rows = ast_json_object_get(ch, "rows");
    if (!rows || !ast_json_object_get(ch, "first_frame") || !ast_json_object_get(ch, "frame_count")) return 1;
    printf("%s{\"first_frame\": %d, \"frame_count\": %d, \"rows\": [", c ? ", " : "",
           (int)ast_json_integer_get(ast_json_object_get(ch, "first_frame")),
           (int)ast_json_integer_get(ast_json_object_get(ch, "frame_count")));
    for (i = 0; i < ast_json_array_size(rows); i++) {
      struct ast_json* j = ast_json_array_get(rows, i);
      printf("%s{\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"hash\": \"%s\", \"match_count\": %d, \"frame_count\": %d",
             i ? ", " : "", ast_json_string_get(ast_json_object_get(j, "uuid")),
             ast_json_string_get(ast_json_object_get(j, "name")), ast_json_string_get(ast_json_object_get(j, "context")),
             ast_json_string_get(ast_json_object_get(j, "hash")), (int)ast_json_integer_get(ast_json_object_get(j, "match_count")),
             (int)ast_json_integer_get(ast_json_object_get(j, "frame_count")));
      for (f = 0; f < 5; f++) {
        struct ast_json* v = ast_json_object_get(j, five[f]);
        if ((v != NULL) != aligned) return 1; /* all five on an aligned row, none on a plain one */
        if (v) printf(", \"%s\": %d", five[f], (int)ast_json_integer_get(v));
      }
      printf("}");
    }
    printf("]}");
  }
  printf("]");
  ast_json_unref(arr);
  return 0;
}

int main(int argc, char** argv) {
  static const char* const ctx[2] = {"a", "b"};
  static const char* const no_ctx[2] = {"a", NULL};
  int k, tick = 0, c, ask = 10, printed = 0;
  double tol;
  bool ok[2];
  FILE* fp[2];
  uint8_t blk[2][160];
  int32_t n[2];
  fp_live* lv;
  if (argc < 11) return 2;
  tol = atof(argv[2]);
  k = atoi(argv[3]);
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
  /* a NULL object, NULL contexts, a NULL context, no window and no row asked for are refused */
  if (fp_live_window_aligned(NULL, ctx, 100, tol, -1, -1, k) || fp_live_window_aligned(lv, NULL, 100, tol, -1, -1, k) ||
      fp_live_window_aligned(lv, no_ctx, 100, tol, -1, -1, k) || fp_live_window_aligned(lv, ctx, 0, tol, -1, -1, k) ||
      fp_live_window_aligned(lv, ctx, -5, tol, -1, -1, k) || fp_live_window_aligned(lv, ctx, 100, tol, -1, -1, 0))
    return 7;
  fp[0] = fopen(argv[4], "rb");
  fp[1] = fopen(argv[5], "rb");
  if (!fp[0] || !fp[1]) return 6;
  for (;;) {
    for (c = 0; c < 2; c++) n[c] = (int32_t)fread(blk[c], 1, 160, fp[c]);
    if (n[0] == 0 && n[1] == 0) break;
    if (!fp_live_push_g711(lv, &blk[0][0], 160, TFP_G711_ULAW, n)) return 6;
    tick++;
    while (ask < argc) {
      int at = 0, ms = 0;
      if (sscanf(argv[ask], "%d:%d", &at, &ms) != 2) return 2;
      if (at != tick) break;
      printf("%s{\"tick\": %d, \"window_ms\": %d, \"plain\": ", printed++ ? ", " : "", at, ms);
      if (print_windows(fp_live_window(lv, ctx, ms, tol, -1, -1, k), false)) return 8;
      printf(", \"aligned\": ");
      if (print_windows(fp_live_window_aligned(lv, ctx, ms, tol, -1, -1, k), true)) return 8;
      printf("}");
      ask++;
    }
  }
  fclose(fp[0]);
  fclose(fp[1]);
  if (ask != argc) return 9; /* a tick the calls never reached */
  fp_live_close(lv);
  printf("]}\n");
  return fp_term() ? 0 : 5;
}
