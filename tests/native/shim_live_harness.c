/* TEST HARNESS (tests/test_gpu_live_shim.py; not product code): live calls through the module's facade
 * from C, on the Asterisk stubs of shim_harness.c (linked in with its main renamed):
 *   shim_live BACKUP_DB TOL DURATION_MS MID_TICK CODES0 CODES1 WAV0 WAV1 A1 A2 B1 B2
 * enrols prompts A1 A2 into context "a" and B1 B2 into context "b", opens two live calls (channel 0 in
 * context "a", channel 1 in "b"), pushes the raw mu-law codes of CODES0 / CODES1 in 160-byte ticks
 * with fp_live_push_g711 (a short last tick through nsamples) and takes fp_live_verdict after tick
 * MID_TICK and at the end, beside fp_search_fingerprint_in_context of WAV0 / WAV1 (the same audio
 * expanded). One JSON line:
 *   {"catalog": {"a": [{uuid, name}...], "b": [...]}, "mid": [V, V], "end": [V, V], "search": [OBJ|null, OBJ|null]}
 * V = {decided, complete, remaining, rival_match_count[, uuid, name, context, hash, match_count, frame_count]}. */
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"
#include "tiresias_fp.h"

static void print_clip(struct ast_json* j) {
  printf("\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"hash\": \"%s\", \"match_count\": %d, \"frame_count\": %d",
         ast_json_string_get(ast_json_object_get(j, "uuid")), ast_json_string_get(ast_json_object_get(j, "name")),
         ast_json_string_get(ast_json_object_get(j, "context")), ast_json_string_get(ast_json_object_get(j, "hash")),
         (int)ast_json_integer_get(ast_json_object_get(j, "match_count")),
         (int)ast_json_integer_get(ast_json_object_get(j, "frame_count")));
}

static int print_verdicts(struct ast_json* arr) {
  size_t i;
  if (!arr || ast_json_array_size(arr) != 2) return 1;
  printf("[");
  for (i = 0; i < 2; i++) {
    struct ast_json* j = ast_json_array_get(arr, i);
    printf("%s{\"decided\": %d, \"complete\": %d, \"remaining\": %d, \"rival_match_count\": %d", i ? ", " : "",
           (int)ast_json_integer_get(ast_json_object_get(j, "decided")),
           (int)ast_json_integer_get(ast_json_object_get(j, "complete")),
           (int)ast_json_integer_get(ast_json_object_get(j, "remaining")),
           (int)ast_json_integer_get(ast_json_object_get(j, "rival_match_count")));
    if (ast_json_object_get(j, "uuid")) {
      printf(", ");
      print_clip(j);
    }
    printf("}");
  }
  printf("]");
  ast_json_unref(arr);
  return 0;
}

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

int main(int argc, char** argv) {
  static const char* const ctx[2] = {"a", "b"};
  int dur[2], mid, tick = 0, c;
  double tol;
  bool ok[2];
  FILE* fp[2];
  uint8_t blk[2][160];
  int32_t n[2];
  int16_t slin[2][160];
  fp_live* lv;
  if (argc != 13) return 2;
  tol = atof(argv[2]);
  dur[0] = dur[1] = atoi(argv[3]);
  mid = atoi(argv[4]);
  fpc_set_backup_path(argv[1]);
  if (fp_live_open(2, 8000, 1000)) return 3; /* before fp_init: refused */
  if (!fp_init()) return 3;
  if (fp_create_audio_list_infos("a", (const char* const*)(argv + 9), 2, ok) != 2 || !ok[0] || !ok[1]) return 4;
  if (fp_create_audio_list_infos("b", (const char* const*)(argv + 11), 2, ok) != 2 || !ok[0] || !ok[1]) return 4;
  printf("{\"catalog\": {");
  print_catalog("a");
  printf(", ");
  print_catalog("b");
  printf("}, \"mid\": ");
  if (fp_live_open(0, 8000, 1000) || fp_live_open(2, 8000, 0)) return 5;
  lv = fp_live_open(2, 8000, dur[0]);
  if (!lv) return 5;
  memset(blk, 0xFF, sizeof blk);
  memset(slin, 0, sizeof slin);
  /* a bad law, a NULL payload and a NULL object are refused; a tick past max_ms ingests nothing */
  if (fp_live_push_g711(lv, &blk[0][0], 160, 2, NULL) || fp_live_push_g711(lv, NULL, 160, TFP_G711_ULAW, NULL) ||
      fp_live_push_g711(NULL, &blk[0][0], 160, TFP_G711_ULAW, NULL) || fp_live_push(lv, NULL, 160, NULL))
    return 7;
  /* an SLIN tick and a reset: the calls below start empty */
  if (!fp_live_push(lv, &slin[0][0], 160, NULL)) return 7;
  fp_live_reset(lv, -1);
  fp[0] = fopen(argv[5], "rb");
  fp[1] = fopen(argv[6], "rb");
  if (!fp[0] || !fp[1]) return 6;
  for (;;) {
    for (c = 0; c < 2; c++) n[c] = (int32_t)fread(blk[c], 1, 160, fp[c]);
    if (n[0] == 0 && n[1] == 0) break;
    if (!fp_live_push_g711(lv, &blk[0][0], 160, TFP_G711_ULAW, n)) return 6;
    if (++tick == mid && print_verdicts(fp_live_verdict(lv, ctx, dur, tol, -1, -1))) return 8;
  }
  fclose(fp[0]);
  fclose(fp[1]);
  if (tick < mid) return 8;
  printf(", \"end\": ");
  if (print_verdicts(fp_live_verdict(lv, ctx, dur, tol, -1, -1))) return 8;
  dur[1] -= 20; /* a duration below what the channel has taken: refused */
  if (fp_live_verdict(lv, ctx, dur, tol, -1, -1) || fp_live_verdict(lv, NULL, dur, tol, -1, -1)) return 9;
  fp_live_close(lv);
  printf(", \"search\": [");
  for (c = 0; c < 2; c++) {
    struct ast_json* arr = fp_search_fingerprint_in_context(ctx[c], argv[7 + c], 1, tol, -1, -1, 1);
    if (!arr) return 10;
    printf("%s", c ? ", " : "");
    if (ast_json_array_size(arr) == 0) {
      printf("null");
    } else {
      printf("{");
      print_clip(ast_json_array_get(arr, 0));
      printf("}");
    }
    ast_json_unref(arr);
  }
  printf("]}\n");
  return fp_term() ? 0 : 5;
}
