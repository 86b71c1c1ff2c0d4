/* TEST HARNESS (tests/test_gpu_sliding_aligned_shim.py; not product code): the module's sliding aligned
 * search from C, fp_search_fingerprint_timeline_aligned, on the Asterisk stubs of shim_harness.c
 * (linked in with its main renamed):
 *   shim_sliding_aligned BACKUP_DB COEFS TOL REC_WAV WINDOW HOP MAX_RESULTS NA WAV...
 * enrols the first NA files in context "a" one by one (fp_craete_audio_list_info) and the others in
 * context "b" as one list (fp_create_audio_list_infos), then searches every window of REC_WAV.
 * Prints one JSON line {"all": TL, "a": TL, "b": TL, "nowhere": TL, "long": TL, "bad": TL},
 *   TL = [{"frame": N, "rows": [OBJ, ...]}, ...] | null
 *   OBJ = {uuid, name, context, frame_count, match_count, aligned_count, offset, first_frame,
 *          last_frame, clip_start_frame};
 * "all" without in_context, "a" / "b" / "nowhere" within that context, "long" with a window of
 * 100,000 frames (no full window), "bad" with hop 0. */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"

static int geti(struct ast_json* j, const char* key) { return (int)ast_json_integer_get(ast_json_object_get(j, key)); }

static void print_timeline(const char* key, struct ast_json* tl) {
  size_t w, r;
  printf("\"%s\": ", key);
  if (!tl) {
    printf("null");
    return;
  }
  printf("[");
  for (w = 0; w < ast_json_array_size(tl); w++) {
    struct ast_json* win = ast_json_array_get(tl, w);
    struct ast_json* rows = ast_json_object_get(win, "rows");
    printf("%s{\"frame\": %d, \"rows\": [", w ? ", " : "", geti(win, "frame"));
    for (r = 0; r < ast_json_array_size(rows); r++) {
      struct ast_json* j = ast_json_array_get(rows, r);
      printf("%s{\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"frame_count\": %d, \"match_count\": %d, "
             "\"aligned_count\": %d, \"offset\": %d, \"first_frame\": %d, \"last_frame\": %d, \"clip_start_frame\": %d}",
             r ? ", " : "", ast_json_string_get(ast_json_object_get(j, "uuid")),
             ast_json_string_get(ast_json_object_get(j, "name")), ast_json_string_get(ast_json_object_get(j, "context")),
             geti(j, "frame_count"), geti(j, "match_count"), geti(j, "aligned_count"), geti(j, "offset"),
             geti(j, "first_frame"), geti(j, "last_frame"), geti(j, "clip_start_frame"));
    }
    printf("]}");
  }
  printf("]");
  ast_json_unref(tl);
}

int main(int argc, char** argv) {
  int i, na, coefs, window, hop, k;
  double tol;
  const char* rec;
  if (argc < 10) return 2;
  coefs = atoi(argv[2]);
  tol = atof(argv[3]);
  rec = argv[4];
  window = atoi(argv[5]);
  hop = atoi(argv[6]);
  k = atoi(argv[7]);
  na = atoi(argv[8]);
  if (na < 0 || 9 + na > argc) return 2;
  fpc_set_backup_path(argv[1]);
  if (!fp_init()) return 3;
  for (i = 0; i < na; i++)
    if (!fp_craete_audio_list_info("a", argv[9 + i])) return 4;
  if (fp_create_audio_list_infos("b", (const char* const*)(argv + 9 + na), argc - 9 - na, NULL) != argc - 9 - na) return 4;
  printf("{");
  print_timeline("all", fp_search_fingerprint_timeline_aligned("a", rec, coefs, tol, -1, -1, window, hop, k, false));
  printf(", ");
  print_timeline("a", fp_search_fingerprint_timeline_aligned("a", rec, coefs, tol, -1, -1, window, hop, k, true));
  printf(", ");
  print_timeline("b", fp_search_fingerprint_timeline_aligned("b", rec, coefs, tol, -1, -1, window, hop, k, true));
  printf(", ");
  print_timeline("nowhere", fp_search_fingerprint_timeline_aligned("nowhere", rec, coefs, tol, -1, -1, window, hop, k, true));
  printf(", ");
  print_timeline("long", fp_search_fingerprint_timeline_aligned("a", rec, coefs, tol, -1, -1, 100000, hop, k, false));
  printf(", ");
  print_timeline("bad", fp_search_fingerprint_timeline_aligned("a", rec, coefs, tol, -1, -1, window, 0, k, false));
  printf("}\n");
  return fp_term() ? 0 : 5;
}
