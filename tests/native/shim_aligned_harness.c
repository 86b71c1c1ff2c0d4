/* TEST HARNESS (tests/test_gpu_aligned_shim.py; not product code): the module's aligned search from C,
 * fp_search_fingerprint_aligned beside fp_search_fingerprint_candidates, on the Asterisk stubs of
 * shim_harness.c (linked in with its main renamed):
 *   shim_aligned BACKUP_DB CONTEXT MAX_RESULTS COEFS TOL QUERY_WAV ENROL_WAV...
 * enrols the files, searches QUERY_WAV both ways and prints one JSON line
 *   {"candidates": [OBJ, ...] | null, "aligned": [OBJ + {aligned_count, offset, first_frame, last_frame}, ...] | null}
 *   OBJ = {uuid, name, frame_count, match_count}. */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"

static int geti(struct ast_json* j, const char* key) { return (int)ast_json_integer_get(ast_json_object_get(j, key)); }

static void print_array(struct ast_json* a, bool aligned) {
  size_t r;
  if (!a) {
    printf("null");
    return;
  }
  printf("[");
  for (r = 0; r < ast_json_array_size(a); r++) {
    struct ast_json* j = ast_json_array_get(a, r);
    printf("%s{\"uuid\": \"%s\", \"name\": \"%s\", \"frame_count\": %d, \"match_count\": %d", r ? ", " : "",
           ast_json_string_get(ast_json_object_get(j, "uuid")), ast_json_string_get(ast_json_object_get(j, "name")),
           geti(j, "frame_count"), geti(j, "match_count"));
    if (aligned) {
      if (!ast_json_object_get(j, "aligned_count") || !ast_json_object_get(j, "offset") ||
          !ast_json_object_get(j, "first_frame") || !ast_json_object_get(j, "last_frame"))
        exit(6);
      printf(", \"aligned_count\": %d, \"offset\": %d, \"first_frame\": %d, \"last_frame\": %d", geti(j, "aligned_count"),
             geti(j, "offset"), geti(j, "first_frame"), geti(j, "last_frame"));
    }
    printf("}");
  }
  printf("]");
}

int main(int argc, char** argv) {
  struct ast_json *cand, *al;
  int i;
  if (argc < 8) return 2;
  fpc_set_backup_path(argv[1]);
  if (!fp_init()) return 3;
  for (i = 7; i < argc; i++)
    if (!fp_craete_audio_list_info(argv[2], argv[i])) return 4;
  cand = fp_search_fingerprint_candidates(argv[2], argv[6], atoi(argv[4]), atof(argv[5]), -1, -1, atoi(argv[3]));
  al = fp_search_fingerprint_aligned(argv[2], argv[6], atoi(argv[4]), atof(argv[5]), -1, -1, atoi(argv[3]));
  printf("{\"candidates\": ");
  print_array(cand, false);
  printf(", \"aligned\": ");
  print_array(al, true);
  printf("}\n");
  ast_json_unref(cand);
  ast_json_unref(al);
  return fp_term() ? 0 : 5;
}
