/* TEST HARNESS (tests/test_gpu_ranked_shim.py; not product code): the module's ranked search from C,
 * fp_search_fingerprint_candidates beside fp_search_fingerprint_info, on the Asterisk stubs of
 * shim_harness.c (linked in with its main renamed):
 *   shim_ranked BACKUP_DB CONTEXT MAX_RESULTS COEFS TOL QUERY_WAV ENROL_WAV...
 * enrols the files, searches QUERY_WAV both ways and prints one JSON line
 *   {"info": OBJ | null, "candidates": [OBJ, ...] | null}   OBJ = {uuid, name, frame_count, match_count}. */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"

static void print_obj(struct ast_json* j) {
  if (!j) {
    printf("null");
    return;
  }
  printf("{\"uuid\": \"%s\", \"name\": \"%s\", \"frame_count\": %d, \"match_count\": %d}",
         ast_json_string_get(ast_json_object_get(j, "uuid")), ast_json_string_get(ast_json_object_get(j, "name")),
         (int)ast_json_integer_get(ast_json_object_get(j, "frame_count")),
         (int)ast_json_integer_get(ast_json_object_get(j, "match_count")));
}

int main(int argc, char** argv) {
  struct ast_json *info, *cand;
  size_t r;
  int i;
  if (argc < 8) return 2;
  fpc_set_backup_path(argv[1]);
  if (!fp_init()) return 3;
  for (i = 7; i < argc; i++)
    if (!fp_craete_audio_list_info(argv[2], argv[i])) return 4;
  info = fp_search_fingerprint_info(argv[2], argv[6], atoi(argv[4]), atof(argv[5]), -1, -1);
  cand = fp_search_fingerprint_candidates(argv[2], argv[6], atoi(argv[4]), atof(argv[5]), -1, -1, atoi(argv[3]));
  printf("{\"info\": ");
  print_obj(info);
  printf(", \"candidates\": ");
  if (!cand) {
    printf("null");
  } else {
    printf("[");
    for (r = 0; r < ast_json_array_size(cand); r++) {
      if (r) printf(", ");
      print_obj(ast_json_array_get(cand, r));
    }
    printf("]");
  }
  printf("}\n");
  ast_json_unref(info);
  ast_json_unref(cand);
  return fp_term() ? 0 : 5;
}
