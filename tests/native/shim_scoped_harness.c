/* TEST HARNESS (tests/test_gpu_scoped_shim.py; not product code): the module's context-scoped search
 * from C, fp_search_fingerprint_in_context beside fp_search_fingerprint_candidates, on the Asterisk
 * stubs of shim_harness.c (linked in with its main renamed):
 *   shim_scoped BACKUP_DB COEFS TOL QUERY_WAV NA WAV...
 * enrols the first NA files in context "a" one by one (fp_craete_audio_list_info) and the others in
 * context "b" as one list (fp_create_audio_list_infos), searches QUERY_WAV, restarts the module
 * (fp_term, fp_init: the index and the scopes come back from the backup file) and searches again.
 * Prints one JSON line {"before": SET, "after": SET},
 *   SET = {"all": ROWS, "a": ROWS, "b": ROWS, "nowhere": ROWS}   ROWS = [OBJ, ...] | null
 *   OBJ = {uuid, name, context, frame_count, match_count}. */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"

static void print_rows(const char* key, struct ast_json* rows) {
  size_t r;
  printf("\"%s\": ", key);
  if (!rows) {
    printf("null");
    return;
  }
  printf("[");
  for (r = 0; r < ast_json_array_size(rows); r++) {
    struct ast_json* j = ast_json_array_get(rows, r);
    printf("%s{\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"frame_count\": %d, \"match_count\": %d}",
           r ? ", " : "", ast_json_string_get(ast_json_object_get(j, "uuid")),
           ast_json_string_get(ast_json_object_get(j, "name")), ast_json_string_get(ast_json_object_get(j, "context")),
           (int)ast_json_integer_get(ast_json_object_get(j, "frame_count")),
           (int)ast_json_integer_get(ast_json_object_get(j, "match_count")));
  }
  printf("]");
  ast_json_unref(rows);
}

static void print_set(const char* key, const char* q, int coefs, double tol) {
  printf("\"%s\": {", key);
  print_rows("all", fp_search_fingerprint_candidates("a", q, coefs, tol, -1, -1, 32));
  printf(", ");
  print_rows("a", fp_search_fingerprint_in_context("a", q, coefs, tol, -1, -1, 32));
  printf(", ");
  print_rows("b", fp_search_fingerprint_in_context("b", q, coefs, tol, -1, -1, 32));
  printf(", ");
  print_rows("nowhere", fp_search_fingerprint_in_context("nowhere", q, coefs, tol, -1, -1, 32));
  printf("}");
}

int main(int argc, char** argv) {
  int i, na, coefs;
  double tol;
  if (argc < 7) return 2;
  coefs = atoi(argv[2]);
  tol = atof(argv[3]);
  na = atoi(argv[5]);
  if (na < 0 || 6 + na > argc) return 2;
  fpc_set_backup_path(argv[1]);
  if (!fp_init()) return 3;
  for (i = 0; i < na; i++)
    if (!fp_craete_audio_list_info("a", argv[6 + i])) return 4;
  if (fp_create_audio_list_infos("b", (const char* const*)(argv + 6 + na), argc - 6 - na, NULL) != argc - 6 - na) return 4;
  printf("{");
  print_set("before", argv[4], coefs, tol);
  if (!fp_term()) return 5;
  if (!fp_init()) return 6;
  printf(", ");
  print_set("after", argv[4], coefs, tol);
  printf("}\n");
  return fp_term() ? 0 : 5;
}
