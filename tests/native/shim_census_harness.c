/* TEST HARNESS (tests/test_gpu_census_shim.py; not product code): the module's match census from C,
 * fp_search_fingerprint_census beside fp_search_fingerprint_in_context, on the Asterisk stubs of
 * shim_harness.c (linked in with its main renamed):
 *   shim_census BACKUP_DB COEFS TOL QUERY_WAV NA WAV...
 * enrols the first NA files in context "a" and the others in context "b", and prints one JSON line
 *   {"a": CENSUS, "b": CENSUS, "nowhere": CENSUS}   CENSUS = null |
 *   {"winner": OBJ | null, "first": OBJ | null, "frame_count", "population", "clips_at_or_above", "clips_tied",
 *    "histogram": [[count, clips], ...]}
 * "first" being fp_search_fingerprint_in_context's first object; OBJ = {uuid, name, context, frame_count, match_count}. */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"

static void print_obj(struct ast_json* j) {
  if (!j || !ast_json_object_get(j, "uuid")) {
    printf("null");
    return;
  }
  printf("{\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"frame_count\": %d, \"match_count\": %d}",
         ast_json_string_get(ast_json_object_get(j, "uuid")), ast_json_string_get(ast_json_object_get(j, "name")),
         ast_json_string_get(ast_json_object_get(j, "context")), (int)ast_json_integer_get(ast_json_object_get(j, "frame_count")),
         (int)ast_json_integer_get(ast_json_object_get(j, "match_count")));
}

static void print_census(const char* ctx, const char* q, int coefs, double tol) {
  struct ast_json* c = fp_search_fingerprint_census(ctx, q, coefs, tol, -1, -1);
  struct ast_json* rows = fp_search_fingerprint_in_context(ctx, q, coefs, tol, -1, -1, 1);
  struct ast_json* h;
  size_t i;
  printf("\"%s\": ", ctx);
  if (!c) {
    printf("null");
    if (rows) ast_json_unref(rows);
    return;
  }
  printf("{\"winner\": ");
  print_obj(ast_json_object_get(c, "winner"));
  printf(", \"first\": ");
  print_obj(rows && ast_json_array_size(rows) ? ast_json_array_get(rows, 0) : NULL);
  printf(", \"frame_count\": %d, \"population\": %d, \"clips_at_or_above\": %d, \"clips_tied\": %d, \"histogram\": [",
         (int)ast_json_integer_get(ast_json_object_get(c, "frame_count")),
         (int)ast_json_integer_get(ast_json_object_get(c, "population")),
         (int)ast_json_integer_get(ast_json_object_get(c, "clips_at_or_above")),
         (int)ast_json_integer_get(ast_json_object_get(c, "clips_tied")));
  h = ast_json_object_get(c, "histogram");
  for (i = 0; i < ast_json_array_size(h); i++) {
    struct ast_json* b = ast_json_array_get(h, i);
    printf("%s[%d, %d]", i ? ", " : "", (int)ast_json_integer_get(ast_json_array_get(b, 0)),
           (int)ast_json_integer_get(ast_json_array_get(b, 1)));
  }
  printf("]}");
  ast_json_unref(c);
  if (rows) ast_json_unref(rows);
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
  print_census("a", argv[4], coefs, tol);
  printf(", ");
  print_census("b", argv[4], coefs, tol);
  printf(", ");
  print_census("nowhere", argv[4], coefs, tol);
  printf("}\n");
  if (fp_search_fingerprint_census("a", argv[4], 3, tol, -1, -1) != NULL) return 7; /* coefs outside [1, 2] */
  if (fp_search_fingerprint_census("a", NULL, coefs, tol, -1, -1) != NULL) return 7;
  return fp_term() ? 0 : 5;
}
