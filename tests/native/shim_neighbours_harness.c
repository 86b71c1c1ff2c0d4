/* TEST HARNESS (tests/test_gpu_neighbours_shim.py; not product code): the module's catalog neighbours
 * from C, fp_get_audio_list_neighbours and fp_get_audio_neighbours, on the Asterisk stubs of
 * shim_harness.c (linked in with its main renamed):
 *   shim_neighbours BACKUP_DB COEFS TOL K NA WAV...
 * enrols the first NA files in context "a" and the others in context "b" (fp_create_audio_list_infos),
 * asks for both contexts' neighbours, for a context nobody has and for the first audio of "b" across all
 * contexts, and ends the module (fp_term writes BACKUP_DB, which the Python mirror then loads: the same
 * uuids). Prints one JSON line
 *   {"a": LIST, "b": LIST, "nowhere": LIST, "one": AUDIO | null, "calls": [after a, after b, after one], "bad": N}
 *   LIST = [AUDIO, ...] | null    AUDIO = {uuid, name, context, hash, frame_count, neighbours: [ROW, ...]}
 *   ROW = {uuid, name, context, hash, match_count, aligned_count, offset, first_frame, last_frame};
 * calls: fp_get_neighbour_stats since fp_init; bad: how many of the bad-argument calls returned non-NULL. */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"

static void print_fields(struct ast_json* j) {
  printf("\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"hash\": \"%s\"",
         ast_json_string_get(ast_json_object_get(j, "uuid")), ast_json_string_get(ast_json_object_get(j, "name")),
         ast_json_string_get(ast_json_object_get(j, "context")), ast_json_string_get(ast_json_object_get(j, "hash")));
}

static void print_audio(struct ast_json* j) {
  static const char* const keys[] = {"match_count", "aligned_count", "offset", "first_frame", "last_frame"};
  struct ast_json* rows;
  size_t r, f;
  if (!j) {
    printf("null");
    return;
  }
  rows = ast_json_object_get(j, "neighbours");
  printf("{");
  print_fields(j);
  printf(", \"frame_count\": %d, \"neighbours\": [", (int)ast_json_integer_get(ast_json_object_get(j, "frame_count")));
  for (r = 0; r < ast_json_array_size(rows); r++) {
    struct ast_json* row = ast_json_array_get(rows, r);
    printf("%s{", r ? ", " : "");
    print_fields(row);
    for (f = 0; f < sizeof(keys) / sizeof(keys[0]); f++)
      printf(", \"%s\": %d", keys[f], (int)ast_json_integer_get(ast_json_object_get(row, keys[f])));
    printf("}");
  }
  printf("]}");
}

static void print_list(const char* key, struct ast_json* list) {
  size_t a;
  printf("\"%s\": ", key);
  if (!list) {
    printf("null");
    return;
  }
  printf("[");
  for (a = 0; a < ast_json_array_size(list); a++) {
    printf("%s", a ? ", " : "");
    print_audio(ast_json_array_get(list, a));
  }
  printf("]");
  ast_json_unref(list);
}

int main(int argc, char** argv) {
  int na, coefs, k, bad = 0;
  double tol;
  int64_t calls[3] = {-1, -1, -1};
  struct ast_json* j;
  char first_b[64] = "";
  if (argc < 7) return 2;
  coefs = atoi(argv[2]);
  tol = atof(argv[3]);
  k = atoi(argv[4]);
  na = atoi(argv[5]);
  if (na < 0 || 6 + na > argc) return 2;
  fpc_set_backup_path(argv[1]);
  if (!fp_init()) return 3;
  if (fp_create_audio_list_infos("a", (const char* const*)(argv + 6), na, NULL) != na) return 4;
  if (fp_create_audio_list_infos("b", (const char* const*)(argv + 6 + na), argc - 6 - na, NULL) != argc - 6 - na) return 4;
  j = fp_get_audio_lists_by_contextname("b");
  if (j && ast_json_array_size(j) > 0)
    snprintf(first_b, sizeof first_b, "%s", ast_json_string_get(ast_json_object_get(ast_json_array_get(j, 0), "uuid")));
  ast_json_unref(j);
  printf("{");
  print_list("a", fp_get_audio_list_neighbours("a", coefs, tol, -1, -1, k));
  fp_get_neighbour_stats(&calls[0]);
  printf(", ");
  print_list("b", fp_get_audio_list_neighbours("b", coefs, tol, -1, -1, k));
  fp_get_neighbour_stats(&calls[1]);
  printf(", ");
  print_list("nowhere", fp_get_audio_list_neighbours("nowhere", coefs, tol, -1, -1, k));
  printf(", \"one\": ");
  j = first_b[0] ? fp_get_audio_neighbours(first_b, coefs, tol, -1, -1, k) : NULL;
  print_audio(j);
  ast_json_unref(j);
  fp_get_neighbour_stats(&calls[2]);
  bad += fp_get_audio_list_neighbours(NULL, coefs, tol, -1, -1, k) != NULL;
  bad += fp_get_audio_list_neighbours("a", 3, tol, -1, -1, k) != NULL;
  bad += fp_get_audio_list_neighbours("a", coefs, tol, -1, -1, 0) != NULL;
  bad += fp_get_audio_neighbours(NULL, coefs, tol, -1, -1, k) != NULL;
  bad += fp_get_audio_neighbours("no-such-uuid", coefs, tol, -1, -1, k) != NULL;
  printf(", \"calls\": [%lld, %lld, %lld], \"bad\": %d}\n", (long long)calls[0], (long long)calls[1], (long long)calls[2], bad);
  return fp_term() ? 0 : 5;
}
