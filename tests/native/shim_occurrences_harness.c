/* TEST HARNESS (tests/test_gpu_occurrences_shim.py; not product code): the module's occurrence search
 * from C, fp_search_fingerprint_occurrences, on the Asterisk stubs of shim_harness.c (linked in with
 * its main renamed):
 *   shim_occurrences BACKUP_DB COEFS TOL REC_WAV WINDOW HOP K MAX_GAP MIN_HITS NA WAV...
 * enrols the first NA files in context "a" one by one (fp_craete_audio_list_info) and the others in
 * context "b" as one list (fp_create_audio_list_infos), then searches REC_WAV.
 * Prints one JSON line {"a": L, "b": L, "nowhere": L, "long": L, "bad": L, "strict": L},
 *   L = [OBJ, ...] | null
 *   OBJ = {uuid, name, context, frame_count, match_count, clip_start_frame, first_frame, last_frame,
 *          hits, diagonal_hits, overlap, windows};
 * "a" / "b" / "nowhere" within that context, "long" with a window of 100,000 frames (no full window),
 * "bad" with min_hits 0, "strict" within "a" with min_hits 100,000 (nothing reaches it). */
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"

static int geti(struct ast_json* j, const char* key) { return (int)ast_json_integer_get(ast_json_object_get(j, key)); }

static void print_list(const char* key, struct ast_json* l) {
  size_t r;
  printf("\"%s\": ", key);
  if (!l) {
    printf("null");
    return;
  }
  printf("[");
  for (r = 0; r < ast_json_array_size(l); r++) {
    struct ast_json* j = ast_json_array_get(l, r);
    printf("%s{\"uuid\": \"%s\", \"name\": \"%s\", \"context\": \"%s\", \"frame_count\": %d, \"match_count\": %d, "
           "\"clip_start_frame\": %d, \"first_frame\": %d, \"last_frame\": %d, \"hits\": %d, \"diagonal_hits\": %d, "
           "\"overlap\": %d, \"windows\": %d}",
           r ? ", " : "", ast_json_string_get(ast_json_object_get(j, "uuid")),
           ast_json_string_get(ast_json_object_get(j, "name")), ast_json_string_get(ast_json_object_get(j, "context")),
           geti(j, "frame_count"), geti(j, "match_count"), geti(j, "clip_start_frame"), geti(j, "first_frame"),
           geti(j, "last_frame"), geti(j, "hits"), geti(j, "diagonal_hits"), geti(j, "overlap"), geti(j, "windows"));
  }
  printf("]");
  ast_json_unref(l);
}

int main(int argc, char** argv) {
  int i, na, coefs, window, hop, k, gap, hits;
  double tol;
  const char* rec;
  if (argc < 12) return 2;
  coefs = atoi(argv[2]);
  tol = atof(argv[3]);
  rec = argv[4];
  window = atoi(argv[5]);
  hop = atoi(argv[6]);
  k = atoi(argv[7]);
  gap = atoi(argv[8]);
  hits = atoi(argv[9]);
  na = atoi(argv[10]);
  if (na < 0 || 11 + na > argc) return 2;
  fpc_set_backup_path(argv[1]);
  if (!fp_init()) return 3;
  for (i = 0; i < na; i++)
    if (!fp_craete_audio_list_info("a", argv[11 + i])) return 4;
  if (fp_create_audio_list_infos("b", (const char* const*)(argv + 11 + na), argc - 11 - na, NULL) != argc - 11 - na) return 4;
  printf("{");
  print_list("a", fp_search_fingerprint_occurrences("a", rec, coefs, tol, -1, -1, window, hop, k, gap, hits));
  printf(", ");
  print_list("b", fp_search_fingerprint_occurrences("b", rec, coefs, tol, -1, -1, window, hop, k, gap, hits));
  printf(", ");
  print_list("nowhere", fp_search_fingerprint_occurrences("nowhere", rec, coefs, tol, -1, -1, window, hop, k, gap, hits));
  printf(", ");
  print_list("long", fp_search_fingerprint_occurrences("a", rec, coefs, tol, -1, -1, 100000, hop, k, gap, hits));
  printf(", ");
  print_list("bad", fp_search_fingerprint_occurrences("a", rec, coefs, tol, -1, -1, window, hop, k, gap, 0));
  printf(", ");
  print_list("strict", fp_search_fingerprint_occurrences("a", rec, coefs, tol, -1, -1, window, hop, k, gap, 100000));
  printf("}\n");
  return fp_term() ? 0 : 5;
}
