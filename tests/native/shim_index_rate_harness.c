/* TEST HARNESS (tests/test_gpu_index_rate_shim.py; not product code): the module's facade with an index
 * rate, from C, on the Asterisk stubs of shim_harness.c (linked in with its main renamed):
 *   shim_index_rate BACKUP_DB RATE COEFS TOL QUERY_WAV BAD_FILE FILE...
 * calls fp_set_index_rate(RATE) when RATE > 0 (never with 0: the default must be the shim as it was),
 * enrols FILE... into context "ctx" in one fp_create_audio_list_infos scan, tries BAD_FILE both through the
 * scan and through fp_craete_audio_list_info, searches QUERY_WAV, and ends with fp_term, which writes the
 * backup. One JSON line:
 *   {"enrolled": N, "ok": [0 | 1, ...], "bad_scan": N, "bad_single": 0 | 1, "query": OBJ | null}
 * OBJ = {name, context, frame_count, match_count}. */
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "asterisk/json.h"
#include "fp_catalog.h"
#include "fp_handler_tfp.h"
#include "tiresias_fp.h"

static void print_obj(struct ast_json* j) {
  if (!j || !ast_json_object_get(j, "uuid")) {
    printf("null");
    return;
  }
  printf("{\"name\": \"%s\", \"context\": \"%s\", \"frame_count\": %d, \"match_count\": %d}",
         ast_json_string_get(ast_json_object_get(j, "name")), ast_json_string_get(ast_json_object_get(j, "context")),
         (int)ast_json_integer_get(ast_json_object_get(j, "frame_count")),
         (int)ast_json_integer_get(ast_json_object_get(j, "match_count")));
  ast_json_unref(j);
}

int main(int argc, char** argv) {
  int i, rate, coefs, nfiles, enrolled, bad_scan;
  double tol;
  bool* ok;
  bool bad_ok = false, bad_single;
  const char* bad;
  if (argc < 8) return 2;
  rate = atoi(argv[2]);
  coefs = atoi(argv[3]);
  tol = atof(argv[4]);
  bad = argv[6];
  nfiles = argc - 7;
  fpc_set_backup_path(argv[1]);
  if (rate > 0) fp_set_index_rate(rate);
  if (!fp_init()) return 3;
  ok = calloc((size_t)nfiles, sizeof(bool));
  if (!ok) return 3;
  enrolled = fp_create_audio_list_infos("ctx", (const char* const*)(argv + 7), nfiles, ok);
  printf("{\"enrolled\": %d, \"ok\": [", enrolled);
  for (i = 0; i < nfiles; i++) printf("%s%d", i ? ", " : "", ok[i] ? 1 : 0);
  free(ok);
  bad_scan = fp_create_audio_list_infos("ctx", &bad, 1, &bad_ok);
  bad_single = fp_craete_audio_list_info("ctx", bad);
  printf("], \"bad_scan\": %d, \"bad_single\": %d, \"query\": ", bad_scan + (bad_ok ? 1 : 0), bad_single ? 1 : 0);
  print_obj(fp_search_fingerprint_info("ctx", argv[5], coefs, tol, -1, -1));
  printf("}\n");
  return fp_term() ? 0 : 5;
}
