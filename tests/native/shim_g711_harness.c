/* TEST HARNESS (tests/test_gpu_g711_shim.py; not product code): G.711 through the module's facade
 * from C, on the Asterisk stubs of shim_harness.c (linked in with its main renamed):
 *   shim_g711 BACKUP_DB COEFS TOL LAW CODES_FILE RECORDING_WAV FILE...
 * enrols FILE... (WAVs of any kind and headerless .ulaw / .alaw files) into context "ctx" in one
 * fp_create_audio_list_infos scan, searches each file by itself, then pushes the raw codes of
 * CODES_FILE (law LAW) into a live channel in 160-byte frames with fp_channel_push_g711 and searches
 * it, beside fp_search_fingerprint_info of RECORDING_WAV (the same audio expanded). One JSON line:
 *   {"files": [OBJ | null, ...], "channel": OBJ | null, "recording": OBJ | null}
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
  int i, coefs, law, nfiles;
  double tol;
  bool* ok;
  FILE* fp;
  uint8_t frame[160];
  size_t got;
  fp_channel* ch;
  if (argc < 8) return 2;
  coefs = atoi(argv[2]);
  tol = atof(argv[3]);
  law = atoi(argv[4]);
  nfiles = argc - 7;
  fpc_set_backup_path(argv[1]);
  if (!fp_init()) return 3;
  ok = calloc((size_t)nfiles, sizeof(bool));
  if (!ok) return 3;
  if (fp_create_audio_list_infos("ctx", (const char* const*)(argv + 7), nfiles, ok) != nfiles) return 4;
  for (i = 0; i < nfiles; i++)
    if (!ok[i]) return 4;
  free(ok);
  printf("{\"files\": [");
  for (i = 0; i < nfiles; i++) {
    printf("%s", i ? ", " : "");
    print_obj(fp_search_fingerprint_info("ctx", argv[7 + i], coefs, tol, -1, -1));
  }
  printf("], \"channel\": ");
  ch = fp_channel_open(8000, 10000);
  if (!ch) return 5;
  if (fp_channel_push_g711(ch, frame, 160, 2) || fp_channel_push_g711(ch, NULL, 160, law) ||
      fp_channel_push_g711(NULL, frame, 160, law) || !fp_channel_push_g711(ch, NULL, 0, law))
    return 7; /* a bad law, a NULL payload and a NULL channel are refused; an empty push is fine */
  fp = fopen(argv[5], "rb");
  if (!fp) return 6;
  while ((got = fread(frame, 1, sizeof frame, fp)) > 0)
    if (!fp_channel_push_g711(ch, frame, (int)got, law)) return 6;
  fclose(fp);
  print_obj(fp_channel_search(ch, "ctx", coefs, tol, -1, -1));
  fp_channel_close(ch);
  printf(", \"recording\": ");
  print_obj(fp_search_fingerprint_info("ctx", argv[6], coefs, tol, -1, -1));
  printf("}\n");
  return fp_term() ? 0 : 5;
}
