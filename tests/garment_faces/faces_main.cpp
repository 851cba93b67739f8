// The camera's host-side triangle-table builder (csrc/agx_garment.h) outside the library, for tests/test_garment_cpu.py:
//   * as a shared library (g++ -shared): agx_test_garment_faces, called through ctypes and compared with the numpy derivation of
//     tests/garment_ref.py;
//   * as a program (-DFACES_MAIN, built with -fsanitize=address,undefined): reads a file of blobs -- int32 count, then per blob int32 nwords,
//     int32 expected face count (-1: the section is malformed and must be refused), int32[nwords] -- runs the builder over every one, on a heap
//     copy of exactly nwords words, and prints the totals.  Exit status 1 when a blob does not meet its expectation.
#include "agx_garment.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// -> face count (the first `cap` faces written to out3), or -1 with the reason in msg
extern "C" int agx_test_garment_faces(const int32_t* words, int nwords, int* out3, int cap, char* msg, int msg_cap) {
  std::vector<int> tris; const char* err = "";
  if (agxgarment::garment_faces(words, (size_t)nwords, tris, &err) != 0) { if (msg && msg_cap > 0) { strncpy(msg, err, (size_t)msg_cap - 1); msg[msg_cap - 1] = 0; } return -1; }
  const int n = (int)(tris.size() / 3);
  for (int k = 0; k < 3 * n && k < 3 * cap; k++) out3[k] = tris[k];
  return n;
}

#ifdef FACES_MAIN
int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s blobs.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int count = 0;
  if (fread(&count, 4, 1, f) != 1) { fclose(f); return 2; }
  long faces = 0; int refused = 0, wrong = 0;
  for (int b = 0; b < count; b++) {
    int nwords = 0, expect = 0;
    if (fread(&nwords, 4, 1, f) != 1 || fread(&expect, 4, 1, f) != 1 || nwords < 0) { fclose(f); return 2; }
    int32_t* w = (int32_t*)malloc((size_t)(nwords ? nwords : 1) * 4);      // exactly the blob: a read beyond it is the sanitizer's to find
    if (!w || (nwords && fread(w, 4, (size_t)nwords, f) != (size_t)nwords)) { free(w); fclose(f); return 2; }
    std::vector<int> tris; const char* err = "";
    const int rc = agxgarment::garment_faces(w, (size_t)nwords, tris, &err);
    free(w);
    const int got = rc ? -1 : (int)(tris.size() / 3);
    if (got != expect) { fprintf(stderr, "blob %d: %d faces (%s), expected %d\n", b, got, err, expect); wrong++; }
    if (rc) refused++; else faces += got;
  }
  fclose(f);
  printf("blobs %d faces %ld refused %d\n", count, faces, refused);
  return wrong ? 1 : 0;
}
#endif
