// The camera's host-side plane builder (csrc/agx_hull.h) outside the library, for tests/test_camera_cpu.py:
//   * as a shared library (g++ -shared): agx_test_hull_planes / agx_test_grown_bound, called through ctypes and compared with
//     model/cloth.py hull_planes;
//   * as a program (-DPLANES_MAIN, built with -fsanitize=address,undefined): reads a file of hulls -- int32 count, then per hull int32 nv, float32
//     radius, float32[3] centre, float32[nv][3] -- runs both functions over every one and prints the plane total.
#include "agx_hull.h"

#include <stdio.h>
#include <stdlib.h>

extern "C" int agx_test_hull_planes(const float* verts, int nv, double* out4, int cap) {
  std::vector<agxhull::Plane> pl;
  agxhull::hull_planes(verts, nv, pl);
  for (int k = 0; k < (int)pl.size() && k < cap; k++) { out4[4 * k] = pl[k].n[0]; out4[4 * k + 1] = pl[k].n[1]; out4[4 * k + 2] = pl[k].n[2]; out4[4 * k + 3] = pl[k].off; }
  return (int)pl.size();
}

extern "C" double agx_test_grown_bound(const float* verts, int nv, double grow, const double* centre3) {
  std::vector<agxhull::Plane> pl;
  agxhull::hull_planes(verts, nv, pl);
  return agxhull::grown_bound(pl, grow, centre3);
}

#ifdef PLANES_MAIN
int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s hulls.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int count = 0;
  if (fread(&count, 4, 1, f) != 1) { fclose(f); return 2; }
  long total = 0; double radius_sum = 0;
  for (int h = 0; h < count; h++) {
    int nv = 0; float radius = 0, centre[3];
    if (fread(&nv, 4, 1, f) != 1 || fread(&radius, 4, 1, f) != 1 || fread(centre, 4, 3, f) != 3 || nv < 0 || nv > 4096) { fclose(f); return 2; }
    std::vector<float> v((size_t)3 * nv);
    if (nv && fread(v.data(), 4, v.size(), f) != v.size()) { fclose(f); return 2; }
    std::vector<agxhull::Plane> pl;
    agxhull::hull_planes(v.data(), nv, pl);
    const double c[3] = {centre[0], centre[1], centre[2]};
    const double b = agxhull::grown_bound(pl, radius, c);
    total += (long)pl.size(); if (b < 1e30) radius_sum += b;
  }
  fclose(f);
  printf("hulls %d planes %ld bound sum %.6f\n", count, total, radius_sum);
  return 0;
}
#endif
