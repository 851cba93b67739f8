// agx_hull.h -- host side of the camera (csrc/agx_render.hip): the face planes of a collider's convex core, built once when a camera is first set
// on a handle.  Plain C++ without HIP, so that g++ compiles it alone (tests/camera_planes/).  The rule is model/cloth.py hull_planes: the
// outward unit normals and offsets (n.x = off on the face) of the convex hull of the vertices, coplanar facets merged on hull_planes' grid
// (normals to 5 decimals, offsets to 6); a flat or degenerate vertex set becomes its bounding box.  Brute force over vertex triples:
// a collider has at most 64 vertices.
#pragma once
#include <math.h>
#include <vector>

namespace agxhull {

struct Plane { double n[3], off; };

inline void bounding_box(const float* v, int nv, std::vector<Plane>& out) {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int k = 0; k < 3; k++) { lo[k] = hi[k] = nv > 0 ? (double)v[k] : 0.0; }
  for (int i = 1; i < nv; i++) for (int k = 0; k < 3; k++) { const double x = v[3 * i + k]; if (x < lo[k]) lo[k] = x; if (x > hi[k]) hi[k] = x; }
  out.clear();
  for (int k = 0; k < 3; k++) {      // hull_planes' order: +x, -x, +y, -y, +z, -z
    Plane p = {{0, 0, 0}, hi[k]}; p.n[k] = 1; out.push_back(p);
    Plane m = {{0, 0, 0}, -lo[k]}; m.n[k] = -1; out.push_back(m);
  }
}

// thickness of the vertex set: the largest distance of a vertex from the plane through the farthest pair and the vertex farthest from their line
inline double thickness(const float* v, int nv, double* scale_out) {
  auto P = [&](int i, int k) { return (double)v[3 * i + k]; };
  double scale = 0; int a = 0, b = 0;
  for (int i = 0; i < nv; i++) for (int j = i + 1; j < nv; j++) {
    double d = 0; for (int k = 0; k < 3; k++) d += (P(i, k) - P(j, k)) * (P(i, k) - P(j, k));
    if (d > scale) { scale = d; a = i; b = j; }
  }
  scale = sqrt(scale); *scale_out = scale;
  if (!(scale > 0)) return 0;
  double e[3]; for (int k = 0; k < 3; k++) e[k] = (P(b, k) - P(a, k)) / scale;
  double best = 0, nb[3] = {0, 0, 0};
  for (int i = 0; i < nv; i++) {
    double w[3]; for (int k = 0; k < 3; k++) w[k] = P(i, k) - P(a, k);
    const double c[3] = {e[1] * w[2] - e[2] * w[1], e[2] * w[0] - e[0] * w[2], e[0] * w[1] - e[1] * w[0]};
    const double l = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    if (l > best) { best = l; for (int k = 0; k < 3; k++) nb[k] = c[k] / l; }
  }
  if (!(best > 0)) return 0;
  double th = 0;
  for (int i = 0; i < nv; i++) { double s = 0; for (int k = 0; k < 3; k++) s += nb[k] * (P(i, k) - P(a, k)); if (fabs(s) > th) th = fabs(s); }
  return th;
}

// the planes of the hull of nv vertices (float[3] each, body frame)
inline void hull_planes(const float* v, int nv, std::vector<Plane>& out) {
  double scale = 0;
  const double th = nv >= 4 ? thickness(v, nv, &scale) : 0.0;
  if (nv < 4 || !(th > 1e-9 * scale)) { bounding_box(v, nv, out); return; }
  const double tol = 1e-9 * scale;
  out.clear();
  std::vector<long long> keys;      // 4 per plane: the rounded normal and offset
  auto P = [&](int i, int k) { return (double)v[3 * i + k]; };
  for (int i = 0; i < nv; i++) for (int j = i + 1; j < nv; j++) for (int k = j + 1; k < nv; k++) {
    const double a[3] = {P(j, 0) - P(i, 0), P(j, 1) - P(i, 1), P(j, 2) - P(i, 2)}, b[3] = {P(k, 0) - P(i, 0), P(k, 1) - P(i, 1), P(k, 2) - P(i, 2)};
    double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double l = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(l > 1e-12 * scale * scale)) continue;      // collinear
    for (int c = 0; c < 3; c++) n[c] /= l;
    const double off = n[0] * P(i, 0) + n[1] * P(i, 1) + n[2] * P(i, 2);
    bool below = true, above = true;
    for (int m = 0; m < nv && (below || above); m++) {
      const double s = n[0] * P(m, 0) + n[1] * P(m, 1) + n[2] * P(m, 2) - off;
      if (s > tol) below = false;
      if (s < -tol) above = false;
    }
    if (!below && !above) continue;
    Plane p;
    const double sg = below ? 1.0 : -1.0;
    for (int c = 0; c < 3; c++) p.n[c] = sg * n[c];
    p.off = sg * off;
    const long long key[4] = {llround(p.n[0] * 1e5), llround(p.n[1] * 1e5), llround(p.n[2] * 1e5), llround(p.off * 1e6)};
    bool seen = false;
    for (size_t q = 0; q + 3 < keys.size() && !seen; q += 4) seen = keys[q] == key[0] && keys[q + 1] == key[1] && keys[q + 2] == key[2] && keys[q + 3] == key[3];
    if (seen) continue;
    for (int c = 0; c < 4; c++) keys.push_back(key[c]);
    out.push_back(p);
  }
  if (out.size() < 4) bounding_box(v, nv, out);
}

// radius about `centre` of a sphere that holds the polytope {x: n.x <= off + grow for every plane}: the farthest of its vertices (the
// intersections of three planes that satisfy all others); 1e30 where none is found
inline double grown_bound(const std::vector<Plane>& pl, double grow, const double* centre) {
  const int np = (int)pl.size();
  double ext = 0; for (int i = 0; i < np; i++) if (fabs(pl[i].off) + grow > ext) ext = fabs(pl[i].off) + grow;
  const double tol = 1e-9 * (ext > 1e-3 ? ext : 1e-3);
  double best = -1;
  for (int i = 0; i < np; i++) for (int j = i + 1; j < np; j++) for (int k = j + 1; k < np; k++) {
    const double *a = pl[i].n, *b = pl[j].n, *c = pl[k].n;
    const double bc[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    const double det = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2];
    if (fabs(det) < 1e-9) continue;
    const double ca[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
    const double ab[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double d0 = pl[i].off + grow, d1 = pl[j].off + grow, d2 = pl[k].off + grow;
    double x[3]; for (int m = 0; m < 3; m++) x[m] = (d0 * bc[m] + d1 * ca[m] + d2 * ab[m]) / det;
    bool inside = true;
    for (int m = 0; m < np && inside; m++) inside = pl[m].n[0] * x[0] + pl[m].n[1] * x[1] + pl[m].n[2] * x[2] <= pl[m].off + grow + tol;
    if (!inside) continue;
    const double r = sqrt((x[0] - centre[0]) * (x[0] - centre[0]) + (x[1] - centre[1]) * (x[1] - centre[1]) + (x[2] - centre[2]) * (x[2] - centre[2]));
    if (r > best) best = r;
  }
  return best >= 0 ? best : 1e30;
}

}  // namespace agxhull
