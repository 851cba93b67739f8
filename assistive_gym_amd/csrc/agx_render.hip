// agx_render.hip -- the camera's ray caster behind agx_render (include/agx.h): depth, segmentation and RGB of the collision geometry, one ray per
// pixel.  Variant independent: it reads the model blob, the collider frames the variant's frames kernel left ([n_envs][ncoll][12], agx_kernels.hip)
// and the tables agx_camera_set built on the host (face planes of the hulls, visibility per gender, bounding radii: agx_render.h, agx_hull.h).
//
// One workgroup = one wavefront = one 16 x 4 tile of one environment's image.
//   1. Cull: the lanes test the bounding spheres of the colliders (and water particles), 64 per round, against the cone around the tile's rays;
//      a ballot and a prefix count compact the survivors, in index order, into a list in LDS.
//   2. Cast: one lane per pixel walks the list.  The list entry is wave uniform, so the collider record, its frame and a hull's planes come
//      through scalar loads, once per wave; what differs per lane is the ray direction.  The ray goes into the body frame; spheres and capsules
//      are solved in closed form about the point of the ray closest to them (short vectors: no cancellation against the camera distance), hulls
//      by a slab test over their planes, after a vote: a collider whose bounding sphere no ray of the wave comes near is skipped by the whole
//      wave (at policy sizes a tile's cone is wide and most of its list falls here).  A convex collider meets the ray in an interval [t_in, t_out]; its hit is t_in, or t_out where t_in
//      lies before the near plane; the nearest hit within [near, far] wins, the lower index on a tie (the list is ascending, the test strict).
//   3. Shade and write: 4-byte stores, consecutive lanes on consecutive pixels of a row.
// The ray direction is not normalised -- its component along the view direction is 1 -- so the ray parameter is the view-space depth.
// The garment of a dressing scene is drawn over these images by a second kernel on the same tiles, agx_render_garment_kernel below.
#include "agx_wave.h"
#include "agx_math.h"
#include "agx_render.h"
#include "../../include/agx_blob.h"

namespace {

// the hit of the interval [t_in, t_out] (t_in <= t_out) inside [near, far]: 0 none, 1 t_in, 2 t_out
AGX_DEV int pick_hit(float t_in, float t_out, float near, float far) {
  if (t_in >= near) return t_in <= far ? 1 : 0;
  return (t_out >= near && t_out <= far) ? 2 : 0;
}

// sphere of radius r about the origin, ray m + s d with m the ray's point closest to the origin (m . d = 0): half length of the chord, < 0 = miss
AGX_DEV float sphere_half(v3 m, float r, float inv_dd) {
  const float h = (r * r - dot(m, m)) * inv_dd;
  return h >= 0.f ? sqrtf(h) : -1.f;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(64)
agx_render_kernel(const agx_render_args A) {
  __shared__ int list[AGX_RENDER_LIST];
  const int lane = (int)threadIdx.x;
  const int* bi = (const int*)A.blob; const float* bf = (const float*)A.blob;
  const int ncoll = bi[AGX_H_NCOLL], o_coll = bi[AGX_H_OFF_COLL], o_vert = bi[AGX_H_OFF_VERT];
  const int tiles_x = (A.width + AGX_RENDER_TW - 1) / AGX_RENDER_TW;
  const int x0 = ((int)blockIdx.x % tiles_x) * AGX_RENDER_TW, y0 = ((int)blockIdx.x / tiles_x) * AGX_RENDER_TH;
  const int env = A.env0 + (int)blockIdx.y;
  const int gender_bit = 1 << (((const int*)A.state)[(size_t)env * A.sw + bi[AGX_H_S_ENV] + AGX_E_GENDER] == 1 ? 1 : 0);
  const float* frames = A.frames + (size_t)env * ncoll * 12;
  const float* water = A.water ? A.water + (size_t)env * A.cloth_words : nullptr;
  const v3 eye = mk3(A.eye[0], A.eye[1], A.eye[2]), right = mk3(A.right[0], A.right[1], A.right[2]), up = mk3(A.up[0], A.up[1], A.up[2]),
           fwd = mk3(A.fwd[0], A.fwd[1], A.fwd[2]);
  const float sx = 2.f * A.tx / (float)A.width, sy = 2.f * A.ty / (float)A.height;

  // ---- 1. cull against the cone around the tile: axis through the tile's middle, opening to its farthest corner
  int n = 0;
  {
    const int x1 = x0 + AGX_RENDER_TW < A.width ? x0 + AGX_RENDER_TW : A.width, y1 = y0 + AGX_RENDER_TH < A.height ? y0 + AGX_RENDER_TH : A.height;
    const float ul = (float)x0 * sx - A.tx, ur = (float)x1 * sx - A.tx, vt = A.ty - (float)y0 * sy, vb = A.ty - (float)y1 * sy;
    v3 axis = 0.5f * (ul + ur) * right + 0.5f * (vt + vb) * up + fwd;
    axis = (1.f / sqrtf(dot(axis, axis))) * axis;
    float cos_t = 1.f;
    for (int k = 0; k < 4; k++) {
      const v3 c = (k & 1 ? ur : ul) * right + (k & 2 ? vb : vt) * up + fwd;
      cos_t = fminf(cos_t, dot(c, axis) / sqrtf(dot(c, c)));
    }
    cos_t = fmaxf(cos_t - 1e-6f, 0.f);
    const float sin_t = sqrtf(1.f - cos_t * cos_t);
    const int total = ncoll + A.npart;
    for (int base = 0; base < total; base += 64) {
      const int idx = base + lane;
      bool keep = false;
      if (idx < total) {
        v3 cw; float r;
        if (idx < ncoll) {
          const float* F = frames + 12 * idx; const float* C = bf + o_coll + AGX_C_STRIDE * idx;
          const m3 R = ldm3(F + 3);
          cw = mul(R, ld3(C + AGX_C_AABB_C)) + ld3(F);
          const agx_render_coll rc = A.coll[idx];
          r = rc.bound; keep = (rc.genders & gender_bit) != 0;
        } else { cw = ld3(water + 3 * (idx - ncoll)); r = A.part_radius; keep = true; }
        // distance of the centre from the cone's surface (negative inside); behind the apex it underestimates, which only keeps more
        const v3 v = cw - eye; const float along = dot(v, axis); const v3 cr = cross(v, axis);
        keep = keep && sqrtf(dot(cr, cr)) * cos_t - along * sin_t <= r * 1.0001f + 1e-4f;
      }
      const uint64_t m = wave_ballot(keep);
      if (keep) list[n + wave_rank(m)] = idx;
      n += popc64(m);
    }
  }
  wave_sync();

  // ---- 2. cast
  const int px = x0 + (lane & (AGX_RENDER_TW - 1)), py = y0 + lane / AGX_RENDER_TW;
  const float cx = ((float)px + 0.5f) * sx - A.tx, cy = A.ty - ((float)py + 0.5f) * sy;
  const v3 dw = cx * right + cy * up + fwd;
  const float dd = dot(dw, dw), inv_dd = 1.f / dd;
  const float near = A.near, far = A.far;
  float best_t = 3.0e38f; int best = -1; v3 best_n = mk3(0.f, 0.f, 0.f);      // the normal in the frame of the collider's body
  for (int k = 0; k < n; k++) {
    const int idx = wave_uniform(list[k]);
    if (idx >= ncoll) {      // a water particle: a sphere in world coordinates
      const v3 oc = eye - ld3(water + 3 * (idx - ncoll));
      const float t0 = -dot(oc, dw) * inv_dd; const v3 m = oc + t0 * dw;
      const float s = sphere_half(m, A.part_radius, inv_dd);
      const int hit = s >= 0.f ? pick_hit(t0 - s, t0 + s, near, far) : 0;
      const float t = hit == 1 ? t0 - s : t0 + s;
      if (hit && t < best_t) { best_t = t; best = idx; best_n = (1.f / A.part_radius) * (m + (t - t0) * dw); }
      continue;
    }
    const float* F = frames + 12 * idx; const int* Ci = bi + o_coll + AGX_C_STRIDE * idx; const float* Cf = bf + o_coll + AGX_C_STRIDE * idx;
    const m3 R = ldm3(F + 3);
    const v3 ob = tmul(R, eye - ld3(F)), d = tmul(R, dw);
    const agx_render_coll rc = A.coll[idx];
    {      // no ray of this tile within the collider's bounding sphere (the cone of the cull is wider than the tile): the wave skips it
      const v3 oc = ob - ld3(Cf + AGX_C_AABB_C);
      const v3 m = oc - (dot(oc, d) * inv_dd) * d;
      const float reach = rc.bound * 1.0001f + 1e-4f;
      if (!wave_any(dot(m, m) <= reach * reach)) continue;
    }
    const int nv = Ci[AGX_C_NVERT]; const float rad = Cf[AGX_C_RADIUS];
    const float* V = bf + o_vert + 3 * Ci[AGX_C_VOFF];
    if (nv == 1) {
      const v3 oc = ob - ld3(V);
      const float t0 = -dot(oc, d) * inv_dd; const v3 m = oc + t0 * d;
      const float s = sphere_half(m, rad, inv_dd);
      const int hit = s >= 0.f ? pick_hit(t0 - s, t0 + s, near, far) : 0;
      const float t = hit == 1 ? t0 - s : t0 + s;
      if (hit && t < best_t) { best_t = t; best = idx; best_n = (1.f / rad) * (m + (t - t0) * d); }
    } else if (nv == 2) {
      // capsule = two spheres and the cylinder between them; the ray meets their union in one interval
      const v3 va = ld3(V), vb = ld3(V + 3);
      const v3 hv = 0.5f * (vb - va), oc = ob - 0.5f * (va + vb);      // half axis; ray origin relative to the capsule's middle
      const float t0 = -dot(oc, d) * inv_dd; const v3 o = oc + t0 * d;      // ... moved to the point closest to the middle
      float t_in = 3.0e38f, t_out = -3.0e38f;
      for (int e = 0; e < 2; e++) {
        const v3 oe = e ? o - hv : o + hv;      // relative to the end's centre
        const float te = -dot(oe, d) * inv_dd; const v3 m = oe + te * d;
        const float s = sphere_half(m, rad, inv_dd);
        if (s >= 0.f) { t_in = fminf(t_in, te - s); t_out = fmaxf(t_out, te + s); }
      }
      const float hh = dot(hv, hv);
      if (hh > 0.f) {
        const float hd = dot(hv, d), ho = dot(hv, o);
        const float a = hh * dd - hd * hd, b = hh * dot(o, d) - ho * hd, c = hh * dot(o, o) - ho * ho - rad * rad * hh;
        float lo = -3.0e38f, hi = 3.0e38f; bool ok = true;
        if (a > 1e-12f * hh * dd) { const float h = b * b - a * c; ok = h >= 0.f; const float s = sqrtf(fmaxf(h, 0.f)); lo = (-b - s) / a; hi = (-b + s) / a; }
        else ok = c <= 0.f;
        // between the end planes: |ho + t hd| <= hh
        if (hd != 0.f) { const float ta = (-hh - ho) / hd, tb = (hh - ho) / hd; lo = fmaxf(lo, fminf(ta, tb)); hi = fminf(hi, fmaxf(ta, tb)); }
        else ok = ok && fabsf(ho) <= hh;
        if (ok && lo <= hi) { t_in = fminf(t_in, lo); t_out = fmaxf(t_out, hi); }
      }
      const int hit = t_in <= t_out ? pick_hit(t0 + t_in, t0 + t_out, near, far) : 0;
      const float ts = hit == 1 ? t_in : t_out, t = t0 + ts;
      if (hit && t < best_t) {
        const v3 x = o + ts * d;
        const float u = hh > 0.f ? wave_clamp(dot(x, hv) / hh, -1.f, 1.f) : 0.f;
        best_t = t; best = idx; best_n = (1.f / rad) * (x - u * hv);
      }
    } else {
      const v3 o = ob - ld3(Cf + AGX_C_AABB_C);
      float t_in = -3.0e38f, t_out = 3.0e38f; int p_in = rc.plane0, p_out = rc.plane0; bool outside = false;
      for (int p = rc.plane0; p < rc.plane0 + rc.nplane; p++) {
        const float4 P = A.planes[p];
        const float den = P.x * d.x + P.y * d.y + P.z * d.z, num = P.w - (P.x * o.x + P.y * o.y + P.z * o.z);
        const float t = num * __builtin_amdgcn_rcpf(den);
        if (den < 0.f && t > t_in) { t_in = t; p_in = p; }
        if (den > 0.f && t < t_out) { t_out = t; p_out = p; }
        outside = outside || (den == 0.f && num < 0.f);
      }
      const int hit = (!outside && t_in <= t_out) ? pick_hit(t_in, t_out, near, far) : 0;
      const float t = hit == 1 ? t_in : t_out;
      if (hit && t < best_t) { const float4 P = A.planes[hit == 1 ? p_in : p_out]; best_t = t; best = idx; best_n = mk3(P.x, P.y, P.z); }
    }
  }

  // ---- 3. shade and write
  if (px >= A.width || py >= A.height) return;
  const size_t pix = ((size_t)blockIdx.y * A.height + py) * A.width + px;
  if (A.depth) A.depth[pix] = best >= 0 ? best_t : far;
  if (A.seg) A.seg[pix] = best;
  if (A.rgba) {
    int ci = AGX_COLOUR_BACKGROUND; float shade = 1.f;
    if (best >= 0) {
      v3 nw = best_n;
      if (best < ncoll) {
        const int tag = bi[o_coll + AGX_C_STRIDE * best + AGX_C_TAG];
        ci = tag >= 1 && tag <= 9 ? tag : 0;
        nw = mul(ldm3(frames + 12 * best + 3), best_n);
      } else ci = AGX_COLOUR_WATER;
      shade = A.ambient + A.diffuse * fmaxf(0.f, nw.x * A.light[0] + nw.y * A.light[1] + nw.z * A.light[2]);
    }
    const float* col = A.colours + 3 * ci;
    const uint32_t r = (uint32_t)rintf(255.f * fminf(1.f, col[0] * shade)), g = (uint32_t)rintf(255.f * fminf(1.f, col[1] * shade)),
                   b = (uint32_t)rintf(255.f * fminf(1.f, col[2] * shade));
    A.rgba[pix] = r | g << 8 | b << 16 | 255u << 24;
  }
}

// The garment of a dressing scene (agx_camera_garment), drawn over the images agx_render_kernel has left: the same tiles, wavefronts and rays.  A
// kernel of its own and not a phase compiled into the rigid caster: a second instantiation of that kernel is scheduled and contracted differently
// by the compiler, and its rigid pixels then differ in the last bits from the garment-off image (measured on the device); this way the rigid
// caster is the same machine code whether the garment is drawn or not, and a pixel no face wins is not touched at all.
//   1. A lane takes up its pixel's depth and segmentation value from the images (A.depth and A.seg are never null here: where the caller asked
//      for neither, agx_render lends buffers of its own).
//   2. Cull, 64 faces per round: a lane loads its face's node indices (one 16-byte entry of A.tris) and the three positions from the environment's
//      garment record (47 KB per environment: the tiles of an environment are neighbours in the grid, so it stays in L2), makes them eye-relative
//      and tests the box of their projection against the tile's box on the image plane; a face with a vertex before the near plane or behind the
//      eye is kept without projecting, one wholly before the near plane or beyond the far plane is dropped.  Ballot + prefix count compact the
//      survivors into the list in ascending order.
//   3. Cast whenever the next round might not fit into the list, and after the last round: the entry is wave uniform, so the face's indices and
//      nine coordinates come through scalar loads, once per wave.  Moeller-Trumbore on eye-relative vertices, the edges formed first, the triple
//      products turned so that everything but three dot products with the ray is the same in every lane.  Ascending order and the strict test
//      give the tie rule across flushes: a collider before a face, a lower face before a higher one.  Every comparison is false for a NaN: a face
//      with a node that is not finite is never hit.
//   4. A lane whose pixel a face has won writes depth, seg = ncoll + face and the shaded garment colour; the others write nothing.
// Loop bounds come from counts (faces, ballot sums), never from the garment's data; no per-lane array is indexed dynamically.
extern "C" __global__ void __launch_bounds__(64)
agx_render_garment_kernel(const agx_render_args A) {
  __shared__ int list[AGX_RENDER_LIST];
  const int lane = (int)threadIdx.x;
  const int ncoll = ((const int*)A.blob)[AGX_H_NCOLL];
  const int tiles_x = (A.width + AGX_RENDER_TW - 1) / AGX_RENDER_TW;
  const int x0 = ((int)blockIdx.x % tiles_x) * AGX_RENDER_TW, y0 = ((int)blockIdx.x / tiles_x) * AGX_RENDER_TH;
  const int env = A.env0 + (int)blockIdx.y;
  const float* X = A.garment + (size_t)env * A.cloth_words;
  const v3 eye = mk3(A.eye[0], A.eye[1], A.eye[2]), right = mk3(A.right[0], A.right[1], A.right[2]), up = mk3(A.up[0], A.up[1], A.up[2]),
           fwd = mk3(A.fwd[0], A.fwd[1], A.fwd[2]);
  const float sx = 2.f * A.tx / (float)A.width, sy = 2.f * A.ty / (float)A.height;
  const float near = A.near, far = A.far;
  // the ray, exactly as the rigid caster forms it
  const int px = x0 + (lane & (AGX_RENDER_TW - 1)), py = y0 + lane / AGX_RENDER_TW;
  const float cx = ((float)px + 0.5f) * sx - A.tx, cy = A.ty - ((float)py + 0.5f) * sy;
  const v3 dw = cx * right + cy * up + fwd;
  const bool inside = px < A.width && py < A.height;
  const size_t pix = ((size_t)blockIdx.y * A.height + (inside ? py : 0)) * A.width + (inside ? px : 0);
  float best_t = inside && A.seg[pix] >= 0 ? A.depth[pix] : 3.0e38f;      // (the background's depth is `far`, which a face at t = far still beats)
  int best = -1; v3 best_n = mk3(0.f, 0.f, 0.f);      // the face that has won this pixel, its unit normal towards the eye
  // the tile's box on the image plane (camera space at depth 1); the pixel centres lie half a pixel inside it
  const int x1 = x0 + AGX_RENDER_TW < A.width ? x0 + AGX_RENDER_TW : A.width, y1 = y0 + AGX_RENDER_TH < A.height ? y0 + AGX_RENDER_TH : A.height;
  const float slack = 4e-5f;      // eye-relative coordinates carry 1e-7 m of rounding, projected from no nearer than the near plane's 0.01 m: 1e-5
  const float ul = (float)x0 * sx - A.tx - slack, ur = (float)x1 * sx - A.tx + slack, vt = A.ty - (float)y0 * sy + slack, vb = A.ty - (float)y1 * sy - slack;
  const int ntri = A.ntri;
  int m = 0;
  for (int base = 0; base < ntri; base += 64) {
    const int f = base + lane;
    bool keep = false;
    if (f < ntri) {
      const int4 T = A.tris[f];
      const v3 a = ld3(X + 3 * T.x) - eye, b = ld3(X + 3 * T.y) - eye, c = ld3(X + 3 * T.z) - eye;
      const float za = dot(a, fwd), zb = dot(b, fwd), zc = dot(c, fwd);
      const float zmin = fminf(za, fminf(zb, zc)), zmax = fmaxf(za, fmaxf(zb, zc));
      if (zmax >= 0.99f * near && zmin <= 1.01f * far) {      // a hit's depth lies between the vertices' depths
        if (zmin < near) keep = true;      // a vertex before the near plane or behind the eye: not projected
        else {
          const float ia = 1.f / za, ib = 1.f / zb, ic = 1.f / zc;
          const float xa = dot(a, right) * ia, xb = dot(b, right) * ib, xc = dot(c, right) * ic;
          const float ya = dot(a, up) * ia, yb = dot(b, up) * ib, yc = dot(c, up) * ic;
          keep = !(fmaxf(xa, fmaxf(xb, xc)) < ul || fminf(xa, fminf(xb, xc)) > ur || fmaxf(ya, fmaxf(yb, yc)) < vb || fminf(ya, fminf(yb, yc)) > vt);
        }
      }
    }
    const uint64_t mask = wave_ballot(keep);
    if (keep) list[m + wave_rank(mask)] = f;
    m += popc64(mask);
    if (m + 64 <= AGX_RENDER_LIST && base + 64 < ntri) continue;
    wave_sync();
    for (int k = 0; k < m; k++) {
      const int fi = wave_uniform(list[k]);
      const int4 T = A.tris[fi];
      const v3 a = ld3(X + 3 * T.x), e1 = ld3(X + 3 * T.y) - a, e2 = ld3(X + 3 * T.z) - a;      // wave uniform: scalar loads
      // from the eye: tv = eye - a, det = e1 . (d x e2), u = tv . (d x e2) / det, v = d . (tv x e1) / det, t = e2 . (tv x e1) / det
      const v3 tv = eye - a, nrm = cross(e1, e2), q = cross(tv, e1), w = cross(e2, tv);
      const float det = -dot(dw, nrm), inv = __builtin_amdgcn_rcpf(det);
      const float u = dot(dw, w) * inv, v = dot(dw, q) * inv, t = dot(e2, q) * inv;
      if (det != 0.f && u >= 0.f && v >= 0.f && u + v <= 1.f && t >= near && t <= far && t < best_t) {      // false for every NaN
        const float s = (det > 0.f ? 1.f : -1.f) * wave_rsqrt(dot(nrm, nrm));      // the unit normal on the side of the eye: n . d < 0
        best_t = t; best = fi; best_n = s * nrm;
      }
    }
    wave_sync();      // before the next round writes the list
    m = 0;
  }
  if (!inside || best < 0) return;
  A.depth[pix] = best_t;
  A.seg[pix] = ncoll + best;
  if (A.rgba) {
    const float shade = A.ambient + A.diffuse * fmaxf(0.f, best_n.x * A.light[0] + best_n.y * A.light[1] + best_n.z * A.light[2]);
    const float* col = A.colours + 3 * AGX_COLOUR_GARMENT;
    const uint32_t r = (uint32_t)rintf(255.f * fminf(1.f, col[0] * shade)), g = (uint32_t)rintf(255.f * fminf(1.f, col[1] * shade)),
                   b = (uint32_t)rintf(255.f * fminf(1.f, col[2] * shade));
    A.rgba[pix] = r | g << 8 | b << 16 | 255u << 24;
  }
}

void agx_launch_render(hipStream_t st, const agx_render_args& A, int count, bool garment) {
  const int tiles = ((A.width + AGX_RENDER_TW - 1) / AGX_RENDER_TW) * ((A.height + AGX_RENDER_TH - 1) / AGX_RENDER_TH);
  hipLaunchKernelGGL(agx_render_kernel, dim3(tiles, count), dim3(64), 0, st, A);
  if (garment) hipLaunchKernelGGL(agx_render_garment_kernel, dim3(tiles, count), dim3(64), 0, st, A);
}
