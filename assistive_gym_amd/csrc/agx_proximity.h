// agx_proximity.h -- closest points between collider pairs of many environments (agx_proximity_set / agx_proximity, include/agx.h): what
// agx_api.hip hands to the kernel of csrc/agx_proximity.hip, and the kernel's body.  Variant independent: it reads the model blob, the collider
// frames the variant's frames kernel left ([n_envs][ncoll][12], agx_kernels.hip) and the pair list of agx_proximity_set.  The body is compiled
// for the device by agx_proximity.hip and, unchanged, for the CPU wave emulator (tests/emu/emu_proximity.cpp).
//
// A work item is one (environment, pair).  The lanes of a wave are split into groups of G = next_pow2(max(npairs, nqueries)) lanes, 64 at the
// most: a group serves one environment, lane g of it pair g -- 64 / G whole environments per wave -- and where there are more than 32 pairs one
// environment fills the wave and takes its pairs in rounds of 64.  Every lane runs its own GJK (csrc/agx_gjk.h); the collectives inside are
// taken by all 64 lanes, idle ones with has = false.
//   record (12 words, one 48-byte piece written as three 16-byte stores):
//     0 dist | 1-3 point on A | 4-6 point on B | 7-9 unit normal from B towards A | 10 int kind | 11 int pair index
//     kind 1: closest points of the cores, radii taken off along the normal; kind 2: overlapping cores, answered by the direction sampler;
//     kind 0: nothing reported -- dist = +inf, words 1-9 zero.  A NaN is never written.
//   nearest record, per (environment, query): the record of smallest dist among the query's pairs with kind != 0, the lower pair on a tie;
//     none: kind 0, pair -1.  Lane q of a group keeps the running best of query q in registers: per round and query one butterfly over the
//     group ranks (dist, lane) -- lane order is pair order inside a round, and a later round wins only by a strictly smaller dist -- and the
//     winner's words come over by shuffles.  No atomics, no workspace: the result does not depend on how environments fall into waves.
#pragma once
#include "agx_math.h"
#include "agx_gjk.h"
#include "../../include/agx_blob.h"

#define AGX_PROX_WORDS 12
#define AGX_PROX_MAX_PAIRS 8192
#define AGX_PROX_MAX_QUERIES 16
// per collider, built on the host by agx_proximity_set: bit 0 / bit 1 = part of a male / female environment (the rule of the camera's tables),
// bit 2 = every vertex, the radius and the body-frame box are finite
#define AGX_PROX_FINITE 4

struct agx_prox_args {
  const uint32_t* blob; const float* state; int sw;
  const float* frames;                 // [n_envs][ncoll][12]: position, rotation (row-major) of every collider's body, from the frames kernel
  const int* pairs;                    // [npairs][4]: collider a, collider b, query, 0
  const int* cflags;                   // [ncoll], see above
  int npairs, nqueries, group;         // group: G above
  int env0, count; float max_distance;
  float* records;                      // [count][npairs][12] or null
  float* nearest;                      // [count][nqueries][12] or null
};

#ifdef __HIPCC__
void agx_launch_proximity(hipStream_t st, const agx_prox_args& A);      // one launch, nothing allocated, copied or synchronised
#endif

namespace agxprox {

// gjk_distance stops at the first separating axis that proves a pair this far beyond max_distance (the margin the build kernel's callers use,
// GJK_FAR_MARGIN of csrc/agx_collide.h: it dwarfs the rounding of the bound, so what is reported is decided by the converged distance)
constexpr float FAR_MARGIN = 1e-4f;
// the cull's lower bound is a float32 expression of world coordinates (a few metres: ulps of 5e-7) a dozen operations long: a pair is dropped
// only where the bound clears max_distance by this much, two hundred such roundings
constexpr float CULL_MARGIN = 1e-4f;

AGX_DEV float i2f(int i) { float f; __builtin_memcpy(&f, &i, 4); return f; }
AGX_DEV int f2i(float f) { int i; __builtin_memcpy(&i, &f, 4); return i; }
AGX_DEV bool finite3(v3 a) { return fabsf(a.x) < 3.0e38f && fabsf(a.y) < 3.0e38f && fabsf(a.z) < 3.0e38f; }      // false for a NaN
AGX_DEV void st4(float* p, float a, float b, float c, float d) { float4 v; v.x = a; v.y = b; v.z = c; v.w = d; *(float4*)p = v; }
AGX_DEV void st_record(float* p, const float (&w)[AGX_PROX_WORDS]) { st4(p, w[0], w[1], w[2], w[3]); st4(p + 4, w[4], w[5], w[6], w[7]); st4(p + 8, w[8], w[9], w[10], w[11]); }
AGX_DEV void empty_record(float (&w)[AGX_PROX_WORDS], int pair) {
  w[0] = __builtin_huge_valf();
#pragma unroll
  for (int k = 1; k < 10; k++) w[k] = 0.f;
  w[10] = i2f(0); w[11] = i2f(pair);
}

// the boxes face_box() of csrc/agx_collide.h recognises: a static axis-aligned world box of any size
AGX_DEV bool world_box(const int* Ci) {
  return Ci[AGX_C_BODY] == AGX_BODY_WORLD && Ci[AGX_C_NVERT] == 8 && (Ci[AGX_C_TAG] == AGX_TAG_TABLE || Ci[AGX_C_TAG] == AGX_TAG_PLANE);
}
// lower bound on the surface distance of colliders x and y, as sphere_box_apart of csrc/agx_collide.h: x lies within |half extents| + radius of
// the centre cx of its box, y within its body-frame box grown by its radius
AGX_DEV float sphere_box_bound(v3 cx, const float* Cx, const m3& Ry, v3 py, const float* Cy) {
  const v3 hx = ld3(Cx + AGX_C_AABB_H);
  const float rx = sqrtf(dot(hx, hx)) + Cx[AGX_C_RADIUS];
  const v3 pl = tmul(Ry, cx - py) - ld3(Cy + AGX_C_AABB_C);
  const float dx = fmaxf(fabsf(pl.x) - Cy[AGX_C_AABB_H], 0.f), dy = fmaxf(fabsf(pl.y) - Cy[AGX_C_AABB_H + 1], 0.f), dz = fmaxf(fabsf(pl.z) - Cy[AGX_C_AABB_H + 2], 0.f);
  return sqrtf(dx * dx + dy * dy + dz * dz) - rx - Cy[AGX_C_RADIUS];
}

// the record of pair `pair` of environment `env`.  Called by ALL lanes of the wave (gjk_distance holds ballots); has = false: an idle lane.
AGX_DEV void pair_record(const agx_prox_args& A, int env, int pair, bool has, float (&w)[AGX_PROX_WORDS]) {
  const int* bi = (const int*)A.blob; const float* bf = (const float*)A.blob;
  const int ncoll = bi[AGX_H_NCOLL], o_coll = bi[AGX_H_OFF_COLL], o_vert = bi[AGX_H_OFF_VERT], o_prm = bi[AGX_H_OFF_PARAMS];
  gjk_shape sa, sb;
  sa.v = nullptr; sa.n = 0; sa.box = false; sa.c = mk3(0.f, 0.f, 0.f); sa.p = sa.c; sa.lo = sa.c; sa.hi = sa.c;
#pragma unroll
  for (int k = 0; k < 9; k++) sa.R.a[k] = (k % 4 == 0) ? 1.f : 0.f;
  sb = sa;
  v3 shift = mk3(0.f, 0.f, 0.f);
  float ra = 0.f, rb = 0.f;
  bool ok = has, swapped = false;
  if (has) {
    int a = A.pairs[4 * pair], b = A.pairs[4 * pair + 1];
    // a static world box is collider B of the narrowphase: the pair is turned round here and its answer turned back below
    if (world_box(bi + o_coll + AGX_C_STRIDE * a) && !world_box(bi + o_coll + AGX_C_STRIDE * b)) { const int t = a; a = b; b = t; swapped = true; }
    const int* Cai = bi + o_coll + AGX_C_STRIDE * a; const float* Ca = bf + o_coll + AGX_C_STRIDE * a;
    const int* Cbi = bi + o_coll + AGX_C_STRIDE * b; const float* Cb = bf + o_coll + AGX_C_STRIDE * b;
    // a human collider of the other gender is not part of this environment; a collider with a vertex that is not finite reports nothing
    const int gender_bit = 1 << (((const int*)A.state)[(size_t)env * A.sw + bi[AGX_H_S_ENV] + AGX_E_GENDER] == 1 ? 1 : 0);
    const int fa = A.cflags[a], fb = A.cflags[b];
    ok = (fa & gender_bit) && (fb & gender_bit) && (fa & AGX_PROX_FINITE) && (fb & AGX_PROX_FINITE);
    const float* Fa = A.frames + ((size_t)env * ncoll + a) * 12; const float* Fb = A.frames + ((size_t)env * ncoll + b) * 12;
    const v3 pa = ld3(Fa), pb = ld3(Fb);
    sa.R = ldm3(Fa + 3); sb.R = ldm3(Fb + 3);
    {
      float s = 0.f;      // a sum of absolute values is finite exactly when every term is (no overflow: rotation entries and world coordinates)
#pragma unroll
      for (int k = 0; k < 9; k++) s += fabsf(sa.R.a[k]) + fabsf(sb.R.a[k]);
      ok = ok && s < 3.0e38f && finite3(pa) && finite3(pb);
    }
    ra = Ca[AGX_C_RADIUS]; rb = Cb[AGX_C_RADIUS];
    const v3 ha = ld3(Ca + AGX_C_AABB_H);
    const v3 cwa = mul(sa.R, ld3(Ca + AGX_C_AABB_C)) + pa, cwb = mul(sb.R, ld3(Cb + AGX_C_AABB_C)) + pb;
    // cull: out of reach by the bounding sphere of one against the box of the other, with room for the bound's own rounding (CULL_MARGIN);
    // what this cannot prove goes through GJK
    if (ok) {
      const float lb = fmaxf(sphere_box_bound(cwa, Ca, sb.R, pb, Cb), sphere_box_bound(cwb, Cb, sa.R, pa, Ca));
      if (lb - CULL_MARGIN > A.max_distance) ok = false;
    }
    // the pair's own frame: shifted to the centre of A's box, as make_shape of csrc/agx_collide.h does with its shift point
    shift = cwa;
    sa.n = Cai[AGX_C_NVERT]; sa.v = bf + o_vert + 3 * Cai[AGX_C_VOFF]; sa.p = pa - shift;
    sa.c = mul(sa.R, ld3(Ca + AGX_C_AABB_C)) + sa.p;
    sb.n = Cbi[AGX_C_NVERT]; sb.v = bf + o_vert + 3 * Cbi[AGX_C_VOFF]; sb.p = pb - shift;
    sb.c = mul(sb.R, ld3(Cb + AGX_C_AABB_C)) + sb.p;
    if (world_box(Cbi)) {
      // the box itself, from its eight vertices (world coordinates: the world body's frame is the identity), clipped to A's world box
      // (centre cwa, half extents |R| h) grown by a bound g on the core distance.  Exact: the point of an axis-aligned box nearest to a convex
      // set A is the clamp of a point ca of A into the box, |clamp(ca) - ca| is the core distance d, and ca lies in A's world box.
      // The bound: some point of A lies within the half diagonal |wh| of the centre cwa, the centre within e = |clamp(cwa) - cwa| of the box,
      // so d <= e + |wh|.  NOT max_distance + r_a + r_b, which bounds d as well for every pair that is reported: the corners of the clipped box
      // are GJK's support points, and with them the last bits of a record -- on a face, where the closest points are not unique, the points
      // themselves -- would follow max_distance.  This way a record is the same at every max_distance above its dist.
      // An empty clip (numbers that are not finite): nothing reported.
      sb.box = true;
      v3 lo = ld3(sb.v), hi = lo;
#pragma unroll
      for (int k = 1; k < 8; k++) {
        const v3 x = ld3(sb.v + 3 * k);
        lo = mk3(fminf(lo.x, x.x), fminf(lo.y, x.y), fminf(lo.z, x.z)); hi = mk3(fmaxf(hi.x, x.x), fmaxf(hi.y, x.y), fmaxf(hi.z, x.z));
      }
      v3 wh = mk3(fabsf(sa.R.a[0]) * ha.x + fabsf(sa.R.a[1]) * ha.y + fabsf(sa.R.a[2]) * ha.z, fabsf(sa.R.a[3]) * ha.x + fabsf(sa.R.a[4]) * ha.y + fabsf(sa.R.a[5]) * ha.z,
                  fabsf(sa.R.a[6]) * ha.x + fabsf(sa.R.a[7]) * ha.y + fabsf(sa.R.a[8]) * ha.z);
      const v3 off = mk3(fminf(fmaxf(cwa.x, lo.x), hi.x), fminf(fmaxf(cwa.y, lo.y), hi.y), fminf(fmaxf(cwa.z, lo.z), hi.z)) - cwa;
      const float g = 1.0001f * (sqrtf(dot(off, off)) + sqrtf(dot(wh, wh))) + FAR_MARGIN;      // (room for the rounding of the bound itself)
      wh = wh + mk3(g, g, g);
      lo = mk3(fmaxf(lo.x, cwa.x - wh.x), fmaxf(lo.y, cwa.y - wh.y), fmaxf(lo.z, cwa.z - wh.z));
      hi = mk3(fminf(hi.x, cwa.x + wh.x), fminf(hi.y, cwa.y + wh.y), fminf(hi.z, cwa.z + wh.z));
      if (!(hi.x >= lo.x && hi.y >= lo.y && hi.z >= lo.z)) ok = false;
      sb.lo = lo - shift; sb.hi = hi - shift; sb.c = 0.5f * (sb.lo + sb.hi);
    }
  }
  float d; v3 pa, pb;
  const bool pen = gjk_distance(sa, sb, bf[o_prm + AGX_P_GJK_TOL], (int)bf[o_prm + AGX_P_GJK_MAXIT], A.max_distance + ra + rb + FAR_MARGIN, ok, d, pa, pb);
  empty_record(w, pair);
  if (!ok) return;
  v3 n; int kind;
  if (!pen) {
    if (!(d - ra - rb < A.max_distance)) return;      // points closer than max_distance only
    n = (1.0f / d) * (pa - pb); kind = 1;
  } else {
    float depth; gjk_penetration(sa, sb, bf + bi[AGX_H_OFF_DIRS], bi[AGX_H_NDIR], depth, n, pa, pb);
    d = -depth; kind = 2;
  }
  v3 wa = pa - ra * n + shift, wb = pb + rb * n + shift;
  const float dist = d - ra - rb;
  if (swapped) { const v3 t = wa; wa = wb; wb = t; n = -n; }
  if (!(fabsf(dist) < 3.0e38f && finite3(wa) && finite3(wb) && finite3(n))) return;      // a NaN is never written
  w[0] = dist; w[1] = wa.x; w[2] = wa.y; w[3] = wa.z; w[4] = wb.x; w[5] = wb.y; w[6] = wb.z; w[7] = n.x; w[8] = n.y; w[9] = n.z; w[10] = i2f(kind);
}

// the body of one wave: wave `wave` of the launch, lane `lane`
AGX_DEV void prox_wave(const agx_prox_args& A, int wave, int lane) {
  const int G = A.group, gl = lane & (G - 1), gbase = lane - gl;
  const int el = wave * (AGX_WAVE / G) + lane / G;      // environment of this lane's group, counted from env0
  const bool env_ok = el < A.count;
  const int env = A.env0 + (env_ok ? el : 0);
  const int rounds = (A.npairs + G - 1) / G;      // 1 unless G = 64
  float best[AGX_PROX_WORDS];
  empty_record(best, -1);
  for (int r = 0; r < rounds; r++) {
    const int pair = r * G + gl;
    const bool has = env_ok && pair < A.npairs;
    float w[AGX_PROX_WORDS];
    pair_record(A, env, has ? pair : 0, has, w);
    if (has && A.records) st_record(A.records + ((size_t)el * A.npairs + pair) * AGX_PROX_WORDS, w);
    if (!A.nearest) continue;
    const int mine = has && f2i(w[10]) != 0 ? A.pairs[4 * pair + 2] : -1;
    for (int q = 0; q < A.nqueries; q++) {
      float d = mine == q ? w[0] : __builtin_huge_valf(); int l = gl;
      for (int m = 1; m < G; m <<= 1) {
        const float od = wave_shfl(d, lane ^ m); const int ol = wave_shfl_i(l, lane ^ m);
        if (od < d || (od == d && ol < l)) { d = od; l = ol; }
      }
      const bool take = gl == q && d < best[0];
      if (!wave_any(take)) continue;
#pragma unroll
      for (int k = 0; k < AGX_PROX_WORDS; k++) { const float t = wave_shfl(w[k], gbase + l); if (take) best[k] = t; }
    }
  }
  if (A.nearest && env_ok && gl < A.nqueries) st_record(A.nearest + ((size_t)el * A.nqueries + gl) * AGX_PROX_WORDS, best);
}

}  // namespace agxprox
