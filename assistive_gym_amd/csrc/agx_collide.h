// agx_collide.h -- K2/K3 collision: speculative AABBs, pair-group broadphase, per-lane GJK narrowphase, contact selection.
// Part of the stepper (see agx_step.h for the overview); included by agx_step.h only.
#pragma once

namespace agx {

// ---- K2/K3: collision ----------------------------------------------------------------------------
struct Cand { v3 pa, pb, n; float dist, gap; };
constexpr float GJK_FAR_MARGIN = 1e-4f;   // the separating-axis early-out of gjk_distance only fires this far beyond the contact limit

AGX_DEV void make_shape(const Ctx& c, int col, v3 shift, gjk_shape& s) {
  s.n = CLI(c, col, AGX_C_NVERT);
  s.v = c.bf + c.o_vert + 3 * CLI(c, col, AGX_C_VOFF);
  v3 p; body_xf(c, CLI(c, col, AGX_C_BODY), s.R, p);
  s.p = p - shift; s.box = false;
  s.c = mul(s.R, mk3(CLF(c, col, AGX_C_AABB_C), CLF(c, col, AGX_C_AABB_C + 1), CLF(c, col, AGX_C_AABB_C + 2))) + s.p;
}
// closest features of colliders (ca, cb); true if the separation (radii included) is below limit.
// Wave-uniform: every lane calls it, lanes without a pair pass has = false.
AGX_DEV bool narrowphase(const Ctx& c, int ca, int cb, float limit, Cand& out, bool has) {
  const float* AB = c.lds + L_ARENA;
  gjk_shape sa, sb;
  sa.v = nullptr; sa.n = 0; sa.box = false; sa.c = mk3(0.f, 0.f, 0.f); sb.v = nullptr; sb.n = 0; sb.box = false; sb.c = sa.c;
  v3 shift = mk3(0.f, 0.f, 0.f);
  float ra = 0.f, rb = 0.f;
  bool ok = has;
  if (has) {
    shift = mk3(0.5f * (AB[ABS * ca] + AB[ABS * ca + 3]), 0.5f * (AB[ABS * ca + 1] + AB[ABS * ca + 4]), 0.5f * (AB[ABS * ca + 2] + AB[ABS * ca + 5]));
    make_shape(c, ca, shift, sa); make_shape(c, cb, shift, sb);
    // large static world boxes (table top, ground): clip to the neighbourhood of A (see oracle)
    if (CLI(c, cb, AGX_C_BODY) == AGX_BODY_WORLD && sb.n == 8 && (CLI(c, cb, AGX_C_TAG) == AGX_TAG_TABLE || CLI(c, cb, AGX_C_TAG) == AGX_TAG_PLANE)) {
      sb.box = true;
      float lo[3], hi[3];
      for (int k = 0; k < 3; k++) {
        lo[k] = fmaxf(AB[ABS * cb + k], AB[ABS * ca + k] - AGX_BOX_CLIP); hi[k] = fminf(AB[ABS * cb + 3 + k], AB[ABS * ca + 3 + k] + AGX_BOX_CLIP);
        if (hi[k] < lo[k]) ok = false;
      }
      sb.lo = mk3(lo[0], lo[1], lo[2]) - shift; sb.hi = mk3(hi[0], hi[1], hi[2]) - shift; sb.c = 0.5f * (sb.lo + sb.hi);
    }
    ra = CLF(c, ca, AGX_C_RADIUS); rb = CLF(c, cb, AGX_C_RADIUS);
  }
  float d; v3 pa, pb, n;
  const bool pen = gjk_distance(sa, sb, PRM(c, AGX_P_GJK_TOL), (int)PRM(c, AGX_P_GJK_MAXIT), limit + ra + rb + GJK_FAR_MARGIN, ok, d, pa, pb);
  if (!ok) return false;
  if (!pen) {
    if (d - ra - rb >= limit) return false;
    n = (1.0f / d) * (pa - pb);
  } else {
    float depth; gjk_penetration(sa, sb, c.bf + c.o_dirs, c.bi[AGX_H_NDIR], depth, n, pa, pb);
    d = -depth;
  }
  out.pa = pa - ra * n + shift; out.pb = pb + rb * n + shift; out.n = n; out.dist = d - ra - rb;
  return true;
}
AGX_DEV float pair_mu(const Ctx& c, int ca, int cb) {
  float plane_mu = c.lds[L_ST + c.s_env + AGX_E_PLANE_FRICTION];
  float mua = CLI(c, ca, AGX_C_TAG) == AGX_TAG_PLANE ? plane_mu : CLF(c, ca, AGX_C_FRICTION);
  float mub = CLI(c, cb, AGX_C_TAG) == AGX_TAG_PLANE ? plane_mu : CLF(c, cb, AGX_C_FRICTION);
  return mua * mub;
}
AGX_DEV void emit_contact(Ctx& c, int slot, int ca, int cb, const Cand& k) {
  float* o = c.gcon + CON_STRIDE * slot; int* oi = (int*)o;
  oi[C_CA] = ca; oi[C_CB] = cb; oi[C_BA] = CLI(c, ca, AGX_C_BODY); oi[C_BB] = CLI(c, cb, AGX_C_BODY);
  st3(o + C_PA, k.pa); st3(o + C_PB, k.pb); st3(o + C_N, k.n); o[C_DIST] = k.dist; o[C_MU] = pair_mu(c, ca, cb); o[C_LAM] = 0.f;
}
// Collision pipeline per substep (K2 + K3), all inside the wave:
//   1. world AABB of every collider (lanes over colliders) -> LDS table
//   2. per static pair group: body-level cull (union AABBs), then a lane-parallel sweep over the
//      |A|x|B| pair grid appends the overlapping pairs to an LDS worklist IN ENUMERATION ORDER
//   3. narrowphase over the worklist, 64 pairs per pass, every lane running its own GJK
//   4. selection: per A collider the `keep` candidates with the smallest predicted gap (or all of
//      them, in order) become contacts.
// The contact order (group, a, selection order) is what the oracle produces, so the solver rows
// are identical.
constexpr int CAND_STRIDE = 8;
constexpr int TW_WORDS = 6 * (MAX_DOF + MAX_FREE);        // twist (w, v at the reference point M_REF) of every moving body, see rel_travel()
constexpr int WL_FIT = (ARENA_WORDS - ABS * MAX_COLL - TW_WORDS) / (1 + CAND_STRIDE);
constexpr int WL_MAX = WL_FIT < 200 ? WL_FIT : 200;      // worklist entries the arena has room for
constexpr int A_WL = ABS * MAX_COLL;                      // int[WL_MAX]: a | b << 9 | group << 18 | face-manifold point << 24
constexpr int WL_KEY_MASK = ~((511 << 9) | (3 << 24));    // (group, A collider) of a worklist entry
constexpr int A_CAND = A_WL + WL_MAX;                   // float[WL_MAX][CAND_STRIDE]: gap, pa, n, dist (pb = pa - dist n)
constexpr int A_TW = A_CAND + WL_MAX * CAND_STRIDE;     // float[MAX_DOF + MAX_FREE][6]
static_assert(A_TW + TW_WORDS <= ARENA_WORDS, "collision workspace exceeds the arena");
static_assert(MAX_COLL <= 512, "collider indices are packed in 9 bits");
// the candidate words of the last entries hold the two collider lists of a sweep (128 + 128 indices; afterwards the selection's slot list, 64 ints):
// bytes where collider indices fit a byte -- 8 entries instead of 16.  For the feeding variant that is 174 usable entries instead of 166, and an
// ordinary FeedingJaco substep has ~170 candidate pairs (150 of them food x spoon pieces): one flush of three narrowphase passes instead of
// 163 + 6 = four (profiles/r05/r05x_*)
constexpr bool LIST_BYTES = MAX_COLL <= 256;
constexpr int LIST_TAIL = LIST_BYTES ? 8 : 16;
#ifdef AGX_WL_TEST_CAP   // test-only: a short worklist, so that ordinary substeps go through the flush between groups, the batches of A colliders and the overflow (tests/test_emu_collide_front.py)
constexpr int WL_CAP = AGX_WL_TEST_CAP;
static_assert(WL_CAP >= 1 && WL_CAP <= WL_MAX - LIST_TAIL, "AGX_WL_TEST_CAP only lowers the cap");
#else
constexpr int WL_CAP = WL_MAX - LIST_TAIL;
static_assert(WL_CAP >= 128, "a flush of at least two full passes");
static_assert(!(TASK == AGX_TASK_FEEDING && MAX_COLL == 256 && ARENA_WORDS == 3592) || WL_CAP == 174, "the feeding variant: 174 entries make three narrowphase passes instead of four");
#endif
template <bool B> struct ListIndex { typedef unsigned short type; };
template <> struct ListIndex<true> { typedef uint8_t type; };
typedef ListIndex<LIST_BYTES>::type list_t;
// AGX_COLLIDE_FRONT.  The group cull and the contact selection around the narrowphase decide WHICH groups are swept and WHICH candidate takes which
// contact slot; no floating-point expression of theirs reaches a result except through fminf / fmaxf (exact, order-free) and comparisons.
// 1 (the DEFAULT):
//   * cull: lane l first reduces a block of 2^k consecutive colliders (64 blocks cover the table) to one box in the candidate area (dead until the
//     first flush); lane g then builds the union box of each of its two ranges from the few head and tail colliders and the whole blocks in
//     between -- about 40 steps for the 134-collider range of the feeding scene instead of 134;
//   * selection: every worklist entry finds its own (group, A collider) segment from ballots of the segment starts, ranks itself among the
//     entries of that segment by (gap, index) and takes slot = contacts before the flush + selected entries of earlier segments + rank -- two
//     rounds of ballots for the whole list instead of a wave_min + ballot round per kept contact of every segment.
//   * sweep: a WINDOW of consecutive live groups is swept at once (collide_sweep_window below).  Level 1 takes the collider ranges of all its
//     groups, concatenated, 64 per round, and packs the surviving colliders of every (group, side) into the list area one list behind the other;
//     the window ends in front of the first group whose lists no longer fit there.  Level 2 runs ONE pair grid over the concatenated pair counts:
//     a lane finds its group from the prefix sums, then (a, b, face point) inside it, and survivors are appended by ballot rank -- group-major
//     concatenation plus ballot rank is the enumeration order of the serial sweep.  The grid queues what passes the box test and runs the tests
//     that read the blob 64 queued pairs at a time (half as many rounds of load chains as grid rounds in the feeding scene).  The grid counts survivors per group, so the first group that
//     does not fit behind the pending entries is found and the units are flushed exactly where the serial loop flushes them.
// 0: one lane walks each range collider by collider, the selection takes one segment at a time and every live group is swept on its own (two
//    levels, a load chain per group), as before this switch existed
//    (lib/variants/frontplain.so; tests/test_gpu_collide_front.py and tests/test_emu_collide_front.py compare the bits).
#ifndef AGX_COLLIDE_FRONT
#define AGX_COLLIDE_FRONT 1
#endif
#if AGX_COLLIDE_FRONT < 0 || AGX_COLLIDE_FRONT > 1
#error "AGX_COLLIDE_FRONT: 0 or 1"
#endif
// the two parts on their own, for same-box A/B runs (profiles/collide_front/)
#ifndef AGX_FRONT_CULL
#define AGX_FRONT_CULL AGX_COLLIDE_FRONT
#endif
#ifndef AGX_FRONT_SELECT
#define AGX_FRONT_SELECT AGX_COLLIDE_FRONT
#endif
#ifndef AGX_FRONT_SWEEP      // (lib/variants/sweepserial.so: the windowed sweep alone switched off; tests/test_gpu_collide_sweep.py, tests/test_emu_collide_sweep.py)
#define AGX_FRONT_SWEEP AGX_COLLIDE_FRONT
#endif
// the list area behind the worklist holds 256 collider indices (bytes in 8 candidate entries, or 16-bit words in 16)
constexpr int LIST_N = 256;
static_assert(LIST_N * (int)sizeof(list_t) == LIST_TAIL * CAND_STRIDE * 4, "the two collider lists fill the tail of the candidate area");
#ifdef AGX_SWEEP_TEST_LIST   // test-only: a short list area, so that ordinary substeps cut their windows by list space (tests/test_emu_collide_sweep.py)
constexpr int LIST_CAP = AGX_SWEEP_TEST_LIST;
static_assert(LIST_CAP >= 2 && LIST_CAP <= LIST_N, "AGX_SWEEP_TEST_LIST only lowers the capacity");
#else
constexpr int LIST_CAP = LIST_N;
#endif
#ifdef AGX_SWEEP_TEST_WINDOW   // test-only: at most this many groups per window
constexpr int SWEEP_WINDOW = AGX_SWEEP_TEST_WINDOW;
static_assert(SWEEP_WINDOW >= 1 && SWEEP_WINDOW <= 64, "AGX_SWEEP_TEST_WINDOW: 1 to 64 groups");
#else
constexpr int SWEEP_WINDOW = 64;
#endif

AGX_DEV void emit_from_cand(Ctx& c, int slot, int idx) {
  const float* L = c.lds; const int pr = c.ldsi[L_ARENA + A_WL + idx]; const float* cd = L + L_ARENA + A_CAND + CAND_STRIDE * idx;
  Cand k; k.gap = cd[0]; k.pa = ld3(cd + 1); k.n = ld3(cd + 4); k.dist = cd[7]; k.pb = k.pa - k.dist * k.n;
  emit_contact(c, slot, pr & 511, (pr >> 9) & 511, k);
}
// Face manifold (see face_manifold in oracle/agx_oracle.c and AGX_FACE_* in agx_blob.h): a collider resting on the top
// face of a static world box touches it along a face or an edge, where GJK's closest point is not unique and a single
// contact point makes the body rock.  Such a pair occupies 1 + AGX_FACE_EXTRA consecutive worklist entries: entry 0
// is the pair's first contact (GJK decides whether the pair is in contact and gives the normal; the point itself is
// re-anchored at the first vertex, in model order, within AGX_FACE_BAND of the lowest one, because GJK's witness point
// on a flat face is arbitrary), entry e the e-th additional vertex contact -- among the vertices of A above the box's
// footprint and inside the band, the one farthest (horizontally) from the points chosen before it, if that is at
// least AGX_FACE_SPREAD.
AGX_DEV bool face_box(const Ctx& c, int cb) {
  return CLI(c, cb, AGX_C_BODY) == AGX_BODY_WORLD && CLI(c, cb, AGX_C_NVERT) == 8 && (CLI(c, cb, AGX_C_TAG) == AGX_TAG_TABLE || CLI(c, cb, AGX_C_TAG) == AGX_TAG_PLANE);
}
// contact e of the face manifold of pair (ca, cb): e = 0 the re-anchored first contact, e >= 1 the e-th extra one given
// the first contact point p0; false if there is none
AGX_DEV bool face_point(const Ctx& c, int ca, int cb, int e, v3 p0, Cand& out) {
  const float* AB = c.lds + L_ARENA;
  const int n = CLI(c, ca, AGX_C_NVERT);
  const float* V = c.bf + c.o_vert + 3 * CLI(c, ca, AGX_C_VOFF);
  m3 R; v3 p; body_xf(c, CLI(c, ca, AGX_C_BODY), R, p);
  const float x0 = AB[ABS * cb], y0 = AB[ABS * cb + 1], x1 = AB[ABS * cb + 3], y1 = AB[ABS * cb + 4], top = AB[ABS * cb + 5];   // radius included
  float zmin = 3.0e38f;
  for (int v = 0; v < n; v++) { const v3 w = mul(R, mk3(V[3 * v], V[3 * v + 1], V[3 * v + 2])) + p; if (w.x >= x0 && w.x <= x1 && w.y >= y0 && w.y <= y1 && w.z < zmin) zmin = w.z; }
  float cx[1 + AGX_FACE_EXTRA], cy[1 + AGX_FACE_EXTRA];
  cx[0] = p0.x; cy[0] = p0.y;
#pragma unroll
  for (int q = 1; q <= AGX_FACE_EXTRA; q++) { cx[q] = 0.f; cy[q] = 0.f; }
  v3 pick = mk3(0.f, 0.f, 0.f);
  if (e == 0) {   // the pair's first contact, re-anchored at the first vertex (model order) inside the band
    bool found = false;
    for (int v = 0; v < n && !found; v++) {
      const v3 w = mul(R, mk3(V[3 * v], V[3 * v + 1], V[3 * v + 2])) + p;
      if (w.x >= x0 && w.x <= x1 && w.y >= y0 && w.y <= y1 && w.z <= zmin + AGX_FACE_BAND) { pick = w; found = true; }
    }
    if (!found) return false;
  }
#pragma unroll
  for (int q = 1; q <= AGX_FACE_EXTRA; q++) {
    if (q > e) break;
    int bi = -1; float bd = AGX_FACE_SPREAD * AGX_FACE_SPREAD; v3 bw = mk3(0.f, 0.f, 0.f);
    for (int v = 0; v < n; v++) {
      const v3 w = mul(R, mk3(V[3 * v], V[3 * v + 1], V[3 * v + 2])) + p;
      if (!(w.x >= x0 && w.x <= x1 && w.y >= y0 && w.y <= y1) || w.z > zmin + AGX_FACE_BAND) continue;
      float dmin = 3.0e38f;
#pragma unroll
      for (int k = 0; k <= AGX_FACE_EXTRA; k++) if (k < q) { const float dx = w.x - cx[k], dy = w.y - cy[k]; dmin = fminf(dmin, dx * dx + dy * dy); }
      if (dmin > bd) { bd = dmin; bi = v; bw = w; }
    }
    if (bi < 0) return false;
    cx[q] = bw.x; cy[q] = bw.y; pick = bw;
  }
  const float ra = CLF(c, ca, AGX_C_RADIUS);
  out.n = mk3(0.f, 0.f, 1.f); out.pa = mk3(pick.x, pick.y, pick.z - ra); out.pb = mk3(pick.x, pick.y, top); out.dist = pick.z - ra - top;
  return true;
}
// AGX_FACE.  What the face pairs of a pass cost is a chain of memory round trips, and most of it buys nothing:
//   * face_point above walks the hull one vertex per loop round (zmin, the first-in-band search, one farthest-point loop per extra contact), each
//     round waiting for its own 12-byte blob load, and the lanes sub = 1..3 of a pair each repeat the zmin scan of lane sub = 0;
//   * entry 0 of the pair runs GJK to convergence (5-6 iterations, the longest of the substep, two served hull scans each), and when it hits with
//     n.z > 0.999 everything GJK computed is overwritten by face_point(.., 0, ..): two booleans survive.
// 1: face_point_wide below -- the same comparisons in the same order over EIGHT vertices per round (the load pattern of gjk_support, indices
//    clamped to n - 1: a repeated vertex never wins a strict comparison and cannot be the first in the band before itself), every value that
//    leaves the function taken from `R v + p` on a fresh 12-byte load by index, the first-in-band search still ending at the round that finds
//    one; zmin computed once per pair, by lane sub = 0, and handed to the pair's other entries through word 0 of their own CD[] slots (which
//    they overwrite at the end of their pass, also across a pass boundary).  The first contact is computed BEFORE narrowphase() (it never looked
//    at GJK's point) and parked in the lane's own CD[] slot.
// 2 (the DEFAULT): as 1, and a lane whose pair is provably a face contact does not run GJK at all (collide_flush).
// 0 (or -DAGX_FACE_PLAIN): GJK for every pair and the one-vertex loops, as before this switch existed (lib/variants/faceplain.so; tests/test_gpu_face_proof.py
//    and tests/test_emu_face_proof.py compare the bits).
#ifdef AGX_FACE_PLAIN
#undef AGX_FACE
#define AGX_FACE 0
#endif
#ifndef AGX_FACE
#define AGX_FACE 2
#endif
#if AGX_FACE < 0 || AGX_FACE > 2
#error "AGX_FACE: 0, 1 or 2"
#endif
// The proof of value 2, for entry 0 of a face_box pair (A a hull of >= 2 vertices, B the static box), from the AB[] boxes and the zmin that
// face_point_wide has just computed from A's vertices.  With every comparison below true:
//   footprint: A's world box lies inside B's in x and y by FACE_PROOF_GUARD.  A's core vertices lie inside A's box (radius and travel only widen
//     it), so all of them are inside B's footprint -- zmin is the minimum over ALL vertices and face_point finds its first contact -- and inside
//     the footprint of the clipped box narrowphase() builds (B's box cut to A's box grown by AGX_BOX_CLIP); that box is not empty (the z test).
//   gap: dcore = zmin - top > FACE_PROOF_GUARD: every core vertex is above the box's top face and over it, so in exact arithmetic the core
//     distance IS dcore, attained along +z.  |v| never falls below the true distance during the iteration: no `vv < 1e-12` exit (1e-6 m), no
//     enclosed origin, no penetration sampler.
//   limit: dcore - r_a - r_b < lim - FACE_PROOF_GUARD_LIM.  At the tolerance exit of gjk_distance (vv - vw <= GJK_TOL vv, GJK_TOL = 1e-6) v.w <= |v| d for
//     the true distance d, so |v| <= d / (1 - GJK_TOL): 6e-9 m too long at these 6 mm, and v within sqrt(GJK_TOL) = 1e-3 rad of +z, n.z >= 1 - 5e-7.
//     The lower bounds of the separating-axis exit never exceed d, and it fires GJK_FAR_MARGIN = 1e-4 beyond the limit only.
// Rounding: GJK works in a frame shifted to A's box (coordinates of centimetres, 1e-8), but the shift, the body position and the box are world
// coordinates (|x| < 2 m: 1.2e-7 each), as are zmin and the AB[] boxes used here: a few times 1e-7 in all, with the 6e-9 above.
// FACE_PROOF_GUARD = GJK_FAR_MARGIN = 1e-4 (a thousand roundings, a hundred times the 1e-6 m of the `vv < 1e-12` exit) for the footprint and the
// lower side of the gap, where a resting piece clears it by millimetres; FACE_PROOF_GUARD_LIM = 1e-5 (some thirty roundings; the same allowance
// as the 1e-5 in the limits of collide_flush and collide_sweep) towards the limit, because that is where the pieces of a resting bowl ARE: its
// upper ring sits 5.87 mm above the table under a limit of 5.93 mm.  With all of this GJK would converge to a hit with n.z > 0.999 and its numbers
// would be overwritten: the lane skips it.  For the other exits of gjk_distance (a repeated support point, no
// progress, maxit) there is no such argument; the bit comparisons of the two test files at volume are the check.  Anything else -- a piece
// overhanging an edge, tilted off its footprint, in the shell around either guard, overlapping cores, non-finite numbers (the comparisons are
// false), no first contact -- runs GJK as before.
constexpr float FACE_PROOF_GUARD = 1e-4f, FACE_PROOF_GUARD_LIM = 1e-5f;

#if AGX_FACE
// face_point with the wide loops.  e = 0: computes zmin (3e38 if no vertex is above the footprint) and the first contact; e >= 1: takes zmin from the caller.
AGX_DEV bool face_point_wide(const Ctx& c, int ca, int cb, int e, v3 p0, float& zmin, Cand& out) {
  const float* AB = c.lds + L_ARENA;
  const int n = CLI(c, ca, AGX_C_NVERT), last = n - 1;
  const float* V = c.bf + c.o_vert + 3 * CLI(c, ca, AGX_C_VOFF);
  m3 R; v3 p; body_xf(c, CLI(c, ca, AGX_C_BODY), R, p);
  const float x0 = AB[ABS * cb], y0 = AB[ABS * cb + 1], x1 = AB[ABS * cb + 3], y1 = AB[ABS * cb + 4], top = AB[ABS * cb + 5];   // radius included
#define FACE_LDV(j, kk) const int i##j = (kk) < last ? (kk) : last; const float vx##j = V[3 * i##j], vy##j = V[3 * i##j + 1], vz##j = V[3 * i##j + 2];
#define FACE_LD8(k) FACE_LDV(0, k) FACE_LDV(1, k + 1) FACE_LDV(2, k + 2) FACE_LDV(3, k + 3) FACE_LDV(4, k + 4) FACE_LDV(5, k + 5) FACE_LDV(6, k + 6) FACE_LDV(7, k + 7)
#define FACE_W(j) const v3 w = mul(R, mk3(vx##j, vy##j, vz##j)) + p; const bool in = w.x >= x0 && w.x <= x1 && w.y >= y0 && w.y <= y1;
#define FACE_ALL8(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define FACE_FRESH(i) (mul(R, mk3(V[3 * (i)], V[3 * (i) + 1], V[3 * (i) + 2])) + p)
  float cx[1 + AGX_FACE_EXTRA], cy[1 + AGX_FACE_EXTRA];
  cx[0] = p0.x; cy[0] = p0.y;
#pragma unroll
  for (int q = 1; q <= AGX_FACE_EXTRA; q++) { cx[q] = 0.f; cy[q] = 0.f; }
  v3 pick = mk3(0.f, 0.f, 0.f);
  if (e == 0) {
    int iz = -1; float zm = 3.0e38f;
#define FACE_ZMIN(j) { FACE_W(j) const bool t = in && w.z < zm; zm = t ? w.z : zm; iz = t ? i##j : iz; }
    for (int k = 0; k < n; k += 8) { FACE_LD8(k) FACE_ALL8(FACE_ZMIN) }
#undef FACE_ZMIN
    zmin = 3.0e38f;
    if (iz < 0) return false;
    zmin = FACE_FRESH(iz).z;
    int first = -1;   // the first vertex (model order) inside the band
#define FACE_BAND(j) { FACE_W(j) const bool t = first < 0 && in && w.z <= zmin + AGX_FACE_BAND; first = t ? i##j : first; }
    for (int k = 0; k < n && first < 0; k += 8) { FACE_LD8(k) FACE_ALL8(FACE_BAND) }
#undef FACE_BAND
    if (first < 0) return false;
    pick = FACE_FRESH(first);
  }
#pragma unroll
  for (int q = 1; q <= AGX_FACE_EXTRA; q++) {
    if (q > e) break;
    int bi = -1; float bd = AGX_FACE_SPREAD * AGX_FACE_SPREAD;
#define FACE_FAR(j) { FACE_W(j) float dmin = 3.0e38f; \
      _Pragma("unroll") for (int kk = 0; kk <= AGX_FACE_EXTRA; kk++) if (kk < q) { const float dx = w.x - cx[kk], dy = w.y - cy[kk]; dmin = fminf(dmin, dx * dx + dy * dy); } \
      const bool t = in && !(w.z > zmin + AGX_FACE_BAND) && dmin > bd; bd = t ? dmin : bd; bi = t ? i##j : bi; }
    for (int k = 0; k < n; k += 8) { FACE_LD8(k) FACE_ALL8(FACE_FAR) }
#undef FACE_FAR
    if (bi < 0) return false;
    const v3 bw = FACE_FRESH(bi);
    cx[q] = bw.x; cy[q] = bw.y; pick = bw;
  }
#undef FACE_LDV
#undef FACE_LD8
#undef FACE_W
#undef FACE_ALL8
#undef FACE_FRESH
  const float ra = CLF(c, ca, AGX_C_RADIUS);
  out.n = mk3(0.f, 0.f, 1.f); out.pa = mk3(pick.x, pick.y, pick.z - ra); out.pb = mk3(pick.x, pick.y, top); out.dist = pick.z - ra - top;
  return true;
}
#endif
struct CollideState { int ncon, near_mask, overflow, maxc, nqpt; };
// the pair-group table, one group per lane (lane g = group g): read from the blob once per substep and
// broadcast with v_readlane where a group's parameters are needed (a dependent blob load costs an L2 trip)
struct GroupRegs { int a0, a1, b0, b1, flags, keep; float alo[3], ahi[3], blo[3], bhi[3]; };   // + union boxes of the two collider ranges
// |angular velocity| of the body a collider is attached to (0 for the static ones), from the table
// filled at the start of collide()
AGX_DEV float body_wmag(const Ctx& c, int code) {
  if (code >= 0 && code < AGX_BODY_ROBOT_BASE) return c.lds[L_WMAG + code];
  if (code >= AGX_BODY_FREE0 && code < AGX_BODY_HUMAN0) return c.lds[L_WMAG + MAX_DOF + (code - AGX_BODY_FREE0)];
  return 0.f;
}
// twist of the body a collider is attached to, about the common reference point M_REF: velocity field u(x) = v + w x (x - ref); zero for
// the static bodies.  Filled at the start of collide().
AGX_DEV void body_twist(const Ctx& c, int code, v3& w, v3& v) {
  int slot = -1;
  if (code >= 0 && code < AGX_BODY_ROBOT_BASE) slot = code;
  else if (code >= AGX_BODY_FREE0 && code < AGX_BODY_HUMAN0) slot = MAX_DOF + (code - AGX_BODY_FREE0);
  if (slot < 0) { w = mk3(0.f, 0.f, 0.f); v = w; return; }
  const float* T = c.lds + L_ARENA + A_TW + 6 * slot;
  w = ld3(T); v = ld3(T + 3);
}
// Upper bound on |v_n| dt of a contact of the pair (a, b) from the RELATIVE motion of the two bodies.  With the relative velocity field
// u(x) = v_A(x) - v_B(x) = dv + dw x (x - ref) the contact's normal velocity is v_n = n . (v_A(pa) - v_B(pb)) = n . u(pa), because
// pa - pb is parallel to n (closest points, or the penetration direction).  pa lies within ext_a (half the diagonal of a's world box) of
// the box centre ca:  |v_n| <= |u(ca)| + |dw| ext_a.  For a sphere (one-vertex core) pa - ca = -r n and the rotation term has no normal
// component at all: |v_n| <= |u(c)| at the sphere's centre, whichever side the sphere is on.
// The per-collider travel distances (AB[.][6], absolute speeds) bound the same quantity by |v_A| + |v_B|: for bodies that move TOGETHER
// -- the food riding on the spoon while the arm swings it, 180 of the ~225 narrowphase pairs of a FeedingJaco substep -- that is the speed
// of the arm, this is ~0.  Used wherever a pair is dropped because it cannot produce a solver row (predicted gap = dist + v_n dt >=
// slack): the set of contacts is unchanged, only the work is.
AGX_DEV float rel_travel(const Ctx& c, int a, int b) {
  const float* AB = c.lds + L_ARENA;
#ifdef AGX_NO_REL_TRAVEL   // build-time knob for same-box A/B runs and the bit-identity check of tests/test_emu_parity.py
  return AB[ABS * a + 6] + AB[ABS * b + 6];
#endif
  v3 wa, va, wb, vb;
  body_twist(c, CLI(c, a, AGX_C_BODY), wa, va); body_twist(c, CLI(c, b, AGX_C_BODY), wb, vb);
  const bool sa = CLI(c, a, AGX_C_NVERT) == 1, sb = CLI(c, b, AGX_C_NVERT) == 1;
  const int e = (!sa && sb) ? b : a;                               // evaluate at the sphere's centre if there is one
  const v3 lo = ld3(AB + ABS * e), hi = ld3(AB + ABS * e + 3);
  const v3 ce = 0.5f * (lo + hi), d = hi - lo;
  const v3 dw = wa - wb;
  const v3 u = (va - vb) + cross(dw, ce - ld3(c.lds + L_MISC + M_REF));
  const float rot = (sa || sb) ? 0.f : sqrtf(dot(dw, dw)) * 0.5f * sqrtf(dot(d, d));
  const float t = 1.001f * (sqrtf(dot(u, u)) + rot) * c.dt + 1e-6f;
  return fminf(t, AB[ABS * a + 6] + AB[ABS * b + 6]);             // never above the sum of the absolute travels
}
// conservative separation test: every point of collider x lies within |half extents| + radius of
// the centre of its box; collider y lies within its body-frame box inflated by its radius.  True if
// the two are certainly further apart than `reach`.
AGX_DEV bool sphere_box_apart(const Ctx& c, int x, int y, float reach) {
  const float* AB = c.lds + L_ARENA;
  const v3 cx = mk3(0.5f * (AB[ABS * x] + AB[ABS * x + 3]), 0.5f * (AB[ABS * x + 1] + AB[ABS * x + 4]), 0.5f * (AB[ABS * x + 2] + AB[ABS * x + 5]));
  const v3 hx = mk3(CLF(c, x, AGX_C_AABB_H), CLF(c, x, AGX_C_AABB_H + 1), CLF(c, x, AGX_C_AABB_H + 2));
  const float rx = sqrtf(dot(hx, hx)) + CLF(c, x, AGX_C_RADIUS);
  m3 R; v3 p; body_xf(c, CLI(c, y, AGX_C_BODY), R, p);
  const v3 pl = tmul(R, cx - p) - mk3(CLF(c, y, AGX_C_AABB_C), CLF(c, y, AGX_C_AABB_C + 1), CLF(c, y, AGX_C_AABB_C + 2));
  const float dx = fmaxf(fabsf(pl.x) - CLF(c, y, AGX_C_AABB_H), 0.f), dy = fmaxf(fabsf(pl.y) - CLF(c, y, AGX_C_AABB_H + 1), 0.f),
              dz = fmaxf(fabsf(pl.z) - CLF(c, y, AGX_C_AABB_H + 2), 0.f);
  const float lb = sqrtf(dx * dx + dy * dy + dz * dz) - rx - CLF(c, y, AGX_C_RADIUS);
  return lb > reach;
}

// narrowphase + selection over the current worklist (entries of one or several whole groups, in
// enumeration order); appends the resulting contacts
AGX_DEV void collide_flush(Ctx& c, int wn, CollideState& cs, float brk, float slack, const GroupRegs& G) {
  float* L = c.lds; int* WL = c.ldsi + L_ARENA + A_WL; float* CD = L + L_ARENA + A_CAND; const int lane = c.lane;
  const float* AB = L + L_ARENA;
  const int food0 = c.bi[AGX_H_FOOD0];
  if (wn == 0) return;
  wave_sync();
  long long ct0 = c.timing ? wave_clock() : 0;
  if (c.timing) { c.tm[13] += wn; c.tm[14] += (wn + 63) / 64; }   // debug: narrowphase pairs / passes
  // 3. narrowphase, 64 pairs per pass
  bool any_manifold_query = false;
  for (int base = 0; base < wn; base += 64) {
    const int i = base + lane; const bool has = i < wn;
    Cand k; k.gap = 3.0e38f; bool near = false; int a = 0, g = 0;
    int b = 0, sub = 0;
    float lim = brk;
    if (has) {
      const int pr = WL[i]; a = pr & 511; b = (pr >> 9) & 511; g = (pr >> 18) & 63; sub = (pr >> 24) & 3;
      // A row is only built for predicted gap = dist + v_n dt < slack, and |v_n| dt is bounded by the travel distances
      // the AABBs were grown by.  Unless the task asks whether a manifold point exists (group flag bit 1), a pair
      // further apart than that is of no interest and its GJK may stop at the first separating axis that proves it
      // (pairs such as two idle fingers 4 mm apart otherwise run to full convergence every substep).
      if (!(GRI(c, g, AGX_G_FLAGS) & (2 | 64))) lim = fminf(brk, slack + rel_travel(c, a, b) + 1e-5f);
    }
    k.n = mk3(0.f, 0.f, 0.f); k.pa = k.n; k.pb = k.n; k.dist = 0.f;
#if AGX_FACE
    // entry 0 of a face pair (AGX_FACE above): the re-anchored first contact, parked in the lane's CD[] slot (point, distance, and in word 0
    // whether there is one -- 1 -- and whether the pair is proven to be a face contact -- 2) until GJK, or the proof, says that it is one;
    // zmin to the pair's other entries.  (Parked in LDS, not in registers: nothing of this is live across gjk_distance.)
    bool proven = false;
    if (has && sub == 0) {
      float* cd = CD + CAND_STRIDE * i; float state = 0.f;
      if (face_box(c, b) && CLI(c, a, AGX_C_NVERT) >= 2) {
        Cand k0; k0.pa = k.pa; k0.dist = 0.f; float zmin;
        const bool first = face_point_wide(c, a, b, 0, k.pa, zmin, k0);
        st3(cd + 1, k0.pa); cd[7] = k0.dist;
#pragma unroll
        for (int q = 1; q <= AGX_FACE_EXTRA; q++) if (i + q < wn) CD[CAND_STRIDE * (i + q)] = zmin;
        state = first ? 1.f : 0.f;
#if AGX_FACE >= 2
        const float* Aa = AB + ABS * a; const float* Bb = AB + ABS * b; const float top = Bb[5], dcore = zmin - top;
        proven = first && Aa[0] >= Bb[0] + FACE_PROOF_GUARD && Aa[3] <= Bb[3] - FACE_PROOF_GUARD && Aa[1] >= Bb[1] + FACE_PROOF_GUARD && Aa[4] <= Bb[4] - FACE_PROOF_GUARD &&
                 Aa[0] <= Aa[3] && Aa[1] <= Aa[4] && Aa[2] - AGX_BOX_CLIP <= top && Aa[5] + AGX_BOX_CLIP >= top && Bb[2] <= top &&
                 dcore > FACE_PROOF_GUARD && dcore - CLF(c, a, AGX_C_RADIUS) - CLF(c, b, AGX_C_RADIUS) < lim - FACE_PROOF_GUARD_LIM;
        if (proven) state = 2.f;
#endif
      }
      cd[0] = state;
    }
    bool hit = narrowphase(c, a, b, lim, k, has && sub == 0 && !proven);
    if (has && sub == 0) {
      const float* cd = CD + CAND_STRIDE * i; const float state = cd[0];
      if (state == 2.f || (state == 1.f && hit && k.n.z > 0.999f)) {
        hit = true; k.n = mk3(0.f, 0.f, 1.f); k.pa = ld3(cd + 1); k.pb = mk3(k.pa.x, k.pa.y, AB[ABS * b + 5]); k.dist = cd[7];
      }
    }
#else
    bool hit = narrowphase(c, a, b, lim, k, has && sub == 0);
    // (timed with every narrowphase run twice, round 4: 473 -> 427 k env-steps/s, the ceiling of any gain here; profiles/r04/r04u_ab_feeding_narrowphase_twice.txt)
    // on a face GJK's closest point is an arbitrary point of the face: the first contact of a pair resting on a static
    // world box is re-anchored at a vertex as well (oracle: face_manifold)
    if (has && sub == 0 && hit && k.n.z > 0.999f && face_box(c, b) && CLI(c, a, AGX_C_NVERT) >= 2) { Cand k0; k0.gap = k.gap; if (face_point(c, a, b, 0, k.pa, k0)) k = k0; }
#endif
    if (wave_any(has && sub > 0)) {   // face-manifold entries: the GJK contact of the pair is `sub` entries back
      if (has && sub == 0) { float* cd = CD + CAND_STRIDE * i; st3(cd + 1, k.pa); st3(cd + 4, k.n); }
      wave_sync();
      if (has && sub > 0) {
        const float* sd = CD + CAND_STRIDE * (i - sub);
#if AGX_FACE
        float zmin = CD[CAND_STRIDE * i];
        hit = sd[6] > 0.999f && face_point_wide(c, a, b, sub, ld3(sd + 1), zmin, k) && k.dist < brk;
#else
        hit = sd[6] > 0.999f && face_point(c, a, b, sub, ld3(sd + 1), k) && k.dist < brk;
#endif
      }
    }
    if (has) {
      if (hit) {
        near = true;
        v3 vr = point_velocity(c, CLI(c, a, AGX_C_BODY), k.pa) - point_velocity(c, CLI(c, b, AGX_C_BODY), k.pb);
        float pg = k.dist + dot(vr, k.n) * c.dt;
        if (pg < ((GRI(c, g, AGX_G_FLAGS) & 64) ? brk : slack)) k.gap = pg;      // bit6: a row for every contact of the group inside the break distance (agx_blob.h)
      }
      float* cd = CD + CAND_STRIDE * i;
      cd[0] = k.gap; st3(cd + 1, k.pa); st3(cd + 4, k.n); cd[7] = k.dist;
    }
    // a manifold point exists: what getContactPoints(food, human) reports (agent.py:100-116)
    if constexpr (TASK == AGX_TASK_FEEDING) {
      const bool mq = has && near && (GRI(c, g, AGX_G_FLAGS) & 2) && CLI(c, a, AGX_C_TAG) == AGX_TAG_FOOD;
      if (wave_any(mq)) { any_manifold_query = true; for (int f = 0; f < c.nfood; f++) if (wave_any(mq && CLI(c, a, AGX_C_BODY) - AGX_BODY_FREE0 - food0 == f)) cs.near_mask |= 1 << f; }
    }
    if constexpr (TASK != AGX_TASK_FEEDING) {
      // manifold points of the wiping pad / the scratcher's tool links on the human: what tool.get_contact_points(human) reports for
      // those linkA, whether or not they carry force (bed_bathing.py:47-58, scratch_itch.py:51-57); the point on the human and the
      // human's link go to the finish kernel
      const bool qp = has && near && (GRI(c, g, AGX_G_FLAGS) & 2) && CLI(c, a, AGX_C_TAG) == AGX_TAG_TOOL && (TKI(c, AGX_T_PAD_LINK) >> (CLI(c, a, AGX_C_LINK) + 1) & 1) &&
                      CLI(c, b, AGX_C_TAG) == AGX_TAG_HUMAN;
      const uint64_t qm = wave_ballot(qp);
      const int slot = cs.nqpt + wave_rank(qm);
      if (qp && slot < MAX_QPT) { float* o = c.gqpt + QPT_STRIDE * slot; st3(o, k.pb); ((int*)o)[3] = CLI(c, b, AGX_C_LINK); }
      cs.nqpt += popc64(qm);
    }
  }
  (void)any_manifold_query;
  wave_sync();
  if (c.timing) { long long t = wave_clock(); c.tm[11] += t - ct0; ct0 = t; }
  // 4. selection per (group, A collider) segment: in one pass over the whole list (AGX_COLLIDE_FRONT), or one segment at a time in the loop
  // below (-DAGX_COLLIDE_FRONT=0, and any flush with a run of more than 128 entries).  Either only decides which candidate
  // becomes which contact slot (SEL[]); the contact records are then written by one lane per contact, so
  // that their blob reads (bodies, friction) overlap instead of queueing up behind each other.
  int* SEL = c.ldsi + L_ARENA + A_CAND + CAND_STRIDE * WL_CAP;      // the sweep's lists are dead by now
  const int ncon0 = cs.ncon;
  int cur = 0;
#if AGX_FRONT_SELECT
  // one pass (AGX_COLLIDE_FRONT above): lane l holds the entries l, l + 64, ...; a segment is a run of entries with the same key
  constexpr int SEL_R = (WL_CAP + 63) / 64;
  uint64_t SB[SEL_R], QB[SEL_R];      // segment starts, selected entries
#pragma unroll
  for (int r = 0; r < SEL_R; r++) {
    const int i = 64 * r + lane;
    SB[r] = wave_ballot(i < wn && (i == 0 || ((WL[i > 0 ? i - 1 : 0] ^ WL[i < wn ? i : 0]) & WL_KEY_MASK) != 0));
  }
  int total = 0, seg0[SEL_R], rank[SEL_R]; bool longrun = false;
#pragma unroll
  for (int r = 0; r < SEL_R; r++) {
    const int i = 64 * r + lane; const bool has = i < wn;
    int s = 0, e = wn;      // the last start at or before the entry, the first one behind it
#pragma unroll
    for (int q = 0; q <= r; q++) { const uint64_t m = q < r ? SB[q] : SB[q] & (~0ull >> (63 - lane)); if (m) s = 64 * q + 63 - clz64(m); }
#pragma unroll
    for (int q = SEL_R - 1; q >= r; q--) { const uint64_t m = q > r ? SB[q] : (lane < 63 ? SB[q] & (~0ull << (lane + 1)) : 0ull); if (m) e = 64 * q + ffs64(m); }
    longrun = longrun || (has && e - s > 128);
    const float gi = has ? CD[CAND_STRIDE * i] : 3.0e38f;
    const int keep = wave_shfl_i(G.keep, has ? (WL[i] >> 18) & 63 : 0);
    int rk = 0;
    if (gi < 1.0e38f) {
      if (keep == 0) { for (int j = s; j < i; j++) rk += CD[CAND_STRIDE * j] < 1.0e38f ? 1 : 0; }      // everything, in enumeration order
      else for (int j = s; j < e; j++) { const float gj = CD[CAND_STRIDE * j]; rk += (gj < gi || (gj == gi && j < i)) ? 1 : 0; }   // equal gaps: the lower index first
    }
    seg0[r] = s; rank[r] = rk;
    QB[r] = wave_ballot(gi < 1.0e38f && (keep == 0 || rk < keep));
    total += popc64(QB[r]);
  }
  // a run of more than 128 entries is cut there and its remainder selected on its own: left to the loop below, with everything else of this flush
  if (!wave_any(longrun)) {
#pragma unroll
    for (int r = 0; r < SEL_R; r++) {
      if (!(QB[r] >> lane & 1)) continue;
      int before = 0;      // selected entries of the earlier segments
#pragma unroll
      for (int q = 0; q <= r; q++) { const int d = seg0[r] - 64 * q; before += d <= 0 ? 0 : popc64(d >= 64 ? QB[q] : QB[q] & ((1ull << d) - 1ull)); }
      const int slot = ncon0 + before + rank[r];
      if (slot < cs.maxc) SEL[slot - ncon0] = 64 * r + lane;
    }
    int room = cs.maxc - cs.ncon; if (room < 0) room = 0;
    if (total > room) { cs.overflow += total - room; total = room; }
    cs.ncon += total;
    cur = wn;
  }
#endif
  while (cur < wn) {
    const int key = WL[cur] & WL_KEY_MASK;            // group and A collider
    const int g = (key >> 18) & 63, keep = wave_bcast_i(G.keep, g);
    const int i0 = cur + lane, i1 = cur + 64 + lane;
    const bool s0 = i0 < wn && (WL[i0 < wn ? i0 : 0] & WL_KEY_MASK) == key, s1 = i1 < wn && (WL[i1 < wn ? i1 : 0] & WL_KEY_MASK) == key;
    const uint64_t b0 = wave_ballot(s0), b1 = wave_ballot(s1);
    // segments are contiguous: the run of matching entries starting at cur
    const int len0 = (~b0) ? ffs64(~b0) : 64;
    const int len = len0 < 64 ? len0 : 64 + ((~b1) ? ffs64(~b1) : 64);
    const bool in0 = lane < len, in1 = 64 + lane < len;
    float g0 = in0 ? CD[CAND_STRIDE * i0] : 3.0e38f, g1 = in1 ? CD[CAND_STRIDE * i1] : 3.0e38f;
    if (keep == 0) {   // keep everything, in enumeration order
      for (int pass = 0; pass < 2; pass++) {
        const bool has = (pass ? g1 : g0) < 1.0e38f;
        const uint64_t m = wave_ballot(has);
        int cnt = popc64(m); const int slot = cs.ncon + wave_rank(m);
        if (has && slot < cs.maxc) SEL[slot - ncon0] = pass ? i1 : i0;
        int room = cs.maxc - cs.ncon; if (room < 0) room = 0;
        if (cnt > room) { cs.overflow += cnt - room; cnt = room; }
        cs.ncon += cnt;
      }
    } else {           // the `keep` smallest predicted gaps, in selection order
      for (int q = 0; q < keep; q++) {
        const float mg = wave_min(fminf(g0, g1));
        if (mg > 1.0e38f) break;
        const uint64_t m0 = wave_ballot(g0 == mg);
        int slot1 = 0, win;
        if (m0) win = ffs64(m0); else { win = ffs64(wave_ballot(g1 == mg)); slot1 = 1; }
        if (cs.ncon < cs.maxc) { if (lane == win) SEL[cs.ncon - ncon0] = slot1 ? i1 : i0; cs.ncon++; } else cs.overflow++;
        if (lane == win) { if (slot1) g1 = 3.0e38f; else g0 = 3.0e38f; }
      }
    }
    cur += len;
  }
  wave_sync();
  if (ncon0 + lane < cs.ncon) emit_from_cand(c, ncon0 + lane, SEL[lane]);      // at most MAX_CON = 64 new contacts
  wave_sync();
  if (c.timing) { long long t = wave_clock(); c.tm[12] += t - ct0; }
}

struct SweepStat { int windows, rounds1, rounds2, rounds3; };      // debug path: sweeps (windows) of a substep, their level-1 and level-2 rounds, and the level-2 rounds that ran level 3
#if !AGX_FRONT_SWEEP
// broadphase sweep of A colliders [aa, ab) x B range of group g, appended to the worklist at wn.
// returns the new count (may exceed WL_MAX: entries beyond it are not stored)
AGX_DEV int collide_sweep(Ctx& c, int g, int aa, int ab, int b0, int b1, int gflags, float mg, int wn, int rep, const GroupRegs& G, SweepStat& stat) {
  const float* AB = c.lds + L_ARENA; int* WL = c.ldsi + L_ARENA + A_WL; const int lane = c.lane;
  const bool same = gflags & 1, no_adjacent = gflags & 4;   // bit2, self-collision: not the same link, not parent and child
  // level 1: the A colliders whose box reaches the union box of the B range and vice versa (the union
  // boxes were computed by the group cull, lane g holds them), compacted in ascending order into two
  // index lists (list_t) in the tail of the candidate area (unused until the flush).  Filtering both sides
  // matters for pairs of compounds (64 spoon pieces x 44 wheelchair pieces: a handful of each are close).
  float ulo[2][3], uhi[2][3];
  for (int q = 0; q < 3; q++) { ulo[0][q] = wave_bcast(G.blo[q], g); uhi[0][q] = wave_bcast(G.bhi[q], g); ulo[1][q] = wave_bcast(G.alo[q], g); uhi[1][q] = wave_bcast(G.ahi[q], g); }
  list_t* LIST = (list_t*)(c.ldsi + L_ARENA + A_CAND + CAND_STRIDE * WL_CAP);   // [0,128): A side, [128,256): B side
  int nlive[2] = {0, 0};
  for (int side = 0; side < 2; side++) {
    const int r0 = side == 0 ? aa : b0, r1 = side == 0 ? ab : b1;
    for (int base = r0; base < r1; base += 64) {
      const int x = base + lane; bool ok = x < r1;
      if (ok) for (int q = 0; q < 3; q++) if (AB[ABS * x + q] > uhi[side][q] + mg || ulo[side][q] > AB[ABS * x + 3 + q] + mg) ok = false;
      const uint64_t m = wave_ballot(ok);
      if (ok) LIST[128 * side + nlive[side] + wave_rank(m)] = (list_t)x;
      nlive[side] += popc64(m);
      stat.rounds1++;
    }
  }
  stat.windows++;
  const int na_live = nlive[0], nb = nlive[1];
  wave_sync();
  // level 2: the pair grid of the surviving A colliders, in enumeration order
  // (groups against static world boxes: every pair is enumerated rep = 1 + AGX_FACE_EXTRA times, entry `sub` > 0
  // standing for the sub-th extra point of the face manifold)
  const int npairs = na_live * nb * rep;
  for (int base = 0; base < npairs; base += 64) {
    const int p = base + lane; bool ok = p < npairs;
    const int pq = ok ? p / rep : 0, sub = ok ? p - pq * rep : 0;
    const int ai = pq / nb; const int a = LIST[ai], b = LIST[128 + pq - ai * nb];
    ok = ok && (!same || b > a) && (sub == 0 || (face_box(c, b) && CLI(c, a, AGX_C_NVERT) >= 2));
    if (ok && no_adjacent) {
      const int la = CLI(c, a, AGX_C_BODY), lb = CLI(c, b, AGX_C_BODY);
      if (la == lb) ok = false;
      else if (la >= 0 && la < AGX_BODY_ROBOT_BASE && lb >= 0 && lb < AGX_BODY_ROBOT_BASE && (RBI(c, la, AGX_R_PARENT) == lb || RBI(c, lb, AGX_R_PARENT) == la)) ok = false;
    }
    if (ok) for (int q = 0; q < 3; q++) if (AB[ABS * a + q] > AB[ABS * b + 3 + q] + mg || AB[ABS * b + q] > AB[ABS * a + 3 + q] + mg) ok = false;
    // level 3: bounding sphere of one collider against the body-frame box of the other, both ways
    // (the second test -- b's bounding sphere against a's body-frame box -- cannot reject what the first one passed when a is a sphere: its
    // box is the point itself, so the test degenerates to two bounding spheres; skipped then.  Both tests always: 468 k either way, round 4;
    // profiles/r04/r04q_ab_feeding_one_sided_sphere_cull.txt)
    if (ok) { const float reach = mg + rel_travel(c, a, b) + 1e-5f; ok = !sphere_box_apart(c, a, b, reach) && (CLI(c, a, AGX_C_NVERT) == 1 || !sphere_box_apart(c, b, a, reach)); }
    const uint64_t m = wave_ballot(ok);
    const int slot = wn + wave_rank(m);
    if (ok && slot < WL_CAP) WL[slot] = a | (b << 9) | (g << 18) | (sub << 24);
    wn += popc64(m);
    stat.rounds2++; stat.rounds3++;
  }
  wave_sync();
  return wn;
}
#else
AGX_DEV uint64_t lanes_below(int e) { return e <= 0 ? 0ull : e >= 64 ? ~0ull : (1ull << e) - 1ull; }      // the lanes 0 .. e - 1
// the group (bit of `rem`, lane = group) whose half-open interval of positions holds x: the intervals start at `start` (ascending with the group,
// one behind the other), this round covers the positions [base, base + 64).  Groups that end in front of the round are taken out of rem.
AGX_DEV int window_group(uint64_t& rem, int start, int base, int x, int l) {
  for (uint64_t m = rem; m; m &= m - 1) {
    const int q = ffs64(m), s = wave_bcast_i(start, q);
    if (s >= base + 64) break;
    l = x >= s ? q : l; rem = m;
  }
  return l;
}
// what a sweep of a window accepted: nacc of its groups fit behind the pending entries and end the worklist at wn; over: the group `gnext` behind
// them did not fit (otherwise gnext is the first group behind the window); end0: where the window's first group alone ends the list (not capped)
struct SweepOut { int nacc, wn, end0, gnext; bool over; };
// Broadphase sweep of a window of live groups, appended to the worklist at wn0 (AGX_COLLIDE_FRONT above).  The window: the live groups from g0 on,
// at most maxg of them, as far as their level-1 lists fit the list area; of g0 the A colliders [aa, ab) only (a batch of a split group comes with
// maxg = 1).  Lane = group throughout: the group's parameters and boxes are G's, its list offsets, counts and prefix sums live beside them.
AGX_DEV void collide_sweep_window(Ctx& c, int g0, int aa, int ab, int maxg, uint64_t live_groups, int wn0, float brk, float slack, const GroupRegs& G,
                                  CollideState& cs, SweepOut& o, SweepStat& stat) {
  const float* AB = c.lds + L_ARENA; int* WL = c.ldsi + L_ARENA + A_WL; const int lane = c.lane;
  list_t* LIST = (list_t*)(c.ldsi + L_ARENA + A_CAND + CAND_STRIDE * WL_CAP);   // LIST_CAP indices: the A list, then the B list, of one group after the other
  uint64_t cand = live_groups & (~0ull << g0);
  if (maxg < 64) { uint64_t t = cand; cand = 0; for (int k = 0; k < maxg && t; k++) { cand |= t & (~t + 1ull); t &= t - 1; } }
  const bool in = cand >> lane & 1;
  const int ra0 = lane == g0 ? aa : G.a0, lenA = in ? (lane == g0 ? ab : G.a1) - ra0 : 0, lenB = in ? G.b1 - G.b0 : 0;
  const int mgbit = (G.flags & (2 | 64)) ? 1 : 0;      // the group's margin: brk (bit1: existence query; bit6: every contact inside the break distance), or slack
  // level 1: the colliders whose box reaches the union box of the opposite range (computed by the group cull, lane g holds them), in ascending
  // order.  Position x of the concatenated ranges (A range, then B range, group after group) is one collider of one (group, side).
  int S = 0, T = 0;
  for (uint64_t m = cand; m; m &= m - 1) { const int q = ffs64(m), v = wave_bcast_i(lenA + lenB, q); if (lane == q) S = T; T += v; }
  const int pk1 = ra0 | (G.b0 << 9) | (lenA << 18) | (mgbit << 28);
  int cA = 0, cB = 0, cE = 0;      // list entries in front of this group's A list, its B list, and behind both
  {
    uint64_t rem = cand; int run = 0;
    for (int base = 0; base < T; base += 64) {
      const int x = base + lane;
      const int l = window_group(rem, S, base, x, g0);
      const int pk = wave_shfl_i(pk1, l), xs = x - wave_shfl_i(S, l);
      const bool sideB = xs >= ((pk >> 18) & 1023);
      const int col = sideB ? ((pk >> 9) & 511) + xs - ((pk >> 18) & 1023) : (pk & 511) + xs;
      const float mg = (pk >> 28 & 1) ? brk : slack;
      bool ok = x < T;
      for (int q = 0; q < 3; q++) {
        const float alo = wave_shfl(G.alo[q], l), ahi = wave_shfl(G.ahi[q], l), blo = wave_shfl(G.blo[q], l), bhi = wave_shfl(G.bhi[q], l);
        const float ulo = sideB ? alo : blo, uhi = sideB ? ahi : bhi;
        if (ok && (AB[ABS * col + q] > uhi + mg || ulo > AB[ABS * col + 3 + q] + mg)) ok = false;
      }
      const uint64_t m = wave_ballot(ok);
      const int slot = run + wave_rank(m);
      if (ok && slot < LIST_CAP) LIST[slot] = (list_t)col;
      cA += popc64(m & lanes_below(S - base)); cB += popc64(m & lanes_below(S + lenA - base)); cE += popc64(m & lanes_below(S + lenA + lenB - base));
      run += popc64(m);
      stat.rounds1++;
    }
  }
  // the window ends in front of the first group whose lists do not fit behind the earlier ones
  const uint64_t nofit = wave_ballot(in && cE > LIST_CAP);
  uint64_t win = nofit ? cand & lanes_below(ffs64(nofit)) : cand;
  if (!win) {      // lists longer than the whole area: the group is swept with what fits of them, the rest is counted as overflow
    win = 1ull << g0; cs.overflow += wave_bcast_i(cE, g0) - LIST_CAP;
    cB = cB < LIST_CAP ? cB : LIST_CAP; cE = LIST_CAP;
  }
  const bool w = win >> lane & 1;
  const int nA = cB - cA, nB = cE - cB;
  wave_sync();
  // level 2: one pair grid over the pair counts of the window's groups, one behind the other, in enumeration order (groups against static world
  // boxes: every pair is enumerated rep = 1 + AGX_FACE_EXTRA times, entry `sub` > 0 standing for the sub-th extra point of the face manifold)
  const bool face = w && face_box(c, G.b0);      // B ranges are homogeneous (table boxes, the ground plane, ...)
  const int np = w ? nA * nB * (face ? 1 + AGX_FACE_EXTRA : 1) : 0;
  int P = 0, NP = 0;
  for (uint64_t m = win; m; m &= m - 1) { const int q = ffs64(m), v = wave_bcast_i(np, q); if (lane == q) P = NP; NP += v; }
  const int pk2 = cA | (cB << 9) | (nB << 18) | ((face ? 1 : 0) << 27) | ((G.flags & 1) << 28) | ((G.flags & 4) << 27) | (mgbit << 30);
  const int pend0 = wave_bcast_i(np, g0);
  // The grid runs in two stages.  Stage A, 64 grid points per round, needs the lists and the LDS box table only: the point's group and pair, the
  // `same` rule and the box test with the group's margin; what passes is queued as a worklist word, in order.  Stage B, whenever 64 pairs are
  // queued (and for the rest at the end), runs the tests that read the blob -- the face-point rule for sub > 0, no_adjacent, rel_travel and the two
  // sphere_box_apart -- so that their load chains are paid per 64 box-test survivors and not per 64 grid points.  A conjunction of the same
  // tests in another order, and the queue keeps the order: the same survivors in the same order.
  int* Q = c.ldsi + L_ARENA + A_CAND;      // ring of 128 queued pairs at the head of the candidate area (dead until the flush; the lists are in its tail)
  constexpr int QM = 127;
  static_assert(CAND_STRIDE * WL_CAP >= QM + 1, "the queue of the sweep lies in front of the lists");
  int E = 0, wn = wn0;      // survivors up to the end of this group; of the whole window
  int Aq = 0, qh = 0, qn = 0, popped = 0;      // pairs queued up to the end of this group; head and length of the queue, pairs taken from it
  uint64_t rem = wave_ballot(np > 0);
  for (int base = 0;; base += 64) {
    const bool more = base < NP;
    if (more) {
      const int p = base + lane; bool ok = p < NP;
      const int l = window_group(rem, P, base, p, g0);
      const int pk = wave_shfl_i(pk2, l), ps = wave_shfl_i(P, l), lp = ok ? p - ps : 0;
      const bool rep = pk >> 27 & 1, same = pk >> 28 & 1;
      const float mg = (pk >> 30 & 1) ? brk : slack;
      const int pq = rep ? lp / (1 + AGX_FACE_EXTRA) : lp, sub = rep ? lp - pq * (1 + AGX_FACE_EXTRA) : 0;
      const int nb = ok ? (pk >> 18) & 511 : 1;
      int ai = (int)((float)pq / (float)nb), bi = pq - ai * nb;      // pq < 2^16: the quotient is off by one at most
      if (bi < 0) { ai--; bi += nb; } else if (bi >= nb) { ai++; bi -= nb; }
      const int a = ok ? LIST[(pk & 511) + ai] : 0, b = ok ? LIST[((pk >> 9) & 511) + bi] : 0;
      ok = ok && (!same || b > a);
      if (ok) for (int q = 0; q < 3; q++) if (AB[ABS * a + q] > AB[ABS * b + 3 + q] + mg || AB[ABS * b + q] > AB[ABS * a + 3 + q] + mg) ok = false;
      const uint64_t m = wave_ballot(ok);
      if (ok) Q[(qh + qn + wave_rank(m)) & QM] = a | (b << 9) | (l << 18) | (sub << 24);
      Aq += popc64(m & lanes_below(P + np - base));
      qn += popc64(m);
      stat.rounds2++;
    }
    if (!more && qn == 0) break;
    if (more && qn < 64) continue;
    wave_sync();
    const int n = qn < 64 ? qn : 64;
    bool ok = lane < n;
    const int e = ok ? Q[(qh + lane) & QM] : 0;
    const int a = e & 511, b = (e >> 9) & 511, l = (e >> 18) & 63, sub = (e >> 24) & 3;
    const int pk = wave_shfl_i(pk2, l);
    const bool no_adjacent = pk >> 29 & 1;   // bit2 of the flags, self-collision: not the same link, not parent and child
    const float mg = (pk >> 30 & 1) ? brk : slack;
    ok = ok && (sub == 0 || (face_box(c, b) && CLI(c, a, AGX_C_NVERT) >= 2));
    if (ok && no_adjacent) {
      const int la = CLI(c, a, AGX_C_BODY), lb = CLI(c, b, AGX_C_BODY);
      if (la == lb) ok = false;
      else if (la >= 0 && la < AGX_BODY_ROBOT_BASE && lb >= 0 && lb < AGX_BODY_ROBOT_BASE && (RBI(c, la, AGX_R_PARENT) == lb || RBI(c, lb, AGX_R_PARENT) == la)) ok = false;
    }
    // level 3: bounding sphere of one collider against the body-frame box of the other, both ways
    // (the second test -- b's bounding sphere against a's body-frame box -- cannot reject what the first one passed when a is a sphere: its
    // box is the point itself, so the test degenerates to two bounding spheres; skipped then.  Both tests always: 468 k either way, round 4;
    // profiles/r04/r04q_ab_feeding_one_sided_sphere_cull.txt)
    if (ok) { const float reach = mg + rel_travel(c, a, b) + 1e-5f; ok = !sphere_box_apart(c, a, b, reach) && (CLI(c, a, AGX_C_NVERT) == 1 || !sphere_box_apart(c, b, a, reach)); }
    const uint64_t m = wave_ballot(ok);
    const int slot = wn + wave_rank(m);
    if (ok && slot < WL_CAP) WL[slot] = e;
    E += popc64(m & lanes_below(Aq - popped));      // the queue holds the groups in order: its first Aq pairs are those up to the end of this group
    wn += popc64(m);
    qh = (qh + n) & QM; qn -= n; popped += n;
    stat.rounds3++;
    // the list is full and the first group is complete: the group that does not fit has been seen, and every group in front of it is complete
    if (wn > WL_CAP && base + 64 >= pend0 && popped >= wave_bcast_i(Aq, g0)) break;
  }
  wave_sync();
  stat.windows++;
  // the first group whose end lies beyond the worklist is not accepted, nor is any behind it
  const uint64_t overm = wave_ballot(w && wn0 + E > WL_CAP);
  const uint64_t acc = overm ? win & lanes_below(ffs64(overm)) : win;
  o.over = overm != 0ull; o.nacc = popc64(acc);
  o.gnext = overm ? ffs64(overm) : 64 - clz64(win);
  o.wn = acc ? wn0 + wave_bcast_i(E, 63 - clz64(acc)) : wn0;
  o.end0 = wn0 + wave_bcast_i(E, g0);
}
#endif

#if AGX_FRONT_CULL
// union box of the colliders [r0, r1) (into lo / hi, which hold the identity or an earlier union): the colliders up to the first block boundary,
// the whole blocks in between (their boxes at AB[A_CAND], 2^bsh colliders each), the colliders behind the last boundary.  fminf / fmaxf in
// another order than one collider after the other: the same floats.
AGX_DEV void range_box(const float* AB, int bsh, int r0, int r1, float* lo, float* hi) {
  int bl0 = (r0 + (1 << bsh) - 1) >> bsh, bl1 = r1 >> bsh;
  int h1 = bl0 << bsh, t0 = bl1 << bsh;
  if (bl0 >= bl1) { h1 = r1; t0 = r1; bl1 = bl0; }      // no whole block inside
  for (int i = r0; i < h1; i++) for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], AB[ABS * i + k]); hi[k] = fmaxf(hi[k], AB[ABS * i + 3 + k]); }
  for (int b = bl0; b < bl1; b++) for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], AB[A_CAND + 6 * b + k]); hi[k] = fmaxf(hi[k], AB[A_CAND + 6 * b + 3 + k]); }
  for (int i = t0; i < r1; i++) for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], AB[ABS * i + k]); hi[k] = fmaxf(hi[k], AB[ABS * i + 3 + k]); }
}
#endif

AGX_DEV void collide(Ctx& c) {
  float* L = c.lds; float* AB = L + L_ARENA; const int lane = c.lane;
  const float brk = PRM(c, AGX_P_CONTACT_BREAK), slack = PRM(c, AGX_P_CONTACT_SLACK);
  CollideState cs; cs.ncon = 0; cs.near_mask = 0; cs.overflow = 0; cs.nqpt = 0;
  cs.maxc = (int)PRM(c, AGX_P_MAX_CONTACTS); if (cs.maxc > MAX_CON) cs.maxc = MAX_CON;
  long long ct0 = c.timing ? wave_clock() : 0, ct1;
#define AGX_CTICK(k) if (c.timing) { ct1 = wave_clock(); c.tm[k] += ct1 - ct0; ct0 = ct1; }
  // 1. world AABBs, grown by the distance the collider can travel in this substep (speculative):
  //    the broadphase margin then only has to cover the solver slack
  if (lane < MAX_DOF + MAX_FREE) {     // twist and angular speed of every moving body, once (the chain walk is per body, not per collider)
    v3 w = mk3(0, 0, 0), v = w;
    if (lane < MAX_DOF) { if (lane < c.ndof) for (int d = lane; d >= 0; d = RBI(c, d, AGX_R_PARENT)) { const float qd = L[L_VEL + d]; w = w + qd * ld3(L + L_S + 6 * d); v = v + qd * ld3(L + L_S + 6 * d + 3); } }
    else if (lane - MAX_DOF < c.nfree) {
      const int fb = lane - MAX_DOF, o = c.ndof + 6 * fb;
      w = ld3(L + L_VEL + o + 3);
      v = ld3(L + L_VEL + o) + cross(w, ld3(L + L_MISC + M_REF) - ld3(L + L_ST + c.s_free + 13 * fb));
    }
    L[L_WMAG + lane] = sqrtf(dot(w, w));
    st3(AB + A_TW + 6 * lane, w); st3(AB + A_TW + 6 * lane + 3, v);
  }
  wave_sync();
  for (int col = lane; col < c.ncoll; col += 64) {
    const int code = CLI(c, col, AGX_C_BODY);
    m3 R; v3 p; body_xf(c, code, R, p);
    v3 cl = mk3(CLF(c, col, AGX_C_AABB_C), CLF(c, col, AGX_C_AABB_C + 1), CLF(c, col, AGX_C_AABB_C + 2));
    v3 hl = mk3(CLF(c, col, AGX_C_AABB_H), CLF(c, col, AGX_C_AABB_H + 1), CLF(c, col, AGX_C_AABB_H + 2));
    v3 cw = mul(R, cl) + p; float r = CLF(c, col, AGX_C_RADIUS);
    v3 vc = point_velocity(c, code, cw);
    const float wmag = body_wmag(c, code);
    const float grow = (sqrtf(dot(vc, vc)) + wmag * (sqrtf(dot(hl, hl)) + r)) * c.dt;
    for (int k = 0; k < 3; k++) {
      float h = fabsf(R.a[3 * k]) * hl.x + fabsf(R.a[3 * k + 1]) * hl.y + fabsf(R.a[3 * k + 2]) * hl.z + r;
      AB[ABS * col + k] = comp(cw, k) - h - grow; AB[ABS * col + 3 + k] = comp(cw, k) + h + grow;
    }
    AB[ABS * col + 6] = grow;
  }
  wave_sync();
  AGX_CTICK(8)
  const int gender = c.ldsi[L_ST + c.s_env + AGX_E_GENDER];
#if AGX_FRONT_CULL
  // the boxes of 64 blocks of 2^bsh consecutive colliders, lane l = block l (AGX_COLLIDE_FRONT above)
  int bsh = 0; while ((64 << bsh) < c.ncoll) bsh++;
  {
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    const int i0 = lane << bsh, i1 = i0 + (1 << bsh) < c.ncoll ? i0 + (1 << bsh) : c.ncoll;
    for (int i = i0; i < i1; i++) for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], AB[ABS * i + k]); hi[k] = fmaxf(hi[k], AB[ABS * i + 3 + k]); }
    for (int k = 0; k < 3; k++) { AB[A_CAND + 6 * lane + k] = lo[k]; AB[A_CAND + 6 * lane + 3 + k] = hi[k]; }
  }
  wave_sync();
#endif
  // body-level cull of every group at once: lane g builds the union boxes of both collider ranges of group g
  uint64_t live_groups = 0;
  GroupRegs G; G.a0 = 0; G.a1 = 0; G.b0 = 0; G.b1 = 0; G.flags = 0; G.keep = 0;
  for (int k = 0; k < 3; k++) { G.alo[k] = 0.f; G.ahi[k] = 0.f; G.blo[k] = 0.f; G.bhi[k] = 0.f; }
  {
    const int g = lane; bool live = false;
    if (g < c.ngroup) {
      G.a0 = GRI(c, g, AGX_G_A0); G.a1 = GRI(c, g, AGX_G_A1); G.b0 = GRI(c, g, AGX_G_B0); G.b1 = GRI(c, g, AGX_G_B1);
      if (gender == 1 && GRI(c, g, AGX_G_B0F) >= 0) { G.b0 = GRI(c, g, AGX_G_B0F); G.b1 = GRI(c, g, AGX_G_B1F); }
      G.flags = GRI(c, g, AGX_G_FLAGS); G.keep = GRI(c, g, AGX_G_KEEP);
      const int a0 = G.a0, a1 = G.a1, b0 = G.b0, b1 = G.b1;
      const float mg = (G.flags & (2 | 64)) ? brk : slack;
      // bit3 / bit4: male / female only; bit5: only while some human DoF is dynamic
      const bool wanted = !((G.flags & 8) && gender != 0) && !((G.flags & 16) && gender != 1) &&
                          !((G.flags & 32) && c.nrobot + c.nhdof <= 32 && ((~c.frozen >> c.nrobot) & ((1u << c.nhdof) - 1u)) == 0);
      if (a1 > a0 && b1 > b0 && wanted) {
        float alo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, ahi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, blo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, bhi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
#if AGX_FRONT_CULL
        range_box(AB, bsh, a0, a1, alo, ahi); range_box(AB, bsh, b0, b1, blo, bhi);
#else
        for (int i = a0; i < a1; i++) for (int k = 0; k < 3; k++) { alo[k] = fminf(alo[k], AB[ABS * i + k]); ahi[k] = fmaxf(ahi[k], AB[ABS * i + 3 + k]); }
        for (int i = b0; i < b1; i++) for (int k = 0; k < 3; k++) { blo[k] = fminf(blo[k], AB[ABS * i + k]); bhi[k] = fmaxf(bhi[k], AB[ABS * i + 3 + k]); }
#endif
        live = true;
        for (int k = 0; k < 3; k++) if (alo[k] > bhi[k] + mg || blo[k] > ahi[k] + mg) live = false;
        for (int k = 0; k < 3; k++) { G.alo[k] = alo[k]; G.ahi[k] = ahi[k]; G.blo[k] = blo[k]; G.bhi[k] = bhi[k]; }
      }
    }
    live_groups = wave_ballot(live);   // the pair table has at most 64 groups (checked in agx_create)
  }
  AGX_CTICK(9)
  // 2.-4. The work is a sequence of units (group, range of its A colliders), normally one unit per
  // live group.  Units are swept into the shared worklist until one does not fit behind the pending
  // entries; then the pending entries are flushed (narrowphase + selection) and the unit is retried
  // on the empty list, split into batches of whole A colliders if it still does not fit.  One sweep
  // and one flush call site keep the kernel's code size down.
  // (AGX_FRONT_SWEEP: one sweep takes a window of whole groups and accepts those that fit; the first one that does not is the unit that is
  // retried, so the flushes fall where they fall one group at a time.  A batch of a split group is a window of its own.)
  int wn = 0, g = 0, ab = -1, abatch = 0;
  SweepStat stat; stat.windows = 0; stat.rounds1 = 0; stat.rounds2 = 0; stat.rounds3 = 0;
  while (true) {
    while (g < c.ngroup && !(live_groups >> g & 1)) g++;
    if (g >= c.ngroup) {
      if (wn == 0) break;
    } else {
      const int a0 = wave_bcast_i(G.a0, g), a1 = wave_bcast_i(G.a1, g), b0 = wave_bcast_i(G.b0, g), b1 = wave_bcast_i(G.b1, g);
      const int gflags = wave_bcast_i(G.flags, g);
      const float mg = (gflags & (2 | 64)) ? brk : slack;   // bit1: getContactPoints-style existence query; bit6: every contact inside the break distance is solved
      const int rep = face_box(c, b0) ? 1 + AGX_FACE_EXTRA : 1;   // B ranges are homogeneous (table boxes, the ground plane, ...)
      const int nb = (b1 - b0) * rep;
      if (ab < 0) { ab = a0; abatch = a1 - a0; }
      const int ae = ab + abatch < a1 ? ab + abatch : a1;
#if AGX_FRONT_SWEEP
      SweepOut so;
      collide_sweep_window(c, g, ab, ae, (ab > a0 || ae < a1) ? 1 : SWEEP_WINDOW, live_groups, wn, brk, slack, G, cs, so, stat);
      bool fits = so.nacc > 0, cut = fits && so.over;   // cut: the group behind the accepted ones does not fit behind them
      int wn2 = fits ? so.wn : so.end0, gnext = so.gnext;
      (void)gflags; (void)mg;
#else
      int wn2 = collide_sweep(c, g, ab, ae, b0, b1, gflags, mg, wn, rep, G, stat);
      bool fits = wn2 <= WL_CAP, cut = false; int gnext = g + 1;
#endif
      AGX_CTICK(10)
      if (!fits && wn == 0) {
        const int small = WL_CAP / nb > 0 ? WL_CAP / nb : 1;   // a batch of WL_CAP / nb colliders cannot overflow
        if (abatch > small) { abatch = small; continue; }       // retry this unit in smaller batches
        cs.overflow += wn2 - WL_CAP; wn2 = WL_CAP; fits = true; gnext = g + 1; cut = false;  // a single A collider with more than WL_CAP partners
      }
      if (fits) {
        wn = wn2; ab = ae;
        if (ab >= a1) { g = gnext; ab = -1; }
        // a unit that was split is flushed batch by batch; whole groups keep accumulating
        if (ab < 0 && !cut) continue;
      }
    }
    collide_flush(c, wn, cs, brk, slack, G); wn = 0;
    ct0 = c.timing ? wave_clock() : 0;
  }
  // debug: sweeps (windows) of this substep, their level-2 and level-1 rounds, live groups (tools/gpu_build_phases.py, tests/test_emu_collide_sweep.py)
  if (c.timing) c.tm[15] += stat.rounds3;      // ... and the rounds of the blob-reading tests (level 3)
  if (c.timing && lane == 0) { c.dbg[DBG_TIME + 20] = (float)stat.windows; c.dbg[DBG_TIME + 21] = (float)stat.rounds2; c.dbg[DBG_TIME + 22] = (float)stat.rounds1; c.dbg[DBG_TIME + 23] = (float)popc64(live_groups); }
  c.ncon = cs.ncon; c.near_mask = cs.near_mask; c.overflow = cs.overflow; c.nqpt = cs.nqpt < MAX_QPT ? cs.nqpt : MAX_QPT;
  wave_sync();
#undef AGX_CTICK
}

}  // namespace agx
