// agx_env.h -- K7 integration and hooks, state load / store, warm start, persistent manifold and the bodies of the build and solve kernels
// (the task layer and the bodies of the observe and finish kernels: agx_task.h).
// Part of the stepper (see agx_step.h for the overview); included by agx_step.h only.
#pragma once

namespace agx {

// ---- K7 + post-substep hooks -----------------------------------------------------------------------------
AGX_DEV void integrate(Ctx& c, const float* gvel, float dv0, float dv1) {
  float* L = c.lds; const int lane = c.lane, n = c.ndof; const float dt = c.dt;
  L[L_VEL + lane] = gvel[lane] + dv0;
  L[L_VEL + lane + 64] = gvel[lane + 64] + dv1;
  wave_sync();
  if (lane < n) {
    const int d = lane;
    float qd = L[L_VEL + d], q = L[L_ST + c.s_q + d] + dt * qd;
    // Agent.enforce_joint_limits on the human after every stepSimulation (env.py:229, agent.py:240-250)
    if (c.hooks && (RBI(c, d, AGX_R_KIND) & 5) == 1 && !FROZEN(c, d)) {
      const float lo = DLO(c, d), hi = DHI(c, d);
      if (q < lo - AGX_LIMIT_EPS) { q = lo; qd = 0.f; } else if (q > hi + AGX_LIMIT_EPS) { q = hi; qd = 0.f; }
    }
    L[L_ST + c.s_qd + d] = qd; L[L_ST + c.s_q + d] = q;
  }
  if (lane < c.nfree) {
    const int b = lane, o = n + 6 * b; float* r = L + L_ST + c.s_free + 13 * b;
    v3 v = ld3(L + L_VEL + o), w = ld3(L + L_VEL + o + 3);
    st3(r + 7, v); st3(r + 10, w); st3(r, ld3(r) + dt * v);
    float wn = sqrtf(dot(w, w)), th = wn * dt; float dq[4];
    if (th > 1e-12f) { float sc = sinf(0.5f * th) / wn; dq[0] = w.x * sc; dq[1] = w.y * sc; dq[2] = w.z * sc; dq[3] = cosf(0.5f * th); }
    else { dq[0] = 0.5f * dt * w.x; dq[1] = 0.5f * dt * w.y; dq[2] = 0.5f * dt * w.z; dq[3] = 1.f; }
    const float ax = dq[0], ay = dq[1], az = dq[2], aw = dq[3], bx = r[3], by = r[4], bz = r[5], bw = r[6];
    float x = aw * bx + ax * bw + ay * bz - az * by, y = aw * by - ax * bz + ay * bw + az * bx;
    float z = aw * bz + ax * by - ay * bx + az * bw, w2 = aw * bw - ax * bx - ay * by - az * bz;
    float nn = 1.0f / sqrtf(x * x + y * y + z * z + w2 * w2);
    r[3] = x * nn; r[4] = y * nn; r[5] = z * nn; r[6] = w2 * nn;
  }
  wave_sync();
}
// Human.enforce_realistic_joint_limits (human.py:134-152) after Agent.enforce_joint_limits (env.py:229-231): the four arm angles,
// remapped as the training data was (human.py:142-145), go through the Keras classifier Dense(4->64, tanh) x3 -> Dense(64->1,
// sigmoid) (assets/realistic_arm_limits_model.h5, weights in the blob's MLP section).  Class 1 (sigma > 0.5 <=> logit > 0): the pose
// is remembered; class 0: the four joints are put back to the last valid pose with zero velocity (set_joint_angles, agent.py:154-156).
// lane = hidden unit; the activations of a layer are exchanged through 64 words of LDS (`X`, dead storage of the caller).
AGX_DEV void arm_limits(Ctx& c, float* X) {
  if (!TKI(c, AGX_T_ARM_LIMIT_ON) || !c.hooks) return;
  float* L = c.lds; int* Li = c.ldsi; const int lane = c.lane;
  const float* W1 = c.bf + c.bi[AGX_H_OFF_MLP]; const float* W2 = W1 + 4 * 64 + 64; const float* W3 = W2 + 64 * 64 + 64; const float* W4 = W3 + 64 * 64 + 64;
  const int s_task = c.bi[AGX_H_S_TASK];
  const float sg = TKF(c, AGX_T_ARM_LIMIT_SIGN), TWO_PI = 6.28318530717959f;
  int dof[4]; float a[4];
  for (int k = 0; k < 4; k++) {
    dof[k] = TKI(c, AGX_T_ARM_LIMIT_DOF + k);
    // the reference reads the angles after its strict limit reset; here the reset has the tolerance AGX_LIMIT_EPS, so clamp what is read
    a[k] = wave_clamp(L[L_ST + c.s_q + dof[k]], DLO(c, dof[k]), DHI(c, dof[k]));
  }
  const float x0 = sg * a[0] + TWO_PI, x1 = a[1] + TWO_PI, x2 = sg * a[2], x3 = -a[3] + TWO_PI;
  const float in0 = x0 - TWO_PI * floorf(x0 / TWO_PI), in1 = x1 - TWO_PI * floorf(x1 / TWO_PI), in3 = x3 - TWO_PI * floorf(x3 / TWO_PI);
  float h = W1[256 + lane] + in0 * W1[lane] + in1 * W1[64 + lane] + x2 * W1[128 + lane] + in3 * W1[192 + lane];
  h = tanhf(h);
  for (int layer = 0; layer < 2; layer++) {
    const float* W = layer == 0 ? W2 : W3;
    wave_sync(); X[lane] = h; wave_sync();
    float acc = W[4096 + lane];
    for (int k = 0; k < 64; k++) acc += X[k] * W[64 * k + lane];
    h = tanhf(acc);
  }
  const float z = wave_sum(h * W4[lane]) + W4[64];
  wave_sync();
  if (lane == 0) {
    if (z > 0.f) {
      for (int k = 0; k < 4; k++) L[L_ST + s_task + AGX_BB_PREV + k] = L[L_ST + c.s_q + dof[k]];
      Li[L_ST + s_task + AGX_BB_HAS_PREV] = 1;
    } else if (Li[L_ST + s_task + AGX_BB_HAS_PREV]) {
      for (int k = 0; k < 4; k++) {
        L[L_ST + c.s_q + dof[k]] = wave_clamp(L[L_ST + s_task + AGX_BB_PREV + k], DLO(c, dof[k]), DHI(c, dof[k]));
        L[L_ST + c.s_qd + dof[k]] = 0.f;
      }
    }
  }
  wave_sync();
}
// FeedingEnv.update_targets (feeding.py:192-196): mouth = head pose o mouth offset.  Needs the link
// frames of a preceding kinematics(); the target is only consumed by the observation / reward code.
AGX_DEV void update_target(Ctx& c) {
  float* L = c.lds;
  wave_sync();
  if ((TASK == AGX_TASK_FEEDING || TASK == AGX_TASK_DRINKING) && c.lane == 0) {      // (drinking.py:192-196: the same target, and the head moves there)
    const int hl = TKI(c, AGX_T_HEAD_LINK), o = c.gender == 1 ? AGX_T_MOUTH_F : AGX_T_MOUTH_M;
    st3(L + L_ST + c.s_env + AGX_E_TARGET, mul(ldm3(L + L_LINKR + 9 * hl), mk3(TKF(c, o), TKF(c, o + 1), TKF(c, o + 2))) + ld3(L + L_LINKP + 3 * hl));
  }
  wave_sync();
}

// ---- state load / store ---------------------------------------------------------------------------------
AGX_DEV void load_env(Ctx& c, const float* gstate, int sw) {
  float* L = c.lds; const int lane = c.lane;
  for (int k = lane; k < sw; k += 64) L[L_ST + k] = gstate[k];
  wave_sync();
  c.gender = c.ldsi[L_ST + c.s_env + AGX_E_GENDER]; c.frozen = c.ldsi[L_ST + c.s_env + AGX_E_FROZEN];
  { const float ls = c.lds[L_ST + c.s_env + AGX_E_LIMIT_SCALE]; c.limit_scale = ls > 0.f ? ls : 1.f; }   // records written before v6 carry 0
  c.coop = TKI(c, AGX_T_COOP) == 1;
  if (lane == 0) { const float* r = L + L_ST + c.s_base; st3(L + L_BASE, ld3(r)); stm3(L + L_BASE + 3, quat_to_m3(r[3], r[4], r[5], r[6])); }
  if (lane < c.nhuman) { const float* r = L + L_ST + c.s_human + 7 * lane; float* h = L + L_HUMAN + 12 * lane; st3(h, ld3(r)); stm3(h + 3, quat_to_m3(r[3], r[4], r[5], r[6])); }
  if (lane < c.ndof) {
    uint64_t m = 0; for (int d = lane; d >= 0; d = RBI(c, d, AGX_R_PARENT)) m |= 1ull << d;
    c.ldsi[L_MISC + M_ANC + ANC_WORDS * lane] = (int)(uint32_t)m;
    if (ANC_WORDS == 2) c.ldsi[L_MISC + M_ANC + 2 * lane + 1] = (int)(uint32_t)(m >> 32);
  }
  wave_sync();
}
AGX_DEV void store_env(Ctx& c, float* gstate, int sw) {
  wave_sync();
  for (int k = c.lane; k < sw; k += 64) gstate[k] = c.lds[L_ST + k];
}

// ============================================================================================
// Kernel bodies.  One env.step() = frame_skip x [build, solve] + finish:
//   build  (register/LDS heavy, ~1/3 of the time): state -> kinematics, ABA + M^-1, predicted
//          velocities, collision, constraint rows -> per-env scratch record (rows, v*, contacts)
//   solve  (lean: ~64 VGPRs, 5 KB LDS -> many waves per SIMD): 50 PGS sweeps streaming the rows
//          from L2, integration, mouth-target update -> state
//   finish (once per step): forces, observation, food state machine, preferences, reward, done.
// ============================================================================================
struct Scratch { float* ent; float* hdr; float* vel; float* con; int* meta; float* qpt; float* warm; float* man; };
AGX_DEV Scratch scratch_of(float* base) {
  Scratch s; s.ent = base + SCR_O_ENT; s.hdr = base + SCR_O_HDR; s.vel = base + SCR_O_VEL; s.con = base + SCR_O_CON; s.meta = (int*)(base + SCR_O_META); s.qpt = base + SCR_O_QPT; s.warm = base + SCR_O_WARM; s.man = base + SCR_O_MAN;
  return s;
}

// ---- warm starting (AGX_P_WARMSTART, a [BULLET-UNVERIFIED] switch, default off) -------------------------------------------------------
// key of this lane's contact: collider a | collider b << 9 | ordinal among the contacts of the same pair << 18 (the face manifold gives a pair
// up to four); lanes >= ncon return -1.  Wave-uniform call.
AGX_DEV int warm_key(const Ctx& c, int lane) {
  const bool has = lane < c.ncon;
  const int* ki = (const int*)(c.gcon + CON_STRIDE * (has ? lane : 0));
  const int pair = has ? (ki[C_CA] | (ki[C_CB] << 9)) : -1;
  int ord = 0;
  for (int j = 0; j < c.ncon; j++) { const int pj = wave_bcast_i(pair, j); if (has && j < lane && pj == pair) ord++; }
  return has ? (pair | (ord << 18)) : -1;
}
// build kernel, after the contacts of the substep are in the scratch record: C_LAM := factor x the impulse of the same contact in the memory
AGX_DEV void warm_seed(const Ctx& c, const Scratch& scr, int lane) {
  const float wsf = PRM(c, AGX_P_WARMSTART);
  if (!(wsf > 0.f)) return;
  const int nw = scr.meta[META_NWARM];
  const int key = warm_key(c, lane);
  float lam = 0.f;
  for (int p = 0; p < nw && p < MAX_CON; p++) if (((const int*)scr.warm)[p] == key) { lam = wsf * scr.warm[MAX_CON + p]; break; }
  if (lane < c.ncon) c.gcon[CON_STRIDE * lane + C_LAM] = lam;
}
// solve kernel, after the sweeps: this substep's contacts and their solved impulses become the memory
AGX_DEV void warm_remember(const Ctx& c, const Scratch& scr, int lane) {
  if (!(PRM(c, AGX_P_WARMSTART) > 0.f)) return;
  const int key = warm_key(c, lane);
  if (lane < c.ncon) { ((int*)scr.warm)[lane] = key; scr.warm[MAX_CON + lane] = c.gcon[CON_STRIDE * lane + C_LAM]; }
  if (lane == 0) scr.meta[META_NWARM] = c.ncon;
}

// ---- persistent contact manifold (AGX_P_MANIFOLD, a [BULLET-UNVERIFIED] switch, default off; include/agx_blob.h) ---------------------------
// Build kernel, after collide(): the substep's GJK contacts (c.gcon[0 .. c.ncon)) update the cached points of the environment (scratch record,
// lane = cached point while they are in registers) and the contact list is rebuilt from the cache.  Contacts on a static world box keep their
// face manifold and pass through.  Mirrors manifold_update() of oracle/agx_oracle.c step by step (same order, same tie breaks).
struct MPoint { int key; v3 la, lb, n; float dist, mu; };
AGX_DEV MPoint mp_bcast(const MPoint& e, int src) {
  MPoint r; r.key = wave_bcast_i(e.key, src);
  r.la = mk3(wave_bcast(e.la.x, src), wave_bcast(e.la.y, src), wave_bcast(e.la.z, src)); r.lb = mk3(wave_bcast(e.lb.x, src), wave_bcast(e.lb.y, src), wave_bcast(e.lb.z, src));
  r.n = mk3(wave_bcast(e.n.x, src), wave_bcast(e.n.y, src), wave_bcast(e.n.z, src)); r.dist = wave_bcast(e.dist, src); r.mu = wave_bcast(e.mu, src);
  return r;
}
AGX_DEV void manifold_update(Ctx& c, const Scratch& scr) {
  const int lane = c.lane;
  const float brk = PRM(c, AGX_P_CONTACT_BREAK), slack = PRM(c, AGX_P_CONTACT_SLACK);
  int maxc = (int)PRM(c, AGX_P_MAX_CONTACTS); if (maxc > MAX_CON) maxc = MAX_CON;
  float* MP = scr.man;
  int nm = scr.meta[META_NMAN]; if (nm > MAX_CON) nm = MAX_CON;
  // (1) refresh (lane = cached point), order-preserving compaction through the scratch record
  MPoint e; e.key = -1; e.la = mk3(0, 0, 0); e.lb = e.la; e.n = e.la; e.dist = 0.f; e.mu = 0.f;
  bool keep = false;
  if (lane < nm) {
    const float* q = MP + MP_STRIDE * lane;
    e.key = ((const int*)q)[MP_KEY]; e.la = ld3(q + MP_LA); e.lb = ld3(q + MP_LB); e.n = ld3(q + MP_N); e.mu = q[MP_MU];
    m3 Ra, Rb; v3 oa, ob; body_xf(c, CLI(c, e.key & 511, AGX_C_BODY), Ra, oa); body_xf(c, CLI(c, (e.key >> 9) & 511, AGX_C_BODY), Rb, ob);
    const v3 pa = mul(Ra, e.la) + oa, pb = mul(Rb, e.lb) + ob;
    e.dist = dot(pa - pb, e.n);
    const v3 drift = pb - (pa - e.dist * e.n);
    keep = e.dist <= brk && dot(drift, drift) <= brk * brk;
  }
  wave_sync();
  {
    const uint64_t km = wave_ballot(keep);
    if (keep) { float* q = MP + MP_STRIDE * wave_rank(km); ((int*)q)[MP_KEY] = e.key; st3(q + MP_LA, e.la); st3(q + MP_LB, e.lb); st3(q + MP_N, e.n); q[MP_DIST] = e.dist; q[MP_MU] = e.mu; }
    nm = popc64(km);
  }
  wave_sync();
  e.key = -1;
  if (lane < nm) { const float* q = MP + MP_STRIDE * lane; e.key = ((const int*)q)[MP_KEY]; e.la = ld3(q + MP_LA); e.lb = ld3(q + MP_LB); e.n = ld3(q + MP_N); e.dist = q[MP_DIST]; e.mu = q[MP_MU]; }
  // (2) merge the substep's contacts, one after the other (every lane reads the same record)
  const int nnew = c.ncon;
  for (int i = 0; i < nnew; i++) {
    const float* k = c.gcon + CON_STRIDE * i; const int* ki = (const int*)k;
    const int ca = ki[C_CA], cb = ki[C_CB];
    if (face_box(c, cb)) continue;
    MPoint q; q.key = ca | (cb << 9); q.n = ld3(k + C_N); q.dist = k[C_DIST]; q.mu = k[C_MU];
    { m3 Ra, Rb; v3 oa, ob; body_xf(c, ki[C_BA], Ra, oa); body_xf(c, ki[C_BB], Rb, ob); q.la = tmul(Ra, ld3(k + C_PA) - oa); q.lb = tmul(Rb, ld3(k + C_PB) - ob); }
    const bool match = lane < nm && e.key == q.key;
    const v3 dl = e.la - q.la; const float d2 = dot(dl, dl);
    const bool close = match && d2 < brk * brk;
    const float dmin = wave_min(close ? d2 : 3.0e38f);
    int target = -1;
    const uint64_t mm = wave_ballot(match);
    if (dmin < 3.0e38f) target = ffs64(wave_ballot(close && d2 == dmin));      // getCacheEntry: the nearest cached point (lowest index on ties)
    else if (popc64(mm) < 4) { if (nm < MAX_CON) { target = nm; nm++; } }       // append
    else {
      // four cached (sortCachedPoints): the deepest of the five stays, the replacement leaves the largest area
      int idx[4]; uint64_t t = mm; for (int j = 0; j < 4; j++) { idx[j] = ffs64(t); t &= t - 1ull; }
      const MPoint p0 = mp_bcast(e, idx[0]), p1 = mp_bcast(e, idx[1]), p2 = mp_bcast(e, idx[2]), p3 = mp_bcast(e, idx[3]);
      int deepest = -1; float pen = q.dist;
      if (p0.dist < pen) { deepest = 0; pen = p0.dist; }
      if (p1.dist < pen) { deepest = 1; pen = p1.dist; }
      if (p2.dist < pen) { deepest = 2; pen = p2.dist; }
      if (p3.dist < pen) { deepest = 3; pen = p3.dist; }
      float res[4] = {0.f, 0.f, 0.f, 0.f};
      if (deepest != 0) { const v3 x = cross(q.la - p1.la, p3.la - p2.la); res[0] = dot(x, x); }
      if (deepest != 1) { const v3 x = cross(q.la - p0.la, p3.la - p2.la); res[1] = dot(x, x); }
      if (deepest != 2) { const v3 x = cross(q.la - p0.la, p3.la - p1.la); res[2] = dot(x, x); }
      if (deepest != 3) { const v3 x = cross(q.la - p0.la, p2.la - p1.la); res[3] = dot(x, x); }
      int bi = -1; float bv = -3.0e38f;
      for (int j = 0; j < 4; j++) if (fabsf(res[j]) > bv) { bv = fabsf(res[j]); bi = j; }
      target = idx[bi];
    }
    if (lane == target) e = q;
  }
  // (3) the contact list: face-manifold contacts in place, every pair of the substep's contacts with its cached points in cache order, then the
  // cached pairs without a new point; a cached point becomes a contact when its predicted gap is below the slack
  bool live = false; v3 wpa = mk3(0, 0, 0), wpb = wpa; int eba = 0, ebb = 0;
  if (lane < nm) {
    eba = CLI(c, e.key & 511, AGX_C_BODY); ebb = CLI(c, (e.key >> 9) & 511, AGX_C_BODY);
    m3 Ra, Rb; v3 oa, ob; body_xf(c, eba, Ra, oa); body_xf(c, ebb, Rb, ob);
    wpa = mul(Ra, e.la) + oa; wpb = mul(Rb, e.lb) + ob;
    const v3 vr = point_velocity(c, eba, wpa) - point_velocity(c, ebb, wpb);
    live = e.dist + dot(vr, e.n) * c.dt < slack;
  }
  float rec[CON_STRIDE];                                       // lane i < nnew: the i-th contact of the substep, kept while the list is rewritten
  for (int w = 0; w < CON_STRIDE; w++) rec[w] = lane < nnew ? c.gcon[CON_STRIDE * lane + w] : 0.f;
  int my_face_slot = -1, out_slot = -1, no = 0, overflow = 0;
  bool used = false;
  for (int i = 0; i <= nnew; i++) {
    int key_i = -1; bool face = false;
    if (i < nnew) { const int* ki = (const int*)(c.gcon + CON_STRIDE * i); key_i = ki[C_CA] | (ki[C_CB] << 9); face = face_box(c, ki[C_CB]); }
    if (face) { if (no < maxc) { if (lane == i) my_face_slot = no; no++; } else overflow++; continue; }
    const bool sel = lane < nm && !used && (i == nnew || e.key == key_i);
    used = used || sel;
    const bool em = sel && live;
    const uint64_t m = wave_ballot(em);
    const int slot = no + wave_rank(m), cnt = popc64(m);
    if (em && slot < maxc) out_slot = slot;
    const int room = maxc - no;
    if (cnt > room) { overflow += cnt - room; no = maxc; } else no += cnt;
  }
  wave_sync();
  if (my_face_slot >= 0) for (int w = 0; w < CON_STRIDE; w++) c.gcon[CON_STRIDE * my_face_slot + w] = rec[w];
  if (out_slot >= 0) {
    float* o = c.gcon + CON_STRIDE * out_slot; int* oi = (int*)o;
    oi[C_CA] = e.key & 511; oi[C_CB] = (e.key >> 9) & 511; oi[C_BA] = eba; oi[C_BB] = ebb;
    st3(o + C_PA, wpa); st3(o + C_PB, wpb); st3(o + C_N, e.n); o[C_DIST] = e.dist; o[C_MU] = e.mu; o[C_LAM] = 0.f;
  }
  if (lane < nm) { float* q = MP + MP_STRIDE * lane; ((int*)q)[MP_KEY] = e.key; st3(q + MP_LA, e.la); st3(q + MP_LB, e.lb); st3(q + MP_N, e.n); q[MP_DIST] = e.dist; q[MP_MU] = e.mu; }
  if (lane == 0) scr.meta[META_NMAN] = nm;
  c.ncon = no; c.overflow += overflow;
  wave_sync();
}

// build: `gaction` non-null on the first substep of an env.step() (take_step, env.py:174-222)
// returns the number of contacts dropped by a budget (contact, row or coefficient cap)
// MANIFOLD: the build kernel with the persistent-manifold stage (AGX_P_MANIFOLD).  A second kernel, not a branch: compiled into the default build
// kernel -- even as a function that is never called -- the stage costs the DEFAULT path 9.5 % (same-box A/B, session r04k: 467 -> 423 k
// env-steps/s, build kernel 8.2 -> 10.8 ms per step; scratch 176 -> 736 bytes per lane).  libagx launches it for blobs with the switch on.
template <bool MANIFOLD = false>
AGX_DEV int env_build(const uint32_t* blob, float* gstate, const float* gaction, float* gscratch, float* gdebug, float* lds, int lane, float* gtrace = nullptr) {
  Ctx c; ctx_init(c, blob, lds, lane);
  c.timing = gdebug != nullptr; c.dbg = gdebug;
  float* L = c.lds; int* Li = c.ldsi;
  const int sw = c.bi[AGX_H_STATE_WORDS];
  Scratch scr = scratch_of(gscratch);
  c.E = scr.ent; c.H = scr.hdr; c.gcon = scr.con; c.gqpt = scr.qpt;
  load_env(c, gstate, sw);
  if (gaction) {
    const int nsub = (int)PRM(c, AGX_P_FRAME_SKIP);
    // clip, scale, 5x accumulate against the joint limits -> motor targets (kept in the state record)
    const int iteration = Li[L_ST + c.s_env + AGX_E_ITERATION] + 1;       // env.py:185
    wave_sync();
    if (lane == 0) { Li[L_ST + c.s_env + AGX_E_ITERATION] = iteration; ((int*)gstate)[c.s_env + AGX_E_ITERATION] = iteration; }
    if (lane < c.ndof) {
      const int d = lane, ai = RBI(c, d, AGX_R_ACT);
      const bool is_human = d >= c.nrobot;
      const int k2 = is_human ? d - c.nrobot : 0;
      const float tsign = (iteration % 2 == 0) ? 1.f : -1.f;
      bool tremor_on = false;                         // impairment == 'tremor'
      for (int k = 0; k < c.nhdof; k++) if (L[L_ST + c.s_tremor + k] != 0.f) tremor_on = true;
      if (ai >= 0 && (!is_human || c.coop)) {
        // the limit test of take_step is discontinuous (an action that would cross a limit is zeroed,
        // env.py:206-211); it is evaluated in double like the reference's numpy code so that a joint
        // resting exactly on a limit takes the same branch
        // Robot.action_multiplier scales a joint's action (env.py:196-197), Robot.action_duplication hands one joint's new target to
        // several (env.py:218-220): such a joint accumulates from the angle and the limits of its source joint (AGX_R_ACT_SRC)
        const float mult = RBF(c, d, AGX_R_ACT_MULT);
        const int ds = RBI(c, d, AGX_R_ACT_SRC) > 0 ? RBI(c, d, AGX_R_ACT_SRC) - 1 : d;
        const float a32 = fminf(fmaxf(gaction[ai], -1.f), 1.f) * PRM(c, AGX_P_ACTION_SCALE) * (mult != 0.f ? mult : 1.f);
        double a = (double)a32, qa = (double)L[L_ST + c.s_q + ds]; const double lo = (double)DLO(c, ds), hi = (double)DHI(c, ds);
        double tt = (double)L[L_ST + c.s_tremor + c.nhdof + k2];
        for (int k = 0; k < nsub; k++) {
          bool below = qa + a < lo, above = qa + a > hi;
          if (below || above) a = 0.0;
          if (below) qa = lo; if (above) qa = hi;
          if (is_human && tremor_on) { tt += a; qa = tt + (double)(L[L_ST + c.s_tremor + k2] * tsign); }   // env.py:212-215
          else qa += a;
        }
        L[L_ST + c.s_qt + d] = (float)qa; gstate[c.s_qt + d] = (float)qa;
        if (is_human && tremor_on) { L[L_ST + c.s_tremor + c.nhdof + k2] = (float)tt; gstate[c.s_tremor + c.nhdof + k2] = (float)tt; }
      }
      if (is_human && !c.coop) {   // tremor without control (env.py:212-215): target + tremors * (+1 on even iterations, -1 on odd)
        const float qt = L[L_ST + c.s_tremor + c.nhdof + k2] + L[L_ST + c.s_tremor + k2] * tsign;
        L[L_ST + c.s_qt + d] = qt; gstate[c.s_qt + d] = qt;
      }
    }
    wave_sync();
  }
  long long t0 = c.timing ? wave_clock() : 0, t1;
#define AGX_TICK(k) if (c.timing) { t1 = wave_clock(); c.tm[k] += t1 - t0; t0 = t1; }
  kinematics(c); AGX_TICK(0)
  // models with a cloth: the world frames of the moving links where this substep starts, for the cloth kernel (one-way coupling)
  if (gtrace) {
    for (int k = lane; k < 3 * c.ndof; k += 64) gtrace[12 * (k / 3) + k % 3] = L[L_LINKP + k]; for (int k = lane; k < 9 * c.ndof; k += 64) gtrace[12 * (k / 9) + 3 + k % 9] = L[L_LINKR + k];
    // ... and of the free bodies behind them (the water's cup; the garment's scene has none): a trace slot is 12 (NDOF + NFREE) words
    for (int k = lane; k < 12 * c.nfree; k += 64) { const int b = k / 12, t = k % 12; gtrace[12 * (c.ndof + b) + t] = t < 3 ? L[L_ST + c.s_free + 13 * b + t] : L[L_FREER + 9 * b + t - 3]; }
  }
  aba_and_minv(c); AGX_TICK(1)
  predict_velocities(c); AGX_TICK(2)
  collide(c); AGX_TICK(3)
  if constexpr (MANIFOLD) { if (PRM(c, AGX_P_MANIFOLD) > 0.f) manifold_update(c, scr); }
  warm_seed(c, scr, lane);
  build_rows(c); AGX_TICK(4)
#undef AGX_TICK
  // hand-over to the solve kernel
  for (int k = lane; k < SCR_VEL; k += 64) scr.vel[k] = L[L_VEL + k];
  if (lane == 0) { scr.meta[META_NCON] = c.ncon; scr.meta[META_NROWS] = c.nrows; scr.meta[META_NNC] = c.first_normal; scr.meta[META_NEAR] = c.near_mask; scr.meta[META_OVERFLOW] = c.overflow; scr.meta[META_NENT] = c.nent; scr.meta[META_NQPT] = c.nqpt; }
  if (gdebug) {   // first-substep internals for the parity tests and the phase cycle counters
    if (lane == 0) { gdebug[0] = (float)c.ncon; gdebug[1] = (float)c.nrows; gdebug[2] = (float)c.overflow; gdebug[3] = (float)c.first_normal; gdebug[4] = (float)c.nent; }   // qdd at DBG_QDD
    for (int q = lane; q < MAX_CON * CON_STRIDE; q += 64) gdebug[DBG_CON + q] = scr.con[q];
    for (int q = lane; q < MAX_DOF * MAX_DOF; q += 64) gdebug[DBG_MINV + q] = L[L_MINV + q];
    wave_sync();
    for (int q = lane; q < SCR_HDR; q += 64) gdebug[DBG_HDR + q] = scr.hdr[q];
    if (lane == 0) { for (int k = 0; k < 16; k++) if (k != 5 && k != 6 && k != 7) gdebug[DBG_TIME + k] = (float)c.tm[k]; }
  }
  return c.overflow;
}

// Collision flags of a state whose contacts the build kernel has just written to the per-env scratch record (agx_check_collisions):
//   AGX_COLLIDE_ENV  -- a robot link or the tool touches (distance <= 0) the human or the furniture: what init_robot_pose and
//                       ik_random_restarts reject (env.py:299-308, robot.py:103-108: get_closest_points(obj, distance=0));
//   AGX_COLLIDE_SELF -- two robot links, or a robot link and the tool, interpenetrate by more than 1 cm (not checked by the reference,
//                       whose null-space IK keeps away from folded arms; the host-side least-squares IK needs it).
// Wave-uniform result.
AGX_DEV int collision_flags(const uint32_t* __restrict__ blob, const float* __restrict__ gscratch, int lane) {
  const int* bi = (const int*)blob;
  const int* meta = (const int*)(gscratch + SCR_O_META);
  const int ncon = meta[META_NCON];
  bool env = false, self = false;
  if (lane < ncon) {
    const float* k = gscratch + SCR_O_CON + CON_STRIDE * lane; const int* ki = (const int*)k;
    const int ta = bi[bi[AGX_H_OFF_COLL] + ki[C_CA] * AGX_C_STRIDE + AGX_C_TAG], tb = bi[bi[AGX_H_OFF_COLL] + ki[C_CB] * AGX_C_STRIDE + AGX_C_TAG];
    const bool ra = ta == AGX_TAG_ROBOT || ta == AGX_TAG_TOOL, rb = tb == AGX_TAG_ROBOT || tb == AGX_TAG_TOOL;
    const bool oa = ta == AGX_TAG_HUMAN || ta == AGX_TAG_TABLE || ta == AGX_TAG_WHEELCHAIR || ta == AGX_TAG_BED;
    const bool ob = tb == AGX_TAG_HUMAN || tb == AGX_TAG_TABLE || tb == AGX_TAG_WHEELCHAIR || tb == AGX_TAG_BED;
    env = ((ra && ob) || (rb && oa)) && k[C_DIST] <= 0.f;
    self = ra && rb && k[C_DIST] < -0.01f;
  }
  return (wave_any(env) ? AGX_COLLIDE_ENV : 0) | (wave_any(self) ? AGX_COLLIDE_SELF : 0);
}

// the part of the solve kernels after the Gauss-Seidel sweeps: state copy, hooks decision, integration, arm limits, store
AGX_DEV void solve_tail(Ctx& c, float* gstate, Scratch& scr, int sw, int phase, float dv0, float dv1) {
  float* lds = c.lds; const int lane = c.lane;
  for (int k = lane; k < sw; k += 64) lds[L_ST + k] = gstate[k];
  wave_sync();
  c.gender = c.ldsi[L_ST + c.s_env + AGX_E_GENDER]; c.frozen = c.ldsi[L_ST + c.s_env + AGX_E_FROZEN];
  { const float ls = c.lds[L_ST + c.s_env + AGX_E_LIMIT_SCALE]; c.limit_scale = ls > 0.f ? ls : 1.f; }   // records written before v6 carry 0
  c.coop = TKI(c, AGX_T_COOP) == 1;
  // hooks (env.py:227-231) run after the last internal substep of a p.stepSimulation() call of take_step -- not in the reset-time settle
  // loops, which are plain engine steps (AGX_PHASE_SETTLE), and only while the human is in env.agents: controllable or tremor
  // (env.py:130-131).  A human arm that is dynamic because of a reactive hold only (scratch itch, arm manipulation, dressing;
  // human.py:108,124-127) is never limit-reset by the reference.
  { const int S = c.bi[AGX_H_SIM_SUBSTEPS], ph = phase & ~AGX_PHASE_SETTLE;
    const bool tremor_on = wave_any(lane < c.nhdof && lds[L_ST + c.s_tremor + lane] != 0.f);
    c.hooks = (S <= 1 || (ph + 1) % S == 0) && !(phase & AGX_PHASE_SETTLE) && (c.coop || tremor_on); }
  integrate(c, scr.vel, dv0, dv1);
  if constexpr (TASK != AGX_TASK_FEEDING) arm_limits(c, lds + L_VEL);   // the velocity vector is dead after the integration
  store_env(c, gstate, sw);
}
// solve: PGS + integration + post-substep hooks of one p.stepSimulation() (env.py:226-232)
// lds_words: the solve kernel's LDS (LDS_SOLVE_WORDS, or more / less when libagx was told so: the row-local sweep sizes its window from it)
AGX_DEV void env_solve(const uint32_t* blob, float* gstate, float* gscratch, float* gdebug, float* lds, int lane, int phase = 0, int lds_words = LDS_SOLVE_WORDS) {
  Ctx c; ctx_init(c, blob, lds, lane);
  const int sw = c.bi[AGX_H_STATE_WORDS];
  Scratch scr = scratch_of(gscratch);
  c.E = scr.ent; c.H = scr.hdr; c.gcon = scr.con; c.dbg = gdebug;
  c.ncon = scr.meta[META_NCON]; c.nrows = scr.meta[META_NROWS]; c.first_normal = scr.meta[META_NNC]; c.nent = scr.meta[META_NENT];
  const long long t0 = gdebug ? wave_clock() : 0;
  float dv0 = 0.f, dv1 = 0.f;
  bool solved = false;
  if constexpr (LVW_COMPILED) { if (lvw_eligible(c, lds_words)) solved = pgs_lvw(c, lds, lds_words, dv0, dv1); }              // the wide row-local sweep: up to four rows per visit (agx_pgs_lvw.h)
  if constexpr (LVS_COMPILED) { if (!solved && lvs_eligible(c, lds_words)) { pgs_lvs(c, lds, lds_words, dv0, dv1); solved = true; } }   // the row-local sweep, pairs and velocities in LDS (agx_pgs_lvs.h)
  if (!solved) {
    // environments with few rows take the row-space sweep (pgs_rowspace; it needs all pairs inside the window)
    const bool rowspace = RS_MAX_ROWS > 0 && c.nrows <= RS_MAX_ROWS && c.nv <= 64 && c.nv <= RS_NVP && c.nrows > 0 && c.nent <= SOLVE_LDS_PAIRS;
    { const int np = c.nent < SOLVE_LDS_PAIRS ? c.nent : SOLVE_LDS_PAIRS;
      const f2* src = (const f2*)scr.ent; f2* dst = (f2*)(lds + L_SOLVE_ENT);
      for (int k = lane; k < np; k += 64) dst[k] = src[k]; }
    wave_sync();
    if (!(rowspace && pgs_rowspace(c, lds + L_SOLVE_ENT, dv0, dv1))) pgs(c, dv0, dv1);
  }
  warm_remember(c, scr, lane);
  const long long t1 = gdebug ? wave_clock() : 0;
  solve_tail(c, gstate, scr, sw, phase, dv0, dv1);
  if (gdebug && lane == 0) { gdebug[DBG_TIME + 5] = (float)(t1 - t0); gdebug[DBG_TIME + 6] = (float)(wave_clock() - t1); }
}
#if AGX_SOLVE_PAIR
// solve of two consecutive environments in one wavefront (agx_pgs_lvw.h, pgs_lvw_pair): gstate and gscratch are the first environment's, the second's
// lie sw and SCR_WORDS words behind; lds holds 2 x lds_words words.  Returns false, with nothing touched but LDS, when the two cannot share the
// wide sweep (one of them is not eligible for it or overflows the scheduler two rows wide): the caller runs env_solve on each.
AGX_DEV void env_solve_load(Ctx& c, Scratch& scr, const uint32_t* blob, float* gscratch, float* lds, int lane) {
  ctx_init(c, blob, lds, lane);
  scr = scratch_of(gscratch);
  c.E = scr.ent; c.H = scr.hdr; c.gcon = scr.con;
  c.ncon = scr.meta[META_NCON]; c.nrows = scr.meta[META_NROWS]; c.first_normal = scr.meta[META_NNC]; c.nent = scr.meta[META_NENT];
}
AGX_DEV bool env_solve_pair(const uint32_t* blob, float* gstate, float* gscratch, float* lds, int lane, int phase, int lds_words) {
  if constexpr (!LVW_PAIRED) { (void)blob; (void)gstate; (void)gscratch; (void)lds; (void)lane; (void)phase; (void)lds_words; return false; }
  else {
    { Ctx c0, c1; Scratch s0, s1;
      env_solve_load(c0, s0, blob, gscratch, lds, lane); env_solve_load(c1, s1, blob, gscratch + SCR_WORDS, lds + lds_words, lane);
      if (!lvw_eligible(c0, lds_words) || !lvw_eligible(c1, lds_words)) return false;
      if (!pgs_lvw_pair(c0, c1, lds, lds_words)) return false; }
    // the tails, one environment after the other (ONE copy of the code; nothing of the sweeps' context stays in registers)
    _Pragma("nounroll") for (int e = 0; e < 2; e++) {
      Ctx c; Scratch scr;
      env_solve_load(c, scr, blob, gscratch + (size_t)e * SCR_WORDS, lds + e * lds_words, lane);
      const int sw = c.bi[AGX_H_STATE_WORDS];
      float dv0, dv1;
      lvw_pair_result(c, c.lds, dv0, dv1);
      warm_remember(c, scr, lane);
      solve_tail(c, gstate + (size_t)e * sw, scr, sw, phase, dv0, dv1);
    }
    return true;
  }
}
#endif

}  // namespace agx
