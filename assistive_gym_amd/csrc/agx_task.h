// agx_task.h -- the task layer: what the six environments do after take_step (contact-force sums, observation, event state machines,
// preferences, reward, done) and the bodies of the observe and finish kernels.  Every block the tasks share is written once: finish_begin /
// finish_end, lane_contact, tool_boxes, for_tool_human_pairs, teleport_draw and the observation cursor ObsOut.
// Part of the stepper (see agx_step.h for the overview); included by agx_step.h only, after agx_env.h.
#pragma once

namespace agx {

// ---- draws ----------------------------------------------------------------------------------------------
AGX_DEV uint32_t rng_next(uint32_t& s0, uint32_t& s1) {
  uint64_t x = ((uint64_t)s1 << 32) | s0;
  x = x * 6364136223846793005ULL + 1442695040888963407ULL;
  s0 = (uint32_t)x; s1 = (uint32_t)(x >> 32);
  return (uint32_t)(x >> 33) ^ (uint32_t)(x >> 11);
}
// where a particle goes once it is eaten or drunk (feeding.py:70, drinking.py:74): three draws, x then y then z
AGX_DEV v3 teleport_draw(uint32_t& s0, uint32_t& s1) {
  const float px = 1000.0f + 1000.0f * (float)(rng_next(s0, s1) >> 8) * (1.0f / 16777216.0f);
  const float py = 1000.0f + 1000.0f * (float)(rng_next(s0, s1) >> 8) * (1.0f / 16777216.0f);
  const float pz = 1000.0f + 1000.0f * (float)(rng_next(s0, s1) >> 8) * (1.0f / 16777216.0f);
  return mk3(px, py, pz);
}

// ---- poses the tasks read -------------------------------------------------------------------------------
// Robot.get_base_pos_orient() (agent.py:142-150), the frame of convert_to_realworld: the pose of the state record, or the moving link
// that is the base link of a robot on a floating base (AGX_H_BASE_LINK)
AGX_DEV void robot_base_pose(const Ctx& c, v3& p, m3& R) {
  const float* L = c.lds; const int bl = c.bi[AGX_H_BASE_LINK];
  if (bl > 0) { p = ld3(L + L_LINKP + 3 * (bl - 1)); R = ldm3(L + L_LINKR + 9 * (bl - 1)); } else { p = ld3(L + L_BASE); R = ldm3(L + L_BASE + 3); }
}
// pose of the tool frame the task reads: the base frame of the spoon (feeding.py:86), link 1 of the wiper (bed_bathing.py:81)
AGX_DEV void tool_base_pose_of(const Ctx& c, int tb, v3& p, m3& R) {
  const float* L = c.lds;
  m3 FR = ldm3(L + L_FREER + 9 * tb); v3 fp = ld3(L + L_ST + c.s_free + 13 * tb);
  p = mul(FR, mk3(FBF(c, tb, AGX_F_REFPOS), FBF(c, tb, AGX_F_REFPOS + 1), FBF(c, tb, AGX_F_REFPOS + 2))) + fp;
  R = mul(FR, quat_to_m3(FBF(c, tb, AGX_F_REFQUAT), FBF(c, tb, AGX_F_REFQUAT + 1), FBF(c, tb, AGX_F_REFQUAT + 2), FBF(c, tb, AGX_F_REFQUAT + 3)));
  if constexpr (TASK != AGX_TASK_FEEDING && TASK != AGX_TASK_DRINKING) {      // (the cup is observed in its base frame; AGX_T_TOOL_OBS_* is the frame of its reward terms)
    p = mul(R, mk3(TKF(c, AGX_T_TOOL_OBS_POS), TKF(c, AGX_T_TOOL_OBS_POS + 1), TKF(c, AGX_T_TOOL_OBS_POS + 2))) + p;
    R = mul(R, quat_to_m3(TKF(c, AGX_T_TOOL_OBS_QUAT), TKF(c, AGX_T_TOOL_OBS_QUAT + 1), TKF(c, AGX_T_TOOL_OBS_QUAT + 2), TKF(c, AGX_T_TOOL_OBS_QUAT + 3)));
  }
}
AGX_DEV void tool_base_pose(const Ctx& c, v3& p, m3& R) { tool_base_pose_of(c, c.bi[AGX_H_TOOL_BODY], p, R); }
// world position of the scratch-itch target: limb frame o target_on_arm (scratch_itch.py:148-152)
AGX_DEV v3 scratch_target(const Ctx& c) {
  const float* L = c.lds; const int s_task = c.bi[AGX_H_S_TASK];
  const int link = TKI(c, AGX_T_ARM_LINK + c.ldsi[L_ST + s_task + AGX_SI_LIMB]);
  return mul(ldm3(L + L_LINKR + 9 * link), ld3(L + L_ST + s_task + AGX_SI_TARGET)) + ld3(L + L_LINKP + 3 * link);
}
// shoulder, elbow, wrist (k = 0, 1, 2) of the arm the task is about
AGX_DEV v3 obs_link_pos(const Ctx& c, int k) { return ld3(c.lds + L_LINKP + 3 * TKI(c, AGX_T_OBS_LINK + k)); }

// ---- observation -----------------------------------------------------------------------------------------
// Every _get_obs writes the same quantities twice: in the frame of the robot's base (convert_to_realworld) and, for a co-operative human, in the
// frame of the human's base (collision body 0).
struct Frame { v3 p; m3 R; };
AGX_DEV v3 frame_pos(const Frame& F, v3 x) { return tmul(F.R, x - F.p); }
AGX_DEV q4 frame_rot(const Frame& F, const m3& X) { return m3_to_quat(mul_at(F.R, X)); }
AGX_DEV Frame robot_frame(const Ctx& c) { Frame f; robot_base_pose(c, f.p, f.R); return f; }
AGX_DEV Frame human_frame(const Ctx& c) { Frame f; f.p = ld3(c.lds + L_HUMAN); f.R = ldm3(c.lds + L_HUMAN + 3); return f; }
// the cursor of an observation writer: words go out in the order of the put calls
struct ObsOut { float* g; int o; };
AGX_DEV void put(ObsOut& o, float x) { o.g[o.o++] = x; }
AGX_DEV void put(ObsOut& o, v3 v) { put(o, v.x); put(o, v.y); put(o, v.z); }
AGX_DEV void put_pose(ObsOut& o, v3 p, q4 q) { put(o, p); put(o, q.x); put(o, q.y); put(o, q.z); put(o, q.w); }
// the robot's controllable joints, wrapped to [-pi, pi) (robot_joint_angles of every _get_obs)
AGX_DEV void put_robot_angles(ObsOut& o, const Ctx& c) {
  for (int d = 0; d < c.nrobot; d++) if (RBI(c, d, AGX_R_ACT) >= 0 && !RBI(c, d, AGX_R_OBS_SKIP)) {
    float a = c.lds[L_ST + c.s_q + d] + 3.14159265358979f;
    put(o, (a - 6.28318530717959f * floorf(a / 6.28318530717959f)) - 3.14159265358979f);
  }
}
AGX_DEV void put_human_angles(ObsOut& o, const Ctx& c) { for (int d = c.nrobot; d < c.ndof; d++) if (RBI(c, d, AGX_R_ACT) >= 0) put(o, c.lds[L_ST + c.s_q + d]); }
// The writers below: every lane computes the robot's part, lane 0 writes it and, for a co-operative human, computes and writes the human's part.

// BedBathingEnv._get_obs (bed_bathing.py:80-110)
// tool_force = all contacts of the tool, total_force = total_force_on_human, pad_force = tool_force_on_human
AGX_DEV void observe_bed(const Ctx& c, float tool_force, float total_force, float pad_force, float* gobs) {
  const Frame B = robot_frame(c);
  v3 sp; m3 sR; tool_base_pose(c, sp, sR);
  const v3 spr = frame_pos(B, sp); const q4 sq = frame_rot(B, sR);
  v3 jp[3], jpr[3];
  for (int k = 0; k < 3; k++) { jp[k] = obs_link_pos(c, k); jpr[k] = frame_pos(B, jp[k]); }
  if (c.lane != 0) return;
  ObsOut o = {gobs, 0};
  put_pose(o, spr, sq); put_robot_angles(o, c);
  for (int k = 0; k < 3; k++) put(o, jpr[k]);
  put(o, tool_force);
  if (c.coop) {   // human_obs (bed_bathing.py:101-106)
    const Frame H = human_frame(c);
    put_pose(o, frame_pos(H, sp), frame_rot(H, sR)); put_human_angles(o, c);
    for (int k = 0; k < 3; k++) put(o, frame_pos(H, jp[k]));
    put(o, total_force); put(o, pad_force);
  }
}
// ArmManipulationEnv._get_obs (arm_manipulation.py:71-110).  Single-arm robot: the one tool is tool_right AND tool_left (:12-14) and the arm
// joints are listed twice (robot_arm = 'both', robot.py:16).  Two-armed robot (AGX_T_TOOL2_BODY > 0): tool 0 = tool_right, the second tool
// = tool_left, 14 joint angles = right arm then left arm.
// tf_r / tf_l = all contacts of the right / left tool, thf_r / thf_l = the same on the human, total_force = total_force_on_human
AGX_DEV void observe_arm(const Ctx& c, float tf_r, float tf_l, float total_force, float thf_r, float thf_l, float* gobs) {
  const float* L = c.lds;
  const int tb2 = TKI(c, AGX_T_TOOL2_BODY); const bool dual = tb2 > 0;
  const Frame B = robot_frame(c);
  v3 sp[2]; m3 sR[2];
  tool_base_pose(c, sp[0], sR[0]);
  if (dual) tool_base_pose_of(c, tb2, sp[1], sR[1]); else { sp[1] = sp[0]; sR[1] = sR[0]; }
  v3 jp[5], jpr[5];
  for (int k = 0; k < 3; k++) jp[k] = obs_link_pos(c, k);
  jp[3] = ld3(L + L_HUMAN + 12 * TKI(c, AGX_T_STOMACH_BODY)); jp[4] = ld3(L + L_HUMAN + 12 * TKI(c, AGX_T_WAIST_BODY));
  for (int k = 0; k < 5; k++) jpr[k] = frame_pos(B, jp[k]);
  if (c.lane != 0) return;
  ObsOut o = {gobs, 0};
  for (int t = 0; t < 2; t++) put_pose(o, frame_pos(B, sp[t]), frame_rot(B, sR[t]));
  for (int rep = 0; rep < (dual ? 1 : 2); rep++) put_robot_angles(o, c);
  for (int k = 0; k < 5; k++) put(o, jpr[k]);
  put(o, tf_l); put(o, tf_r);                 // [tool_left_force, tool_right_force] (:92)
  if (c.coop) {   // human_obs (:98-107)
    const Frame H = human_frame(c);
    for (int t = 0; t < 2; t++) put_pose(o, frame_pos(H, sp[t]), frame_rot(H, sR[t]));
    put_human_angles(o, c);
    for (int k = 0; k < 5; k++) put(o, frame_pos(H, jp[k]));
    put(o, total_force); put(o, thf_l); put(o, thf_r);
  }
}
// ScratchItchEnv._get_obs (scratch_itch.py:59-91)
// tool_force = all contacts of the tool, total_force = total_force_on_human, target_force = tool_force_at_target
AGX_DEV void observe_scratch(const Ctx& c, float tool_force, float total_force, float target_force, float* gobs) {
  const Frame B = robot_frame(c);
  v3 sp; m3 sR; tool_base_pose(c, sp, sR);                       // tool.get_pos_orient(1)
  const v3 spr = frame_pos(B, sp); const q4 sq = frame_rot(B, sR);
  const v3 tg = scratch_target(c), tgr = frame_pos(B, tg);
  v3 jp[3], jpr[3];
  for (int k = 0; k < 3; k++) { jp[k] = obs_link_pos(c, k); jpr[k] = frame_pos(B, jp[k]); }
  if (c.lane != 0) return;
  ObsOut o = {gobs, 0};
  put_pose(o, spr, sq); put(o, spr - tgr); put(o, tgr); put_robot_angles(o, c);
  for (int k = 0; k < 3; k++) put(o, jpr[k]);
  put(o, tool_force);
  if (c.coop) {   // human_obs (scratch_itch.py:79-88)
    const Frame H = human_frame(c);
    const v3 sph = frame_pos(H, sp); const q4 sqh = frame_rot(H, sR); const v3 tgh = frame_pos(H, tg);
    put_pose(o, sph, sqh); put(o, sph - tgh); put(o, tgh); put_human_angles(o, c);
    for (int k = 0; k < 3; k++) put(o, frame_pos(H, jp[k]));
    put(o, total_force); put(o, target_force);
  }
}
// FeedingEnv._get_obs (feeding.py:85-112); DrinkingEnv has the same layout
AGX_DEV void observe(const Ctx& c, float robot_force, float tool_force, float* gobs) {
  const float* L = c.lds;
  const Frame B = robot_frame(c);
  v3 sp; m3 sR; tool_base_pose(c, sp, sR);
  const v3 spr = frame_pos(B, sp); const q4 sq = frame_rot(B, sR);
  const int hl = TKI(c, AGX_T_HEAD_LINK);
  const v3 hpr = frame_pos(B, ld3(L + L_LINKP + 3 * hl)); const q4 hq = frame_rot(B, ldm3(L + L_LINKR + 9 * hl));
  const v3 tpr = frame_pos(B, ld3(L + L_ST + c.s_env + AGX_E_TARGET));
  if (c.lane != 0) return;
  ObsOut o = {gobs, 0};
  put_pose(o, spr, sq); put(o, spr - tpr); put_robot_angles(o, c); put_pose(o, hpr, hq);
  put(o, tool_force);
  if (c.coop) {   // human_obs (feeding.py:102-108)
    const Frame H = human_frame(c);
    const v3 sph = frame_pos(H, sp); const q4 sqh = frame_rot(H, sR);
    const v3 hph = frame_pos(H, ld3(L + L_LINKP + 3 * hl)); const q4 hqh = frame_rot(H, ldm3(L + L_LINKR + 9 * hl));
    const v3 tph = frame_pos(H, ld3(L + L_ST + c.s_env + AGX_E_TARGET));
    put_pose(o, sph, sqh); put(o, sph - tph); put_human_angles(o, c); put_pose(o, hph, hqh);
    put(o, robot_force); put(o, tool_force);
  }
}
// DressingEnv._get_obs (dressing.py:78-110)
AGX_DEV void observe_dressing(const Ctx& c, float cloth_force_sum, float robot_force, float* gobs) {
  const Frame B = robot_frame(c);
  const v3 ep = ld3(c.lds + L_MISC + M_EEP); const m3 eR = ldm3(c.lds + L_MISC + M_EER);
  const v3 epr = frame_pos(B, ep); const q4 eq = frame_rot(B, eR);
  v3 jp[3], jpr[3];
  for (int k = 0; k < 3; k++) { jp[k] = obs_link_pos(c, k); jpr[k] = frame_pos(B, jp[k]); }
  if (c.lane != 0) return;
  ObsOut o = {gobs, 0};
  put_pose(o, epr, eq); put_robot_angles(o, c);
  for (int k = 0; k < 3; k++) put(o, jpr[k]);
  put(o, cloth_force_sum);
  if (c.coop) {   // human_obs (dressing.py:100-106)
    const Frame H = human_frame(c);
    put_pose(o, frame_pos(H, ep), frame_rot(H, eR)); put_human_angles(o, c);
    for (int k = 0; k < 3; k++) put(o, frame_pos(H, jp[k]));
    put(o, cloth_force_sum); put(o, robot_force);
  }
}
AGX_DEV void env_observe(const uint32_t* blob, float* gstate, float* gobs, float* lds, int lane) {
  Ctx c; ctx_init(c, blob, lds, lane);
  load_env(c, gstate, c.bi[AGX_H_STATE_WORDS]);
  kinematics(c); update_target(c);
  if constexpr (TASK == AGX_TASK_BED_BATHING) observe_bed(c, 0.f, 0.f, 0.f, gobs);
  else if constexpr (TASK == AGX_TASK_SCRATCH_ITCH) observe_scratch(c, 0.f, 0.f, 0.f, gobs);
  else if constexpr (TASK == AGX_TASK_DRESSING) observe_dressing(c, c.lds[L_ST + c.bi[AGX_H_S_TASK] + AGX_DR_FORCE_SUM], 0.f, gobs);
  else if constexpr (TASK == AGX_TASK_ARM_MANIPULATION) observe_arm(c, 0.f, 0.f, 0.f, 0.f, 0.f, gobs);
  else observe(c, 0.f, 0.f, gobs);
}

// ---- the frame of a finish function ------------------------------------------------------------------------
// what the finish kernel reads and writes for one environment
struct FinishIO { float* state; const float* action; float* scratch; float* obs; float* reward; uint8_t* done; float* info; const float* report; float* water; };
// what a task hands to finish_end.  total / robot / tool: the forces of the info record (tool = the force the task's success is about: pad, target,
// tool-on-human, cloth); event: what happened in this step (food reward, wiped points, scratch reward, close points, dressing reward)
struct FinishOut { float reward, total_force; bool success; float robot_force, tool_force, event, pref; };

// the prologue: context, the build kernel's counts, the state record into LDS, |action|^2, and the poses as the getters of _get_obs see them
// after the last stepSimulation
AGX_DEV float finish_begin(Ctx& c, Scratch& scr, const uint32_t* blob, const FinishIO& io, float* lds, int lane) {
  ctx_init(c, blob, lds, lane);
  scr = scratch_of(io.scratch);
  c.ncon = scr.meta[META_NCON]; c.nrows = scr.meta[META_NROWS]; c.first_normal = scr.meta[META_NNC]; c.nqpt = scr.meta[META_NQPT]; c.near_mask = scr.meta[META_NEAR];
  load_env(c, io.state, c.bi[AGX_H_STATE_WORDS]);
  const int act_dim = c.bi[AGX_H_ACT_DIM];
  float an2 = 0.f;
  for (int k = 0; k < act_dim; k++) an2 += io.action[k] * io.action[k];
  wave_sync();
  kinematics(c);
  return an2;
}
// the epilogue: lane 0 writes the task's own state words (own_state, a lambda of the task function), reward, done and the info record in ONE
// block, then the state record goes back.  Why one block: the optimiser sinks a task's reward arithmetic into the block that stores the reward and
// chooses its fused multiply-adds there; with the state words in a block of their own the last bit of rewards and observations changes.  No
// standing test guards this (the oracle tolerances are 1e-3): it was measured against the previous build (profiles/task_layer/), and a
// compiler upgrade may move those bits again without a test failing.
template <class OwnState>
AGX_DEV void finish_end(Ctx& c, const FinishIO& io, const FinishOut& r, OwnState own_state) {
  const int iteration = c.ldsi[L_ST + c.s_env + AGX_E_ITERATION];
  wave_sync();
  if (c.lane == 0) {
    own_state();
    *io.reward = r.reward;
    *io.done = (uint8_t)(iteration >= (int)TKF(c, AGX_T_EPISODE_LEN));
    if (io.info) {
      io.info[AGX_INFO_TOTAL_FORCE] = r.total_force;
      io.info[AGX_INFO_TASK_SUCCESS] = (float)r.success;
      io.info[AGX_INFO_ROBOT_FORCE] = r.robot_force; io.info[AGX_INFO_TOOL_FORCE] = r.tool_force; io.info[AGX_INFO_FOOD_REWARD] = r.event;
      io.info[AGX_INFO_PREF] = r.pref; io.info[AGX_INFO_NCONTACT] = (float)c.ncon; io.info[AGX_INFO_NROWS] = (float)c.nrows;
    }
  }
  store_env(c, io.state, c.bi[AGX_H_STATE_WORDS]);
}
// task_success of the counting tasks: enough of the episode's food / targets / scratches
AGX_DEV bool enough_of_total(const Ctx& c, int success) { return success >= c.ldsi[L_ST + c.s_env + AGX_E_TOTAL_FOOD] * TKF(c, AGX_T_SUCCESS_FRAC); }

// this lane's contact of the last substep, for the get_total_force of every task: colliders and tags of both sides, which kinds of body take
// part, f = impulse / dt.  Lanes >= ncon: no tags, no flags, f = 0.
struct LaneContact { const float* rec; int ca, cb, ta, tb; bool human, tool, robot; float f; };
AGX_DEV LaneContact lane_contact(const Ctx& c, const Scratch& scr) {
  LaneContact k; k.rec = nullptr; k.ca = 0; k.cb = 0; k.ta = -1; k.tb = -1; k.human = false; k.tool = false; k.robot = false; k.f = 0.f;
  if (c.lane < c.ncon) {
    k.rec = scr.con + CON_STRIDE * c.lane; const int* ki = (const int*)k.rec;
    k.ca = ki[C_CA]; k.cb = ki[C_CB]; k.ta = CLI(c, k.ca, AGX_C_TAG); k.tb = CLI(c, k.cb, AGX_C_TAG);
    k.f = k.rec[C_LAM] / c.dt;
    k.human = k.ta == AGX_TAG_HUMAN || k.tb == AGX_TAG_HUMAN; k.tool = k.ta == AGX_TAG_TOOL || k.tb == AGX_TAG_TOOL; k.robot = k.ta == AGX_TAG_ROBOT || k.tb == AGX_TAG_ROBOT;
  }
  return k;
}
// is the tool's side of the contact one of the links that count for the task (AGX_T_PAD_LINK, a mask over link + 1)?
AGX_DEV bool on_pad_link(const Ctx& c, const LaneContact& k) { return TKI(c, AGX_T_PAD_LINK) >> (CLI(c, k.ta == AGX_TAG_TOOL ? k.ca : k.cb, AGX_C_LINK) + 1) & 1; }

// world box of a collider at the current poses: centre and half extents (radius included)
AGX_DEV void collider_world_box(const Ctx& c, int col, v3& cw, float h[3]) {
  m3 R; v3 p; body_xf(c, CLI(c, col, AGX_C_BODY), R, p);
  v3 cl = mk3(CLF(c, col, AGX_C_AABB_C), CLF(c, col, AGX_C_AABB_C + 1), CLF(c, col, AGX_C_AABB_C + 2));
  v3 hl = mk3(CLF(c, col, AGX_C_AABB_H), CLF(c, col, AGX_C_AABB_H + 1), CLF(c, col, AGX_C_AABB_H + 2));
  cw = mul(R, cl) + p; const float r = CLF(c, col, AGX_C_RADIUS);
  for (int k = 0; k < 3; k++) h[k] = fabsf(R.a[3 * k]) * hl.x + fabsf(R.a[3 * k + 1]) * hl.y + fabsf(R.a[3 * k + 2]) * hl.z + r;
}
// ... into the arena's table, where narrowphase centres its arithmetic (the broadphase of agx_collide.h writes the same table, grown by the
// distance the collider can travel in a substep)
AGX_DEV void store_world_box(const Ctx& c, int col) {
  float* AB = c.lds + L_ARENA;
  v3 cw; float h[3]; collider_world_box(c, col, cw, h);
  for (int k = 0; k < 3; k++) { AB[ABS * col + k] = comp(cw, k) - h[k]; AB[ABS * col + 3 + k] = comp(cw, k) + h[k]; }
}
AGX_DEV void tool_boxes(const Ctx& c, int first, int last) {                              // lane = collider of [first, last)
  for (int col = first + c.lane; col < last; col += 64) store_world_box(c, col);
  wave_sync();
}
AGX_DEV void tool_and_food_boxes(const Ctx& c) {                                          // lane = collider
  for (int col = c.lane; col < c.ncoll; col += 64) { const int tag = CLI(c, col, AGX_C_TAG); if (tag == AGX_TAG_TOOL || tag == AGX_TAG_FOOD) store_world_box(c, col); }
  wave_sync();
}
// the collider ranges of the tool [t0, t1) and of the human [h0, h1): the (tool, human) group carries both, a female human may have her own
AGX_DEV void tool_human_ranges(const Ctx& c, int& t0, int& t1, int& h0, int& h1) {
  t0 = -1; t1 = -1; h0 = -1; h1 = -1;
  for (int g = 0; g < c.ngroup; g++) {
    const int a0 = GRI(c, g, AGX_G_A0), b0 = GRI(c, g, AGX_G_B0);
    if (CLI(c, a0, AGX_C_TAG) == AGX_TAG_TOOL && CLI(c, b0, AGX_C_TAG) == AGX_TAG_HUMAN) {
      t0 = a0; t1 = GRI(c, g, AGX_G_A1); h0 = b0; h1 = GRI(c, g, AGX_G_B1);
      if (c.gender == 1 && GRI(c, g, AGX_G_B0F) >= 0) { h0 = GRI(c, g, AGX_G_B0F); h1 = GRI(c, g, AGX_G_B1F); }
      return;
    }
  }
}
// tool.get_closest_points(human, distance=limit) at the poses after the last substep: lane = (tool collider, human collider) pair.  Every lane of
// every pass calls narrowphase (it is wave uniform) and then fn(hit, candidate, tool collider); a lane without a pair reports no hit.
template <class Fn>
AGX_DEV void for_tool_human_pairs(const Ctx& c, float limit, Fn fn) {
  int t0, t1, h0, h1; tool_human_ranges(c, t0, t1, h0, h1);
  tool_boxes(c, t0, t1);
  const int nh = h1 - h0, np = (t1 - t0) * nh;
  for (int base = 0; base < np; base += 64) {
    const int p = base + c.lane; const bool has = p < np;
    const int ti = has ? p / nh : 0, hi = has ? p - ti * nh : 0;
    Cand k; k.dist = limit; k.n = mk3(0.f, 0.f, 0.f); k.pa = k.n; k.pb = k.n; k.gap = 0.f;
    const bool hit = narrowphase(c, t0 + ti, h0 + hi, limit, k, has);
    fn(hit, k, t0 + ti);
  }
}

// end-effector speed: norm of getLinkState(ee, computeLinkVelocity)[6] (feeding.py:22, bed_bathing.py:19)
AGX_DEV float frame_speed(const Ctx& c, int link, v3 p) {
  const float* L = c.lds;
  float sv[6] = {0, 0, 0, 0, 0, 0};
  for (int d = link; d >= 0; d = RBI(c, d, AGX_R_PARENT)) { float qd = L[L_ST + c.s_qd + d]; for (int j = 0; j < 6; j++) sv[j] += L[L_S + 6 * d + j] * qd; }
  v3 xr = p - ld3(L + L_MISC + M_REF);
  v3 v = mk3(sv[3], sv[4], sv[5]) + cross(mk3(sv[0], sv[1], sv[2]), xr);
  return sqrtf(dot(v, v));
}
AGX_DEV float ee_speed_of(const Ctx& c) { return frame_speed(c, TKI(c, AGX_T_EE_LINK), ld3(c.lds + L_MISC + M_EEP)); }

// ---- the tasks ---------------------------------------------------------------------------------------------
// finish, bed bathing: everything BedBathingEnv.step does after take_step (bed_bathing.py:15-39)
AGX_DEV void env_finish_bed(const uint32_t* blob, const FinishIO& io, float* lds, int lane) {
  Ctx c; Scratch scr;
  const float an2 = finish_begin(c, scr, blob, io, lds, lane);
  float* L = c.lds; int* Li = c.ldsi;
  // get_total_force (bed_bathing.py:41-78) from the last substep's contact impulses:
  //   total_force_on_human = robot-human + tool-human, tool_force = every contact of the tool,
  //   tool_force_on_human = (tool link 1, human)
  float rf = 0.f, tf = 0.f, thf = 0.f, pf = 0.f;
  {
    const LaneContact k = lane_contact(c, scr);
    if (k.tool) tf = k.f;
    if (k.human && k.robot) rf = k.f;
    if (k.human && k.tool) { thf = k.f; if (on_pad_link(c, k)) pf = k.f; }
  }
  const float robot_f = wave_sum(rf), tool_f = wave_sum(tf), pad_f = wave_sum(pf), total_f = robot_f + wave_sum(thf);
  observe_bed(c, tool_f, total_f, pad_f, io.obs);
  // targets wiped by the manifold points of the pad on the human's links (not its base, bed_bathing.py:52-53): lane = target
  int success = Li[L_ST + c.s_env + AGX_E_TASK_SUCCESS];
  const int s_task = c.bi[AGX_H_S_TASK];
  int new_points = 0;
  {
    const int g = c.gender, nt = TKI(c, AGX_T_NT + 2 * g) + TKI(c, AGX_T_NT + 2 * g + 1);
    const float* TT = c.bf + c.bi[AGX_H_OFF_TARGETS] + 4 * g * TKI(c, AGX_T_NT_MAX);
    const float r2 = TKF(c, AGX_T_TARGET_RADIUS) * TKF(c, AGX_T_TARGET_RADIUS);
    for (int base = 0; base < nt; base += 64) {
      const int t = base + lane; bool hit = false;
      const uint32_t w0 = (uint32_t)Li[L_ST + s_task + AGX_BB_ALIVE + (base >> 5)], w1 = (uint32_t)Li[L_ST + s_task + AGX_BB_ALIVE + (base >> 5) + 1];
      const uint64_t alive = (uint64_t)w0 | ((uint64_t)w1 << 32);
      if (t < nt && (alive >> lane & 1)) {
        const int link = TKI(c, AGX_T_ARM_LINK + ((const int*)TT)[4 * t + 3]);
        const v3 w = mul(ldm3(L + L_LINKR + 9 * link), ld3(TT + 4 * t)) + ld3(L + L_LINKP + 3 * link);   // update_targets (bed_bathing.py:190-203)
        for (int q = 0; q < c.nqpt; q++) {
          const float* o = scr.qpt + QPT_STRIDE * q; const int lb = ((const int*)o)[3];
          if (lb < 0) continue;
          const v3 d = ld3(o) - w;
          if (dot(d, d) < r2) hit = true;
        }
      }
      const uint64_t hm = wave_ballot(hit);
      new_points += popc64(hm);
      wave_sync();
      if (lane == 0) { const uint64_t na = alive & ~hm; Li[L_ST + s_task + AGX_BB_ALIVE + (base >> 5)] = (int)(uint32_t)na; Li[L_ST + s_task + AGX_BB_ALIVE + (base >> 5) + 1] = (int)(uint32_t)(na >> 32); }
      wave_sync();
    }
  }
  success += new_points;
  // reward_distance = -min distance tool <-> human within CLOSEST_DIST (bed_bathing.py:23)
  const float lim = TKF(c, AGX_T_CLOSEST_DIST); float dmin = lim;
  for_tool_human_pairs(c, lim, [&](bool hit, const Cand& k, int) { dmin = fminf(dmin, wave_min(hit ? k.dist : lim)); });
  // human_preferences (env.py:237-274), non-feeding branch: forces away from the target area, high forces at the target
  const float ee_speed = ee_speed_of(c);
  const float pref = TKF(c, AGX_T_C_V) * (-ee_speed) + TKF(c, AGX_T_C_F) * (-(total_f - pad_f)) + TKF(c, AGX_T_C_HF) * (pad_f < 10.f ? 0.f : -pad_f);
  const float reward = TKF(c, AGX_T_W_DISTANCE) * (-dmin) + TKF(c, AGX_T_W_ACTION) * (-sqrtf(an2)) + TKF(c, AGX_T_W_WIPE) * (float)new_points + pref;
  FinishOut r;
  r.reward = reward; r.total_force = total_f; r.success = enough_of_total(c, success); r.robot_force = robot_f; r.tool_force = pad_f; r.event = (float)new_points; r.pref = pref;
  finish_end(c, io, r, [&] { Li[L_ST + c.s_env + AGX_E_TASK_SUCCESS] = success; });
}

// finish, arm manipulation: everything ArmManipulationEnv.step does after take_step (arm_manipulation.py:18-60)
AGX_DEV void env_finish_arm(const uint32_t* blob, const FinishIO& io, float* lds, int lane) {
  Ctx c; Scratch scr;
  const float an2 = finish_begin(c, scr, blob, io, lds, lane);
  float* L = c.lds;
  // get_total_force (:62-69): the one tool of a single-arm robot is counted as tool_right and as tool_left
  const int tb2 = TKI(c, AGX_T_TOOL2_BODY); const bool dual = tb2 > 0; const int code2 = AGX_BODY_FREE0 + tb2;
  float rf = 0.f, tf0 = 0.f, tf1 = 0.f, thf0 = 0.f, thf1 = 0.f;
  {
    const LaneContact k = lane_contact(c, scr);
    if (k.human && k.robot) rf = k.f;
    for (int side = 0; side < 2; side++) {              // a contact between the two tools counts for both
      if ((side ? k.tb : k.ta) != AGX_TAG_TOOL) continue;
      const int body = ((const int*)k.rec)[side ? C_BB : C_BA];
      if (dual && body == code2) { tf1 += k.f; if (k.human) thf1 += k.f; } else { tf0 += k.f; if (k.human) thf0 += k.f; }
    }
  }
  const float robot_f = wave_sum(rf); float tf_r = wave_sum(tf0), tf_l = wave_sum(tf1), thf_r = wave_sum(thf0), thf_l = wave_sum(thf1);
  if (!dual) { tf_l = tf_r; thf_l = thf_r; }
  const float total_f = robot_f + thf_r + thf_l;
  observe_arm(c, tf_r, tf_l, total_f, thf_r, thf_l, io.obs);
  // tool.get_closest_points(human, distance=0.01) (env.py:264-265): one point per (hull of the tool, shape of the human) pair that close
  int near_r = 0, near_l = 0;
  const float lim = TKF(c, AGX_T_PRESSURE_DIST);
  for_tool_human_pairs(c, lim, [&](bool hit, const Cand& k, int tc) {
    const bool close = hit && k.dist < lim, second = dual && CLI(c, tc, AGX_C_BODY) == code2;
    near_r += popc64(wave_ballot(close && !second)); near_l += popc64(wave_ballot(close && second));
  });
  if (!dual) near_l = near_r;
  // right + left end effector (:26-27): the same link on a single-arm robot
  float ee_speed = ee_speed_of(c);
  if (dual) {
    const int l2 = TKI(c, AGX_T_EE2_LINK);
    const v3 e2 = mul(ldm3(L + L_LINKR + 9 * l2), mk3(TKF(c, AGX_T_EE2_POS), TKF(c, AGX_T_EE2_POS + 1), TKF(c, AGX_T_EE2_POS + 2))) + ld3(L + L_LINKP + 3 * l2);
    ee_speed += frame_speed(c, l2, e2);
  } else ee_speed *= 2.f;
  const float pressure = (near_r <= 0 ? 0.f : thf_r / (float)near_r) + (near_l <= 0 ? 0.f : thf_l / (float)near_l);     // env.py:266-269
  // human_preferences (env.py:237-274): reward_force_nontarget = -(total - (right + left)), tool_force_at_target = 0
  const float pref = TKF(c, AGX_T_C_V) * (-ee_speed) + TKF(c, AGX_T_C_F) * (-(total_f - thf_r - thf_l)) + TKF(c, AGX_T_C_P) * (-pressure);
  v3 spr; m3 sRr; tool_base_pose(c, spr, sRr);
  v3 spl = spr; if (dual) { m3 sRl; tool_base_pose_of(c, tb2, spl, sRl); }
  const v3 elbow = obs_link_pos(c, 1), wrist = obs_link_pos(c, 2);
  const v3 stomach = ld3(L + L_HUMAN + 12 * TKI(c, AGX_T_STOMACH_BODY)), waist = ld3(L + L_HUMAN + 12 * TKI(c, AGX_T_WAIST_BODY));
  const v3 d0 = spl - elbow, d3 = spr - wrist, d1 = elbow - stomach, d2 = wrist - waist;
  const float rd_left = -sqrtf(dot(d0, d0)), rd_right = -sqrtf(dot(d3, d3)), rd_human = -sqrtf(dot(d1, d1)) - sqrtf(dot(d2, d2));      // :36-38
  const float we = TKF(c, AGX_T_W_WIPE);                                                                   // distance_end_effector_weight
  const float reward = TKF(c, AGX_T_W_DISTANCE) * rd_human + (dual ? we * rd_left + we * rd_right : 2.f * we * rd_left) + TKF(c, AGX_T_W_ACTION) * (-sqrtf(an2)) + pref;   // :41-44
  const float th_f = dual ? thf_r + thf_l : thf_r; const int near_pts = dual ? near_r + near_l : near_r;
  const int s_task = c.bi[AGX_H_S_TASK];
  const float best0 = L[L_ST + s_task + AGX_AM_BEST], best = (best0 == 0.f || rd_human > best0) ? rd_human : best0;   // :47-48
  FinishOut r;
  r.reward = reward; r.total_force = total_f; r.success = best >= TKF(c, AGX_T_SUCCESS_FRAC); r.robot_force = robot_f; r.tool_force = th_f; r.event = (float)near_pts; r.pref = pref;
  finish_end(c, io, r, [&] { L[L_ST + s_task + AGX_AM_BEST] = best; });
}

// finish, scratch itch: everything ScratchItchEnv.step does after take_step (scratch_itch.py:14-44)
AGX_DEV void env_finish_scratch(const uint32_t* blob, const FinishIO& io, float* lds, int lane) {
  Ctx c; Scratch scr;
  const float an2 = finish_begin(c, scr, blob, io, lds, lane);
  float* L = c.lds; int* Li = c.ldsi;
  const v3 target = scratch_target(c);                            // update_targets after the last substep
  const float r2 = TKF(c, AGX_T_TARGET_RADIUS) * TKF(c, AGX_T_TARGET_RADIUS);
  // get_total_force (scratch_itch.py:46-57) from the last substep's contact impulses
  float rf = 0.f, tf = 0.f, thf = 0.f, gf = 0.f;
  {
    const LaneContact k = lane_contact(c, scr);
    if (k.tool) tf = k.f;
    if (k.human && k.robot) rf = k.f;
    if (k.human && k.tool) {
      thf = k.f;
      const v3 on_human = ld3(k.rec + (k.ta == AGX_TAG_TOOL ? C_PB : C_PA)), d = on_human - target;
      if (on_pad_link(c, k) && dot(d, d) < r2) gf = k.f;          // close to the target (:54)
    }
  }
  const float robot_f = wave_sum(rf), tool_f = wave_sum(tf), target_f = wave_sum(gf), total_f = robot_f + wave_sum(thf);
  observe_scratch(c, tool_f, total_f, target_f, io.obs);
  // target_contact_pos: the LAST manifold point of the tool's links 0 / 1 on the human within TARGET_RADIUS of the target (:52-56)
  bool near = false; v3 qp = mk3(0.f, 0.f, 0.f);
  if (lane < c.nqpt) { qp = ld3(scr.qpt + QPT_STRIDE * lane); const v3 d = qp - target; near = dot(d, d) < r2; }
  const uint64_t nm = wave_ballot(near);
  const int s_task = c.bi[AGX_H_S_TASK];
  int success = Li[L_ST + c.s_env + AGX_E_TASK_SUCCESS];
  float scratch_reward = 0.f;
  if (nm) {
    const int last = 63 - __builtin_clzll((unsigned long long)nm);
    const v3 cp = mk3(wave_bcast(qp.x, last), wave_bcast(qp.y, last), wave_bcast(qp.z, last));
    const v3 dp = cp - ld3(L + L_ST + s_task + AGX_SI_PREV_CONTACT);
    if (sqrtf(dot(dp, dp)) > 0.01f && target_f < 10.f) {         // the tool moved along the skin and does not press too hard (:28-32)
      scratch_reward = 5.f; success += 1;
      wave_sync();
      if (lane == 0) st3(L + L_ST + s_task + AGX_SI_PREV_CONTACT, cp);
      wave_sync();
    }
  }
  v3 sp; m3 sR; tool_base_pose(c, sp, sR);
  const v3 dd = target - sp;
  const float ee_speed = ee_speed_of(c);
  const float pref = TKF(c, AGX_T_C_V) * (-ee_speed) + TKF(c, AGX_T_C_F) * (-(total_f - target_f)) + TKF(c, AGX_T_C_HF) * (target_f < 10.f ? 0.f : -target_f);
  const float reward = TKF(c, AGX_T_W_DISTANCE) * (-sqrtf(dot(dd, dd))) + TKF(c, AGX_T_W_ACTION) * (-sqrtf(an2)) + TKF(c, AGX_T_W_WIPE) * scratch_reward + pref;
  FinishOut r;
  r.reward = reward; r.total_force = total_f; r.success = enough_of_total(c, success); r.robot_force = robot_f; r.tool_force = target_f; r.event = scratch_reward; r.pref = pref;
  finish_end(c, io, r, [&] { Li[L_ST + c.s_env + AGX_E_TASK_SUCCESS] = success; });
}

AGX_DEV float signed_volume6(v3 a, v3 b, v3 c, v3 d) { return dot(cross(b - a, c - a), d - a); }   // 6 x the signed volume: only its sign is used
AGX_DEV int sgnf(float x) { return (x > 0.f) - (x < 0.f); }
// Util.line_intersects_triangle (util.py:125-132)
AGX_DEV bool line_intersects_triangle(v3 p0, v3 p1, v3 p2, v3 q0, v3 q1) {
  if (sgnf(signed_volume6(q0, p0, p1, p2)) == sgnf(signed_volume6(q1, p0, p1, p2))) return false;
  const int a = sgnf(signed_volume6(q0, q1, p0, p1)), b = sgnf(signed_volume6(q0, q1, p1, p2)), cc = sgnf(signed_volume6(q0, q1, p2, p0));
  return a == b && b == cc;
}
// do the six sleeve vertices straddle both planes through `origin` that contain the arm axis (util.py:144-171)?
AGX_DEV bool points_around_axis(const v3* pts, v3 from, v3 to, v3 origin) {
  v3 nrm = to - from; nrm = (1.0f / sqrtf(dot(nrm, nrm))) * nrm;
  v3 tan = cross(mk3(1.f, 1.f, 0.f), nrm); tan = (1.0f / sqrtf(dot(tan, tan))) * tan;
  v3 bin = cross(tan, nrm); bin = (1.0f / sqrtf(dot(bin, bin))) * bin;
  bool tp = false, tn = false, bp = false, bn = false;
  for (int i = 0; i < 6; i++) { const v3 d = pts[i] - origin; const float t = dot(tan, d), b = dot(bin, d); tp |= t > 0.f; tn |= t < 0.f; bp |= b > 0.f; bn |= b < 0.f; }
  return tp && tn && bp && bn;
}
// finish, dressing: everything DressingEnv.step does after take_step (dressing.py:20-76).  io.report: what the cloth kernel left for
// this environment -- the six sleeve vertices and, per node and contact slot, {height, |force|} of the node-vs-rigid contacts of the last substep
AGX_DEV void env_finish_dressing(const uint32_t* blob, const FinishIO& io, float* lds, int lane) {
  Ctx c; Scratch scr;
  const float an2 = finish_begin(c, scr, blob, io, lds, lane);
  float* L = c.lds; const float* greport = io.report;
  const int* cl = c.bi + c.bi[AGX_H_OFF_CLOTH]; const float* clp = c.bf + c.bi[AGX_H_OFF_CLOTH] + cl[AGX_CL_OFF_PARAM];
  // (the three loads written out, not obs_link_pos(c, k): with the helper here the compiler pairs the multiply-adds of the observation's joint
  // positions differently and six observation words move by up to 3 ulp against the build before this file existed, profiles/task_layer/)
  const v3 shoulder = ld3(L + L_LINKP + 3 * TKI(c, AGX_T_OBS_LINK)), elbow = ld3(L + L_LINKP + 3 * TKI(c, AGX_T_OBS_LINK + 1)), wrist = ld3(L + L_LINKP + 3 * TKI(c, AGX_T_OBS_LINK + 2));
  v3 pts[6];
  for (int k = 0; k < 6; k++) pts[k] = greport ? ld3(greport + 3 * k) : mk3(0.f, 0.f, 0.f);
  // Util.sleeve_on_arm_reward (util.py:134-202)
  const float rad = TKF(c, AGX_T_ARM_RADIUS + c.gender);
  const v3 we = wrist - elbow, es = shoulder - elbow; const float lwe = sqrtf(dot(we, we)), les = sqrtf(dot(es, es));
  const v3 hand_end = wrist + (rad * 2.f / lwe) * we, elbow_end = elbow - (rad / lwe) * we, shoulder_end = shoulder + (rad / les) * es;
  const bool around_fore = points_around_axis(pts, elbow_end, hand_end, hand_end), around_upper = points_around_axis(pts, shoulder_end, elbow_end, shoulder_end);
  const bool f1 = line_intersects_triangle(pts[0], pts[1], pts[2], hand_end, elbow_end), f2 = line_intersects_triangle(pts[3], pts[4], pts[5], hand_end, elbow_end);
  const bool u1 = line_intersects_triangle(pts[0], pts[1], pts[2], elbow_end, shoulder_end), u2 = line_intersects_triangle(pts[3], pts[4], pts[5], elbow_end, shoulder_end);
  v3 centre = mk3(0.f, 0.f, 0.f); for (int k = 0; k < 6; k++) centre = centre + (1.0f / 6.0f) * pts[k];
  const v3 dh = hand_end - centre, de = centre - elbow, dfl = hand_end - elbow_end;
  const float distance_to_hand = sqrtf(dot(dh, dh)), distance_along_forearm = distance_to_hand, distance_along_upperarm = sqrtf(dot(de, de));
  const float forearm_length = sqrtf(dot(dfl, dfl)), upperarm_length = les;
  const bool forearm_in = around_fore && (f1 || f2), upperarm_in = around_upper && (u1 || u2);
  // cloth forces (dressing.py:34-46): x 10, only below the end effector and below 20
  const v3 ep = ld3(L + L_MISC + M_EEP);
  float fs = 0.f;
  if (greport) {
    const int entries = 2 * cl[AGX_CL_NN];   // AGX_CLOTH_NODE_CONTACTS slots per node
    const float scale = clp[AGX_CP_FORCE_SCALE], fmax = clp[AGX_CP_FORCE_MAX], below = clp[AGX_CP_EE_BELOW];
    for (int k = lane; k < entries; k += 64) {
      const float z = greport[20 + 2 * k], f = greport[20 + 2 * k + 1] * scale;
      if (f >= 0.f && z < ep.z - below && f < fmax) fs += f;
    }
  }
  const float cloth_force_sum = wave_sum(fs);
  const float ee_speed = ee_speed_of(c);
  const float pref = TKF(c, AGX_T_C_V) * (-ee_speed) + TKF(c, AGX_T_C_D) * (-cloth_force_sum);   // human_preferences(end_effector_velocity, dressing_forces)
  float reward_dressing;
  if (upperarm_in) { reward_dressing = forearm_length; if (distance_along_upperarm < upperarm_length) reward_dressing += distance_along_upperarm; }
  else if (forearm_in && distance_along_forearm < forearm_length) reward_dressing = distance_along_forearm;
  else reward_dressing = -distance_to_hand;
  const float reward = TKF(c, AGX_T_W_WIPE) * reward_dressing + TKF(c, AGX_T_W_ACTION) * (-sqrtf(an2)) + pref;
  float rf = 0.f;
  { const LaneContact k = lane_contact(c, scr); if (k.human && k.robot) rf = k.f; }
  const float robot_f = wave_sum(rf);
  observe_dressing(c, cloth_force_sum, robot_f, io.obs);
  const int s_task = c.bi[AGX_H_S_TASK];
  const float best0 = L[L_ST + s_task + AGX_DR_BEST], best = reward_dressing > best0 ? reward_dressing : best0;
  FinishOut r;
  r.reward = reward; r.total_force = robot_f + cloth_force_sum; r.success = best >= TKF(c, AGX_T_SUCCESS_FRAC); r.robot_force = robot_f; r.tool_force = cloth_force_sum; r.event = reward_dressing; r.pref = pref;
  finish_end(c, io, r, [&] { L[L_ST + s_task + AGX_DR_BEST] = best; L[L_ST + s_task + AGX_DR_FORCE_SUM] = cloth_force_sum; });
}

// finish, feeding and drinking: everything FeedingEnv.step does after take_step (feeding.py:17-43)
AGX_DEV void env_finish_feeding(const uint32_t* blob, const FinishIO& io, float* lds, int lane) {
  Ctx c; Scratch scr;
  const float an2 = finish_begin(c, scr, blob, io, lds, lane);
  float* L = c.lds; int* Li = c.ldsi;
  update_target(c);
  // get_total_force (feeding.py:45-48) from the last substep's contact impulses
  float rf = 0.f, tf = 0.f;
  {
    const LaneContact k = lane_contact(c, scr);
    if (k.human && k.robot) rf = k.f;
    if (k.human && k.tool) tf = k.f;
  }
  const float robot_f = wave_sum(rf), tool_f = wave_sum(tf), total_f = robot_f + tool_f;
  observe(c, robot_f, tool_f, io.obs);
  // get_food_rewards (feeding.py:50-83)
  float food_reward = 0.f, food_hit = 0.f, vel_sum = 0.f;
  int alive = Li[L_ST + c.s_env + AGX_E_FOOD_ALIVE], active = Li[L_ST + c.s_env + AGX_E_FOOD_ACTIVE];
  int success = Li[L_ST + c.s_env + AGX_E_TASK_SUCCESS];
  uint32_t r0 = (uint32_t)Li[L_ST + c.s_env + AGX_E_RNG], r1 = (uint32_t)Li[L_ST + c.s_env + AGX_E_RNG + 1];
  const int active_on_entry = active, hit_mask = c.near_mask, food0 = c.bi[AGX_H_FOOD0];
  const v3 target = ld3(L + L_ST + c.s_env + AGX_E_TARGET);
  tool_and_food_boxes(c);   // for the 0.1 m closest-point query (agent.py:118-130)
  int tool0 = -1, tool1 = -1, foodc0 = -1;
  for (int g = 0; g < c.ngroup; g++) {   // the (food, tool) group carries both collider ranges
    int a0 = GRI(c, g, AGX_G_A0), b0 = GRI(c, g, AGX_G_B0);
    if (CLI(c, a0, AGX_C_TAG) == AGX_TAG_FOOD && CLI(c, b0, AGX_C_TAG) == AGX_TAG_TOOL) { foodc0 = a0; tool0 = b0; tool1 = GRI(c, g, AGX_G_B1); break; }
  }
  const float spill = TKF(c, AGX_T_SPILL_DIST);
  // The query below only asks "is some tool piece within `spill` of particle k?", and with the food on the spoon the answer is yes by centimetres --
  // yet at this limit the separating-axis early-out of gjk_distance never fires and every lane of every pass iterates to convergence.  The AABB
  // table above proves the common case (lane = tool piece): piece j, radius included, lies inside AABB_j, and the particle's core inside its own
  // AABB shrunk by its radius r_k (a point for a sphere), so the separation of (k, j) is at most the farthest distance between those two boxes
  // minus r_k.  Below spill - SPILL_PROOF_GUARD (GJK_TOL is 1e-6, f32 rounding at this scale 1e-7) the converged narrowphase decides the same
  // way and is skipped; everything else -- the shell around the limit, fallen food, non-finite boxes (the comparisons are false) -- runs it as
  // before.  The loop below changes neither the table nor the pose of a particle it has yet to ask about.  -DAGX_FINISH_SPILL_GJK: no shortcut
  // (lib/variants/finishgjk.so, tests/test_gpu_step_tail.py)
  int proven_near = 0;
#ifndef AGX_FINISH_SPILL_GJK
  {
    constexpr float SPILL_PROOF_GUARD = 1e-3f, FINITE_MAX = 3.0e38f;
    const float* AB = L + L_ARENA;
    for (int k = 0; k < c.nfood; k++) {
      const int fc = foodc0 + k; const float rk = CLF(c, fc, AGX_C_RADIUS);
      bool proof = false;
      for (int base = tool0; base < tool1; base += 64) {
        const int tc = base + lane;
        if (tc < tool1) {
          float far2 = 0.f; bool finite = fabsf(rk) <= FINITE_MAX;
          for (int q = 0; q < 3; q++) {
            const float flo = AB[ABS * fc + q] + rk, fhi = AB[ABS * fc + 3 + q] - rk, tlo = AB[ABS * tc + q], thi = AB[ABS * tc + 3 + q];
            finite = finite && fabsf(flo) <= FINITE_MAX && fabsf(fhi) <= FINITE_MAX && fabsf(tlo) <= FINITE_MAX && fabsf(thi) <= FINITE_MAX;
            const float up = thi - flo, down = fhi - tlo, m = up > down ? up : down;
            far2 += m * m;
          }
          proof = proof || (finite && sqrtf(far2) - rk < spill - SPILL_PROOF_GUARD);
        }
      }
      if (wave_any(proof)) proven_near |= 1 << k;
    }
  }
#endif
  for (int k = 0; k < c.nfood; k++) {
    if (!(alive >> k & 1)) continue;
    const int b = food0 + k; float* r = L + L_ST + c.s_free + 13 * b;
    v3 d = target - ld3(r);
    if (sqrtf(dot(d, d)) < TKF(c, AGX_T_MOUTH_DIST)) {
      food_reward += 20.f; success += 1; vel_sum += sqrtf(dot(ld3(r + 7), ld3(r + 7)));
      alive &= ~(1 << k); active &= ~(1 << k);
      const v3 away = teleport_draw(r0, r1);
      wave_sync();
      if (lane == 0) { st3(r, away); r[3] = 0.f; r[4] = 0.f; r[5] = 0.f; r[6] = 1.f; }
      wave_sync();
      continue;
    }
    bool near = proven_near >> k & 1;
    if (!near) {
      const int fc = foodc0 + k; const float* AB = L + L_ARENA;
      for (int base = tool0; base < tool1; base += 64) {
        const int tc = base + lane;
        bool query = tc < tool1;
        if (query) for (int q = 0; q < 3; q++) if (AB[ABS * fc + q] > AB[ABS * tc + 3 + q] + spill || AB[ABS * tc + q] > AB[ABS * fc + 3 + q] + spill) query = false;
        Cand tmp;
        const bool hitl = narrowphase(c, fc, query ? tc : tool0, spill, tmp, query);
        if (wave_any(hitl)) near = true;
      }
    }
    if (!near) { food_reward -= 5.f; alive &= ~(1 << k); }
  }
  for (int k = 0; k < c.nfood; k++) if ((active_on_entry >> k & 1) && (hit_mask >> k & 1)) { food_hit -= 1.f; active &= ~(1 << k); }
#if AGX_TASK == 5   /* AGX_TASK_DRINKING (an enum: not visible to the preprocessor) */
  // DrinkingEnv.get_water_rewards (drinking.py:52-91), lane = particle: outside the cup's cylinder and within 0.03 m of the mouth -> drunk
  // (+10, teleported), else further than 0.1 m from every piece of the cup -> spilled (-1); a particle of waters_active (as it was on
  // entry) that touched the person in the last internal substep (the water kernel's report) counts for the preferences
  float tilt_term = 0.f; v3 cup_top = mk3(0.f, 0.f, 0.f);
  {
    float* gwater = io.water; const float* greport = io.report;
    float* body = L + L_ARENA;                                   // frames in agx_water.h's slot layout, where this env step ends
    for (int k = lane; k < 3 * c.ndof; k += 64) body[12 * (k / 3) + k % 3] = L[L_LINKP + k];
    for (int k = lane; k < 9 * c.ndof; k += 64) body[12 * (k / 9) + 3 + k % 9] = L[L_LINKR + k];
    agxw::static_frames(blob, L + L_ST, body, lane, true);
    wave_sync();
    v3 cp; m3 cR; tool_base_pose(c, cp, cR);
    const v3 p2 = mul(cR, mk3(TKF(c, AGX_T_TOOL_OBS_POS), TKF(c, AGX_T_TOOL_OBS_POS + 1), TKF(c, AGX_T_TOOL_OBS_POS + 2))) + cp;
    const m3 R2 = mul(cR, quat_to_m3(TKF(c, AGX_T_TOOL_OBS_QUAT), TKF(c, AGX_T_TOOL_OBS_QUAT + 1), TKF(c, AGX_T_TOOL_OBS_QUAT + 2), TKF(c, AGX_T_TOOL_OBS_QUAT + 3)));
    const v3 top = mul(R2, mk3(TKF(c, AGX_T_DK_TOP), TKF(c, AGX_T_DK_TOP + 1), TKF(c, AGX_T_DK_TOP + 2))) + p2;
    const v3 bot = mul(R2, mk3(TKF(c, AGX_T_DK_BOTTOM), TKF(c, AGX_T_DK_BOTTOM + 1), TKF(c, AGX_T_DK_BOTTOM + 2))) + p2;
    cup_top = top;
    const q4 q = m3_to_quat(R2);                                 // cup_euler[0] as p.getEulerFromQuaternion returns it (drinking.py:30-31)
    const float sarg = -2.0f * (q.x * q.z - q.w * q.y);
    const float roll = (sarg <= -0.99999f || sarg >= 0.99999f) ? 0.f : atan2f(2 * (q.y * q.z + q.w * q.x), q.w * q.w - q.x * q.x - q.y * q.y + q.z * q.z);
    tilt_term = -fabsf(roll - 3.14159265358979f * 0.5f);
    const int* cl = c.bi + c.bi[AGX_H_OFF_CLOTH]; const float* clf = c.bf + c.bi[AGX_H_OFF_CLOTH];
    const int NN = cl[AGX_CL_NN], NS = cl[AGX_CL_NSHAPE]; const float margin = clf[cl[AGX_CL_OFF_PARAM] + AGX_CP_MARGIN];
    const int s_task = c.bi[AGX_H_S_TASK];
    const bool mine = lane < NN;
    const bool is_alive = mine && ((uint32_t)Li[L_ST + s_task + AGX_DK_ALIVE + (lane >> 5)] >> (lane & 31) & 1u);
    const bool is_active = mine && ((uint32_t)Li[L_ST + s_task + AGX_DK_ACTIVE + (lane >> 5)] >> (lane & 31) & 1u);
    float x[3] = {0.f, 0.f, 0.f}; float speed = 0.f;
    if (mine) { for (int k = 0; k < 3; k++) x[k] = gwater[3 * lane + k]; const float* vv = gwater + 3 * NN + 3 * lane; speed = sqrtf(vv[0] * vv[0] + vv[1] * vv[1] + vv[2] * vv[2]); }
    bool drunk = false, spilled = false;
    if (is_alive) {
      const v3 xp = mk3(x[0], x[1], x[2]), axis = bot - top, a = xp - top, b = xp - bot, cr = cross(a, axis);
      const float cyl = TKF(c, AGX_T_TARGET_RADIUS) * sqrtf(dot(axis, axis));
      const bool inside = dot(a, axis) >= 0.f && dot(b, axis) <= 0.f && sqrtf(dot(cr, cr)) <= cyl;          // Util.points_in_cylinder (util.py:53-56)
      if (!inside) {
        const v3 d = target - xp;
        if (sqrtf(dot(d, d)) < TKF(c, AGX_T_MOUTH_DIST)) drunk = true;
        else {
          spilled = true;      // decided below: the 0.1 m query against the cup's vertices (every lane takes part in the wave-uniform loops)
        }
      }
    }
    // w.get_closest_points(self.tool, distance=0.1) (drinking.py:77): a candidate is near when one of the cup's VERTICES is within the limit
    // of the particle (the oracle's particle_near_tool: accurate to ~0.5 mm at this range, where the face-plane bound ran 10-30 % low).
    // The shape and vertex loops are wave uniform (scalar / broadcast loads); lanes without a candidate idle.
    if (wave_any(spilled)) {
      for (int sh = 0; sh < NS; sh++) {
        const int col = cl[cl[AGX_CL_OFF_SHAPE] + 4 * sh];
        const int* ci = c.bi + c.bi[AGX_H_OFF_COLL] + col * AGX_C_STRIDE; const float* cf = c.bf + c.bi[AGX_H_OFF_COLL] + col * AGX_C_STRIDE;
        if (ci[AGX_C_TAG] != AGX_TAG_TOOL) continue;
        const float* B = body + 12 * agxw::body_slot(ci[AGX_C_BODY], c.ndof, c.nhuman); const float* R = B + 3;
        const float d0 = x[0] - B[0], d1 = x[1] - B[1], d2 = x[2] - B[2];
        const float xl0 = R[0] * d0 + R[3] * d1 + R[6] * d2, xl1 = R[1] * d0 + R[4] * d1 + R[7] * d2, xl2 = R[2] * d0 + R[5] * d1 + R[8] * d2;
        const float lim = spill + margin + cf[AGX_C_RADIUS], lim2 = lim * lim;
        const float* v = c.bf + c.bi[AGX_H_OFF_VERT] + 3 * ci[AGX_C_VOFF];
        for (int k = 0; k < ci[AGX_C_NVERT]; k++) {
          const float e0 = xl0 - v[3 * k], e1 = xl1 - v[3 * k + 1], e2 = xl2 - v[3 * k + 2];
          if (e0 * e0 + e1 * e1 + e2 * e2 <= lim2) spilled = false;
        }
      }
    }
    const bool hit = is_active && greport && ((const int*)greport)[lane] != 0;
    const uint64_t m_drunk = wave_ballot(drunk), m_spilled = wave_ballot(spilled), m_hit = wave_ballot(hit);
    food_reward = 10.f * (float)popc64(m_drunk) - (float)popc64(m_spilled);
    food_hit = -(float)popc64(m_hit);
    vel_sum = wave_sum(drunk ? speed : 0.f);
    success += popc64(m_drunk);
    for (uint64_t m = m_drunk; m; m &= m - 1) {                   // teleported in ascending order, three draws each (drinking.py:74)
      const v3 away = teleport_draw(r0, r1);
      if (lane == ffs64(m)) st3(gwater + 3 * lane, away);
    }
    wave_sync();
    if (lane < 2) {
      const uint32_t gone = (uint32_t)((m_drunk | m_spilled) >> (32 * lane)), off = (uint32_t)((m_drunk | m_hit) >> (32 * lane));
      Li[L_ST + s_task + AGX_DK_ALIVE + lane] = (int)((uint32_t)Li[L_ST + s_task + AGX_DK_ALIVE + lane] & ~gone);
      Li[L_ST + s_task + AGX_DK_ACTIVE + lane] = (int)((uint32_t)Li[L_ST + s_task + AGX_DK_ACTIVE + lane] & ~off);
    }
    wave_sync();
  }
#endif
  // end-effector speed (feeding.py:22), human_preferences (env.py:237-274, feeding branch), reward
  const float ee_speed = ee_speed_of(c);
  float pref = TKF(c, AGX_T_C_V) * (-ee_speed) + TKF(c, AGX_T_C_F) * (-total_f) + TKF(c, AGX_T_C_HF) * (tool_f < 10.f ? 0.f : -tool_f)
             + TKF(c, AGX_T_C_FD) * food_hit + TKF(c, AGX_T_C_FDV) * (-vel_sum);
  v3 sp; m3 sR; tool_base_pose(c, sp, sR);
  v3 dd = target - sp;
#if AGX_TASK == 5   /* AGX_TASK_DRINKING (an enum: not visible to the preprocessor) */
  dd = target - cup_top;                                           // the top centre of the cup against the mouth (drinking.py:25-26), and the tilt term (:30-31)
  float reward = TKF(c, AGX_T_W_DISTANCE) * (-sqrtf(dot(dd, dd))) + TKF(c, AGX_T_W_ACTION) * (-sqrtf(an2)) + TKF(c, AGX_T_W_TILT) * tilt_term + TKF(c, AGX_T_W_FOOD) * food_reward + pref;
#else
  float reward = TKF(c, AGX_T_W_DISTANCE) * (-sqrtf(dot(dd, dd))) + TKF(c, AGX_T_W_ACTION) * (-sqrtf(an2)) + TKF(c, AGX_T_W_FOOD) * food_reward + pref;
#endif
  FinishOut r;
  r.reward = reward; r.total_force = total_f; r.success = enough_of_total(c, success); r.robot_force = robot_f; r.tool_force = tool_f; r.event = food_reward; r.pref = pref;
  finish_end(c, io, r, [&] {
    Li[L_ST + c.s_env + AGX_E_FOOD_ALIVE] = alive; Li[L_ST + c.s_env + AGX_E_FOOD_ACTIVE] = active;
    Li[L_ST + c.s_env + AGX_E_TASK_SUCCESS] = success; Li[L_ST + c.s_env + AGX_E_RNG] = (int)r0; Li[L_ST + c.s_env + AGX_E_RNG + 1] = (int)r1;
  });
}

AGX_DEV void env_finish(const uint32_t* blob, float* gstate, const float* gaction, float* gscratch, float* gobs, float* greward, uint8_t* gdone,
                        float* ginfo, float* lds, int lane, const float* greport = nullptr, float* gwater = nullptr) {
  const FinishIO io = {gstate, gaction, gscratch, gobs, greward, gdone, ginfo, greport, gwater};
  if constexpr (TASK == AGX_TASK_DRESSING) env_finish_dressing(blob, io, lds, lane);
  else if constexpr (TASK == AGX_TASK_BED_BATHING) env_finish_bed(blob, io, lds, lane);
  else if constexpr (TASK == AGX_TASK_SCRATCH_ITCH) env_finish_scratch(blob, io, lds, lane);
  else if constexpr (TASK == AGX_TASK_ARM_MANIPULATION) env_finish_arm(blob, io, lds, lane);
  else env_finish_feeding(blob, io, lds, lane);
  // Non-finite guard (the reference's nearest analogue is the forced reconnect of env.py:93-97): an environment whose joint or
  // free-body state has become NaN / Inf must not poison a training batch.  Its observation and reward are zeroed, it is reported done
  // -- so the auto-reset (agx_reset_done / the masked agx_reset) replaces its state -- and AGX_INFO_NCONTACT carries AGX_INFO_NONFINITE.
  {
    const int* bi = (const int*)blob; const float* st = lds + L_ST;    // the state copy of the task layer above
    const int ndof = bi[AGX_H_NDOF], nfree = bi[AGX_H_NFREE], s_q = bi[AGX_H_S_Q], s_free = bi[AGX_H_S_FREE], od = bi[AGX_H_OBS_DIM];
    // "not finite" includes velocities nothing in these scenes can reach (1e3 rad/s, m/s): a deep start-up penetration pushed out in one
    // substep (no recovery clamp) blows up over a few steps before it overflows -- it is ended as soon as it is implausible.
    // The outputs themselves are checked too (a finite state can still give an overflowing reward term).
    wave_sync();                       // (the observation was written by lane 0 of the task layer above)
    bool bad = false;
    for (int k = lane; k < 2 * ndof; k += 64) { const float v = st[(k < ndof ? s_q : bi[AGX_H_S_QD] - ndof) + k]; bad = bad || !(fabsf(v) < (k < ndof ? 3.0e38f : 1.0e3f)); }
    for (int k = lane; k < 13 * nfree; k += 64) { const float v = st[s_free + k]; bad = bad || !(fabsf(v) < (k % 13 >= 7 ? 1.0e3f : 3.0e38f)); }
    for (int k = lane; k < od; k += 64) bad = bad || !(fabsf(gobs[k]) < 3.0e38f);
    if (lane == 0) bad = bad || !(fabsf(*greward) < 3.0e38f);
    if (wave_any(bad)) {
      for (int k = lane; k < od; k += 64) gobs[k] = 0.f;
      if (lane == 0) { *greward = 0.f; *gdone = 1; }
      if (ginfo && lane < AGX_INFO_COUNT) ginfo[lane] = lane == AGX_INFO_NCONTACT ? AGX_INFO_NONFINITE : 0.f;
    }
  }
}

}  // namespace agx
