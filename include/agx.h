/* agx.h -- C ABI of libagx: the MI355X-native batched stepper behind Assistive Gym's
 * env.step() hot path.  Plain pointers and sizes only; no torch / C++ types.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo):
 *
 *   agx_create        p.connect(p.DIRECT) + the world build of reset()
 *                     (assistive_gym/envs/env.py:34,91-134; envs/feeding.py:114-172), for N envs.
 *                     The world is handed over as a compiled model blob (include/agx_blob.h).
 *   agx_set_state /   no reference equivalent (the reference has no p.saveState/restoreState,
 *   agx_get_state     SURVEY section 5): state injection for parity tests, checkpoints, reset pools.
 *   agx_settle        the settle loop `for _ in range(25): p.stepSimulation()` (feeding.py:178-179).
 *   (the citations are those of the FeedingJaco model; a BedBathingSawyer blob is served by the bed_bathing kernel
 *    variant, whose task layer replaces BedBathingEnv.step/_get_obs/get_total_force/update_targets,
 *    assistive_gym/envs/bed_bathing.py:12-110,190-203, and the non-feeding branch of human_preferences, env.py:244-247)
 *   agx_step          FeedingEnv.step(action) for every env: AssistiveEnv.take_step
 *                     (envs/env.py:174-235) incl. 5x p.stepSimulation() (env.py:226), _get_obs
 *                     (feeding.py:85-112), get_food_rewards (feeding.py:50-83), human_preferences
 *                     (env.py:237-274), reward / done / info (feeding.py:25-37).
 *   agx_observe       the `return self._get_obs()` of reset() (feeding.py:182).
 *   agx_sample_reset  FeedingEnv.reset() up to its settle loop (feeding.py:114-177) for every env, on the device:
 *                     Human.init draws (agents/human.py:72-92), the posed human (feeding.py:124-126), the mouth
 *                     target (feeding.py:184-196), init_robot_pose -> Robot.ik_random_restarts (env.py:276-310,
 *                     agents/robot.py:84-121, incl. the rejection of IK solutions that touch the human / table / wheelchair,
 *                     robot.py:105-112, env.py:299-308), tool / bowl / food placement (feeding.py:143-166).
 *   agx_reset         the same followed by the settle loop, for the envs selected by a mask (a caller resetting
 *                     the envs that are done), per-env seeds optional.
 *   agx_reset_done    gym's TimeLimit/auto-reset on done (assistive_gym/__init__.py:11), drawing
 *                     the new post-reset state from a caller-provided pool.
 *
 * All `*_dev` pointers are DEVICE pointers (HBM) owned by the caller; `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  Calls on one handle must come from one thread at a
 * time; handles are independent.  Every function returns 0 on success or a negative AGX_E_* code
 * and never calls exit(); agx_last_error() describes the last failure of the calling thread.
 */
#ifndef AGX_H
#define AGX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct agx_handle_s* agx_handle;

enum { AGX_OK = 0, AGX_E_ARG = -1, AGX_E_BLOB = -2, AGX_E_HIP = -3, AGX_E_NOGPU = -4, AGX_E_LIMIT = -5 };

#define AGX_INFO_DIM 8   /* see AGX_INFO_* in agx_blob.h */

/* library / build information */
const char* agx_version(void);
const char* agx_last_error(void);
int agx_device_count(void);
int agx_lds_bytes_per_env(void);

int agx_create(const void* blob, size_t blob_bytes, int n_envs, int device, agx_handle* out);
void agx_destroy(agx_handle h);
int agx_dims(agx_handle h, int* n_envs, int* act_dim, int* obs_dim, int* state_words);

/* host <-> device copies of the per-env state records, [n_envs][state_words] float32 */
int agx_set_state(agx_handle h, const float* host_states);
int agx_get_state(agx_handle h, float* host_states);
/* device address of the state records (e.g. to fill them from a device-resident pool) */
int agx_state_dev(agx_handle h, float** out_dev);

/* n_substeps p.stepSimulation() calls (each AGX_H_SIM_SUBSTEPS internal substeps) without actions, task layer or hooks of env.step */
int agx_settle(agx_handle h, int n_substeps, void* stream);
int agx_step(agx_handle h, const float* actions_dev, float* obs_dev, float* reward_dev,
             uint8_t* done_dev, float* info_dev, void* stream);
/* same as agx_step, additionally dumping first-substep internals ([n_envs][agx_debug_words()]) */
int agx_step_debug(agx_handle h, const float* actions_dev, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev, float* info_dev, float* debug_dev, void* stream);
/* agx_settle, additionally dumping first-substep internals (models without a task layer to finish a step with, e.g. bed_settle) */
int agx_settle_debug(agx_handle h, int n_substeps, float* debug_dev, void* stream);
/* models with a cloth section (DressingBaxter; assistive_gym/envs/dressing.py:149-157, p.loadCloth / p.getSoftBodyData): the garment of
 * every environment is a float[2][nodes][3] record next to its state record -- node positions, node velocities.  agx_step / agx_settle
 * advance it; agx_reset_done also replaces the garment of a finished environment, from the device array [pool_n][2][nodes][3] given once
 * with agx_set_cloth_pool (same pool index as the state record). */
int agx_cloth_nodes(agx_handle h, int* nodes);   /* 0 for models without a cloth */
int agx_set_cloth(agx_handle h, const float* host_cloth);
int agx_get_cloth(agx_handle h, float* host_cloth);
int agx_cloth_dev(agx_handle h, float** out_dev);
int agx_set_cloth_pool(agx_handle h, const float* pool_cloth_dev);
/* models with a cloth: copies the cloth kernel's report of the LAST agx_step to the host -- per environment float[18] the six sleeve vertices
 * (util.py:156-157), 2 unused, then per node and contact slot {height of the node, |contact force| of the last substep, -1 = no contact}
 * (what dressing.py:25,35-43 reads from getSoftBodyData; AGX_CLOTH_REPORT_WORDS in agx_blob.h).  words_per_env (may be NULL) receives the row
 * length; host_report NULL = query the length only.  Synchronises the device.  For parity tests of the cloth-force term (which node contacts
 * are in the sum), not on the step path.
 * Models with a particle section (the water of the drinking scenes): the row is 64 words, int32 behind the float pointer -- per particle 1
 * when it touched a shape of the person in the LAST internal substep of the last agx_step / agx_settle, else 0; 0 beyond the last particle. */
int agx_get_cloth_report(agx_handle h, float* host_report, int* words_per_env);
int agx_debug_words(void);   /* of the FeedingJaco kernel variant; agx_debug_layout for the variant serving a handle */
/* layout of the debug record of the kernel variant serving this handle: out8 = {words per env, contacts offset, M^-1 offset,
 * M^-1 row stride, row headers offset, impulses offset, phase timers offset, qdd offset} */
int agx_debug_layout(agx_handle h, int* out8);
/* name of the compiled kernel variant (limits + task layer) that serves this handle: "feeding", "bed_bathing" */
const char* agx_variant_name(agx_handle h);
/* contacts dropped since agx_create because a budget was exceeded (contact, row or coefficient cap), summed over all envs:
 * they are missing from the dynamics and from total_force_on_human; 0 in a healthy run */
int agx_overflow_count(agx_handle h, int* out);
/* independent chunks of environments every step / settle of this handle is issued as, each on its own stream: AGX_CHUNKS as read by
 * agx_create, else 3 from 2048 environments on and 1 below, 1 for the drinking scenes; within 1..8, and 1 where a chunk would hold fewer
 * than 64 environments */
int agx_chunk_count(agx_handle h, int* out);
/* same as agx_step (same chunk streams) with a HIP event after every kernel launch; blocks until the step
 * is done and returns the summed launch durations of one step in ms3 = {build, solve, finish kernels} and
 * the number of launches of each in launches3 (may be NULL) */
int agx_step_timed(agx_handle h, const float* actions_dev, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev, float* info_dev, void* stream, float* ms3, int* launches3);
int agx_observe(agx_handle h, float* obs_dev, void* stream);
/* ... for the environments with mask_dev[i] != 0 only (the rows of the others are left as they are); mask_dev NULL = all.
 * The first observation of environments replaced mid-batch by agx_reset_done / agx_reset */
int agx_observe_masked(agx_handle h, float* obs_dev, const uint8_t* mask_dev, void* stream);
/* Overwrites the state record of EVERY env of the handle with a freshly sampled pre-settle reset state; env i
 * is a pure function of (seed + i) (counter-based Philox4x32-10 draws, so the result does not depend on
 * how envs are spread over handles or GPUs).  impairment_mode: -1 = random over none/limits/weakness/tremor
 * (human.py:80), -2 = random without tremor, 0..3 = fixed; gender_mode: -1 random, 0 male, 1 female.
 * ik_info_dev (may be NULL): [n_envs][4] float = {IK met the thresholds, restarts used, position error,
 * impairment drawn}; for a free-standing robot, whose base pose is searched as Robot.position_robot_toc does
 * (robot.py:123-215: AGX_X_TOC_ATTEMPTS candidate poses per round, one per lane): {a candidate reached the start
 * pose, rounds used, goals reached by the chosen candidate incl. the start pose, impairment drawn}.
 * Models with a cloth: the garment is placed at the sampled end effector (dressing.py:146-153), at rest.
 * Follow with agx_settle(h, 25, stream) (feeding.py:178-179) and agx_observe -- or use agx_reset, which also
 * switches the garment of a dressing scene from its settle gravity to full gravity when the settle is over.
 * Also zeroes the handle's episode counters. */
int agx_sample_reset(agx_handle h, uint64_t seed, int impairment_mode, int gender_mode, float* ik_info_dev, void* stream);
/* reset() of a SUBSET of the envs (gym semantics: the caller resets the envs that are done): envs with
 * mask_dev[i] != 0 (NULL = all) are re-sampled as by agx_sample_reset -- from seeds_dev[i] if seeds_dev is
 * given, else from seed + i -- and then run `settle_substeps` substeps (25 in feeding.py:178-179) while all
 * other envs are left untouched.  Their episode counters restart at 0. */
int agx_reset(agx_handle h, const uint8_t* mask_dev, const uint64_t* seeds_dev, uint64_t seed, int impairment_mode,
              int gender_mode, int settle_substeps, void* stream);
/* Bed bathing (reference: BedBathingEnv.reset, assistive_gym/envs/bed_bathing.py:119-137): the human of such a model is a rag doll dropped
 * onto the bed and left to settle for 100 simulation steps before the rest of the reset is sampled.  `settle` is a second handle, created
 * by the caller on the rag-doll model blob (bed_settle) with the same number of environments on the same device; agx_sample_reset / agx_reset
 * of `h` then sample that model's drop records from the same seeds, settle them for n_substeps substeps and read the human's resting pose
 * from its state records.  The second handle is not owned (destroy it after `h`); a null `settle` detaches.  Without an attachment the
 * sampler of such a model refuses to run.
 * Arm manipulation (ArmManipulationEnv.reset, assistive_gym/envs/arm_manipulation.py:117-165): two settles.  `settle` is
 * then a handle on the task's FALL model (the same blob with HUMAN_GRAVITY_Z = -1 and AGX_X_FLAGS bit 8: its sampler writes the record the
 * posed arm falls from), n_substeps the length of the fall (100); the rag-doll handle is attached to the fall handle by a second call.
 * agx_sample_reset / agx_reset of `h` run rag doll, fall and the task's sampler in that order. */
int agx_attach_settle_model(agx_handle h, agx_handle settle, int n_substeps);

/* envs with done != 0 get a fresh state from pool_dev ([pool_n][state_words]); the pool entry is
 * (env_offset + env_index + 977 * episode_count) mod pool_n with env_offset = the global index of this handle's first env
 * (agx_set_env_offset, default 0), so results do not depend on how the envs are spread over GPUs */
int agx_reset_done(agx_handle h, const float* pool_dev, int pool_n, const uint8_t* done_dev, void* stream);
/* the same for an environment that ends OUTSIDE the batch's episode boundary (the non-finite guard of agx_step reports done = 1 mid-episode;
 * the reference's nearest analogue is the forced reconnect of env.py:93-97): the replacement state joins the lock-stepped batch at
 * `iteration` (env.py:185; < 0: keep the pool record's own), so that it reaches `done` (feeding.py:37) together with the others */
int agx_reset_done_at(agx_handle h, const float* pool_dev, int pool_n, const uint8_t* done_dev, int iteration, void* stream);
/* Collision rejection for resets sampled on the host (env.py:276-310 init_robot_pose, robot.py:103-108): runs the stepper's collision
 * pass on the states as they are (they are not advanced) and writes one byte of AGX_COLLIDE_* flags per environment to the HOST buffer
 * flags_host[n_envs].  Synchronises the stream. */
#ifndef AGX_COLLIDE_FLAGS
#define AGX_COLLIDE_FLAGS
enum { AGX_COLLIDE_ENV = 1,    /* a robot link or the tool touches (distance <= 0) the human or the furniture               */
       AGX_COLLIDE_SELF = 2 }; /* two robot links, or a robot link and the tool, interpenetrate by more than 1 cm           */
#endif
int agx_check_collisions(agx_handle h, uint8_t* flags_host, void* stream);
int agx_set_env_offset(agx_handle h, long long env_offset);

/* ---- whole-batch observation collation across GPUs: environments are sharded by contiguous index ranges, one
 * process per GPU; the only exchange is an all-gather of the [n_envs, obs_dim] shards over RCCL / xGMI, and only when one
 * consumer wants the whole batch.  RCCL is bound at run time (an instance already loaded into the process is reused).
 * agx_comm_unique_id: rank 0 obtains the 128-byte id and hands it to the other ranks by the host's own means (MPI, TCP, file);
 * agx_comm_init_rank: collective over all ranks; agx_allgather: gathered_dev[rank * floats_per_rank ...] = the shard of `rank`,
 * enqueued on `stream` (use a side stream and an event after agx_step to overlap it with the next step); comm == NULL = one rank. */
int agx_comm_unique_id(void* out128);
/* What is gathered: agx_pack_step writes packed_dev[n_envs][obs_dim + 4] = observation | reward | done (0 / 1) | total_force_on_human |
 * task_success per environment (the sampler's obs, reward, done, info: assistive_gym/learn.py:26,72), enqueued on `stream` after the agx_step
 * that produced them; agx_allgather of n_envs * (obs_dim + 4) floats then collates the whole batch in ONE collective per step. */
int agx_pack_step(agx_handle h, const float* obs_dev, const float* reward_dev, const uint8_t* done_dev, const float* info_dev, float* packed_dev, void* stream);
int agx_comm_init_rank(int device, int rank, int world, const void* unique_id128, void** comm_out);
int agx_comm_destroy(void* comm);
int agx_allgather(agx_handle h, const float* local_dev, float* gathered_dev, size_t floats_per_rank, void* comm, void* stream);

/* ---- the learner's side of a rollout step (assistive_gym/learn.py trains with RLlib PPO; here assistive_gym_amd/ppo.py).  Both entries are
 * STATELESS: no handle, they run on the calling thread's current HIP device and report by return code only (agx_last_error is not set).
 *
 * agx_policy_act: GaussianMLPPolicy.act (assistive_gym_amd/rollout.py; RLlib's fcnet with vf_share_layers False) for n_envs observations in
 * one launch: the tanh MLPs obs -> hidden_a -> hidden_b -> 2 act_dim (mean | log_std, clamped to [-20, 2]) and obs -> hidden_a -> hidden_b -> 1,
 * action = mean + exp(log_std) eps, logp = sum_k(-eps_k^2 / 2 - log_std_k - ln(2 pi) / 2), value.  deterministic != 0: eps = 0.
 * params_dev: one float32 vector in nn.Linear's layout (weight [out][in] row-major, then bias), in the order pi.0, pi.2, pi.4, vf.0, vf.2, vf.4.
 * obs_stride / action_stride: row strides in floats (>= the dims), so the pointers may address a column slice of a wider tensor (the two agents
 * of a co-op batch) or a row of a rollout buffer; columns outside the slice are not touched.  logp_dev, value_dev: [n_envs].
 * Noise: env i draws from Philox4x32-10 with key seed + env_offset + i and counter (k >> 2, step, 1, 0) for component k (the reset generator's
 * counters have third word 0) -- a function of the GLOBAL env index, the step and the component only.  Output words w0..w3: (wa, wb) = (w0, w1)
 * if k & 2 == 0 else (w2, w3); u1 = ((wa >> 8) + 0.5) 2^-24, u2 = (wb >> 8) 2^-24, r = sqrt(-2 ln u1), eps = r cos(2 pi u2) for even k,
 * r sin(2 pi u2) for odd k.
 * Limits (AGX_E_ARG before any device call): obs_dim, hidden_a, hidden_b 1..128, act_dim 1..32, strides >= dims, n_envs >= 0 (0: AGX_OK, no launch).
 *
 * agx_gae: generalised advantage estimation over a finished rollout, one lane per environment walking t = horizon - 1 .. 0:
 * delta = r[t] + gamma v[t+1] live - v[t], adv[t] = delta + gamma lam live adv[t+1], ret[t] = adv[t] + v[t], live = !done[t].
 * rewards / dones / adv / ret: [horizon][n_envs]; values: [horizon + 1][n_envs] (bootstrap value last). */
int agx_policy_act(const float* params_dev, int obs_dim, int hidden_a, int hidden_b, int act_dim,
                   const float* obs_dev, int obs_stride, int n_envs,
                   uint64_t seed, long long env_offset, uint32_t step, int deterministic,
                   float* action_dev, int action_stride, float* logp_dev, float* value_dev, void* stream);
int agx_gae(const float* rewards_dev, const float* values_dev, const uint8_t* dones_dev, int horizon, int n_envs,
            float gamma, float lam, float* adv_dev, float* ret_dev, void* stream);

/* ---- end-effector control: Cartesian commands for the arm(s), turned into joint-space actions on the device (csrc/agx_ik.h, csrc/agx_ik.hip).
 * The reference's teleop_example.py / igibson_drinking_example.py read robot.get_pos_orient(robot.right_end_effector), call robot.ik(...) on a
 * target pose and send (target_joint_angles - current_joint_angles) * 10 as the action; these entries do the same for every environment of a
 * handle.  The IK is the damped-least-squares iteration of assistive_gym_amd/host/kin.py (RobotKin.ik) in float32 -- Bullet's own IK is not
 * reproduced anywhere in this project.  Nothing here writes the state records.
 *
 * agx_ee_arms: arm chains the handle's model has -- 1, 2 for a two-armed robot in arm manipulation (AGX_X_CHAIN2: index 0 = the right arm, 1 =
 * the left), 0 for a robot on wheels (AGX_H_BASE_LINK > 0) and for any blob whose chain is not the serial 7-joint arm agx_create checks for its
 * reset generator.  With 0 arms the two entries below return AGX_E_ARG.
 * agx_ee_pose: pose_dev[n_envs][arms][7] = world position and quaternion (x, y, z, w) of the end-effector frame (AGX_T_EE_*, AGX_T_EE2_*).
 * agx_ee_ik: target_dev rows of target_stride floats, per arm 7 floats (frame AGX_EE_ABSOLUTE: world position, quaternion x y z w, normalised on the
 * device) or 6 (AGX_EE_DELTA: world translation d and world rotation vector r applied to the current pose: p + d, exp(r) (x) q).  `iters`
 * iterations (1..1000) from the state's joint angles: e = [dp; 2 vec(q_t (x) conj(q))] with the quaternion flipped to w >= 0,
 * dq = J^T (J J^T + damping^2 I)^-1 e, the whole step scaled down to max|dq| <= 0.5, q clipped to [AGX_R_LOWER, AGX_R_UPPER]; an
 * environment stops once both error norms are below 1e-4.  Outputs, each may be NULL: q_out_dev[n_envs][arms][7] joint angles; err_dev[n_envs][arms][2]
 * position and orientation error norms at exit; action_dev rows of action_stride floats (>= the action dimension): every chain joint's action
 * column (AGX_R_ACT, and the duplicate column of a single arm driven as 'both', AGX_T_DUP_ACT) = gain (q_out - q), the columns of one arm scaled
 * together so that the largest magnitude is at most 1 (the direction survives where the environment's own clip would bend it).  Columns of no
 * chain -- the human's in a co-op batch -- are not touched.  A state or a target that is not finite: action 0, err +inf, q_out = q; a
 * non-finite action is never written.
 * AGX_E_ARG with agx_last_error text, before any launch: NULL handle, NULL target, 0 arms, iters outside 1..1000, damping <= 0, target_stride <
 * arms x 7 (6), action_stride < the action dimension, an unknown frame. */
#ifndef AGX_EE_FRAMES
#define AGX_EE_FRAMES
enum { AGX_EE_ABSOLUTE = 0, AGX_EE_DELTA = 1 };
#endif
int agx_ee_arms(agx_handle h, int* arms);
int agx_ee_pose(agx_handle h, float* pose_dev, void* stream);
int agx_ee_ik(agx_handle h, const float* target_dev, int target_stride, int frame, int iters, float damping, float gain,
              float* q_out_dev, float* action_dev, int action_stride, float* err_dev, void* stream);

/* ---- the camera: depth, segmentation and RGB images of the environments, ray-cast on the device (csrc/agx_render.hip).  The reference's
 * env.setup_camera / setup_camera_rpy / get_camera_image_depth (assistive_gym/envs/env.py:342-359) hand a view to PyBullet's renderer; here ONE
 * camera is shared by all environments of a handle (every scene sits at the same world coordinates) and what is drawn is the collision geometry
 * of the model blob: every collider by its vertex count -- 1 a sphere, 2 a capsule, 3 and more the convex polytope of the vertices with each face
 * plane pushed outward by AGX_C_RADIUS (a flat or degenerate vertex set: its bounding box) -- for the environment's gender only, where the
 * collide phase places it (a food or water particle the task has retired sits beyond the far plane), and the water particles of a drinking scene as
 * spheres of the section's MARGIN.  The garment of a dressing scene is drawn once agx_camera_garment switches it on (below; off by default).
 * Not Bullet's rasteriser: no visual meshes, no textures, no shadows, no specular term.
 * Pixel (i, j), row 0 at the top, casts one ray through its centre: in camera space ((2 (i + 0.5) / w - 1) aspect tan(fov / 2),
 * (1 - 2 (j + 0.5) / h) tan(fov / 2), -1), not normalised, so the ray parameter t is the view-space depth.  A convex collider meets the ray in an
 * interval; its hit is where the ray enters, or where it leaves if it enters before the near plane.  The nearest hit with near <= t <= far wins,
 * the lower collider index on a tie.
 *
 * agx_camera_set: the view from (eye, target, up) as p.computeViewMatrix builds it, fov_deg the vertical field of view, aspect = width / height
 * (the reference: up = [0, 0, 1], near 0.01, far 100).  The first call on a handle also builds the hulls' face planes on the host and allocates the
 * frame table; later calls only move the camera.
 * agx_render: environments [env0, env0 + count), count <= 65535, into [count][height][width] device arrays, each of which may be NULL (not all):
 *   depth_dev float32: t of the hit, `far` where nothing is hit;
 *   seg_dev   int32:   the collider index, ncoll + k for water particle k (ncoll + f for face f of the garment, below), -1 for the background;
 *   rgba_dev  uint8[4] (4-byte aligned): round(255 min(1, colour (ambient + diffuse max(0, n . l)))) per channel, l = light3 normalised (the
 *             direction towards the light), n the outward normal at the hit, colour by the collider's AGX_C_TAG from the table agx_camera_colours
 *             copies out (float[12][3]: tags 0..9, then the water, then the background, which is not shaded); alpha 255.
 * agx_collider_count / agx_collider_frames: the kinematics half on its own -- frames_dev[count][ncoll][12] = world position (3) and rotation
 * (9, row-major) of the body of every collider.  Nothing here writes the state records.
 * AGX_E_ARG with agx_last_error text, before any launch: a NULL handle or view vector, values that are not finite, fov outside (0, 180), width /
 * height outside 1..8192, near <= 0 or far <= near, eye = target or up along the view direction, agx_render before agx_camera_set, a range
 * outside the handle's environments, a zero light vector, all three outputs NULL.  AGX_E_LIMIT: more than 1,024 colliders + particles. */
int agx_camera_set(agx_handle h, const float* eye3, const float* target3, const float* up3, float fov_deg, int width, int height, float near_plane, float far_plane);
int agx_render(agx_handle h, int env0, int count, const float* light3, float ambient, float diffuse,
               float* depth_dev, int32_t* seg_dev, uint8_t* rgba_dev, void* stream);
int agx_collider_count(agx_handle h, int* ncoll);
int agx_collider_frames(agx_handle h, int env0, int count, float* frames_dev, void* stream);
int agx_camera_colours(float* out36);

/* ---- the garment of a dressing scene in the camera's images (csrc/agx_garment.h, agx_render_garment_kernel of csrc/agx_render.hip: a second
 * kernel that draws the faces over the images of the rigid caster).  Off by default: with it off agx_render launches what it launches without
 * these entries and returns the same bits, for every handle; with it on, a pixel no face wins is that same pixel.
 * Triangle table, from the blob alone: walk the nodes a = 0 .. NN-1 in order and each node's incident-face entries (j, k) (AGX_CL_OFF_FACE, from
 *   AGX_CL_OFF_NODE) in order; keep (a, j, k) when a < j and a < k.  Every face has three rotated entries, so it is kept exactly once and keeps its
 *   winding; face f is the f-th kept triple (dressing_baxter: 7,673 faces from 23,019 entries).  A particle section (AGX_CL_PARTICLES, the water)
 *   has no faces and is not a garment.
 * Positions: the first [nodes][3] floats of the environment's garment record (agx_cloth_dev) as it stands in stream order when agx_render runs.
 *   The record is only read.
 * Hit: the camera's ray eye + t d (d not normalised, t the view-space depth) hits face (a, b, c) when its barycentric coordinates satisfy u >= 0,
 *   v >= 0, u + v <= 1, the determinant is not 0 and near <= t <= far.  Both sides are visible; a zero-area face is never hit; the garment has no
 *   thickness (MARGIN is a contact distance and is not drawn).  A face with a node that is not finite is not hit.
 * Merge with the rigid scene: the smaller t wins; on a tie the lower segmentation value: a collider before a face, a lower face before a higher.
 * Outputs: seg = ncoll + f (a scene with a garment has no water particles); depth = t; rgba by the camera's formula with n the unit normal of the
 *   face at its current node positions, signed against the ray (n . d < 0), and the garment's own colour (139, 195, 74) / 256 (the reference's
 *   gown, dressing.py:153, drawn opaque: alpha 255), which agx_camera_garment_colour copies out (float[3]).
 * agx_camera_garment: the switch.  AGX_E_ARG for on != 0 on a model without a garment (no cloth section, or a particle section) and for any call
 *   before agx_camera_set.  The first enabling call builds the triangle table on the host and uploads it; later calls only flip the switch.
 *   AGX_E_BLOB: the cloth section is malformed (an offset outside the section, a node index >= NN, an entry count that is no multiple of 3).
 * agx_garment_faces: the table as host_tris[count][3]; host_tris may be NULL to ask for the count only; count = 0 for a model without a garment.
 *   It needs no camera.
 * Every check runs before any launch; nothing here writes the state or garment records. */
int agx_camera_garment(agx_handle h, int on);
int agx_garment_faces(agx_handle h, int* count, int* host_tris);
int agx_camera_garment_colour(float* out3);

/* ---- closest points between collider pairs of the environments, on the device (csrc/agx_proximity.h, csrc/agx_proximity.hip).  The reference's
 * Agent.get_closest_points(agentB, distance, linkA, linkB) (assistive_gym/envs/agents/agent.py:118-130) asks PyBullet for the points of two bodies
 * closer than `distance`; here a query is a list of collider pairs of the model blob, answered for a range of environments in one call: the
 * variant's frames kernel into a frame table of the query's own, then one kernel whose work item is one (environment, pair), a lane each, every
 * lane running the narrowphase of the stepper (csrc/agx_gjk.h).
 * A record is 12 words: 0 dist, the surface distance, negative when penetrating | 1-3 the point on A's surface, world | 4-6 the point on B's |
 * 7-9 the unit normal from B towards A (as in the contact records, Bullet's contactNormalOnB) | 10 int32 kind | 11 int32 pair index.
 *   kind 1, closest points: core = convex hull of the collider's vertices placed by its body's frame, d the distance of the cores, (ca, cb) their
 *     closest points; n = (ca - cb) / d, dist = d - r_a - r_b, pa = ca - r_a n, pb = cb + r_b n.
 *   kind 2, overlapping cores (closer than a micron counts): the direction of the blob's table with the smallest max_B(x.d) - min_A(x.d), the first
 *     on ties; n that direction, dist = -that - r_a - r_b, pa = A's first vertex of smallest x.n, less r_a n, pb = pa - dist n.
 *   kind 0, nothing reported: dist = +inf, words 1-9 zero -- dist >= max_distance (Bullet reports closer points only), a human collider that is
 *     not of the environment's gender, a frame or a vertex that is not finite.  A NaN is never written.
 *   A static world box (body AGX_BODY_WORLD, 8 vertices, tag TABLE or PLANE) is taken as the axis-aligned box it is, clipped to the other
 *   collider's world box grown by a bound on their distance (exact: the box's nearest point is the clamp of a point of the other collider;
 *   the bound does not look at max_distance, so a record is the same at every max_distance above its dist);
 *   one point per pair, no face manifold.
 * Nearest records: the same 12 words per (environment, query) -- a query is the subset of the pairs that carry its id: the record of smallest dist
 *   among those with kind != 0, the lower pair index on a tie, word 11 the winning pair; none: kind 0, pair -1, dist = +inf.
 * agx_proximity_set: the pair list [npairs][3] = collider a, collider b, query id, on the host.  The first call allocates the frame table; a later
 *   call replaces the list.  agx_proximity_pairs: what is set (0, 0 before a set).
 * agx_proximity: environments [env0, env0 + count) into records_dev [count][npairs][12] and nearest_dev [count][nqueries][12], float32 device arrays,
 *   16-byte aligned, either of which may be NULL (not both).  Results are bit-reproducible and do not depend on the range asked for.
 * AGX_E_ARG, with agx_last_error text, before any launch: a NULL handle or list, npairs < 1, nqueries outside 1..16, a collider index outside
 * [0, ncoll), a == b, a query id outside [0, nqueries), agx_proximity before a set, a range outside the handle's environments, max_distance
 * negative or not finite, both outputs NULL, an output that is not 16-byte aligned.  AGX_E_LIMIT: more than 8,192 pairs.
 * Nothing here writes the state, garment or camera records. */
int agx_proximity_set(agx_handle h, const int32_t* pairs_host, int npairs, int nqueries);
int agx_proximity_pairs(agx_handle h, int* npairs, int* nqueries);
int agx_proximity(agx_handle h, int env0, int count, float max_distance, float* records_dev, float* nearest_dev, void* stream);

/* convenience wrappers with HOST buffers (copies included; not the timed path) */
int agx_step_host(agx_handle h, const float* actions, float* obs, float* reward, uint8_t* done, float* info);
int agx_observe_host(agx_handle h, float* obs);

/* HIP-event timing of the kernels launched between begin and end on `stream` */
int agx_profile_begin(agx_handle h, void* stream);
int agx_profile_end(agx_handle h, void* stream, float* elapsed_ms);

int agx_synchronize(agx_handle h, void* stream);

/* wave-primitive self test (DPP reductions, ballots, scans): returns 0 if the device matches the
 * host-computed expectations */
int agx_selftest(int device);

#ifdef __cplusplus
}
#endif
#endif
