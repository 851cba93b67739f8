// agx_api.hip -- libagx: C ABI (include/agx.h), handles, streams and launch sequencing for gfx950.
// The kernels are compiled per variant (limits + task layer) in agx_kernels.hip; agx_create picks the variant whose
// task and limits fit the model blob.  One workgroup = one wavefront = one environment (64 threads); an env.step() is
// frame_skip x [build kernel, solve kernel] + finish kernel per chunk of environments.
#include "agx_wave.h"
#include "agx_variant.h"
#include "agx_render.h"
#include "agx_proximity.h"
#include "agx_hull.h"
#include "agx_garment.h"
#include "../../include/agx_blob.h"
#include "../../include/agx.h"

#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;
int fail(int code, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e)); else snprintf(buf, sizeof buf, "%s", what);
  g_err = buf; return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(AGX_E_HIP, #x, e_); } while (0)

// the warm-start memory (AGX_P_WARMSTART) of the environments whose state is replaced from outside is forgotten: their scratch record's
// entry count is zeroed (mask null = every environment)
extern "C" __global__ void __launch_bounds__(256)
agx_forget_warm_kernel(float* scratch, int scr_words, int word, const uint8_t* mask, int n_envs) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env < n_envs && (!mask || mask[env])) { int* m = (int*)scratch + (size_t)env * scr_words + word; m[0] = 0; m[1] = 0; }      // META_NWARM, META_NMAN
}

// done envs take a fresh record from the pool; coalesced copy, one wave per env
extern "C" __global__ void __launch_bounds__(64)
agx_reset_kernel(float* state, const float* pool, int pool_n, const uint8_t* done, int* episode, int n_envs, int sw, long long env_offset, int iter_word, int iteration) {
  const int env = blockIdx.x;
  if (env >= n_envs || !done[env]) return;
  int ep = episode[env] + 1;
  // the pool entry is a function of the GLOBAL environment index: the same env draws the same states on any GPU count
  const float* src = pool + (size_t)((env_offset + env + 977 * (long long)ep) % pool_n) * sw;
  for (int k = threadIdx.x; k < sw; k += 64) state[(size_t)env * sw + k] = src[k];
  if (threadIdx.x == 0) {
    episode[env] = ep;
    // agx_reset_done_at: the replacement joins the lock-stepped batch at its current iteration (env.py:185), so that it ends with the batch
    if (iteration >= 0) ((int*)state)[(size_t)env * sw + iter_word] = iteration;
  }
}

// ... and, for models with a cloth, the garment that belongs to that pool record (launched after agx_reset_kernel: episode[] is already advanced)
extern "C" __global__ void __launch_bounds__(256)
agx_reset_cloth_kernel(float* cloth, const float* pool, int pool_n, const uint8_t* done, const int* episode, int n_envs, int cw, long long env_offset) {
  const int env = blockIdx.x;
  if (env >= n_envs || !done[env]) return;
  const float* src = pool + (size_t)((env_offset + env + 977 * (long long)episode[env]) % pool_n) * cw;
  for (int k = threadIdx.x; k < cw; k += 256) cloth[(size_t)env * cw + k] = src[k];
}

// drinking, device-side reset: the 4 x 4 x 4 grid of water spheres above the cup's base frame position, world axes, at rest (drinking.py:160-167)
extern "C" __global__ void __launch_bounds__(64)
agx_place_water_kernel(float* water, const float* state, const uint32_t* blob, const uint8_t* mask, int n_envs, int sw, int cw) {
  const int env = blockIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  const int* bi = (const int*)blob; const float* bf = (const float*)blob;
  const int oc = bi[AGX_H_OFF_CLOTH]; const int nn = bi[oc + AGX_CL_NN];
  const float* x0 = bf + oc + bi[oc + AGX_CL_OFF_X0];
  const float* cup = state + (size_t)env * sw + bi[AGX_H_S_FREE] + 13 * bi[AGX_H_TOOL_BODY];      // the cup's record holds its base frame (REFPOS = 0, compile_feeding)
  float* c = water + (size_t)env * cw;
  for (int k = threadIdx.x; k < 3 * nn; k += 64) { c[k] = x0[k] + cup[k % 3]; c[3 * nn + k] = 0.f; }
}

// models with a cloth, device-side reset: the garment of a freshly sampled environment is the loaded mesh shifted to the end effector
// (dressing.py:146-153: x = X0 + offset; the reset generator left the offset in the task words, AGX_DR_CLOTH_OFF), at rest
extern "C" __global__ void __launch_bounds__(256)
agx_place_cloth_kernel(float* cloth, const float* state, const uint32_t* blob, const uint8_t* mask, int n_envs, int sw, int cw) {
  const int env = blockIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  const int* bi = (const int*)blob; const float* bf = (const float*)blob;
  const int oc = bi[AGX_H_OFF_CLOTH]; const int nn = bi[oc + AGX_CL_NN];
  const float* x0 = bf + oc + bi[oc + AGX_CL_OFF_X0];
  const float* off = state + (size_t)env * sw + bi[AGX_H_S_TASK] + AGX_DR_CLOTH_OFF;
  float* c = cloth + (size_t)env * cw;
  for (int k = threadIdx.x; k < 3 * nn; k += 256) { c[k] = x0[k] + off[k % 3]; c[3 * nn + k] = 0.f; }
}
// ... and when the settle of reset() is over the garment feels full gravity (dressing.py:195)
extern "C" __global__ void __launch_bounds__(64)
agx_cloth_gravity_kernel(float* state, const uint32_t* blob, const uint8_t* mask, int n_envs, int sw) {
  const int env = blockIdx.x * 64 + threadIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  const int* bi = (const int*)blob; const float* bf = (const float*)blob;
  state[(size_t)env * sw + bi[AGX_H_S_TASK] + AGX_DR_CLOTH_GRAVITY] = bf[bi[AGX_H_OFF_RESET] + AGX_X_CLOTH_GRAVITY];
}

extern "C" __global__ void __launch_bounds__(64) agx_selftest_kernel(float* out_f, int* out_i, unsigned long long* out_m) {
  const int lane = wave_lane();
  float x = (float)(lane * lane % 17) * 0.25f - 1.0f;
  out_f[lane] = wave_sum(x);
  out_f[64 + lane] = wave_min(x + (float)((lane * 7) % 5));
  out_f[128 + lane] = wave_bcast(x, 37);
  out_f[192 + lane] = wave_shfl(x, (lane * 13 + 5) & 63);
  out_i[lane] = wave_sum_i(lane % 7);
  out_i[64 + lane] = wave_scan_excl(lane % 5);
  unsigned long long m = wave_ballot((lane % 3) == 1);
  out_m[lane] = m;
  out_i[128 + lane] = wave_rank(m);
  out_f[256 + lane] = wave_max(x);
}

// the arm chain the IK code is compiled for (agx_reset.h rs_ik, agx_ik.h): `narm` joints in a serial chain -- each joint's parent is the one before, the
// first hangs off the base -- the k-th one driven by action act0 + k, the last one carrying the end-effector frame of link `ee_link`
bool arm_chain_ok(const int32_t* hi, const int32_t* chain, int narm, int act0, int ee_link) {
  for (int k = 0; k < narm; k++) {
    const int d = chain[k];
    if (d < 0 || d >= hi[AGX_H_NROBOT]) return false;
    const int32_t* R = hi + hi[AGX_H_OFF_ROBOT] + d * AGX_R_STRIDE;
    if (R[AGX_R_PARENT] != (k ? chain[k - 1] : -1) || R[AGX_R_ACT] != act0 + k) return false;
    if (k == narm - 1 && ee_link != d) return false;
  }
  return true;
}

}  // namespace

// csrc/agx_ik.hip
void agx_launch_ee_pose(hipStream_t st, const uint32_t* blob, const float* state, int sw, int n_envs, int arms, float* pose);
void agx_launch_ee_ik(hipStream_t st, const uint32_t* blob, const float* state, int sw, int n_envs, int arms, const float* target, int target_stride,
                      int frame, int iters, float damping, float gain, float* q_out, float* action, int action_stride, float* err);

// the camera of a handle (agx_camera_set): the device tables of csrc/agx_render.hip, owned, and the arguments every agx_render passes
struct agx_camera_s {
  agx_render_args A;
  float* frames; agx_render_coll* coll; float4* planes; float* colours;
  int ncoll;
  int4* tris; int ntri;      // the garment's triangle table (csrc/agx_garment.h), null until agx_camera_garment first switches the garment on
  bool garment;              // the switch of agx_camera_garment
  float* lend_depth; int* lend_seg; size_t lend_pixels;      // images the garment kernel merges into where the caller asked for no depth or seg
};

// the closest-point query of a handle (agx_proximity_set): the pair list and the per-collider flags of csrc/agx_proximity.h, the query's own
// frame table, all owned, and the arguments every agx_proximity passes
struct agx_prox_s {
  agx_prox_args A;
  float* frames; int* pairs; int* cflags;
  int ncoll, pairs_cap;
};

struct agx_handle_s {
  const agx_variant* V;   // the compiled kernel variant serving this model
  // what every launch passes: the model blob, the state / scratch records, their strides (agx_variant.h); with a cloth section (DressingBaxter) the
  // garments [n_envs][2][NN][3], the link frames of every substep of an env step for the cloth kernel and its report to the finish kernel
  agx_launch L;
  decltype(agx_variant::build) step_build;   // the build launcher of the step path: the one with the manifold stage where the blob has AGX_P_MANIFOLD > 0
  int collision_tries;    // reset generator: successful IK restarts that may be rejected for a collision (AGX_X_COLLISION_TRIES)
  int* first_restart_dev; uint8_t* work_dev;   // reset generator: per-env retry bookkeeping
  long long env_offset;   // global index of env 0 of this handle (multi-GPU sharding), see agx_set_env_offset
  int device;
  int iter_word;          // index of AGX_E_ITERATION in a state record (agx_reset_done_at)
  int frame_skip;
  int sim_sub;          // internal substeps per p.stepSimulation() (AGX_H_SIM_SUBSTEPS)
  int cloth_nn;
  bool particles;       // the "cloth" section holds the water particles of the drinking scene (AGX_CL_PARTICLES), not a garment
  const float* cloth_pool_dev;   // the garments of the reset pool (agx_set_cloth_pool)
  bool can_sample;      // the variant has a reset generator (agx_reset.h) and the blob fits it
  int ncoll;            // colliders of the model (agx_collider_count)
  int ee_arms;          // arm chains agx_ee_pose / agx_ee_ik serve (agx_ee_arms): 0 for a robot on wheels or a chain that fails arm_chain_ok
  // staging for the *_host convenience calls
  float *act_dev, *obs_dev, *rew_dev, *info_dev; uint8_t* done_dev;
  hipEvent_t ev0, ev1;
  hipEvent_t kev[8][16];   // agx_step_timed: boundaries of the launches of one step, per chunk
  // The environments are stepped in independent chunks on internal streams (AGX_CHUNKS overrides the
  // count): every chunk runs its own build -> solve -> ... chain, so the tail of one chunk's kernel
  // (environments with many rows finish last) overlaps with the next kernel of another chunk and the
  // lean solve kernel shares the CUs with the LDS-heavy build kernel.
  int n_chunks; hipStream_t cs[8]; hipEvent_t fork_ev, join_ev[8];
  int reset_flags;      // AGX_X_FLAGS of the blob's reset section (0 without one)
  agx_handle_s* settle; // bed bathing (AGX_X_FLAGS bit 4): the handle of the rag-doll model whose settled records the sampler reads (agx_attach_settle_model; not owned)
  int settle_substeps;  // substeps of that settle (100 simulation steps: bed_bathing.py:130-131)
  agx_camera_s* cam;    // null until agx_camera_set
  agx_prox_s* prox;     // null until agx_proximity_set
};

static void forget_warm(agx_handle_s* h, const uint8_t* mask_dev, hipStream_t st) {
  hipLaunchKernelGGL(agx_forget_warm_kernel, dim3((h->L.n_envs + 255) / 256), dim3(256), 0, st, h->L.scratch, h->V->scr_words, h->V->scr_warm_word, mask_dev, h->L.n_envs);
}

extern "C" {

const char* agx_version(void) { return "libagx 0.2 (gfx950, wave-per-env stepper)"; }
const char* agx_last_error(void) { return g_err.c_str(); }
int agx_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
int agx_lds_bytes_per_env(void) { return agx_variant_feeding()->lds_bytes; }
int agx_debug_words(void) { return agx_variant_feeding()->dbg_words; }   // FeedingJaco variant; agx_debug_layout(h) for a handle

static int create_fill(agx_handle h, const void* blob, size_t blob_bytes, int n_envs, int device);
void agx_destroy(agx_handle h);
int agx_create(const void* blob, size_t blob_bytes, int n_envs, int device, agx_handle* out) {
  if (!blob || !out || n_envs <= 0 || blob_bytes < sizeof(uint32_t) * AGX_H_COUNT) return fail(AGX_E_ARG, "agx_create: bad argument");
  const uint32_t* w = (const uint32_t*)blob; const int32_t* hi = (const int32_t*)blob;
  if (w[AGX_H_MAGIC] != AGX_BLOB_MAGIC || w[AGX_H_VERSION] != AGX_BLOB_VERSION || (size_t)hi[AGX_H_NWORDS] * 4 != blob_bytes)
    return fail(AGX_E_BLOB, "agx_create: not a model blob of this version");
  const agx_variant* V = nullptr;
  {
    // the first variant, in the order of agx_variants.def, with the model's task layer whose limits hold the model
#define AGX_VARIANT(name, ...) agx_variant_##name(),
    const agx_variant* all[] = {
#include "agx_variants.def"
    };
#undef AGX_VARIANT
    bool task_seen = false;
    for (const agx_variant* v : all) {
      if (v->task_kind != hi[AGX_H_TASK_KIND]) continue;
      task_seen = true;
      if (hi[AGX_H_NDOF] > v->max_dof || hi[AGX_H_NFREE] > v->max_free || hi[AGX_H_NHUMAN] > v->max_human || hi[AGX_H_NCOLL] > v->max_coll ||
          hi[AGX_H_STATE_WORDS] > v->st_words || hi[AGX_H_NROBOT] > v->max_block || hi[AGX_H_NHDOF] > v->max_block) continue;
      V = v; break;
    }
    if (!task_seen) return fail(AGX_E_LIMIT, "agx_create: no kernel variant is compiled for the task of this model");
    if (!V || hi[AGX_H_NDOF] + 6 * hi[AGX_H_NFREE] > 128 || hi[AGX_H_NGROUP] > 64 || hi[AGX_H_NDOF] > 64)
      return fail(AGX_E_LIMIT, "agx_create: model exceeds the limits of the compiled kernel variants");
  }
  for (int g = 0; g < hi[AGX_H_NGROUP]; g++) {   // the broadphase compacts each collider range of a pair group into a 128-entry list
    const int32_t* G = hi + hi[AGX_H_OFF_GROUP] + g * AGX_G_STRIDE;
    if (G[AGX_G_A1] - G[AGX_G_A0] > 128 || G[AGX_G_B1] - G[AGX_G_B0] > 128 || (G[AGX_G_B0F] >= 0 && G[AGX_G_B1F] - G[AGX_G_B0F] > 128))
      return fail(AGX_E_LIMIT, "agx_create: a pair group has a collider range of more than 128 colliders");
  }
  bool can_sample = true;   // every variant carries the reset generator; what follows finds the models it cannot sample
  int ee_arms = 0;
  {   // (scope of X and T)  Its IK is compiled for a serial 7-DoF arm carrying the end effector
    const int32_t* X = hi + hi[AGX_H_OFF_RESET];
    const int32_t* T = hi + hi[AGX_H_OFF_TASK];
    // the arm: rs_narm joints in a serial chain (AGX_X_CHAIN: each joint's parent is the one before, the first hangs off the base), the
    // k-th one driven by action k, the last one carrying the end effector
    const bool ragdoll = (X[AGX_X_FLAGS] & 32) != 0;  // the rag-doll model of bed bathing: its sampler writes the drop record, there is no robot
    const bool mobile = (X[AGX_X_FLAGS] & 8) != 0 || ragdoll;    // a robot on wheels: no arm chain to solve (its NARM only says that the blob has a reset section)
    if (X[AGX_X_NARM] != V->rs_narm || (!ragdoll && hi[AGX_H_NROBOT] < V->rs_narm) || hi[AGX_H_NHUMAN] >= 64 || hi[AGX_H_NDOF] > 64 || X[AGX_X_TOC_ATTEMPTS] > 64 ||
        X[AGX_X_TOC_NGOALS] > 4 || X[AGX_X_PED_N] > 2) can_sample = false;
    if (ragdoll && hi[AGX_H_NDOF] != 6 + X[AGX_X_NJOINT] - 1) can_sample = false;    // virtual joints + every joint of the tree but the fixed waist
    if (mobile && !ragdoll && (X[AGX_X_MOBILE_LIFT_DOF] < 0 || X[AGX_X_MOBILE_LIFT_DOF] >= hi[AGX_H_NROBOT] || X[AGX_X_TOC_ATTEMPTS] != 0 || X[AGX_X_IK_RESTARTS] != 0)) can_sample = false;
    // the arm: AGX_X_CHAIN, driven by the first actions (robot_arm = 'both' lists a single arm twice: the second copy's actions drive it, robot.py:16)
    const int dup = hi[AGX_H_TASK_KIND] == AGX_TASK_ARM_MANIPULATION ? T[AGX_T_DUP_ACT] : 0;
    const bool two = (X[AGX_X_FLAGS] & 512) != 0;     // a two-armed robot: the second chain, driven by the actions behind the first arm's
    const bool chain1 = !mobile && arm_chain_ok(hi, X + AGX_X_CHAIN, V->rs_narm, dup, T[AGX_T_EE_LINK]);
    const bool chain2 = two && arm_chain_ok(hi, X + AGX_X_CHAIN2, V->rs_narm, V->rs_narm, T[AGX_T_EE2_LINK]);
    if (!mobile && !chain1) can_sample = false;
    if (two && !(chain2 && T[AGX_T_TOOL2_BODY] > 0 && T[AGX_T_TOOL2_BODY] < hi[AGX_H_NFREE])) can_sample = false;
    // end-effector control (agx_ik.h) serves the same chains of 7 joints, on a fixed base, whose action columns lie inside the action row
    const bool has_reset = hi[AGX_H_OFF_TARGETS] - hi[AGX_H_OFF_RESET] >= AGX_X_COUNT || hi[AGX_H_NWORDS] - hi[AGX_H_OFF_RESET] >= AGX_X_COUNT;     // (as reset_flags below)
    if (has_reset && X[AGX_X_NARM] == 7 && V->rs_narm == 7 && hi[AGX_H_BASE_LINK] == 0 && chain1 && (!two || chain2) && dup >= 0 && 7 * (two ? 2 : 1) + dup <= hi[AGX_H_ACT_DIM])
      ee_arms = two ? 2 : 1;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(AGX_E_NOGPU, "agx_create: no HIP device (libagx has no CPU path)");
  if (device < 0 || device >= ndev) return fail(AGX_E_ARG, "agx_create: bad device index");
  HIPCHK(hipSetDevice(device));
  agx_handle h = new agx_handle_s();
  memset(h, 0, sizeof *h);
  h->can_sample = can_sample; h->ee_arms = ee_arms; h->V = V;
  const bool manifold = ((const float*)blob)[hi[AGX_H_OFF_PARAMS] + AGX_P_MANIFOLD] > 0.f;
  h->step_build = manifold ? V->build_mf : V->build;
  if (manifold && !V->build_mf) { delete h; return fail(AGX_E_LIMIT, "agx_create: AGX_P_MANIFOLD is set, but this kernel variant is compiled without the manifold stage (feeding, bed_bathing, scratch_itch, arm_manipulation have it)"); }
  h->settle = nullptr; h->settle_substeps = 0;
  h->reset_flags = (hi[AGX_H_OFF_TARGETS] - hi[AGX_H_OFF_RESET] >= AGX_X_COUNT || hi[AGX_H_NWORDS] - hi[AGX_H_OFF_RESET] >= AGX_X_COUNT) ? hi[hi[AGX_H_OFF_RESET] + AGX_X_FLAGS] : 0;
  const int rc = create_fill(h, blob, blob_bytes, n_envs, device);
  if (rc != AGX_OK) { const std::string keep = g_err; agx_destroy(h); g_err = keep; return rc; }   // every error exit releases what was allocated
  *out = h;
  return AGX_OK;
}

// the allocations of agx_create; on failure the caller destroys the partly filled handle
static int create_fill(agx_handle h, const void* blob, size_t blob_bytes, int n_envs, int device) {
  const int32_t* hi = (const int32_t*)blob; const agx_variant* V = h->V; const bool can_sample = h->can_sample;
  h->iter_word = hi[AGX_H_S_ENV] + AGX_E_ITERATION;
  h->ncoll = hi[AGX_H_NCOLL];
  h->device = device; h->L.n_envs = n_envs; h->L.act_dim = hi[AGX_H_ACT_DIM]; h->L.obs_dim = hi[AGX_H_OBS_DIM]; h->L.sw = hi[AGX_H_STATE_WORDS];
  HIPCHK(hipMalloc(&h->L.blob, blob_bytes));
  HIPCHK(hipMemcpy(h->L.blob, blob, blob_bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&h->L.state, (size_t)n_envs * h->L.sw * 4));
  HIPCHK(hipMemset(h->L.state, 0, (size_t)n_envs * h->L.sw * 4));
  HIPCHK(hipMalloc(&h->L.scratch, (size_t)n_envs * V->scr_words * 4));
  HIPCHK(hipMemset(h->L.scratch, 0, (size_t)n_envs * V->scr_words * 4));
  HIPCHK(hipMalloc(&h->L.overflow, 4));
  HIPCHK(hipMemset(h->L.overflow, 0, 4));
  h->collision_tries = can_sample ? hi[hi[AGX_H_OFF_RESET] + AGX_X_COLLISION_TRIES] : 0;
  HIPCHK(hipMalloc(&h->first_restart_dev, (size_t)n_envs * 4)); HIPCHK(hipMalloc(&h->L.chosen, (size_t)n_envs * 4)); HIPCHK(hipMalloc(&h->work_dev, (size_t)n_envs));
  h->frame_skip = (int)((const float*)blob)[hi[AGX_H_OFF_PARAMS] + AGX_P_FRAME_SKIP];
  h->sim_sub = hi[AGX_H_SIM_SUBSTEPS] > 1 ? hi[AGX_H_SIM_SUBSTEPS] : 1;
  if (hi[AGX_H_OFF_CLOTH]) {
    if (!V->cloth || !V->cloth_lds_bytes) return fail(AGX_E_LIMIT, "agx_create: the model has a cloth but the kernel variant of its task has no cloth kernel");
    const int32_t* cl = hi + hi[AGX_H_OFF_CLOTH];
    h->cloth_nn = cl[AGX_CL_NN];
    h->L.cloth_words = 6 * h->cloth_nn; h->L.report_words = AGX_CLOTH_REPORT_WORDS(h->cloth_nn) + AGX_CLOTH_SCRATCH_WORDS(h->cloth_nn);
    h->L.trace_words = h->frame_skip * h->sim_sub * (hi[AGX_H_NDOF] + hi[AGX_H_NFREE]) * 12;      // per substep: the frames of the moving links, then of the free bodies
    h->L.cloth_lds = V->cloth_lds_bytes(h->cloth_nn);          // agxc::lds_words of the variant's own cloth kernel
    h->particles = cl[AGX_CL_PARTICLES] != 0;
    if (cl[AGX_CL_PARTICLES]) {      // the water of the drinking scene (agx_water.h): one wavefront, lane = particle; report = one word per particle
      h->L.report_words = 64;
      if (h->cloth_nn > 64 || cl[AGX_CL_NSHAPE] > 192 || hi[AGX_H_NDOF] + hi[AGX_H_NHUMAN] + hi[AGX_H_NFREE] + 2 > 64 || hi[AGX_H_TASK_KIND] != AGX_TASK_DRINKING)
        return fail(AGX_E_LIMIT, "agx_create: particles exceed the limits of the water kernel");
    } else if (h->L.cloth_lds > 160 * 1024 || h->cloth_nn > 4096 || cl[AGX_CL_NCOLOR] - (AGX_CLOTH_THREADS / 64) * cl[AGX_CL_NPATCH_COLOR] > AGX_CLOTH_MAX_COLORS || cl[AGX_CL_NPATCH_COLOR] < 0 || cl[AGX_CL_MAX_LINKS_PER_COLOR] > 1024 ||
        cl[AGX_CL_NSHAPE] > 192 || hi[AGX_H_NDOF] + hi[AGX_H_NHUMAN] + 2 > 64 || cl[AGX_CL_NN] > 65535 || hi[AGX_H_NFREE] != 0) return fail(AGX_E_LIMIT, "agx_create: cloth exceeds the limits of the cloth kernel");
    HIPCHK(hipMalloc(&h->L.cloth, (size_t)n_envs * h->L.cloth_words * 4)); HIPCHK(hipMemset(h->L.cloth, 0, (size_t)n_envs * h->L.cloth_words * 4));
    HIPCHK(hipMalloc(&h->L.trace, (size_t)n_envs * h->L.trace_words * 4)); HIPCHK(hipMemset(h->L.trace, 0, (size_t)n_envs * h->L.trace_words * 4));
    HIPCHK(hipMalloc(&h->L.report, (size_t)n_envs * h->L.report_words * 4)); HIPCHK(hipMemset(h->L.report, 0, (size_t)n_envs * h->L.report_words * 4));
  }
  HIPCHK(hipMalloc(&h->L.episode, (size_t)n_envs * 4));
  HIPCHK(hipMemset(h->L.episode, 0, (size_t)n_envs * 4));
  HIPCHK(hipMalloc(&h->act_dev, (size_t)n_envs * h->L.act_dim * 4));
  HIPCHK(hipMalloc(&h->obs_dev, (size_t)n_envs * h->L.obs_dim * 4));
  HIPCHK(hipMalloc(&h->rew_dev, (size_t)n_envs * 4));
  HIPCHK(hipMalloc(&h->info_dev, (size_t)n_envs * AGX_INFO_DIM * 4));
  HIPCHK(hipMalloc(&h->done_dev, (size_t)n_envs));
  HIPCHK(hipEventCreate(&h->ev0)); HIPCHK(hipEventCreate(&h->ev1));
  for (int c = 0; c < 8; c++) for (int k = 0; k < 16; k++) HIPCHK(hipEventCreate(&h->kev[c][k]));
  {
    const char* e = getenv("AGX_CHUNKS");
    // default: 3 chunks for large batches (3 chunk streams + the caller's stream = the 4 hardware queues HIP uses
    // by default; measured 335 k -> 386 k env-steps/s at 4096 envs, 4 chunks need GPU_MAX_HW_QUEUES=8), 1 otherwise
    // (the drinking scenes run unchunked: 20 light build / solve pairs and one long water launch per step -- measured 295 k env-steps/s in one chunk
    // under the profiler against 244 k in three)
    int nc = e ? atoi(e) : (h->particles ? 1 : (n_envs >= 2048 ? 3 : 1)); if (nc < 1) nc = 1; if (nc > 8) nc = 8; if (n_envs < 64 * nc) nc = 1;
    h->n_chunks = nc;
    HIPCHK(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
    for (int k = 0; k < nc; k++) { HIPCHK(hipStreamCreateWithFlags(&h->cs[k], hipStreamNonBlocking)); HIPCHK(hipEventCreateWithFlags(&h->join_ev[k], hipEventDisableTiming)); }
  }
  HIPCHK(V->init());
  return AGX_OK;
}

void agx_destroy(agx_handle h) {
  if (!h) return;
  hipSetDevice(h->device);
  hipFree(h->L.scratch); hipFree(h->L.overflow); hipFree(h->first_restart_dev); hipFree(h->L.chosen); hipFree(h->work_dev); hipFree(h->L.blob); hipFree(h->L.state); hipFree(h->L.episode); hipFree(h->act_dev); hipFree(h->obs_dev);
  hipFree(h->rew_dev); hipFree(h->info_dev); hipFree(h->done_dev);
  if (h->L.cloth) { hipFree(h->L.cloth); hipFree(h->L.trace); hipFree(h->L.report); }
  if (h->cam) { hipFree(h->cam->frames); hipFree(h->cam->coll); hipFree(h->cam->planes); hipFree(h->cam->colours); hipFree(h->cam->tris); hipFree(h->cam->lend_depth); hipFree(h->cam->lend_seg); delete h->cam; }
  if (h->ev0) hipEventDestroy(h->ev0); if (h->ev1) hipEventDestroy(h->ev1);      // a handle whose creation failed half way holds nulls
  for (int c = 0; c < 8; c++) for (int k = 0; k < 16; k++) if (h->kev[c][k]) hipEventDestroy(h->kev[c][k]);
  if (h->fork_ev) hipEventDestroy(h->fork_ev);
  for (int k = 0; k < h->n_chunks; k++) { if (h->cs[k]) hipStreamDestroy(h->cs[k]); if (h->join_ev[k]) hipEventDestroy(h->join_ev[k]); }
  if (h->prox) { hipFree(h->prox->frames); hipFree(h->prox->pairs); hipFree(h->prox->cflags); delete h->prox; }
  delete h;
}

int agx_dims(agx_handle h, int* n_envs, int* act_dim, int* obs_dim, int* state_words) {
  if (!h) return fail(AGX_E_ARG, "agx_dims: null handle");
  if (n_envs) *n_envs = h->L.n_envs; if (act_dim) *act_dim = h->L.act_dim; if (obs_dim) *obs_dim = h->L.obs_dim; if (state_words) *state_words = h->L.sw;
  return AGX_OK;
}

int agx_set_state(agx_handle h, const float* host_states) {
  if (!h || !host_states) return fail(AGX_E_ARG, "agx_set_state: bad argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(h->L.state, host_states, (size_t)h->L.n_envs * h->L.sw * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(h->L.episode, 0, (size_t)h->L.n_envs * 4));
  forget_warm(h, nullptr, nullptr); HIPCHK(hipGetLastError()); HIPCHK(hipDeviceSynchronize());
  return AGX_OK;
}
int agx_get_state(agx_handle h, float* host_states) {
  if (!h || !host_states) return fail(AGX_E_ARG, "agx_get_state: bad argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(host_states, h->L.state, (size_t)h->L.n_envs * h->L.sw * 4, hipMemcpyDeviceToHost));
  return AGX_OK;
}
int agx_state_dev(agx_handle h, float** out_dev) { if (!h || !out_dev) return fail(AGX_E_ARG, "agx_state_dev: bad argument"); *out_dev = h->L.state; return AGX_OK; }

// what an env step reads and writes beyond the handle's own buffers (device pointers, [n_envs] rows each)
struct step_io { const float* act; float *obs, *rew; uint8_t* done; float* info; };
// agx_step_timed: the events of one launch_chunked, per chunk -- one before the first launch, one after every launch
struct launch_recorder { hipEvent_t (*ev)[16]; int n[8]; };
// The one launch sequence.  Fork the caller's stream into the chunk streams, run `n_substeps` p.stepSimulation() calls per chunk -- each
// sim_sub times [build, solve] -- and, for an env step (io given), the finish kernel; join back.  Work of one chunk is ordered; chunks are
// independent.  Without io it is a settle, and the solve kernel's phase says so.  dbg: debug records of the first substep, or null.
// active: per-env mask honoured by the build / solve / cloth launches (agx_reset's masked settle), null = every environment
static int launch_chunked(agx_handle h, int n_substeps, const step_io* io, float* dbg, const uint8_t* active, void* stream, launch_recorder* rec) {
  HIPCHK(hipSetDevice(h->device));
  const agx_launch& L = h->L; const agx_variant* V = h->V;
  hipStream_t user = (hipStream_t)stream;
  const int nc = h->n_chunks, per = (L.n_envs + nc - 1) / nc;
  HIPCHK(hipEventRecord(h->fork_ev, user));
  for (int c = 0; c < nc; c++) {
    const int e0 = c * per, ne = (e0 + per <= L.n_envs ? per : L.n_envs - e0);
    if (ne <= 0) continue;
    hipStream_t st = nc == 1 ? user : h->cs[c];
    if (nc > 1) HIPCHK(hipStreamWaitEvent(st, h->fork_ev, 0));
    auto mark = [&]() { return rec ? hipEventRecord(rec->ev[c][rec->n[c]++], st) : hipSuccess; };
    auto launched = [&]() { const hipError_t e = hipGetLastError(); return e != hipSuccess ? e : mark(); };
    HIPCHK(mark());
    // n_substeps counts p.stepSimulation() calls, each sim_sub internal substeps long.  With a cloth, the rigid substeps of up to frame_skip
    // calls run first (leaving their link frames in the trace), then one cloth launch replays them (one-way coupling, agx_cloth.h).
    for (int g0 = 0; g0 < n_substeps; g0 += h->frame_skip) {
      const int gs = n_substeps - g0 < h->frame_skip ? n_substeps - g0 : h->frame_skip, nsub = gs * h->sim_sub;
      for (int k = 0; k < nsub; k++) {
        const bool first = g0 == 0 && k == 0;
        h->step_build(L, st, e0, ne, first && io ? io->act : nullptr, first ? dbg : nullptr, active, k, true);
        HIPCHK(launched());
        V->solve(L, st, e0, ne, first ? dbg : nullptr, active, io ? k : (k | AGX_PHASE_SETTLE));
        HIPCHK(launched());
      }
      if (L.cloth) { V->cloth(L, st, e0, ne, nsub, active); HIPCHK(launched()); }
    }
    if (io) { V->finish(L, st, e0, ne, io->act, io->obs, io->rew, io->done, io->info); HIPCHK(launched()); }
    if (nc > 1) { HIPCHK(hipEventRecord(h->join_ev[c], st)); HIPCHK(hipStreamWaitEvent(user, h->join_ev[c], 0)); }
  }
  return AGX_OK;
}
int agx_settle(agx_handle h, int n_substeps, void* stream) {
  if (!h || n_substeps < 0) return fail(AGX_E_ARG, "agx_settle: bad argument");
  return launch_chunked(h, n_substeps, /*io*/ nullptr, /*dbg*/ nullptr, /*active*/ nullptr, stream, /*rec*/ nullptr);
}
int agx_settle_debug(agx_handle h, int n_substeps, float* dbg, void* stream) {
  if (!h || n_substeps < 1 || !dbg) return fail(AGX_E_ARG, "agx_settle_debug: bad argument");
  return launch_chunked(h, n_substeps, /*io*/ nullptr, dbg, /*active*/ nullptr, stream, /*rec*/ nullptr);
}
int agx_step(agx_handle h, const float* a, float* obs, float* rew, uint8_t* done, float* info, void* stream) {
  if (!h || !a || !obs || !rew || !done) return fail(AGX_E_ARG, "agx_step: bad argument");
  const step_io io = {a, obs, rew, done, info};
  return launch_chunked(h, h->frame_skip, &io, /*dbg*/ nullptr, /*active*/ nullptr, stream, /*rec*/ nullptr);
}
int agx_step_debug(agx_handle h, const float* a, float* obs, float* rew, uint8_t* done, float* info, float* dbg, void* stream) {
  if (!h || !a || !obs || !rew || !done || !dbg) return fail(AGX_E_ARG, "agx_step_debug: bad argument");
  const step_io io = {a, obs, rew, done, info};
  return launch_chunked(h, h->frame_skip, &io, dbg, /*active*/ nullptr, stream, /*rec*/ nullptr);
}
// agx_step with an event around every launch on its chunk stream: per chunk [build, solve] x frame_skip, then finish
int agx_step_timed(agx_handle h, const float* a, float* obs, float* rew, uint8_t* done, float* info, void* stream, float* ms3, int* launches3) {
  if (!h || !a || !obs || !rew || !done || !ms3) return fail(AGX_E_ARG, "agx_step_timed: bad argument");
  if (2 * h->frame_skip * h->sim_sub + 2 > 16 || h->L.cloth) return fail(AGX_E_LIMIT, "agx_step_timed: too many launches per step for the event table (frame_skip x substeps), or a model with a cloth");
  launch_recorder rec = {h->kev, {0, 0, 0, 0, 0, 0, 0, 0}};
  const step_io io = {a, obs, rew, done, info};
  const int rc = launch_chunked(h, h->frame_skip, &io, /*dbg*/ nullptr, /*active*/ nullptr, stream, &rec);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  ms3[0] = ms3[1] = ms3[2] = 0.f;
  int cnt[3] = {0, 0, 0};
  for (int c = 0; c < h->n_chunks; c++) for (int k = 0; k + 1 < rec.n[c]; k++) {
    float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, h->kev[c][k], h->kev[c][k + 1]));
    const int t = k == rec.n[c] - 2 ? 2 : (k & 1);
    ms3[t] += ms; cnt[t]++;
  }
  if (launches3) { launches3[0] = cnt[0]; launches3[1] = cnt[1]; launches3[2] = cnt[2]; }
  return AGX_OK;
}
int agx_chunk_count(agx_handle h, int* out) { if (!h || !out) return fail(AGX_E_ARG, "agx_chunk_count: bad argument"); *out = h->n_chunks; return AGX_OK; }
int agx_observe(agx_handle h, float* obs, void* stream) { return agx_observe_masked(h, obs, nullptr, stream); }
int agx_observe_masked(agx_handle h, float* obs, const uint8_t* mask_dev, void* stream) {
  if (!h || !obs) return fail(AGX_E_ARG, "agx_observe: bad argument");
  HIPCHK(hipSetDevice(h->device));
  h->V->observe(h->L, (hipStream_t)stream, obs, mask_dev);
  HIPCHK(hipGetLastError());
  return AGX_OK;
}
static int launch_sample(agx_handle h, uint64_t seed, const uint64_t* seeds_dev, const uint8_t* mask_dev, int impairment_mode, int gender_mode, float* ik_info_dev, void* stream) {
  if (impairment_mode < -2 || impairment_mode > 3 || gender_mode < -1 || gender_mode > 1) return fail(AGX_E_ARG, "reset: bad impairment / gender mode");
  if (!h->can_sample) return fail(AGX_E_LIMIT, "reset: no device-side reset generator for this model (FeedingJaco-type scenes with a serial 7-DoF arm only); "
                                               "provide post-reset states with agx_set_state / a pool for agx_reset_done");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  forget_warm(h, mask_dev, st);          // the sampled environments start without a warm-start memory
  agx_sample_args A = {(unsigned long long)seed, (const unsigned long long*)seeds_dev, impairment_mode, gender_mode, nullptr, 0, nullptr};
  if (h->reset_flags & 16) {
    // bed bathing (bed_bathing.py:119-137): the human is a rag doll dropped onto the bed -- the attached model samples its drop record from the
    // same seeds, settles for 100 simulation steps, and its state records tell this model's sampler where the human lies.
    // Arm manipulation (arm_manipulation.py:117-146; FLAGS bit 7): the attached model is the FALL model -- this blob at gravity -1, its
    // sampler writing the record the posed arm falls from -- and the rag-doll model is attached to that one: rag doll, then the fall, then here.
    agx_handle_s* hs = h->settle;
    if (!hs) return fail(AGX_E_ARG, "reset: this model's human comes out of a rag-doll settle; attach that model first (agx_attach_settle_model)");
    const bool two = (h->reset_flags & 128) && !(h->reset_flags & 256);
    if (two && !(hs->reset_flags & 256)) return fail(AGX_E_ARG, "reset: this model's reset lets the arm fall in a second handle (ModelBlob.fall_model()); attach that one, and the rag-doll model to it");
    agx_handle_s* hr = two ? hs->settle : hs;
    if (!hr) return fail(AGX_E_ARG, "reset: the fall model has no rag-doll model attached (agx_attach_settle_model)");
    hr->V->sample(hr->L, st, A, mask_dev, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    int rc = launch_chunked(hr, two ? hs->settle_substeps : h->settle_substeps, /*io*/ nullptr, /*dbg*/ nullptr, mask_dev, stream, /*rec*/ nullptr);
    if (rc) return rc;
    A.settled = hr->L.state; A.settled_sw = hr->L.sw;
    if (two) {
      forget_warm(hs, mask_dev, st);
      hs->V->sample(hs->L, st, A, mask_dev, nullptr, nullptr);
      HIPCHK(hipGetLastError());
      rc = launch_chunked(hs, h->settle_substeps, /*io*/ nullptr, /*dbg*/ nullptr, mask_dev, stream, /*rec*/ nullptr);
      if (rc) return rc;
      A.fell = hs->L.state;
    }
  }
  h->V->sample(h->L, st, A, mask_dev, ik_info_dev, nullptr);
  HIPCHK(hipGetLastError());
  // collision rejection (robot.py:105-112, env.py:299-308): the contacts of the sampled state come from the stepper's own build kernel;
  // a state whose arm / tool touches the human, the table or the wheelchair is re-sampled from the next IK restart.  Fixed schedule
  // of `collision_tries` rounds (no host round trip): the kernels of a round exit at once for the environments that are settled.
  for (int t = 0; t < h->collision_tries; t++) {
    const uint8_t* active = t == 0 ? mask_dev : h->work_dev;
    h->V->build(h->L, st, 0, h->L.n_envs, nullptr, nullptr, active, 0, false);      // the plain build kernel, no trace: a collision pass
    HIPCHK(hipGetLastError());
    h->V->verdict(h->L, st, active, h->work_dev, h->first_restart_dev);
    HIPCHK(hipGetLastError());
    h->V->sample(h->L, st, A, h->work_dev, ik_info_dev, h->first_restart_dev);
    HIPCHK(hipGetLastError());
  }
  if (h->L.cloth && h->particles) {       // the water goes into the sampled cup
    hipLaunchKernelGGL(agx_place_water_kernel, dim3(h->L.n_envs), dim3(64), 0, st, h->L.cloth, h->L.state, h->L.blob, mask_dev, h->L.n_envs, h->L.sw, h->L.cloth_words);
    HIPCHK(hipGetLastError());
  }
  if (h->L.cloth && !h->particles) {      // the garment goes where the sampled end effector is (dressing task words; the water has its own placement)
    hipLaunchKernelGGL(agx_place_cloth_kernel, dim3(h->L.n_envs), dim3(256), 0, st, h->L.cloth, h->L.state, h->L.blob, mask_dev, h->L.n_envs, h->L.sw, h->L.cloth_words);
    HIPCHK(hipGetLastError());
  }
  return AGX_OK;
}
int agx_attach_settle_model(agx_handle h, agx_handle settle, int n_substeps) {
  if (!h || n_substeps < 0) return fail(AGX_E_ARG, "agx_attach_settle_model: bad argument");
  if (!settle) { h->settle = nullptr; return AGX_OK; }
  if (!(h->reset_flags & 16)) return fail(AGX_E_ARG, "agx_attach_settle_model: this model's reset does not read a settle record");
  const bool wants_fall = (h->reset_flags & 128) && !(h->reset_flags & 256);      // arm manipulation: the fall model goes here, the rag doll behind it
  if (wants_fall ? !(settle->reset_flags & 256) : !(settle->reset_flags & 32)) return fail(AGX_E_ARG, wants_fall ? "agx_attach_settle_model: this model takes its fall model (the same blob with AGX_X_FLAGS bit 8)" : "agx_attach_settle_model: the second handle is not a rag-doll model with a drop sampler");
  if (!settle->can_sample) return fail(AGX_E_ARG, "agx_attach_settle_model: the second handle has no sampler");
  if (settle->L.n_envs != h->L.n_envs || settle->device != h->device) return fail(AGX_E_ARG, "agx_attach_settle_model: both handles must hold the same number of environments on the same device");
  h->settle = settle; h->settle_substeps = n_substeps;
  return AGX_OK;
}
int agx_sample_reset(agx_handle h, uint64_t seed, int impairment_mode, int gender_mode, float* ik_info_dev, void* stream) {
  if (!h) return fail(AGX_E_ARG, "agx_sample_reset: null handle");
  return launch_sample(h, seed, nullptr, nullptr, impairment_mode, gender_mode, ik_info_dev, stream);
}
int agx_reset(agx_handle h, const uint8_t* mask_dev, const uint64_t* seeds_dev, uint64_t seed, int impairment_mode, int gender_mode, int settle_substeps, void* stream) {
  if (!h || settle_substeps < 0) return fail(AGX_E_ARG, "agx_reset: bad argument");
  int rc = launch_sample(h, seed, seeds_dev, mask_dev, impairment_mode, gender_mode, nullptr, stream);
  if (rc) return rc;
  rc = launch_chunked(h, settle_substeps, /*io*/ nullptr, /*dbg*/ nullptr, mask_dev, stream, /*rec*/ nullptr);   // the settle substeps touch the masked environments only
  if (!rc && h->L.cloth && !h->particles) {
    hipLaunchKernelGGL(agx_cloth_gravity_kernel, dim3((h->L.n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->L.state, h->L.blob, mask_dev, h->L.n_envs, h->L.sw);
    HIPCHK(hipGetLastError());
  }
  return rc;
}
int agx_reset_done(agx_handle h, const float* pool_dev, int pool_n, const uint8_t* done_dev, void* stream) { return agx_reset_done_at(h, pool_dev, pool_n, done_dev, -1, stream); }
int agx_reset_done_at(agx_handle h, const float* pool_dev, int pool_n, const uint8_t* done_dev, int iteration, void* stream) {
  if (!h || !pool_dev || pool_n <= 0 || !done_dev) return fail(AGX_E_ARG, "agx_reset_done: bad argument");
  HIPCHK(hipSetDevice(h->device));
  if (h->L.cloth && !h->cloth_pool_dev) return fail(AGX_E_ARG, "agx_reset_done: the model has a cloth; give the garments of the pool with agx_set_cloth_pool first");
  hipLaunchKernelGGL(agx_reset_kernel, dim3(h->L.n_envs), dim3(64), 0, (hipStream_t)stream, h->L.state, pool_dev, pool_n, done_dev, h->L.episode, h->L.n_envs, h->L.sw, h->env_offset,
                     h->iter_word, iteration);
  forget_warm(h, done_dev, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  if (h->L.cloth) {
    hipLaunchKernelGGL(agx_reset_cloth_kernel, dim3(h->L.n_envs), dim3(256), 0, (hipStream_t)stream, h->L.cloth, h->cloth_pool_dev, pool_n, done_dev, h->L.episode, h->L.n_envs, h->L.cloth_words, h->env_offset);
    HIPCHK(hipGetLastError());
  }
  return AGX_OK;
}
// ---- garments of models with a cloth section: float[n_envs][2][NN][3], node positions then node velocities
int agx_cloth_nodes(agx_handle h, int* nodes) { if (!h || !nodes) return fail(AGX_E_ARG, "agx_cloth_nodes: bad argument"); *nodes = h->cloth_nn; return AGX_OK; }
int agx_set_cloth(agx_handle h, const float* host_cloth) {
  if (!h || !host_cloth || !h->L.cloth) return fail(AGX_E_ARG, "agx_set_cloth: bad argument or a model without a cloth");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(h->L.cloth, host_cloth, (size_t)h->L.n_envs * h->L.cloth_words * 4, hipMemcpyHostToDevice));
  return AGX_OK;
}
int agx_get_cloth(agx_handle h, float* host_cloth) {
  if (!h || !host_cloth || !h->L.cloth) return fail(AGX_E_ARG, "agx_get_cloth: bad argument or a model without a cloth");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(host_cloth, h->L.cloth, (size_t)h->L.n_envs * h->L.cloth_words * 4, hipMemcpyDeviceToHost));
  return AGX_OK;
}
int agx_cloth_dev(agx_handle h, float** out_dev) { if (!h || !out_dev || !h->L.cloth) return fail(AGX_E_ARG, "agx_cloth_dev: bad argument or a model without a cloth"); *out_dev = h->L.cloth; return AGX_OK; }
int agx_get_cloth_report(agx_handle h, float* host_report, int* words_per_env) {
  if (!h || !h->L.cloth || !h->L.report) return fail(AGX_E_ARG, "agx_get_cloth_report: bad argument or a model without a cloth");
  // a particle section's report is the water kernel's: one word per particle slot (agx_water.h REPORT_WORDS), the whole row
  const int words = h->particles ? h->L.report_words : AGX_CLOTH_REPORT_WORDS(h->cloth_nn);
  if (words_per_env) *words_per_env = words;
  if (!host_report) return AGX_OK;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy2D(host_report, (size_t)words * 4, h->L.report, (size_t)h->L.report_words * 4, (size_t)words * 4, (size_t)h->L.n_envs, hipMemcpyDeviceToHost));
  return AGX_OK;
}
int agx_set_cloth_pool(agx_handle h, const float* pool_cloth_dev) {
  if (!h || !h->L.cloth) return fail(AGX_E_ARG, "agx_set_cloth_pool: bad argument or a model without a cloth");
  h->cloth_pool_dev = pool_cloth_dev; return AGX_OK;
}

int agx_check_collisions(agx_handle h, uint8_t* flags_host, void* stream) {
  if (!h || !flags_host) return fail(AGX_E_ARG, "agx_check_collisions: bad argument");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  // the stepper's own collision pass on the states as they are (no motor targets, nothing is integrated: the states do not change)
  h->V->build(h->L, st, 0, h->L.n_envs, nullptr, nullptr, nullptr, 0, false);
  HIPCHK(hipGetLastError());
  h->V->collision_flags(h->L, st, h->work_dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(flags_host, h->work_dev, (size_t)h->L.n_envs, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return AGX_OK;
}

int agx_set_env_offset(agx_handle h, long long env_offset) {
  if (!h || env_offset < 0) return fail(AGX_E_ARG, "agx_set_env_offset: bad argument");
  h->env_offset = env_offset; return AGX_OK;
}
int agx_overflow_count(agx_handle h, int* out) {
  if (!h || !out) return fail(AGX_E_ARG, "agx_overflow_count: bad argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(out, h->L.overflow, 4, hipMemcpyDeviceToHost));
  return AGX_OK;
}
int agx_debug_layout(agx_handle h, int* out8) {
  if (!h || !out8) return fail(AGX_E_ARG, "agx_debug_layout: bad argument");
  const agx_variant* V = h->V;
  out8[0] = V->dbg_words; out8[1] = V->dbg_con; out8[2] = V->dbg_minv; out8[3] = V->max_dof; out8[4] = V->dbg_hdr; out8[5] = V->dbg_lam; out8[6] = V->dbg_time; out8[7] = V->dbg_qdd;
  return AGX_OK;
}
const char* agx_variant_name(agx_handle h) { return h ? h->V->name : ""; }

// ---- observation all-gather over RCCL: the only exchange the sharded path has -------------------------------
// RCCL is bound at run time (dlopen), so a process that never gathers does not need it; a library instance that is already
// loaded (e.g. the one PyTorch ships) is preferred so that the process ends up with ONE RCCL.
namespace {
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, const void*, int) = nullptr;   // ncclUniqueId is passed by value: 128 bytes, see call site
  int (*CommDestroy)(void*) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
struct agx_unique_id { char bytes[128]; };   // layout of ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128)
RcclApi g_rccl;
int rccl_load() {
  if (g_rccl.lib) return AGX_OK;
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  void* lib = nullptr;
  for (const char* n : names) if ((lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL))) break;   // already in the process?
  for (const char* n : names) { if (lib) break; lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); }
  if (!lib) return fail(AGX_E_HIP, "agx_allgather: librccl.so not found");
  g_rccl.GetUniqueId = (int (*)(void*))dlsym(lib, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, const void*, int))dlsym(lib, "ncclCommInitRank");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
  g_rccl.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(lib, "ncclAllGather");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.AllGather) return fail(AGX_E_HIP, "agx_allgather: RCCL symbols missing");
  g_rccl.lib = lib;
  return AGX_OK;
}
int rccl_fail(const char* what, int rc) {
  char buf[256]; snprintf(buf, sizeof buf, "%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error");
  return fail(AGX_E_HIP, buf);
}
}  // namespace

// [n_envs][obs_dim + 4] = observation | reward | done (0 / 1) | info[0] (total_force_on_human) | info[1] (task_success): what one consumer of the
// whole batch reads per step (learn.py:26,72: the sampler's obs, reward, done, info) as ONE record per environment -- one all-gather per step
__global__ void agx_pack_kernel(const float* __restrict__ obs, const float* __restrict__ rew, const uint8_t* __restrict__ done, const float* __restrict__ info,
                                float* __restrict__ out, int n, int od) {
  const int w = od + 4, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * w) return;
  const int e = i / w, c = i - e * w;
  out[i] = c < od ? obs[(size_t)e * od + c] : c == od ? rew[e] : c == od + 1 ? (done[e] ? 1.f : 0.f) : info[(size_t)e * AGX_INFO_DIM + (c - od - 2)];
}
int agx_pack_step(agx_handle h, const float* obs_dev, const float* reward_dev, const uint8_t* done_dev, const float* info_dev, float* packed_dev, void* stream) {
  if (!h || !obs_dev || !reward_dev || !done_dev || !info_dev || !packed_dev) return fail(AGX_E_ARG, "agx_pack_step: bad argument");
  HIPCHK(hipSetDevice(h->device));
  const int total = h->L.n_envs * (h->L.obs_dim + 4);
  hipLaunchKernelGGL(agx_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, obs_dev, reward_dev, done_dev, info_dev, packed_dev, h->L.n_envs, h->L.obs_dim);
  HIPCHK(hipGetLastError());
  return AGX_OK;
}

int agx_comm_unique_id(void* out128) {
  if (!out128) return fail(AGX_E_ARG, "agx_comm_unique_id: null");
  int rc = rccl_load(); if (rc) return rc;
  rc = g_rccl.GetUniqueId(out128);
  return rc ? rccl_fail("ncclGetUniqueId", rc) : AGX_OK;
}
int agx_comm_init_rank(int device, int rank, int world, const void* unique_id128, void** comm_out) {
  if (!unique_id128 || !comm_out || rank < 0 || rank >= world) return fail(AGX_E_ARG, "agx_comm_init_rank: bad argument");
  int rc = rccl_load(); if (rc) return rc;
  HIPCHK(hipSetDevice(device));
  // ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank): the id is a 128-byte struct passed by value
  typedef int (*init_fn)(void**, int, agx_unique_id, int);
  agx_unique_id id; memcpy(id.bytes, unique_id128, sizeof id.bytes);
  rc = ((init_fn)(void*)g_rccl.CommInitRank)(comm_out, world, id, rank);
  return rc ? rccl_fail("ncclCommInitRank", rc) : AGX_OK;
}
int agx_comm_destroy(void* comm) {
  if (!comm) return AGX_OK;
  int rc = rccl_load(); if (rc) return rc;
  rc = g_rccl.CommDestroy(comm);
  return rc ? rccl_fail("ncclCommDestroy", rc) : AGX_OK;
}
int agx_allgather(agx_handle h, const float* local_dev, float* gathered_dev, size_t floats_per_rank, void* comm, void* stream) {
  if (!h || !local_dev || !gathered_dev) return fail(AGX_E_ARG, "agx_allgather: bad argument");
  HIPCHK(hipSetDevice(h->device));
  if (!comm) {   // a single rank: the gathered batch is the local shard
    if (gathered_dev != local_dev) HIPCHK(hipMemcpyAsync(gathered_dev, local_dev, floats_per_rank * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AGX_OK;
  }
  int rc = rccl_load(); if (rc) return rc;
  rc = g_rccl.AllGather(local_dev, gathered_dev, floats_per_rank, 7 /* ncclFloat32 */, comm, (hipStream_t)stream);
  return rc ? rccl_fail("ncclAllGather", rc) : AGX_OK;
}

// ---- end-effector control (csrc/agx_ik.h, csrc/agx_ik.hip): every check before any launch
int agx_ee_arms(agx_handle h, int* arms) {
  if (!h || !arms) return fail(AGX_E_ARG, "agx_ee_arms: bad argument");
  *arms = h->ee_arms; return AGX_OK;
}
int agx_ee_pose(agx_handle h, float* pose_dev, void* stream) {
  if (!h || !pose_dev) return fail(AGX_E_ARG, "agx_ee_pose: bad argument");
  if (h->ee_arms == 0) return fail(AGX_E_ARG, "agx_ee_pose: this model has no arm chain on a fixed base (agx_ee_arms is 0: a robot on wheels, or a chain the IK is not compiled for)");
  HIPCHK(hipSetDevice(h->device));
  agx_launch_ee_pose((hipStream_t)stream, h->L.blob, h->L.state, h->L.sw, h->L.n_envs, h->ee_arms, pose_dev);
  HIPCHK(hipGetLastError());
  return AGX_OK;
}
int agx_ee_ik(agx_handle h, const float* target_dev, int target_stride, int frame, int iters, float damping, float gain,
              float* q_out_dev, float* action_dev, int action_stride, float* err_dev, void* stream) {
  if (!h) return fail(AGX_E_ARG, "agx_ee_ik: null handle");
  if (!target_dev) return fail(AGX_E_ARG, "agx_ee_ik: null target");
  if (h->ee_arms == 0) return fail(AGX_E_ARG, "agx_ee_ik: this model has no arm chain on a fixed base (agx_ee_arms is 0: a robot on wheels, or a chain the IK is not compiled for)");
  if (frame != AGX_EE_ABSOLUTE && frame != AGX_EE_DELTA) return fail(AGX_E_ARG, "agx_ee_ik: unknown frame (AGX_EE_ABSOLUTE, AGX_EE_DELTA)");
  if (iters < 1 || iters > 1000) return fail(AGX_E_ARG, "agx_ee_ik: iters outside 1..1000");
  if (!(damping > 0.f)) return fail(AGX_E_ARG, "agx_ee_ik: damping must be positive");
  if (target_stride < h->ee_arms * (frame == AGX_EE_DELTA ? 6 : 7)) return fail(AGX_E_ARG, "agx_ee_ik: target_stride is smaller than arms x 7 (absolute) / arms x 6 (delta) floats");
  if (action_dev && action_stride < h->L.act_dim) return fail(AGX_E_ARG, "agx_ee_ik: action_stride is smaller than the action dimension");
  HIPCHK(hipSetDevice(h->device));
  agx_launch_ee_ik((hipStream_t)stream, h->L.blob, h->L.state, h->L.sw, h->L.n_envs, h->ee_arms, target_dev, target_stride, frame, iters, damping, gain,
                   q_out_dev, action_dev, action_stride, err_dev);
  HIPCHK(hipGetLastError());
  return AGX_OK;
}

// ---- the camera (csrc/agx_render.hip, csrc/agx_hull.h): every check before any launch
int agx_camera_colours(float* out36) {
  if (!out36) return fail(AGX_E_ARG, "agx_camera_colours: null");
  memcpy(out36, AGX_COLOURS, sizeof AGX_COLOURS);
  return AGX_OK;
}
int agx_collider_count(agx_handle h, int* ncoll) {
  if (!h || !ncoll) return fail(AGX_E_ARG, "agx_collider_count: bad argument");
  *ncoll = h->ncoll; return AGX_OK;
}
int agx_collider_frames(agx_handle h, int env0, int count, float* frames_dev, void* stream) {
  if (!h) return fail(AGX_E_ARG, "agx_collider_frames: null handle");
  if (!frames_dev) return fail(AGX_E_ARG, "agx_collider_frames: null output");
  if (env0 < 0 || count < 1 || count > h->L.n_envs || env0 > h->L.n_envs - count) return fail(AGX_E_ARG, "agx_collider_frames: [env0, env0 + count) is not a range of the handle's environments");
  HIPCHK(hipSetDevice(h->device));
  h->V->collider_frames(h->L, (hipStream_t)stream, env0, count, frames_dev);
  HIPCHK(hipGetLastError());
  return AGX_OK;
}
// the model blob as the device holds it
static int download_blob(agx_handle h, std::vector<uint32_t>& words) {
  int32_t hdr[AGX_H_COUNT];
  HIPCHK(hipMemcpy(hdr, h->L.blob, sizeof hdr, hipMemcpyDeviceToHost));
  words.resize((size_t)hdr[AGX_H_NWORDS]);
  HIPCHK(hipMemcpy(words.data(), h->L.blob, words.size() * 4, hipMemcpyDeviceToHost));
  return AGX_OK;
}
// the genders whose environments a collider is part of (bit 0 male, bit 1 female).  A human collider belongs to one gender only where the pair
// table says so: the B range of a group that has a female alternative is the male human's, the alternative the female's; a group that exists
// for one gender only (flag bits 3, 4) names that gender's human colliders
static std::vector<int> collider_genders(const int32_t* bi) {
  const int ncoll = bi[AGX_H_NCOLL];
  std::vector<int> genders((size_t)ncoll, 3);
  for (int g = 0; g < bi[AGX_H_NGROUP]; g++) {
    const int32_t* G = bi + bi[AGX_H_OFF_GROUP] + g * AGX_G_STRIDE;
    auto only = [&](int c0, int c1, int bits) { for (int c = c0 < 0 ? 0 : c0; c < c1 && c < ncoll; c++) if (bi[bi[AGX_H_OFF_COLL] + c * AGX_C_STRIDE + AGX_C_TAG] == AGX_TAG_HUMAN) genders[c] &= bits; };
    if (G[AGX_G_B0F] >= 0) { only(G[AGX_G_B0], G[AGX_G_B1], 1); only(G[AGX_G_B0F], G[AGX_G_B1F], 2); }
    for (int s = 0; s < 2; s++) if (G[AGX_G_FLAGS] & (8 << s)) { only(G[AGX_G_A0], G[AGX_G_A1], 1 << s); only(G[AGX_G_B0], G[AGX_G_B1], 1 << s); }
  }
  return genders;
}
// the tables of a handle's first camera: per collider the face planes of its hull (none for a sphere or a capsule), the genders that see it and
// its bounding radius; the frame table
static int camera_build(agx_handle h) {
  std::vector<uint32_t> words;
  { const int rc = download_blob(h, words); if (rc) return rc; }
  const int32_t* bi = (const int32_t*)words.data(); const float* bf = (const float*)words.data();
  const int ncoll = bi[AGX_H_NCOLL];
  const int npart = h->particles ? h->cloth_nn : 0;
  if (ncoll + npart > AGX_RENDER_LIST) return fail(AGX_E_LIMIT, "agx_camera_set: more than 1,024 colliders and particles");
  std::vector<agx_render_coll> coll((size_t)ncoll);
  std::vector<float4> planes;
  const std::vector<int> genders = collider_genders(bi);
  for (int c = 0; c < ncoll; c++) coll[c].genders = genders[c];
  std::vector<agxhull::Plane> pl;
  for (int c = 0; c < ncoll; c++) {
    const int32_t* Ci = bi + bi[AGX_H_OFF_COLL] + c * AGX_C_STRIDE; const float* Cf = (const float*)Ci;
    const int nv = Ci[AGX_C_NVERT]; const float* V = bf + bi[AGX_H_OFF_VERT] + 3 * Ci[AGX_C_VOFF];
    const double centre[3] = {Cf[AGX_C_AABB_C], Cf[AGX_C_AABB_C + 1], Cf[AGX_C_AABB_C + 2]}, rad = Cf[AGX_C_RADIUS];
    coll[c].plane0 = (int)planes.size(); coll[c].nplane = 0;
    double bound = 0;
    if (nv <= 2) {
      for (int k = 0; k < nv; k++) { double d = 0; for (int a = 0; a < 3; a++) d += (V[3 * k + a] - centre[a]) * (V[3 * k + a] - centre[a]); if (sqrt(d) > bound) bound = sqrt(d); }
      bound += rad;
    } else {
      agxhull::hull_planes(V, nv, pl);
      coll[c].nplane = (int)pl.size();
      for (const agxhull::Plane& p : pl) planes.push_back(make_float4((float)p.n[0], (float)p.n[1], (float)p.n[2], (float)(p.off + rad - (p.n[0] * centre[0] + p.n[1] * centre[1] + p.n[2] * centre[2]))));
      bound = agxhull::grown_bound(pl, rad, centre);
    }
    coll[c].bound = bound < 1e30 ? (float)(bound * (1.0 + 1e-6)) : 1e30f;
  }
  agx_camera_s* cam = new agx_camera_s();
  memset(cam, 0, sizeof *cam);
  h->cam = cam;      // from here on agx_destroy releases it
  cam->ncoll = ncoll;
  HIPCHK(hipMalloc(&cam->frames, (size_t)h->L.n_envs * (ncoll > 0 ? ncoll : 1) * 12 * 4));
  HIPCHK(hipMalloc(&cam->coll, (coll.size() ? coll.size() : 1) * sizeof(agx_render_coll)));
  HIPCHK(hipMalloc(&cam->planes, (planes.size() ? planes.size() : 1) * sizeof(float4)));
  HIPCHK(hipMalloc(&cam->colours, sizeof AGX_COLOURS + sizeof AGX_GARMENT_COLOUR));
  if (coll.size()) HIPCHK(hipMemcpy(cam->coll, coll.data(), coll.size() * sizeof(agx_render_coll), hipMemcpyHostToDevice));
  if (planes.size()) HIPCHK(hipMemcpy(cam->planes, planes.data(), planes.size() * sizeof(float4), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(cam->colours, AGX_COLOURS, sizeof AGX_COLOURS, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(cam->colours + 3 * AGX_COLOUR_GARMENT, AGX_GARMENT_COLOUR, sizeof AGX_GARMENT_COLOUR, hipMemcpyHostToDevice));
  agx_render_args& A = cam->A;
  A.blob = h->L.blob; A.state = h->L.state; A.sw = h->L.sw; A.frames = cam->frames; A.coll = cam->coll; A.planes = cam->planes; A.colours = cam->colours;
  if (npart) {
    const int oc = bi[AGX_H_OFF_CLOTH];
    A.water = h->L.cloth; A.cloth_words = h->L.cloth_words; A.npart = npart; A.part_radius = bf[oc + bi[oc + AGX_CL_OFF_PARAM] + AGX_CP_MARGIN];
  }
  return AGX_OK;
}
int agx_camera_set(agx_handle h, const float* eye3, const float* target3, const float* up3, float fov_deg, int width, int height, float near_plane, float far_plane) {
  if (!h) return fail(AGX_E_ARG, "agx_camera_set: null handle");
  if (!eye3 || !target3 || !up3) return fail(AGX_E_ARG, "agx_camera_set: null eye, target or up vector");
  for (int k = 0; k < 3; k++) if (!isfinite(eye3[k]) || !isfinite(target3[k]) || !isfinite(up3[k])) return fail(AGX_E_ARG, "agx_camera_set: a view vector is not finite");
  if (!(fov_deg > 0.f && fov_deg < 180.f)) return fail(AGX_E_ARG, "agx_camera_set: fov outside (0, 180) degrees");
  if (width < 1 || width > 8192 || height < 1 || height > 8192) return fail(AGX_E_ARG, "agx_camera_set: width or height outside 1..8192");
  if (!(near_plane > 0.f) || !(far_plane > near_plane) || !isfinite(far_plane)) return fail(AGX_E_ARG, "agx_camera_set: near and far must satisfy 0 < near < far");
  // p.computeViewMatrix: f = unit(target - eye), s = unit(f x up), u = s x f
  double f[3], s[3], u[3], l = 0;
  for (int k = 0; k < 3; k++) { f[k] = (double)target3[k] - (double)eye3[k]; l += f[k] * f[k]; }
  if (!(l > 0)) return fail(AGX_E_ARG, "agx_camera_set: eye and target are the same point");
  for (int k = 0; k < 3; k++) f[k] /= sqrt(l);
  s[0] = f[1] * up3[2] - f[2] * up3[1]; s[1] = f[2] * up3[0] - f[0] * up3[2]; s[2] = f[0] * up3[1] - f[1] * up3[0];
  l = s[0] * s[0] + s[1] * s[1] + s[2] * s[2];
  if (!(l > 1e-24)) return fail(AGX_E_ARG, "agx_camera_set: the up vector lies along the view direction");
  for (int k = 0; k < 3; k++) s[k] /= sqrt(l);
  u[0] = s[1] * f[2] - s[2] * f[1]; u[1] = s[2] * f[0] - s[0] * f[2]; u[2] = s[0] * f[1] - s[1] * f[0];
  HIPCHK(hipSetDevice(h->device));
  if (!h->cam) { const int rc = camera_build(h); if (rc) return rc; }
  agx_render_args& A = h->cam->A;
  for (int k = 0; k < 3; k++) { A.eye[k] = eye3[k]; A.right[k] = (float)s[k]; A.up[k] = (float)u[k]; A.fwd[k] = (float)f[k]; }
  A.ty = (float)tan(0.5 * (double)fov_deg * M_PI / 180.0); A.tx = (float)((double)width / (double)height * tan(0.5 * (double)fov_deg * M_PI / 180.0));
  A.width = width; A.height = height; A.near = near_plane; A.far = far_plane;
  return AGX_OK;
}
int agx_render(agx_handle h, int env0, int count, const float* light3, float ambient, float diffuse, float* depth_dev, int32_t* seg_dev, uint8_t* rgba_dev, void* stream) {
  if (!h) return fail(AGX_E_ARG, "agx_render: null handle");
  if (!h->cam || h->cam->A.width == 0) return fail(AGX_E_ARG, "agx_render: no camera; call agx_camera_set first");
  if (env0 < 0 || count < 1 || count > h->L.n_envs || env0 > h->L.n_envs - count) return fail(AGX_E_ARG, "agx_render: [env0, env0 + count) is not a range of the handle's environments");
  if (count > 65535) return fail(AGX_E_ARG, "agx_render: more than 65535 environments in one call");
  if (!light3) return fail(AGX_E_ARG, "agx_render: null light vector");
  double l = 0; for (int k = 0; k < 3; k++) l += (double)light3[k] * (double)light3[k];
  if (!isfinite(l) || !(l > 0)) return fail(AGX_E_ARG, "agx_render: the light vector is zero or not finite");
  if (!isfinite(ambient) || !isfinite(diffuse)) return fail(AGX_E_ARG, "agx_render: ambient or diffuse is not finite");
  if (!depth_dev && !seg_dev && !rgba_dev) return fail(AGX_E_ARG, "agx_render: all three outputs are null");
  if ((uintptr_t)rgba_dev & 3) return fail(AGX_E_ARG, "agx_render: rgba_dev is not 4-byte aligned");
  HIPCHK(hipSetDevice(h->device));
  agx_camera_s* cam = h->cam;
  if (cam->garment && (!depth_dev || !seg_dev)) {      // the garment kernel takes up a pixel's depth and segmentation value from the images
    const size_t need = (size_t)count * cam->A.width * cam->A.height;
    if (need > cam->lend_pixels) {      // (hipFree waits for the launches that still use the old buffers)
      hipFree(cam->lend_depth); hipFree(cam->lend_seg); cam->lend_depth = nullptr; cam->lend_seg = nullptr; cam->lend_pixels = 0;
      HIPCHK(hipMalloc(&cam->lend_depth, need * sizeof(float))); HIPCHK(hipMalloc(&cam->lend_seg, need * sizeof(int)));
      cam->lend_pixels = need;
    }
  }
  h->V->collider_frames(h->L, (hipStream_t)stream, env0, count, cam->frames + (size_t)env0 * cam->ncoll * 12);
  HIPCHK(hipGetLastError());
  agx_render_args A = cam->A;
  for (int k = 0; k < 3; k++) A.light[k] = (float)((double)light3[k] / sqrt(l));
  A.ambient = ambient; A.diffuse = diffuse; A.env0 = env0;
  A.depth = depth_dev; A.seg = seg_dev; A.rgba = (uint32_t*)rgba_dev;
  if (cam->garment) { if (!A.depth) A.depth = cam->lend_depth; if (!A.seg) A.seg = cam->lend_seg; }
  agx_launch_render((hipStream_t)stream, A, count, cam->garment);
  HIPCHK(hipGetLastError());
  return AGX_OK;
}
// ---- the garment of a dressing scene in the camera's images (csrc/agx_garment.h, the garment kernel of csrc/agx_render.hip)
int agx_camera_garment_colour(float* out3) {
  if (!out3) return fail(AGX_E_ARG, "agx_camera_garment_colour: null");
  memcpy(out3, AGX_GARMENT_COLOUR, sizeof AGX_GARMENT_COLOUR);
  return AGX_OK;
}
// the triangle table of the handle's model, from the blob as the device holds it; empty for a model without a garment
static int garment_table(agx_handle h, const char* who, std::vector<int>& tris) {
  tris.clear();
  if (!h->L.cloth || h->particles) return AGX_OK;
  HIPCHK(hipSetDevice(h->device));
  int32_t hdr[AGX_H_COUNT];
  HIPCHK(hipMemcpy(hdr, h->L.blob, sizeof hdr, hipMemcpyDeviceToHost));
  std::vector<int32_t> words((size_t)hdr[AGX_H_NWORDS]);
  HIPCHK(hipMemcpy(words.data(), h->L.blob, words.size() * 4, hipMemcpyDeviceToHost));
  const char* what = "";
  if (agxgarment::garment_faces(words.data(), words.size(), tris, &what) != 0 || (words[words[AGX_H_OFF_CLOTH] + AGX_CL_NN] != h->cloth_nn))
    return fail(AGX_E_BLOB, (std::string(who) + ": malformed cloth section: " + what).c_str());
  return AGX_OK;
}
int agx_garment_faces(agx_handle h, int* count, int* host_tris) {
  if (!h) return fail(AGX_E_ARG, "agx_garment_faces: null handle");
  if (!count) return fail(AGX_E_ARG, "agx_garment_faces: null count");
  std::vector<int> tris;
  const int rc = garment_table(h, "agx_garment_faces", tris); if (rc) return rc;
  *count = (int)(tris.size() / 3);
  if (host_tris && !tris.empty()) memcpy(host_tris, tris.data(), tris.size() * sizeof(int));
  return AGX_OK;
}
int agx_camera_garment(agx_handle h, int on) {
  if (!h) return fail(AGX_E_ARG, "agx_camera_garment: null handle");
  if (on && (!h->L.cloth || h->particles)) return fail(AGX_E_ARG, "agx_camera_garment: this model has no garment (no cloth section, or the water particles of a drinking scene)");
  if (!h->cam || h->cam->A.width == 0) return fail(AGX_E_ARG, "agx_camera_garment: no camera; call agx_camera_set first");
  agx_camera_s* cam = h->cam;
  if (on && !cam->tris) {      // the first enabling call: the table, as one 16-byte entry per face
    std::vector<int> tris;
    const int rc = garment_table(h, "agx_camera_garment", tris); if (rc) return rc;
    const size_t n = tris.size() / 3;
    std::vector<int4> packed(n);
    for (size_t f = 0; f < n; f++) packed[f] = make_int4(tris[3 * f], tris[3 * f + 1], tris[3 * f + 2], 0);
    int4* dev = nullptr;
    HIPCHK(hipMalloc(&dev, (n ? n : 1) * sizeof(int4)));
    if (n && hipMemcpy(dev, packed.data(), n * sizeof(int4), hipMemcpyHostToDevice) != hipSuccess) { hipFree(dev); return fail(AGX_E_HIP, "agx_camera_garment: upload of the triangle table"); }
    cam->tris = dev; cam->ntri = (int)n;
    cam->A.tris = dev; cam->A.ntri = (int)n; cam->A.garment = h->L.cloth; cam->A.cloth_words = h->L.cloth_words;
  }
  cam->garment = on != 0;
  return AGX_OK;
}

// ---- closest points between collider pairs (csrc/agx_proximity.h, csrc/agx_proximity.hip): every check before any launch
int agx_proximity_set(agx_handle h, const int32_t* pairs_host, int npairs, int nqueries) {
  if (!h) return fail(AGX_E_ARG, "agx_proximity_set: null handle");
  if (!pairs_host) return fail(AGX_E_ARG, "agx_proximity_set: null pair list");
  if (npairs < 1) return fail(AGX_E_ARG, "agx_proximity_set: npairs must be at least 1");
  if (nqueries < 1 || nqueries > AGX_PROX_MAX_QUERIES) return fail(AGX_E_ARG, "agx_proximity_set: nqueries outside 1..16");
  if (npairs > AGX_PROX_MAX_PAIRS) return fail(AGX_E_LIMIT, "agx_proximity_set: more than 8,192 pairs");
  std::vector<int> packed((size_t)npairs * 4);
  for (int k = 0; k < npairs; k++) {
    const int a = pairs_host[3 * k], b = pairs_host[3 * k + 1], q = pairs_host[3 * k + 2];
    if (a < 0 || a >= h->ncoll || b < 0 || b >= h->ncoll) return fail(AGX_E_ARG, "agx_proximity_set: a collider index outside [0, ncoll)");
    if (a == b) return fail(AGX_E_ARG, "agx_proximity_set: a pair of a collider with itself");
    if (q < 0 || q >= nqueries) return fail(AGX_E_ARG, "agx_proximity_set: a query id outside [0, nqueries)");
    packed[4 * k] = a; packed[4 * k + 1] = b; packed[4 * k + 2] = q; packed[4 * k + 3] = 0;
  }
  HIPCHK(hipSetDevice(h->device));
  if (!h->prox) {      // first use: the per-collider flags and the frame table
    std::vector<uint32_t> words;
    { const int rc = download_blob(h, words); if (rc) return rc; }
    const int32_t* bi = (const int32_t*)words.data(); const float* bf = (const float*)words.data();
    const int ncoll = bi[AGX_H_NCOLL];
    std::vector<int> flags = collider_genders(bi);
    for (int c = 0; c < ncoll; c++) {
      const int32_t* Ci = bi + bi[AGX_H_OFF_COLL] + c * AGX_C_STRIDE; const float* Cf = (const float*)Ci;
      bool fin = isfinite(Cf[AGX_C_RADIUS]);
      for (int k = 0; k < 6; k++) fin = fin && isfinite(Cf[AGX_C_AABB_C + k]);
      const float* V = bf + bi[AGX_H_OFF_VERT] + 3 * Ci[AGX_C_VOFF];
      for (int k = 0; k < 3 * Ci[AGX_C_NVERT]; k++) fin = fin && isfinite(V[k]);
      if (fin && Ci[AGX_C_NVERT] >= 1) flags[c] |= AGX_PROX_FINITE;
    }
    agx_prox_s* P = new agx_prox_s();
    memset(P, 0, sizeof *P);
    h->prox = P;      // from here on agx_destroy releases it
    P->ncoll = ncoll;
    HIPCHK(hipMalloc(&P->frames, (size_t)h->L.n_envs * (ncoll > 0 ? ncoll : 1) * 12 * 4));
    HIPCHK(hipMalloc(&P->cflags, (size_t)(ncoll > 0 ? ncoll : 1) * 4));
    if (ncoll) HIPCHK(hipMemcpy(P->cflags, flags.data(), (size_t)ncoll * 4, hipMemcpyHostToDevice));
    P->A.blob = h->L.blob; P->A.state = h->L.state; P->A.sw = h->L.sw; P->A.frames = P->frames; P->A.cflags = P->cflags;
  }
  agx_prox_s* P = h->prox;
  if (npairs > P->pairs_cap) {      // (hipFree waits for the launches that still read the old list)
    hipFree(P->pairs); P->pairs = nullptr; P->pairs_cap = 0; P->A.npairs = 0;
    HIPCHK(hipMalloc(&P->pairs, (size_t)npairs * 16));
    P->pairs_cap = npairs;
  } else HIPCHK(hipDeviceSynchronize());      // a later call replaces the list: no launch may still read it
  HIPCHK(hipMemcpy(P->pairs, packed.data(), (size_t)npairs * 16, hipMemcpyHostToDevice));
  int G = 1; while (G < AGX_WAVE && (G < npairs || G < nqueries)) G <<= 1;
  P->A.pairs = P->pairs; P->A.npairs = npairs; P->A.nqueries = nqueries; P->A.group = G;
  return AGX_OK;
}
int agx_proximity_pairs(agx_handle h, int* npairs, int* nqueries) {
  if (!h) return fail(AGX_E_ARG, "agx_proximity_pairs: null handle");
  if (npairs) *npairs = h->prox ? h->prox->A.npairs : 0;
  if (nqueries) *nqueries = h->prox && h->prox->A.npairs ? h->prox->A.nqueries : 0;
  return AGX_OK;
}
int agx_proximity(agx_handle h, int env0, int count, float max_distance, float* records_dev, float* nearest_dev, void* stream) {
  if (!h) return fail(AGX_E_ARG, "agx_proximity: null handle");
  if (!h->prox || h->prox->A.npairs == 0) return fail(AGX_E_ARG, "agx_proximity: no pair list; call agx_proximity_set first");
  if (env0 < 0 || count < 1 || count > h->L.n_envs || env0 > h->L.n_envs - count) return fail(AGX_E_ARG, "agx_proximity: [env0, env0 + count) is not a range of the handle's environments");
  if (!isfinite(max_distance) || max_distance < 0.f) return fail(AGX_E_ARG, "agx_proximity: max_distance is negative or not finite");
  if (!records_dev && !nearest_dev) return fail(AGX_E_ARG, "agx_proximity: both outputs are null");
  if (((uintptr_t)records_dev | (uintptr_t)nearest_dev) & 15) return fail(AGX_E_ARG, "agx_proximity: an output is not 16-byte aligned");
  HIPCHK(hipSetDevice(h->device));
  agx_prox_s* P = h->prox;
  h->V->collider_frames(h->L, (hipStream_t)stream, env0, count, P->frames + (size_t)env0 * P->ncoll * 12);      // stage A, into the query's own table
  HIPCHK(hipGetLastError());
  agx_prox_args A = P->A;
  A.env0 = env0; A.count = count; A.max_distance = max_distance; A.records = records_dev; A.nearest = nearest_dev;
  agx_launch_proximity((hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return AGX_OK;
}

int agx_step_host(agx_handle h, const float* a, float* obs, float* rew, uint8_t* done, float* info) {
  if (!h || !a || !obs || !rew || !done) return fail(AGX_E_ARG, "agx_step_host: bad argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpy(h->act_dev, a, (size_t)h->L.n_envs * h->L.act_dim * 4, hipMemcpyHostToDevice));
  const step_io io = {h->act_dev, h->obs_dev, h->rew_dev, h->done_dev, h->info_dev};
  int rc = launch_chunked(h, h->frame_skip, &io, /*dbg*/ nullptr, /*active*/ nullptr, /*stream*/ nullptr, /*rec*/ nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpy(obs, h->obs_dev, (size_t)h->L.n_envs * h->L.obs_dim * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rew, h->rew_dev, (size_t)h->L.n_envs * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(done, h->done_dev, (size_t)h->L.n_envs, hipMemcpyDeviceToHost));
  if (info) HIPCHK(hipMemcpy(info, h->info_dev, (size_t)h->L.n_envs * AGX_INFO_DIM * 4, hipMemcpyDeviceToHost));
  return AGX_OK;
}
int agx_observe_host(agx_handle h, float* obs) {
  if (!h || !obs) return fail(AGX_E_ARG, "agx_observe_host: bad argument");
  int rc = agx_observe(h, h->obs_dev, nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpy(obs, h->obs_dev, (size_t)h->L.n_envs * h->L.obs_dim * 4, hipMemcpyDeviceToHost));
  return AGX_OK;
}

int agx_profile_begin(agx_handle h, void* stream) { if (!h) return fail(AGX_E_ARG, "agx_profile_begin: null handle"); HIPCHK(hipSetDevice(h->device)); HIPCHK(hipEventRecord(h->ev0, (hipStream_t)stream)); return AGX_OK; }
int agx_profile_end(agx_handle h, void* stream, float* ms) {
  if (!h || !ms) return fail(AGX_E_ARG, "agx_profile_end: bad argument");
  HIPCHK(hipSetDevice(h->device)); HIPCHK(hipEventRecord(h->ev1, (hipStream_t)stream)); HIPCHK(hipEventSynchronize(h->ev1));
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return AGX_OK;
}
int agx_synchronize(agx_handle h, void* stream) { if (!h) return fail(AGX_E_ARG, "agx_synchronize: null handle"); HIPCHK(hipSetDevice(h->device)); HIPCHK(hipStreamSynchronize((hipStream_t)stream)); return AGX_OK; }

int agx_selftest(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(AGX_E_NOGPU, "agx_selftest: no HIP device");
  HIPCHK(hipSetDevice(device));
  float* of; int* oi; unsigned long long* om;
  HIPCHK(hipMalloc(&of, 320 * 4)); HIPCHK(hipMalloc(&oi, 192 * 4)); HIPCHK(hipMalloc(&om, 64 * 8));
  hipLaunchKernelGGL(agx_selftest_kernel, dim3(1), dim3(64), 0, 0, of, oi, om);
  HIPCHK(hipGetLastError()); HIPCHK(hipDeviceSynchronize());
  std::vector<float> f(320); std::vector<int> i(192); std::vector<unsigned long long> m(64);
  HIPCHK(hipMemcpy(f.data(), of, 320 * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(i.data(), oi, 192 * 4, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(m.data(), om, 64 * 8, hipMemcpyDeviceToHost));
  hipFree(of); hipFree(oi); hipFree(om);
  float x[64]; double sum = 0; float mn = 1e30f, mx = -1e30f; int isum = 0; unsigned long long bm = 0;
  for (int l = 0; l < 64; l++) { x[l] = (float)(l * l % 17) * 0.25f - 1.0f; sum += x[l]; float y = x[l] + (float)((l * 7) % 5); if (y < mn) mn = y; if (x[l] > mx) mx = x[l]; isum += l % 7; if (l % 3 == 1) bm |= 1ull << l; }
  int bad = 0, scan = 0;
  for (int l = 0; l < 64; l++) {
    if (fabs(f[l] - (float)sum) > 1e-4f) bad |= 1;
    if (f[64 + l] != mn) bad |= 2;
    if (f[128 + l] != x[37]) bad |= 4;
    if (f[192 + l] != x[(l * 13 + 5) & 63]) bad |= 8;
    if (i[l] != isum) bad |= 16;
    if (i[64 + l] != scan) bad |= 32;
    scan += l % 5;
    if (m[l] != bm) bad |= 64;
    if (i[128 + l] != __builtin_popcountll(bm & ((1ull << l) - 1ull))) bad |= 128;
    if (f[256 + l] != mx) bad |= 256;
  }
  if (bad) { char b[96]; snprintf(b, sizeof b, "agx_selftest: wave primitive mismatch, mask 0x%x", bad); return fail(AGX_E_HIP, b); }
  return AGX_OK;
}

}  // extern "C"
