// agx_variant.h -- what one compiled variant of the kernels (agx_kernels.hip built with one set of limits and one task
// layer) exposes to the handle code of agx_api.hip: its limits, its LDS / scratch / debug layout and its launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// What every launch of one handle passes unchanged: the device buffers of the handle and their strides.  agx_create fills it once (the handle's
// `L`), the launchers unpack it into the kernels' arguments.
struct agx_launch {
  uint32_t* blob;                        // the model blob (include/agx_blob.h)
  float *state, *scratch;                // [n_envs][sw] state records, [n_envs][scr_words] rows / contacts handed between the kernels
  int n_envs, sw, act_dim, obs_dim;
  int* overflow;                         // contacts dropped by a budget since creation (all envs)
  // models with a cloth section, null / 0 without one: [n_envs][trace_words] link frames of every substep of an env step, written by the build
  // kernels for the cloth kernel; the cloth kernel's report to the finish kernel; the garments (drinking: the water) and the cloth kernel's LDS
  float* trace; int trace_words;
  float* report; int report_words;
  float* cloth; int cloth_words, cloth_lds;
  int *episode, *chosen;                 // reset generator: episode counters, the IK restart each environment's sample came from
};
// what stays the same over the sample launches of one reset (agx_sample_reset / agx_reset)
struct agx_sample_args {
  unsigned long long seed0; const unsigned long long* seeds;    // env i samples from seeds[i], or from seed0 + i where seeds is null
  int impairment_mode, gender_mode;
  const float* settled; int settled_sw;  // [n_envs][settled_sw] records of the attached rag-doll model (or null)
  const float* fell;                     // [n_envs][sw] records of the attached fall model (arm manipulation, or null)
};

struct agx_variant {
  const char* name;
  int task_kind;                         // AGX_TASK_* the finish / observe kernels are compiled for
  int max_dof, max_free, max_block, max_human, max_coll, st_words, max_con, max_rows;
  int lds_bytes, lds_solve_bytes, scr_words, dbg_words;
  int dbg_con, dbg_minv, dbg_hdr, dbg_lam, dbg_time, dbg_qdd;     // debug record layout (agx_debug_layout)
  int rs_narm;                           // arm DoFs the reset generator's IK is compiled for
  // one-time kernel attribute set-up (dynamic LDS sizes)
  hipError_t (*init)(void);
  // Launchers: (the handle's launch record, stream, what varies per call).  build / solve / finish / cloth: grid = ne workgroups, environments
  // [e0, e0 + ne); the others cover every environment.  active / mask: per-env bytes, null = every environment.
  // phase: index of the substep within the env step (hooks after every SIM_SUBSTEPS-th, slot of the link-frame trace);
  // trace: write the link frames of this substep into L.trace (the step path of a model with a cloth; the collision passes never do)
  void (*build)(const agx_launch& L, hipStream_t st, int e0, int ne, const float* actions, float* debug, const uint8_t* active, int phase, bool trace);
  void (*solve)(const agx_launch& L, hipStream_t st, int e0, int ne, float* debug, const uint8_t* active, int phase);
  // the build kernel with the persistent-manifold stage (blobs with AGX_P_MANIFOLD > 0); null in variants compiled without it
  void (*build_mf)(const agx_launch& L, hipStream_t st, int e0, int ne, const float* actions, float* debug, const uint8_t* active, int phase, bool trace);
  // reads L.report; L.cloth is the water buffer for the drinking task layer (teleports drunk particles), unused elsewhere
  void (*finish)(const agx_launch& L, hipStream_t st, int e0, int ne, const float* actions, float* obs, float* reward, uint8_t* done, float* info);
  void (*observe)(const agx_launch& L, hipStream_t st, float* obs, const uint8_t* mask);
  // info4: [n_envs][4] IK report or null; first_restart: per env, the IK restart to begin at (null = 0)
  void (*sample)(const agx_launch& L, hipStream_t st, const agx_sample_args& A, const uint8_t* mask, float* info4, const int* first_restart);
  // the garment (agx_cloth.h): nsub substeps replaying the trace; null in variants without a cloth
  void (*cloth)(const agx_launch& L, hipStream_t st, int e0, int ne, int nsub, const uint8_t* active);
  // collision verdict on freshly sampled states after a build pass (see agx_reset.h reset_collides)
  void (*verdict)(const agx_launch& L, hipStream_t st, const uint8_t* active, uint8_t* work, int* first_restart);
  // collision flags (AGX_COLLIDE_*) of every environment's state after a build pass (agx_check_collisions)
  void (*collision_flags)(const agx_launch& L, hipStream_t st, uint8_t* flags);
  // dynamic LDS bytes of the cloth kernel for a garment of nn nodes (agxc::lds_words); null without a cloth kernel
  int (*cloth_lds_bytes)(int nn);
  // word of the per-environment scratch record that counts the entries of the warm-start memory (AGX_P_WARMSTART): agx_api.hip zeroes it
  // for every environment whose state is replaced from outside (set_state, resets)
  int scr_warm_word;
  // the camera's stage A: frames[k][ncoll][12] = position and rotation of the body of every collider of environment e0 + k, k < ne
  void (*collider_frames)(const agx_launch& L, hipStream_t st, int e0, int ne, float* frames);
};

// one accessor per line of agx_variants.def: agx_variant_<name>()
#define AGX_VARIANT(name, ...) extern "C" const agx_variant* agx_variant_##name(void);
#include "agx_variants.def"
#undef AGX_VARIANT
