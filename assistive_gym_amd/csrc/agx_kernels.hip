// agx_kernels.hip -- the kernels of ONE variant of the stepper for gfx950.  Built once per line of agx_variants.def by
// assistive_gym_amd/build.py, with the line's columns as -D flags (-DAGX_VNAME=feeding_l -DAGX_KSUFFIX=_fl -DAGX_TASK=0 -DAGX_MAX_DOF=16 ...
// -DAGX_HAS_MANIFOLD=0: variants.py, defines()); agx_api.hip picks the variant whose task and limits fit the model blob.
// To add a variant, add a line to agx_variants.def: the build, the accessors of agx_variant.h, agx_create and the emulator follow it.
// One workgroup = one wavefront = one environment (64 threads); an env.step() is
// frame_skip x [build kernel, solve kernel] + finish kernel on one stream.
#if !defined(AGX_VNAME) || !defined(AGX_KSUFFIX) || !defined(AGX_HAS_MANIFOLD)
#error "build with the -D flags of one line of agx_variants.def, see assistive_gym_amd/build.py"
#endif
#define AGX_CAT2_(a, b) a##b
#define AGX_CAT_(a, b) AGX_CAT2_(a, b)
#define AGX_K(name) AGX_CAT_(name, AGX_KSUFFIX)

#include "agx_wave.h"
#include "agx_step.h"
#include "agx_variant.h"
#if AGX_TASK == 3
#include "agx_cloth.h"
#endif

namespace {

// build: kinematics, ABA, collision, constraint rows -> scratch.  Register- and LDS-heavy.  One body, stamped per flavour of agx::env_build
// with its launcher.  `active`: masked settle of agx_reset, null on the step path; overflow_total: contacts dropped by a budget (rare; agx_overflow_count)
#define AGX_BUILD_KERNEL(kernel, launcher, MF) \
extern "C" __global__ void __launch_bounds__(64, 2) \
AGX_K(kernel)(const uint32_t* __restrict__ blob, float* state, const float* actions, float* scratch, float* debug, int env0, int n_envs, int sw, int act_dim, \
              const uint8_t* __restrict__ active, int* overflow_total, float* trace, int trace_words, int phase) { \
  extern __shared__ __attribute__((aligned(16))) float lds[]; \
  const int env = env0 + blockIdx.x; \
  if (env >= n_envs || (active && !active[env])) return; \
  const int dropped = agx::env_build<MF>(blob, state + (size_t)env * sw, actions ? actions + (size_t)env * act_dim : nullptr, scratch + (size_t)env * agx::SCR_WORDS, \
                                         debug ? debug + (size_t)env * agx::DBG_WORDS : nullptr, lds, (int)threadIdx.x, \
                                         trace ? trace + (size_t)env * trace_words + (size_t)phase * 12 * (((const int*)blob)[AGX_H_NDOF] + ((const int*)blob)[AGX_H_NFREE]) : nullptr); \
  if (dropped > 0 && threadIdx.x == 0) atomicAdd(overflow_total, dropped); \
} \
void launcher(const agx_launch& L, hipStream_t st, int e0, int ne, const float* actions, float* debug, const uint8_t* active, int phase, bool trace) { \
  hipLaunchKernelGGL(AGX_K(kernel), dim3(ne), dim3(64), agx::LDS_BYTES, st, L.blob, L.state, actions, L.scratch, debug, e0, L.n_envs, L.sw, L.act_dim, active, L.overflow, \
                     trace ? L.trace : nullptr, trace ? L.trace_words : 0, phase); \
}
AGX_BUILD_KERNEL(agx_build_kernel, v_build, false)
#if AGX_HAS_MANIFOLD
// ... with the persistent-manifold stage between collision and rows (blobs with AGX_P_MANIFOLD > 0 only)
AGX_BUILD_KERNEL(agx_build_mf_kernel, v_build_mf, true)
#endif
// solve: 50 PGS sweeps streaming the rows from the scratch record (L2), integration.  Lean.
// Variants with the wide row-local sweep (AGX_SOLVE_PAIR, agx_pgs_lvw.h): a workgroup takes the environments env0 + 2 b and env0 + 2 b + 1 of
// [env0, env_end) and sweeps them together, each in its own half of the LDS (2 x lds_words words); an environment without a partner (the end of the
// launch, the `active` mask) or a pair that cannot share the sweep goes through env_solve, one environment after the other.  Debug launches: one
// environment per workgroup.
// (The kernel of a variant without the paired sweep, and of every variant with -DAGX_SOLVE_PAIR=0, keeps the arguments and the text it had before.)
#if AGX_SOLVE_PAIR && AGX_PGS_LV == 4 && AGX_MAX_DOF <= 16 && AGX_MAX_BLOCK <= 10 && AGX_TASK == 0      /* = agx::LVW_PAIRED (AGX_TASK_FEEDING is 0) */
#define AGX_SOLVE_PAIRED 1
#define AGX_SOLVE_END_PARAM , int env_end
#define AGX_SOLVE_END_ARG(x) , x
#else
#define AGX_SOLVE_PAIRED 0
#define AGX_SOLVE_END_PARAM
#define AGX_SOLVE_END_ARG(x)
#endif
constexpr bool SOLVE_PAIRED = agx::LVW_PAIRED;
static_assert(SOLVE_PAIRED == (AGX_SOLVE_PAIRED != 0), "the preprocessor's statement of agx::LVW_PAIRED");
// (paired: 160 VGPRs.  The sweeps' assembly owns v80..v127, and what the single path keeps beside the paired one does not fit the other 80 without
// spilling; a paired launch has two wavefronts per SIMD where the unpaired one has four, so three are bound enough)
#ifndef AGX_SOLVE_WAVES
#define AGX_SOLVE_WAVES (SOLVE_PAIRED ? 3 : 4)
#endif
extern "C" __global__ void __launch_bounds__(64, AGX_SOLVE_WAVES)
AGX_K(agx_solve_kernel)(const uint32_t* __restrict__ blob, float* state, float* scratch, float* debug, int env0, int n_envs, int sw, const uint8_t* __restrict__ active, int phase,
                        int lds_words AGX_SOLVE_END_PARAM) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
#if AGX_SOLVE_PAIRED
  {
    const bool pair = debug == nullptr;
    const int envA = wave_uniform(env0 + (pair ? 2 : 1) * (int)blockIdx.x);      // (the sweeps take their record bases as scalar operands)
    if (env_end > n_envs) env_end = n_envs;
    const bool has0 = envA < env_end && (!active || active[envA]), has1 = pair && envA + 1 < env_end && (!active || active[envA + 1]);
    int lane2 = (int)threadIdx.x;
    asm volatile("" : "+v"(lane2));      // (no instruction: keeps the per-lane addresses of the single path below from being computed ahead of the paired sweeps and held across them)
    if (has0 && has1 && agx::env_solve_pair(blob, state + (size_t)envA * sw, scratch + (size_t)envA * agx::SCR_WORDS, lds, lane2, phase, lds_words)) return;
    _Pragma("nounroll") for (int e = 0; e < 2; e++) {
      const int lane = (int)threadIdx.x;
      // (both on the FIRST half of the LDS: the register sweep of agx_pgs.h addresses its window from LDS address 0)
      if (e ? has1 : has0) agx::env_solve(blob, state + (size_t)(envA + e) * sw, scratch + (size_t)(envA + e) * agx::SCR_WORDS, debug ? debug + (size_t)(envA + e) * agx::DBG_WORDS : nullptr,
                                          lds, lane, phase, lds_words);
      wave_sync();
    }
    return;
  }
#endif
  const int env = env0 + blockIdx.x;
  if (env >= n_envs || (active && !active[env])) return;
  agx::env_solve(blob, state + (size_t)env * sw, scratch + (size_t)env * agx::SCR_WORDS, debug ? debug + (size_t)env * agx::DBG_WORDS : nullptr, lds, (int)threadIdx.x, phase,
                 lds_words);
}
// finish: forces, observation, task state machine, reward, done, info
extern "C" __global__ void __launch_bounds__(64, 2)
AGX_K(agx_finish_kernel)(const uint32_t* __restrict__ blob, float* state, const float* actions, float* scratch, float* obs, float* reward, uint8_t* done,
                         float* info, int env0, int n_envs, int sw, int act_dim, int obs_dim, const float* report, int report_words, float* cloth, int cloth_words) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int env = env0 + blockIdx.x;
  if (env >= n_envs) return;
  agx::env_finish(blob, state + (size_t)env * sw, actions + (size_t)env * act_dim, scratch + (size_t)env * agx::SCR_WORDS, obs + (size_t)env * obs_dim,
                  reward + env, done + env, info ? info + (size_t)env * AGX_INFO_COUNT : nullptr, lds, (int)threadIdx.x,
                  report ? report + (size_t)env * report_words : nullptr, cloth ? cloth + (size_t)env * cloth_words : nullptr);
}
#if AGX_TASK == 5
// the water: one wavefront per environment, lane = particle (agx_water.h); replays the frames the build kernels left in the trace
extern "C" __global__ void __launch_bounds__(64)
AGX_K(agx_water_kernel)(const uint32_t* __restrict__ blob, const float* __restrict__ state, const float* __restrict__ trace, float* water, float* report, int env0, int n_envs,
                        int sw, int trace_words, int cloth_words, int report_words, int nsub, const uint8_t* __restrict__ active) {
  __shared__ __attribute__((aligned(16))) float lds[agxw::LDS_WORDS];
  const int env = env0 + blockIdx.x;
  if (env >= n_envs || (active && !active[env])) return;
  agxw::water_env(blob, state + (size_t)env * sw, trace + (size_t)env * trace_words, water + (size_t)env * cloth_words, report ? report + (size_t)env * report_words : nullptr, nsub,
                  lds, (int)threadIdx.x);
}
#endif
#if AGX_TASK == 3
// the garment: one workgroup of AGX_CLOTH_THREADS threads per environment, positions resident in LDS for all substeps of the launch
extern "C" __global__ void __launch_bounds__(AGX_CLOTH_THREADS)
AGX_K(agx_cloth_kernel)(const uint32_t* __restrict__ blob, const float* __restrict__ state, const float* __restrict__ trace, float* cloth, float* report, int env0, int n_envs,
                        int sw, int trace_words, int cloth_words, int report_words, int nsub, const uint8_t* __restrict__ active) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int env = env0 + blockIdx.x;
  if (env >= n_envs || (active && !active[env])) return;
  agxc::cloth_env(blob, state + (size_t)env * sw, trace + (size_t)env * trace_words, cloth + (size_t)env * cloth_words, report ? report + (size_t)env * report_words : nullptr, nsub, lds);
}
#endif
extern "C" __global__ void __launch_bounds__(64, 2)
AGX_K(agx_observe_kernel)(const uint32_t* __restrict__ blob, float* state, float* obs, int n_envs, int sw, int obs_dim, const uint8_t* __restrict__ mask) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int env = blockIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  agx::env_observe(blob, state + (size_t)env * sw, obs + (size_t)env * obs_dim, lds, (int)threadIdx.x);
}
// after a build-kernel pass: the collision flags of every environment's state (agx_check_collisions)
extern "C" __global__ void __launch_bounds__(64)
AGX_K(agx_collision_flags_kernel)(const uint32_t* __restrict__ blob, const float* __restrict__ scratch, uint8_t* flags, int n_envs) {
  const int env = blockIdx.x;
  if (env >= n_envs) return;
  const int f = agx::collision_flags(blob, scratch + (size_t)env * agx::SCR_WORDS, (int)threadIdx.x);
  if (threadIdx.x == 0) flags[env] = (uint8_t)f;
}
// reset generator: FeedingEnv.reset's sampling incl. the IK restarts (64 per round, one per lane), float64
extern "C" __global__ void __launch_bounds__(64)
AGX_K(agx_sample_kernel)(const uint32_t* __restrict__ blob, float* state, unsigned long long seed0, const unsigned long long* __restrict__ seeds, const uint8_t* __restrict__ mask,
                         int impairment_mode, int gender_mode, float* info4, int* episode, int n_envs, int sw, const int* __restrict__ first_restart, int* chosen,
                         const float* __restrict__ settled, int settled_sw, const float* __restrict__ fell) {
  const int env = blockIdx.x;
  if (env >= n_envs || (mask && !mask[env])) return;
  const unsigned long long seed = seeds ? seeds[env] : seed0 + (unsigned long long)env;
  if (threadIdx.x == 0) episode[env] = 0;
  const int r = agx::env_sample(blob, state + (size_t)env * sw, (uint32_t)seed, (uint32_t)(seed >> 32), impairment_mode, gender_mode,
                                info4 ? info4 + (size_t)env * 4 : nullptr, (int)threadIdx.x, first_restart ? first_restart[env] : 0,
                                settled ? settled + (size_t)env * settled_sw : nullptr, fell ? fell + (size_t)env * sw : nullptr);
  if (chosen && threadIdx.x == 0) chosen[env] = r;
}
// after a build-kernel pass over the freshly sampled states: which of them start in collision (and have a restart left to try)?
// work[env] = 1 and first_restart[env] = chosen + 1 for those, work[env] = 0 for the others
extern "C" __global__ void __launch_bounds__(64)
AGX_K(agx_reset_verdict_kernel)(const uint32_t* __restrict__ blob, const float* __restrict__ scratch, const uint8_t* __restrict__ active, uint8_t* work,
                                int* first_restart, const int* __restrict__ chosen, int n_envs) {
  const int env = blockIdx.x;
  if (env >= n_envs) return;
  bool again = false;
  if ((!active || active[env]) && chosen[env] >= 0) again = agx::reset_collides(blob, scratch + (size_t)env * agx::SCR_WORDS, (int)threadIdx.x);
  if (threadIdx.x == 0) { work[env] = again ? 1 : 0; if (again) first_restart[env] = chosen[env] + 1; }
}
// the camera's stage A (agx_collider_frames, agx_render; the ray caster is csrc/agx_render.hip): the world frame of every collider's body --
// position (3), rotation (9, row-major) -- of the environments [env0, env0 + gridDim.x) into frames[blockIdx.x][ncoll][12].  The state is read only.
extern "C" __global__ void __launch_bounds__(64, 2)
AGX_K(agx_frames_kernel)(const uint32_t* __restrict__ blob, const float* __restrict__ state, float* __restrict__ frames, int env0, int n_envs, int sw) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int env = env0 + blockIdx.x;
  if (env >= n_envs) return;
  agx::Ctx c; agx::ctx_init(c, blob, lds, (int)threadIdx.x);
  agx::load_env(c, state + (size_t)env * sw, sw);
  agx::kinematics(c);
  float* out = frames + (size_t)blockIdx.x * c.ncoll * 12;
  for (int col = (int)threadIdx.x; col < c.ncoll; col += 64) {
    m3 R; v3 p; agx::body_xf(c, CLI(c, col, AGX_C_BODY), R, p);
    st3(out + 12 * col, p); stm3(out + 12 * col + 3, R);
  }
}

// LDS of a solve launch.  AGX_SOLVE_LDS_BYTES (tuning knob, read once): the row-local sweeps (agx_pgs_lvw.h, agx_pgs_lvs.h) size their window of resident
// rows from it -- more LDS = fewer rows streamed from L2, fewer wavefronts per CU; never below what the other sweeps and solve_tail() need
constexpr int SWEEP_LDS_BYTES = agx::LVS_COMPILED ? agx::LVS_SOLVE_LDS_BYTES : 0;      // what the row-local sweeps of this variant want (agx_pgs_lvs.h)
int g_solve_lds_bytes = SWEEP_LDS_BYTES > agx::LDS_SOLVE_BYTES ? SWEEP_LDS_BYTES : agx::LDS_SOLVE_BYTES;
hipError_t v_init(void) {
  // (per environment: a paired launch has twice as much, so the knob ends at 32 KB there)
  if (const char* e = getenv("AGX_SOLVE_LDS_BYTES")) { int b = atoi(e) & ~15; if (b >= agx::LDS_SOLVE_BYTES && b <= (SOLVE_PAIRED ? 32 : 64) * 1024) g_solve_lds_bytes = b; }
  hipError_t e = hipFuncSetAttribute((const void*)AGX_K(agx_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (SOLVE_PAIRED ? 2 : 1) * g_solve_lds_bytes);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)AGX_K(agx_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, agx::LDS_BYTES);
#if AGX_HAS_MANIFOLD
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)AGX_K(agx_build_mf_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, agx::LDS_BYTES);
#endif
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)AGX_K(agx_finish_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, agx::LDS_BYTES);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)AGX_K(agx_observe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, agx::LDS_BYTES);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)AGX_K(agx_frames_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, agx::LDS_BYTES);
#if AGX_TASK == 3
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*)AGX_K(agx_cloth_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
#endif
  return e;
}
// the launchers: the handle's launch record unpacked into the kernels' arguments
void v_solve(const agx_launch& L, hipStream_t st, int e0, int ne, float* debug, const uint8_t* active, int phase) {
  const bool pair = SOLVE_PAIRED && !debug;
  hipLaunchKernelGGL(AGX_K(agx_solve_kernel), dim3(pair ? (ne + 1) / 2 : ne), dim3(64), (SOLVE_PAIRED ? 2 : 1) * g_solve_lds_bytes, st, L.blob, L.state, L.scratch, debug, e0, L.n_envs, L.sw,
                     active, phase, g_solve_lds_bytes / 4 AGX_SOLVE_END_ARG(e0 + ne));
}
void v_finish(const agx_launch& L, hipStream_t st, int e0, int ne, const float* actions, float* obs, float* reward, uint8_t* done, float* info) {
  hipLaunchKernelGGL(AGX_K(agx_finish_kernel), dim3(ne), dim3(64), agx::LDS_BYTES, st, L.blob, L.state, actions, L.scratch, obs, reward, done, info, e0, L.n_envs, L.sw, L.act_dim,
                     L.obs_dim, L.report, L.report_words, L.cloth, L.cloth_words);
}
#if AGX_TASK == 5
void v_cloth(const agx_launch& L, hipStream_t st, int e0, int ne, int nsub, const uint8_t* active) {
  hipLaunchKernelGGL(AGX_K(agx_water_kernel), dim3(ne), dim3(64), 0, st, L.blob, L.state, L.trace, L.cloth, L.report, e0, L.n_envs, L.sw, L.trace_words, L.cloth_words,
                     L.report_words, nsub, active);
}
int v_cloth_lds_bytes(int nn) { (void)nn; return 4 * agxw::LDS_WORDS; }
#elif AGX_TASK == 3
void v_cloth(const agx_launch& L, hipStream_t st, int e0, int ne, int nsub, const uint8_t* active) {
  hipLaunchKernelGGL(AGX_K(agx_cloth_kernel), dim3(ne), dim3(AGX_CLOTH_THREADS), L.cloth_lds, st, L.blob, L.state, L.trace, L.cloth, L.report, e0, L.n_envs, L.sw, L.trace_words,
                     L.cloth_words, L.report_words, nsub, active);
}
int v_cloth_lds_bytes(int nn) { return 4 * agxc::lds_words(nn); }
#endif
void v_observe(const agx_launch& L, hipStream_t st, float* obs, const uint8_t* mask) {
  hipLaunchKernelGGL(AGX_K(agx_observe_kernel), dim3(L.n_envs), dim3(64), agx::LDS_BYTES, st, L.blob, L.state, obs, L.n_envs, L.sw, L.obs_dim, mask);
}
void v_sample(const agx_launch& L, hipStream_t st, const agx_sample_args& A, const uint8_t* mask, float* info4, const int* first_restart) {
  hipLaunchKernelGGL(AGX_K(agx_sample_kernel), dim3(L.n_envs), dim3(64), 0, st, L.blob, L.state, A.seed0, A.seeds, mask, A.impairment_mode, A.gender_mode, info4, L.episode, L.n_envs,
                     L.sw, first_restart, L.chosen, A.settled, A.settled_sw, A.fell);
}
void v_verdict(const agx_launch& L, hipStream_t st, const uint8_t* active, uint8_t* work, int* first_restart) {
  hipLaunchKernelGGL(AGX_K(agx_reset_verdict_kernel), dim3(L.n_envs), dim3(64), 0, st, L.blob, L.scratch, active, work, first_restart, L.chosen, L.n_envs);
}
void v_collision_flags(const agx_launch& L, hipStream_t st, uint8_t* flags) {
  hipLaunchKernelGGL(AGX_K(agx_collision_flags_kernel), dim3(L.n_envs), dim3(64), 0, st, L.blob, L.scratch, flags, L.n_envs);
}
void v_frames(const agx_launch& L, hipStream_t st, int e0, int ne, float* frames) {
  hipLaunchKernelGGL(AGX_K(agx_frames_kernel), dim3(ne), dim3(64), agx::LDS_BYTES, st, L.blob, L.state, frames, e0, L.n_envs, L.sw);
}

#define AGX_STR2_(x) #x
#define AGX_STR_(x) AGX_STR2_(x)
const agx_variant g_variant = {
  AGX_STR_(AGX_VNAME), agx::TASK,
  agx::MAX_DOF, agx::MAX_FREE, agx::MAX_BLOCK, agx::MAX_HUMAN, agx::MAX_COLL, agx::ST_WORDS, agx::MAX_CON, agx::MAX_ROWS,
  agx::LDS_BYTES, agx::LDS_SOLVE_BYTES, agx::SCR_WORDS, agx::DBG_WORDS,
  agx::DBG_CON, agx::DBG_MINV, agx::DBG_HDR, agx::DBG_LAM, agx::DBG_TIME, agx::DBG_QDD,
  agx::RS_NARM,
  v_init, v_build, v_solve,
#if AGX_HAS_MANIFOLD
  v_build_mf,
#else
  nullptr,
#endif
  v_finish, v_observe,
  v_sample,
#if AGX_TASK == 3 || AGX_TASK == 5
  v_cloth,
#else
  nullptr,
#endif
  v_verdict,
  v_collision_flags,
#if AGX_TASK == 3 || AGX_TASK == 5
  v_cloth_lds_bytes,
#else
  nullptr,
#endif
  agx::SCR_O_META + agx::META_NWARM,
  v_frames
};

}  // namespace

extern "C" const agx_variant* AGX_CAT_(agx_variant_, AGX_VNAME)(void) { return &g_variant; }
