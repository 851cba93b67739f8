// agx_ik.hip -- the kernels behind agx_ee_pose / agx_ee_ik (include/agx.h): one lane per (environment, arm), 64-thread blocks, blockIdx.y = the arm,
// so a wavefront holds one arm and its reads of the link table are scalar.  The math is csrc/agx_ik.h; what this file adds is the
// lane -> environment map and the wave-wide ballot that ends the iteration loop once every lane of a wavefront has stopped.
// Latency-bound serial code: 4,096 environments are 64 wavefronts per arm.  The launchers are called from agx_api.hip, which owns the handle
// and has checked every argument.
#include "agx_wave.h"
#include "agx_ik.h"

extern "C" __global__ void __launch_bounds__(64)
agx_ee_pose_kernel(const uint32_t* __restrict__ blob, const float* __restrict__ state, int sw, int n_envs, int arms, float* __restrict__ pose) {
  const int env = blockIdx.x * 64 + threadIdx.x, arm = blockIdx.y;
  if (env >= n_envs) return;
  agxik::lane_pose(blob, state + (size_t)env * sw, arm, pose + ((size_t)env * arms + arm) * 7);
}

extern "C" __global__ void __launch_bounds__(64)
agx_ee_ik_kernel(const uint32_t* __restrict__ blob, const float* __restrict__ state, int sw, int n_envs, int arms,
                 const float* __restrict__ target, int target_stride, int frame, int iters, float damping, float gain,
                 float* __restrict__ q_out, float* __restrict__ action, int action_stride, float* __restrict__ err) {
  const int env = blockIdx.x * 64 + threadIdx.x, arm = blockIdx.y;
  const bool live = env < n_envs;
  const size_t e = live ? env : n_envs - 1;         // the lanes past the end of the batch repeat the last environment, vote with it and write nothing
  const size_t slot = e * arms + arm;
  agxik::lane_ik(blob, state + e * sw, arm, target + e * target_stride + arm * (frame == AGX_EE_DELTA ? 6 : 7), frame, iters, damping, gain,
                 q_out ? q_out + slot * 7 : nullptr, err ? err + slot * 2 : nullptr, action ? action + e * action_stride : nullptr, live,
                 [](bool stopped) { return !wave_any(!stopped); });
}

void agx_launch_ee_pose(hipStream_t st, const uint32_t* blob, const float* state, int sw, int n_envs, int arms, float* pose) {
  hipLaunchKernelGGL(agx_ee_pose_kernel, dim3((n_envs + 63) / 64, arms), dim3(64), 0, st, blob, state, sw, n_envs, arms, pose);
}

void agx_launch_ee_ik(hipStream_t st, const uint32_t* blob, const float* state, int sw, int n_envs, int arms, const float* target, int target_stride,
                      int frame, int iters, float damping, float gain, float* q_out, float* action, int action_stride, float* err) {
  hipLaunchKernelGGL(agx_ee_ik_kernel, dim3((n_envs + 63) / 64, arms), dim3(64), 0, st, blob, state, sw, n_envs, arms, target, target_stride, frame, iters,
                     damping, gain, q_out, action, action_stride, err);
}
