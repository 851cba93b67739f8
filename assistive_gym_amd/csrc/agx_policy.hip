// agx_policy.hip -- the learner-side hot path of a rollout step: GaussianMLPPolicy.act (assistive_gym_amd/rollout.py) in ONE launch, and
// generalised advantage estimation over a finished rollout in one launch.  Both entries are stateless (no handle) and run on the calling
// thread's current HIP device.
//
// agx_policy_act.  The work is tiny (two 3-layer tanh MLPs, ~28 k multiply-adds per environment) and bound by latency and by how many CUs
// it reaches, so a workgroup takes a tile of PA_E = 16 environments (4,096 environments = 256 workgroups = every CU) and its 8 waves share
// the output units of both branches.  16 environments are exactly the M of v_mfma_f32_16x16x4_f32: a wave computes
// out[16 envs][16 units] += act[16 envs][4 k] * W^T[4 k][16 units] per instruction, with ONE activation and ONE weight value per lane
// (16x operand reuse against a lane-per-output loop; the f32 MFMA is an exact k-ordered fmaf chain, so the numerics are those of the VALU).
//   * activations live in LDS as [unit][env] (16 consecutive floats per unit): the A fragment of a k-step is 64 consecutive floats, the
//     result registers of a tile (4 consecutive envs of one unit per lane) go back as one 16-byte store;
//   * weights are read from global memory in nn.Linear's own [out][in] layout (112 KB for the product's sizes: L2-resident), a chunk of
//     8 k-steps for two unit tiles at a time, so 16 loads are in flight before the 16 MFMAs that consume them and the two accumulators
//     hide the MFMA's dependent latency;
//   * an environment's row of the tile never meets another row, and the log-probability is summed in component order by one lane, so an
//     environment's outputs do not depend on which batch (or which half of a batch) it is evaluated in.
// Noise: Philox4x32-10 (the rounds of rs_u01, agx_reset.h) keyed by seed + env_offset + i with counter (k >> 2, step, 1, 0) -- the reset
// generator only uses counters whose third word is 0 -- and Box-Muller on the output words, see pa_eps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/agx.h"

namespace {

constexpr int PA_E = 16;          // environments per workgroup (the M of the MFMA)
constexpr int PA_WAVES = 8;
constexpr int PA_THREADS = 64 * PA_WAVES;
constexpr int PA_MAX_IN = 128;    // obs_dim, hidden_a, hidden_b
constexpr int PA_MAX_ACT = 32;
constexpr int PA_KCHUNK = 8;      // k-steps (of 4) whose operands are loaded before their MFMAs are issued

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PolicyDims { int obs, ha, hb, act; };

// one dense layer of both branches: tiles of 16 output units, two per wave at a time.  src0 / src1: LDS activations [K][16] of the policy / value
// branch; w0 / w1: [H0][K] / [H1][K] row-major + bias behind; dst0 / dst1: LDS [H][16].  TANH: hidden layer.
template <bool TANH>
__device__ __forceinline__ void pa_layer(const float* __restrict__ w0, int H0, const float* __restrict__ w1, int H1, int K,
                                         const float* src0, const float* src1, float* dst0, float* dst1, int wave, int lane) {
  const int t0 = (H0 + 15) >> 4, tiles = t0 + ((H1 + 15) >> 4);
  const int c = lane & 15, q = lane >> 4;                      // A: env c, k-slot q;  B: unit c of the tile, k-slot q;  D: unit c, envs 4q .. 4q+3
  for (int pair = wave; 2 * pair < tiles; pair += PA_WAVES) {
    const float* W[2]; const float* S[2]; float* D[2]; int H[2], j[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const int tile = 2 * pair + s;
      const bool second = tile >= t0;
      W[s] = second ? w1 : w0; S[s] = second ? src1 : src0; D[s] = second ? dst1 : dst0;
      H[s] = tile < tiles ? (second ? H1 : H0) : 0;            // an odd tile count: the pair's second half has no units
      j[s] = ((second ? tile - t0 : tile) << 4) + c;
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int k0 = 0; k0 < K; k0 += 4 * PA_KCHUNK) {
      float a[2][PA_KCHUNK], b[2][PA_KCHUNK];
#pragma unroll
      for (int u = 0; u < PA_KCHUNK; u++) {
        const int k = k0 + 4 * u + q;
#pragma unroll
        for (int s = 0; s < 2; s++) {
          const bool on = k < K && j[s] < H[s];
          b[s][u] = on ? W[s][(size_t)j[s] * K + k] : 0.f;
          a[s][u] = k < K ? S[s][k * PA_E + c] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < PA_KCHUNK; u++) {
        if (k0 + 4 * u < K) {                                  // wave-uniform
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][u], b[0][u], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][u], b[1][u], acc[1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 2; s++) {
      if (j[s] < H[s]) {
        const float bias = W[s][(size_t)H[s] * K + j[s]];
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; r++) { const float y = acc[s][r] + bias; o[r] = TANH ? tanhf(y) : y; }
        *reinterpret_cast<f32x4*>(D[s] + j[s] * PA_E + 4 * q) = o;
      }
    }
  }
}

// component k of environment key's noise at `step`: Philox4x32-10, counter (k >> 2, step, 1, 0); output words w0..w3; (wa, wb) = (w0, w1) for
// k & 2 == 0 else (w2, w3); u1 = ((wa >> 8) + 0.5) 2^-24, u2 = (wb >> 8) 2^-24, r = sqrt(-2 ln u1); eps = r cos(2 pi u2) for even k, r sin(2 pi u2)
// for odd k.  The radius is evaluated in float64 (u1 has 25 significant bits, and ln u1 near u1 = 1 would lose them in float32).
__device__ __forceinline__ float pa_eps(uint64_t key, uint32_t step, int k) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  uint32_t c0 = (uint32_t)(k >> 2), c1 = step, c2 = 1u, c3 = 0u;
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const uint32_t wa = (k & 2) ? c2 : c0, wb = (k & 2) ? c3 : c1;
  const double u1 = ((double)(wa >> 8) + 0.5) * (1.0 / 16777216.0);
  const float u2 = (float)(wb >> 8) * (1.0f / 16777216.0f);
  const float rad = (float)sqrt(-2.0 * log(u1));
  const float ang = 6.28318530717958647692f * u2;
  return rad * ((k & 1) ? sinf(ang) : cosf(ang));
}

extern "C" __global__ void __launch_bounds__(PA_THREADS)
agx_policy_act_kernel(const float* __restrict__ params, PolicyDims d, const float* __restrict__ obs, int obs_stride, int n_envs,
                      uint64_t seed, long long env_offset, uint32_t step, int deterministic,
                      float* __restrict__ action, int action_stride, float* __restrict__ logp, float* __restrict__ value) {
  __shared__ __attribute__((aligned(16))) float s_obs[PA_MAX_IN * PA_E];
  __shared__ __attribute__((aligned(16))) float s_h1[2][PA_MAX_IN * PA_E];
  __shared__ __attribute__((aligned(16))) float s_h2[2][PA_MAX_IN * PA_E];
  __shared__ __attribute__((aligned(16))) float s_out[(2 * PA_MAX_ACT + 16) * PA_E];   // policy head rows 0 .. 2 act - 1, the value in row 2 PA_MAX_ACT
  __shared__ float s_term[PA_MAX_ACT * PA_E];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long env0 = (long long)blockIdx.x * PA_E;

  // the parameter vector: pi.0, pi.2, pi.4, vf.0, vf.2, vf.4, each weight [out][in] then bias
  const float* p0 = params;
  const float* p1 = p0 + (size_t)d.ha * d.obs + d.ha;
  const float* p2 = p1 + (size_t)d.hb * d.ha + d.hb;
  const float* v0 = p2 + (size_t)2 * d.act * d.hb + 2 * d.act;
  const float* v1 = v0 + (size_t)d.ha * d.obs + d.ha;
  const float* v2 = v1 + (size_t)d.hb * d.ha + d.hb;

  for (int i = tid; i < PA_E * d.obs; i += PA_THREADS) {         // rows of the tile, coalesced along the observation
    const int e = i / d.obs, k = i - e * d.obs;
    s_obs[k * PA_E + e] = env0 + e < n_envs ? obs[(size_t)(env0 + e) * obs_stride + k] : 0.f;
  }
  __syncthreads();
  pa_layer<true>(p0, d.ha, v0, d.ha, d.obs, s_obs, s_obs, s_h1[0], s_h1[1], wave, lane);
  __syncthreads();
  pa_layer<true>(p1, d.hb, v1, d.hb, d.ha, s_h1[0], s_h1[1], s_h2[0], s_h2[1], wave, lane);
  __syncthreads();
  pa_layer<false>(p2, 2 * d.act, v2, 1, d.hb, s_h2[0], s_h2[1], s_out, s_out + 2 * PA_MAX_ACT * PA_E, wave, lane);
  __syncthreads();

  {                                                               // one lane per (environment, action component): 16 x 32 = the workgroup
    const int k = tid & 31, e = tid >> 5;
    const long long env = env0 + e;
    if (k < d.act && env < n_envs) {
      const float mean = s_out[k * PA_E + e];
      const float log_std = fminf(fmaxf(s_out[(d.act + k) * PA_E + e], -20.0f), 2.0f);
      const float eps = deterministic ? 0.f : pa_eps(seed + (uint64_t)env_offset + (uint64_t)env, step, k);
      action[(size_t)env * action_stride + k] = mean + expf(log_std) * eps;
      s_term[k * PA_E + e] = -0.5f * eps * eps - log_std - 0.918938533204672742f;        // 1/2 ln 2 pi
    }
  }
  __syncthreads();
  if (tid < PA_E && env0 + tid < n_envs) {
    float sum = 0.f;
    for (int k = 0; k < d.act; k++) sum += s_term[k * PA_E + tid];
    logp[env0 + tid] = sum;
    value[env0 + tid] = s_out[2 * PA_MAX_ACT * PA_E + tid];
  }
}

// rollout.gae: one lane per environment walks t = horizon - 1 .. 0; done[t] cuts the bootstrap and the carry
extern "C" __global__ void __launch_bounds__(64)
agx_gae_kernel(const float* __restrict__ rewards, const float* __restrict__ values, const uint8_t* __restrict__ dones, int horizon, int n_envs,
               float gamma, float lam, float* __restrict__ adv, float* __restrict__ ret) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_envs) return;
  float last = 0.f, v_next = values[(size_t)horizon * n_envs + i];
  for (int t = horizon - 1; t >= 0; t--) {
    const size_t o = (size_t)t * n_envs + i;
    const float live = dones[o] ? 0.f : 1.f, v = values[o];
    const float delta = rewards[o] + gamma * v_next * live - v;
    last = delta + gamma * lam * live * last;
    adv[o] = last;
    ret[o] = last + v;
    v_next = v;
  }
}

bool no_device() {
  static const bool none = [] { int n = 0; return hipGetDeviceCount(&n) != hipSuccess || n == 0; }();
  return none;
}

}  // namespace

extern "C" int agx_policy_act(const float* params_dev, int obs_dim, int hidden_a, int hidden_b, int act_dim,
                              const float* obs_dev, int obs_stride, int n_envs,
                              uint64_t seed, long long env_offset, uint32_t step, int deterministic,
                              float* action_dev, int action_stride, float* logp_dev, float* value_dev, void* stream) {
  if (obs_dim < 1 || obs_dim > PA_MAX_IN || hidden_a < 1 || hidden_a > PA_MAX_IN || hidden_b < 1 || hidden_b > PA_MAX_IN || act_dim < 1 || act_dim > PA_MAX_ACT)
    return AGX_E_ARG;
  if (obs_stride < obs_dim || action_stride < act_dim || n_envs < 0) return AGX_E_ARG;
  if (!params_dev || !obs_dev || !action_dev || !logp_dev || !value_dev) return AGX_E_ARG;
  if (n_envs == 0) return AGX_OK;
  if (no_device()) return AGX_E_NOGPU;
  const PolicyDims d = {obs_dim, hidden_a, hidden_b, act_dim};
  hipLaunchKernelGGL(agx_policy_act_kernel, dim3((n_envs + PA_E - 1) / PA_E), dim3(PA_THREADS), 0, (hipStream_t)stream,
                     params_dev, d, obs_dev, obs_stride, n_envs, seed, env_offset, step, deterministic, action_dev, action_stride, logp_dev, value_dev);
  return hipGetLastError() == hipSuccess ? AGX_OK : AGX_E_HIP;
}

extern "C" int agx_gae(const float* rewards_dev, const float* values_dev, const uint8_t* dones_dev, int horizon, int n_envs,
                       float gamma, float lam, float* adv_dev, float* ret_dev, void* stream) {
  if (horizon < 0 || n_envs < 0 || !rewards_dev || !values_dev || !dones_dev || !adv_dev || !ret_dev) return AGX_E_ARG;
  if (horizon == 0 || n_envs == 0) return AGX_OK;
  if (no_device()) return AGX_E_NOGPU;
  hipLaunchKernelGGL(agx_gae_kernel, dim3((n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     rewards_dev, values_dev, dones_dev, horizon, n_envs, gamma, lam, adv_dev, ret_dev);
  return hipGetLastError() == hipSuccess ? AGX_OK : AGX_E_HIP;
}
