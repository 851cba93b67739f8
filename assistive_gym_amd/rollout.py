"""On-device PPO rollouts for the batched environments.

The reference trains with RLlib PPO on ``cpu_count()`` scalar gym workers (assistive_gym/learn.py:9-37:
train_batch_size 19200, lambda 0.95, fcnet_hiddens [100, 100]); observations and actions cross the
process boundary every step.  Here the policy (the same 2 x 100 tanh MLP with a diagonal Gaussian head and a
separate value branch, RLlib's defaults for a Box action space) runs in torch on the GPU that steps the
environments, so a rollout of T steps of N environments is T x (policy forward + libagx step) with every
tensor resident in HBM; only the finished batch is handed to the learner.

With a `seed`, collect() replaces the per-step torch policy call by ONE launch of libagx's agx_policy_act (csrc/agx_policy.hip): the two
MLPs, the Gaussian sample from a counter-based generator addressed by (seed, global env index, step, component) -- so a trajectory does not
depend on how the batch is laid out over processes, like every other draw of this project (agx_reset.h) -- log-probability and value, written
straight into row t of the rollout buffers.  gae() of device tensors is agx_gae, one launch.  The torch forms stay: they are the CPU path and
the reference the device tests compare the kernels with.

This module is plumbing around the stepper (torch for device memory and the MLP); it contains no physics.
"""
import math

import torch
from torch import nn


class GaussianMLPPolicy(nn.Module):
    """fcnet_hiddens [100, 100], tanh, outputs (mean, log_std) per action dimension; value function on its own
    branch (RLlib: vf_share_layers False).  Actions are sampled unclipped -- the env clips to [-1, 1] (env.py:188)."""

    def __init__(self, obs_dim, act_dim, hidden=(100, 100)):
        super().__init__()
        def mlp(out):
            layers, d = [], obs_dim
            for h in hidden:
                layers += [nn.Linear(d, h), nn.Tanh()]
                d = h
            return nn.Sequential(*layers, nn.Linear(d, out))
        self.pi, self.vf = mlp(2 * act_dim), mlp(1)
        self.obs_dim, self.act_dim, self.hidden = obs_dim, act_dim, tuple(hidden)
        for m in self.modules():                      # RLlib's normc initialisation, small final policy layer
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight)
                m.weight.data *= 1.0 / m.weight.data.norm(dim=1, keepdim=True)
                nn.init.zeros_(m.bias)
        self.pi[-1].weight.data *= 0.01

    def forward(self, obs):
        out = self.pi(obs)
        return out[..., :self.act_dim], out[..., self.act_dim:].clamp(-20.0, 2.0), self.vf(obs).squeeze(-1)

    def flat_params(self):
        """every parameter in one float32 vector, the layout agx_policy_act reads: nn.Linear's own (weight [out][in] row-major, then bias) in
        the order pi.0, pi.2, pi.4, vf.0, vf.2, vf.4"""
        return torch.cat([p.detach().reshape(-1) for p in list(self.pi.parameters()) + list(self.vf.parameters())]).float().contiguous()

    def fits_kernel(self):
        """within agx_policy_act's limits (include/agx.h): two hidden layers of at most 128 units, at most 128 observations and 32 actions"""
        from .libagx import POLICY_MAX_ACT, POLICY_MAX_IN
        return len(self.hidden) == 2 and max(self.obs_dim, *self.hidden) <= POLICY_MAX_IN and self.act_dim <= POLICY_MAX_ACT and self.pi[0].weight.dtype == torch.float32

    @torch.no_grad()
    def act(self, obs, generator=None, deterministic=False):
        mean, log_std, value = self(obs)
        eps = torch.zeros_like(mean) if deterministic else torch.randn(mean.shape, device=mean.device, dtype=mean.dtype, generator=generator)
        action = mean + log_std.exp() * eps
        logp = (-0.5 * eps * eps - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        return action, logp, value

    def log_prob(self, obs, action):
        mean, log_std, value = self(obs)
        z = (action - mean) / log_std.exp()
        return (-0.5 * z * z - log_std - 0.5 * math.log(2 * math.pi)).sum(-1), value


def gae(rewards, values, dones, gamma=0.99, lam=0.95):
    """Generalised advantage estimation over a [T, N] rollout.  values: [T + 1, N] (bootstrap value last);
    dones[t] marks that step t ended its episode (the env has already been reset, so nothing is carried over).
    float32 tensors on a GPU: one agx_gae launch; anything else: the loop below (the same recursion)."""
    if rewards.is_cuda and rewards.dtype == torch.float32 and values.dtype == torch.float32 and rewards.dim() == 2 and rewards.numel() > 0:
        from . import libagx
        adv, ret = torch.empty_like(rewards, memory_format=torch.contiguous_format), torch.empty_like(rewards, memory_format=torch.contiguous_format)
        with torch.cuda.device(rewards.device):
            libagx.gae(rewards.contiguous(), values.contiguous(), dones.to(torch.uint8).contiguous(), gamma, lam, adv, ret,
                       stream=torch.cuda.current_stream(rewards.device).cuda_stream)
        return adv, ret
    return gae_loop(rewards, values, dones, gamma, lam)


def gae_loop(rewards, values, dones, gamma=0.99, lam=0.95):
    """the recursion of gae() in torch, one time step after the other"""
    T = rewards.shape[0]
    adv = torch.zeros_like(rewards)
    last = torch.zeros_like(rewards[0])
    for t in range(T - 1, -1, -1):
        live = 1.0 - dones[t].to(rewards.dtype)
        delta = rewards[t] + gamma * values[t + 1] * live - values[t]
        last = delta + gamma * lam * live * last
        adv[t] = last
    return adv, adv + values[:-1]


AGENT_SEED_STRIDE = 1 << 40      # co-op: the human's policy draws from seed + AGENT_SEED_STRIDE (keys are seed + global env index: no overlap below 2^40 envs)


def agent_slices(env, policies):
    """[(policy, observation columns, action columns)]: one entry for a single policy; the robot's and the human's column slices of a co-op
    batch (feeding.py:110-111: the robot's observation comes first, then the human's; actions likewise) for a pair of policies"""
    if isinstance(policies, (tuple, list)):
        assert len(policies) == 2, 'a co-op batch takes (robot policy, human policy)'
        o_r, a_r = env.blob.obs_dim_robot, env.blob.act_dim_robot
        return [(policies[0], slice(0, o_r), slice(0, a_r)), (policies[1], slice(o_r, env.obs_dim), slice(a_r, env.act_dim))]
    return [(policies, slice(0, env.obs_dim), slice(0, env.act_dim))]


@torch.no_grad()
def collect(env, policy, horizon, generator=None, *, seed=None, step0=0, deterministic=False):
    """horizon steps of every environment of a vec env under `policy`; returns device tensors
    obs [T, N, O], actions [T, N, A], logp / rewards / values [T, N], dones [T, N] (uint8), last_value [N],
    and the env's per-step info [T, N, 8].  Call env.reset() once before the first collect; the env auto-resets.
    policy: a GaussianMLPPolicy, or (robot policy, human policy) for a co-op env -- then logp is [2, T, N] and values [2, T + 1, N].
    seed given, env on a GPU, policies within the kernel's limits: every step's policy call is one agx_policy_act launch per policy writing
    into row t of the buffers, the noise of step t addressed by (seed, env.env_offset + env index, step0 + t); otherwise torch, with
    `generator`."""
    n, dev = env.n_envs, env.device
    agents = agent_slices(env, policy)
    pair = isinstance(policy, (tuple, list))
    lead = (2,) if pair else ()
    buf = dict(obs=torch.empty((horizon, n, env.obs_dim), device=dev), actions=torch.empty((horizon, n, env.act_dim), device=dev),
               logp=torch.empty(lead + (horizon, n), device=dev), rewards=torch.empty((horizon, n), device=dev),
               values=torch.empty(lead + (horizon + 1, n), device=dev), dones=torch.empty((horizon, n), dtype=torch.uint8, device=dev),
               info=torch.empty((horizon, n, 8), device=dev))
    logp, values = (buf['logp'], buf['values']) if pair else (buf['logp'][None], buf['values'][None])
    fused = seed is not None and torch.device(dev).type == 'cuda' and all(p.fits_kernel() for p, _, _ in agents)
    if fused:
        from . import libagx
        params = [p.flat_params() for p, _, _ in agents]
        stream = torch.cuda.current_stream(dev).cuda_stream
    obs = env.obs
    for t in range(horizon):
        buf['obs'][t].copy_(obs)
        if fused:
            with torch.cuda.device(dev):
                for a, (p, oc, ac) in enumerate(agents):
                    libagx.policy_act(params[a], p.obs_dim, p.hidden[0], p.hidden[1], p.act_dim, obs[:, oc], n, seed + a * AGENT_SEED_STRIDE, env.env_offset, step0 + t,
                                      buf['actions'][t][:, ac], logp[a][t], values[a][t], deterministic=deterministic, stream=stream)
            action = buf['actions'][t]
        elif not pair and not deterministic:
            action, lp, value = policy.act(obs, generator)
            action = action.contiguous()
            buf['actions'][t], buf['logp'][t], buf['values'][t] = action, lp, value
        else:
            for a, (p, oc, ac) in enumerate(agents):
                buf['actions'][t][:, ac], logp[a][t], values[a][t] = p.act(obs[:, oc], generator, deterministic)
            action = buf['actions'][t]
        obs, rew, done, info = env.step(action)
        buf['rewards'][t].copy_(rew); buf['dones'][t].copy_(done); buf['info'][t].copy_(info)
    for a, (p, oc, _) in enumerate(agents):
        values[a][horizon] = p(obs[:, oc])[2]
    return buf
