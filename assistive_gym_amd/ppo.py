"""PPO on the batched environments: the learner behind `python -m assistive_gym.learn --train / --evaluate`.

The reference trains with RLlib's PPOTrainer (assistive_gym/learn.py:9-17,39-59,71-94) and evaluates trained policies over whole
episodes (learn.py:133-184).  RLlib is not a dependency here: the rollout is rollout.collect (one agx_policy_act launch per policy and
step, the stepper's kernels) and rollout.gae (agx_gae); the learner below is plain torch -- autograd, Adam and plumbing -- with RLlib PPO's
loss and defaults.  Those defaults and the loss are written down from memory of RLlib 1.x's ppo.py / ppo_torch_policy.py, not read from an
installed copy: every such line is tagged [RLLIB-UNVERIFIED], as the project tags Bullet conventions it could not check.
"""
import dataclasses
import glob
import math
import os
import shutil
import time

import torch

from .rollout import GaussianMLPPolicy, agent_slices, collect, gae


@dataclasses.dataclass
class PPOConfig:
    """RLlib PPO's defaults [RLLIB-UNVERIFIED] with the overrides of learn.py:11-17 (train_batch_size 19200, num_sgd_iter 50,
    sgd_minibatch_size 128, lambda 0.95, fcnet_hiddens [100, 100])."""
    lr: float = 5e-5                    # [RLLIB-UNVERIFIED]
    gamma: float = 0.99                 # [RLLIB-UNVERIFIED]
    lam: float = 0.95                   # learn.py:16 ('lambda')
    clip_param: float = 0.3             # [RLLIB-UNVERIFIED]
    kl_coeff: float = 0.2               # [RLLIB-UNVERIFIED] initial coefficient of the KL penalty
    kl_target: float = 0.01             # [RLLIB-UNVERIFIED] coefficient x 1.5 above 2 x target, x 0.5 below target / 2
    vf_clip_param: float = 10.0         # [RLLIB-UNVERIFIED]
    vf_loss_coeff: float = 1.0          # [RLLIB-UNVERIFIED]
    entropy_coeff: float = 0.0          # [RLLIB-UNVERIFIED]
    num_sgd_iter: int = 50              # learn.py:14
    sgd_minibatch_size: int = 128       # learn.py:15
    train_batch_size: int = 19200       # learn.py:13
    hidden: tuple = (100, 100)          # learn.py:17
    horizon: int = 0                    # steps of every environment per iteration; 0: ceil(train_batch_size / n_envs)

    def steps_per_iteration(self, n_envs):
        return self.horizon if self.horizon > 0 else max(1, -(-self.train_batch_size // n_envs))

    @classmethod
    def batched(cls, n_envs, horizon=50):
        """A starting configuration for thousands of lock-stepped environments: n_envs x horizon samples per iteration, minibatches of
        1/8 of that, 8 epochs, a larger step.  NOBODY HAS TUNED THESE VALUES: they are starting points chosen so that an iteration's learning
        phase stays comparable to its rollout, not results of a search, and no learning curve backs them."""
        batch = n_envs * horizon
        return cls(horizon=horizon, train_batch_size=batch, sgd_minibatch_size=max(128, batch // 8), num_sgd_iter=8, lr=3e-4)


HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def ppo_loss(policy, batch, cfg, kl_coeff):
    """RLlib's PPO surrogate loss [RLLIB-UNVERIFIED: ppo_torch_policy.py of RLlib 1.x] on a minibatch.  batch: obs [B, O], actions [B, A], logp
    (of the behaviour policy), adv, ret (value targets), values (the behaviour policy's value predictions) [B], old_mean, old_log_std [B, A].
      ratio     = exp(logp_new - logp)
      surrogate = mean(min(adv ratio, adv clip(ratio, 1 - clip_param, 1 + clip_param)))
      kl        = mean(KL(old || new)) of the diagonal Gaussians
      vf_loss   = mean(max((v - ret)^2, (values + clip(v - values, -vf_clip_param, vf_clip_param) - ret)^2))
      entropy   = mean(sum_k(log_std_k + ln(2 pi e) / 2))
      loss      = -surrogate + kl_coeff kl + vf_loss_coeff vf_loss - entropy_coeff entropy
    Returns (loss, {'surrogate', 'kl', 'vf_loss', 'entropy'}) -- tensors; nothing is read back to the host."""
    mean, log_std, v = policy(batch['obs'])
    z = (batch['actions'] - mean) / log_std.exp()
    logp = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    ratio = (logp - batch['logp']).exp()
    adv = batch['adv']
    surrogate = torch.min(adv * ratio, adv * ratio.clamp(1.0 - cfg.clip_param, 1.0 + cfg.clip_param)).mean()
    old_mean, old_log_std = batch['old_mean'], batch['old_log_std']
    kl = (log_std - old_log_std + ((2.0 * old_log_std).exp() + (old_mean - mean) ** 2) / (2.0 * (2.0 * log_std).exp()) - 0.5).sum(-1).mean()
    vf1 = (v - batch['ret']) ** 2
    vf2 = (batch['values'] + (v - batch['values']).clamp(-cfg.vf_clip_param, cfg.vf_clip_param) - batch['ret']) ** 2
    vf_loss = torch.max(vf1, vf2).mean()
    entropy = (log_std + 0.5 + HALF_LOG_2PI).sum(-1).mean()
    loss = -surrogate + kl_coeff * kl + cfg.vf_loss_coeff * vf_loss - cfg.entropy_coeff * entropy
    return loss, dict(surrogate=surrogate, kl=kl, vf_loss=vf_loss, entropy=entropy)


def adapt_kl_coeff(kl_coeff, sampled_kl, cfg):
    """RLlib's KLCoeffMixin.update_kl [RLLIB-UNVERIFIED]"""
    if sampled_kl > 2.0 * cfg.kl_target:
        return kl_coeff * 1.5
    if sampled_kl < 0.5 * cfg.kl_target:
        return kl_coeff * 0.5
    return kl_coeff


def _is_coop(env):
    blob = getattr(env, 'blob', None)
    return blob is not None and bool(blob.is_coop)


def make_policies(env, hidden=(100, 100)):
    """one GaussianMLPPolicy on env.device; for a co-op env (robot policy, human policy) on their column slices (learn.py:32-36)"""
    if _is_coop(env):
        b = env.blob
        return (GaussianMLPPolicy(b.obs_dim_robot, b.act_dim_robot, hidden).to(env.device),
                GaussianMLPPolicy(env.obs_dim - b.obs_dim_robot, env.act_dim - b.act_dim_robot, hidden).to(env.device))
    return GaussianMLPPolicy(env.obs_dim, env.act_dim, hidden).to(env.device)


class PPOTrainer:
    """`agent.train()` / `.save()` / `.restore()` of learn.py:71-94 for a vec env (assistive_gym_amd.vec_env, or anything with its surface:
    n_envs, device, obs_dim, act_dim, obs, env_offset, reset(), step(actions) -> (obs, reward, done, info))."""

    def __init__(self, env, cfg=None, seed=0, env_name='env'):
        self.env, self.cfg, self.seed, self.env_name = env, cfg or PPOConfig(), int(seed), env_name
        self.coop = _is_coop(env)
        state = torch.random.get_rng_state()
        torch.manual_seed(self.seed)                        # the initial weights are a function of the seed alone
        self.policies = make_policies(env, self.cfg.hidden)
        torch.random.set_rng_state(state)
        self._plist = list(self.policies) if self.coop else [self.policies]
        self.optims = [torch.optim.Adam(p.parameters(), lr=self.cfg.lr) for p in self._plist]
        self.kl_coeffs = [self.cfg.kl_coeff for _ in self._plist]
        # shuffles, and the action noise where the torch path of collect() runs (CPU envs, policies outside the kernel's limits)
        self.generator = torch.Generator(device=env.device); self.generator.manual_seed(self.seed)
        self.training_iteration, self.timesteps_total, self.time_total_s, self.steps_done = 0, 0, 0.0, 0
        self.partial_return = torch.zeros(env.n_envs, device=env.device)     # return so far of the episode every env is in
        self.episode_stats = (float('nan'), float('nan'), float('nan'))
        self.last_terms = []
        self._started = False

    @property
    def kl_coeff(self):
        return self.kl_coeffs[0]

    def _episode_returns(self, rewards, dones):
        """returns of the episodes that ended inside this rollout, partial returns carried over; device tensors in, one host read"""
        T = rewards.shape[0]
        finished = torch.zeros_like(rewards)
        run = self.partial_return
        for t in range(T):
            run = run + rewards[t]
            d = dones[t].bool()
            finished[t] = torch.where(d, run, finished[t])
            run = torch.where(d, torch.zeros_like(run), run)
        self.partial_return = run
        return finished[dones.bool()]

    def train(self):
        """one iteration: collect -> gae -> num_sgd_iter epochs of shuffled minibatches; the result names are those learn.py:86 prints"""
        cfg, env = self.cfg, self.env
        t0 = time.perf_counter()
        if not self._started:
            env.reset()                                     # (a restored trainer starts new episodes too: nothing is carried into them)
            self.partial_return = torch.zeros(env.n_envs, device=env.device)
            self._started = True
        T = cfg.steps_per_iteration(env.n_envs)
        buf = collect(env, self.policies, T, self.generator, seed=self.seed, step0=self.steps_done)
        returns = self._episode_returns(buf['rewards'], buf['dones'])
        if returns.numel():
            # co-op: RLlib adds the two agents' (identical) rewards and learn.py:81-85 halves the sum again -- that is the shared reward the stepper reports once
            r = returns.double()
            self.episode_stats = (float(r.mean()), float(r.min()), float(r.max()))     # (the host read also ends the rollout's timing)
        elif torch.device(env.device).type == 'cuda':
            torch.cuda.synchronize(env.device)
        t1 = time.perf_counter()
        B = T * env.n_envs
        self.last_terms = []
        logp, values = (buf['logp'], buf['values']) if self.coop else (buf['logp'][None], buf['values'][None])
        for a, (policy, oc, ac) in enumerate(agent_slices(env, self.policies)):
            adv, ret = gae(buf['rewards'], values[a], buf['dones'], cfg.gamma, cfg.lam)
            adv = adv.reshape(B)
            adv = (adv - adv.mean()) / adv.std().clamp_min(1e-4)                         # standardize_fields=['advantages'] [RLLIB-UNVERIFIED]
            obs = buf['obs'][:, :, oc].reshape(B, -1)
            with torch.no_grad():
                old_mean, old_log_std, _ = policy(obs)
            batch = dict(obs=obs, actions=buf['actions'][:, :, ac].reshape(B, -1), logp=logp[a].reshape(B), adv=adv, ret=ret.reshape(B),
                         values=values[a][:-1].reshape(B), old_mean=old_mean, old_log_std=old_log_std)
            mb = min(cfg.sgd_minibatch_size, B)
            for epoch in range(cfg.num_sgd_iter):
                perm = torch.randperm(B, device=env.device, generator=self.generator)
                sums, count = None, 0
                for s in range(0, B - mb + 1, mb):                                       # whole minibatches only, as RLlib's minibatches() [RLLIB-UNVERIFIED]
                    idx = perm[s:s + mb]
                    loss, terms = ppo_loss(policy, {k: v[idx] for k, v in batch.items()}, cfg, self.kl_coeffs[a])
                    self.optims[a].zero_grad(set_to_none=True)
                    loss.backward()
                    self.optims[a].step()
                    vals = torch.stack([loss.detach()] + [terms[k].detach() for k in ('surrogate', 'kl', 'vf_loss', 'entropy')])
                    sums, count = (vals if sums is None else sums + vals), count + 1
            last = (sums / count).tolist()                                               # means over the last epoch; the iteration's only other host read
            terms = dict(zip(('loss', 'surrogate', 'kl', 'vf_loss', 'entropy'), last))
            self.kl_coeffs[a] = adapt_kl_coeff(self.kl_coeffs[a], terms['kl'], cfg)
            terms['kl_coeff'] = self.kl_coeffs[a]
            self.last_terms.append(terms)
        t2 = time.perf_counter()
        self.training_iteration += 1
        self.steps_done += T
        self.timesteps_total += B
        self.time_total_s += t2 - t0
        mean, lo, hi = self.episode_stats
        return dict(training_iteration=self.training_iteration, timesteps_total=self.timesteps_total, time_total_s=self.time_total_s,
                    episode_reward_mean=mean, episode_reward_min=lo, episode_reward_max=hi, time_rollout_s=t1 - t0, time_learn_s=t2 - t1,
                    learner=self.last_terms)

    # ---- checkpoints: <dir>/checkpoint_<n>/checkpoint-<n>.pt, the layout learn.py:49-56 searches -------------------------------------
    def save(self, directory):
        n = self.training_iteration
        d = os.path.join(directory, 'checkpoint_%d' % n)
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, 'checkpoint-%d.pt' % n)
        torch.save(dict(policies=[p.state_dict() for p in self._plist], optims=[o.state_dict() for o in self.optims], kl_coeffs=list(self.kl_coeffs),
                        counters=dict(training_iteration=self.training_iteration, timesteps_total=self.timesteps_total, time_total_s=self.time_total_s,
                                      steps_done=self.steps_done),
                        generator=self.generator.get_state(), episode_stats=self.episode_stats, seed=self.seed,
                        dims=[(p.obs_dim, p.act_dim, p.hidden) for p in self._plist]), path)
        return path

    def restore(self, path):
        ck = torch.load(path, map_location='cpu')
        assert [tuple(d[:2]) + (tuple(d[2]),) for d in ck['dims']] == [(p.obs_dim, p.act_dim, p.hidden) for p in self._plist], 'the checkpoint was written for another environment or network'
        for p, o, sp, so in zip(self._plist, self.optims, ck['policies'], ck['optims']):
            p.load_state_dict(sp)
            o.load_state_dict(so)
        self.kl_coeffs = list(ck['kl_coeffs'])
        c = ck['counters']
        self.training_iteration, self.timesteps_total, self.time_total_s, self.steps_done = c['training_iteration'], c['timesteps_total'], c['time_total_s'], c['steps_done']
        self.generator.set_state(ck['generator'])
        self.seed = int(ck['seed'])                         # the noise of the fused rollout is addressed by (seed, env, step): a resumed run continues its streams
        self.episode_stats = tuple(ck['episode_stats'])


def checkpoint_dir(save_dir, algo, env_name):
    return os.path.join(save_dir, algo, env_name)


def latest_checkpoint(path, algo='ppo', env_name=''):
    """learn.py:44-56: a path that names a checkpoint is taken as it is; otherwise the newest checkpoint_<n> under <path>/<algo>/<env>"""
    if not path:
        return None
    if 'checkpoint' in os.path.basename(path.rstrip('/')) and os.path.isfile(path):
        return path
    numbers = []
    for f in glob.glob(os.path.join(checkpoint_dir(path, algo, env_name), 'checkpoint_*')):
        try:
            numbers.append(int(f.split('_')[-1]))
        except ValueError:
            pass
    if not numbers:
        return None
    n = max(numbers)
    p = os.path.join(checkpoint_dir(path, algo, env_name), 'checkpoint_%d' % n, 'checkpoint-%d.pt' % n)
    return p if os.path.isfile(p) else None


def remove_checkpoint(path):
    """learn.py:89-91: the previous checkpoint goes when the next one is written"""
    if path:
        shutil.rmtree(os.path.dirname(path), ignore_errors=True)


@torch.no_grad()
def evaluate(env, policies, n_episodes, seed=0, deterministic=False):
    """learn.py:133-184 for a batch: whole episodes of EVERY environment of `env`, ceil(n_episodes / n_envs) of them each, under `policies`
    (a policy, or (robot, human) for a co-op env).  Per episode: the reward total, the mean of info['total_force_on_human'] over its steps and
    the last info['task_success'] (the info columns AGX_INFO_TOTAL_FORCE, AGX_INFO_TASK_SUCCESS the stepper writes).  Returns their mean and
    std (numpy's population std, as learn.py:174-183) and the number of episodes.  No per-step host read-back."""
    n, dev = env.n_envs, env.device
    rounds = max(1, -(-int(n_episodes) // n))
    steps = rounds * int(env.episode_len)
    env.reset()
    ar = torch.arange(n, device=dev)
    rec = torch.zeros((3, rounds, n), dtype=torch.float64, device=dev)
    count = torch.zeros(n, dtype=torch.long, device=dev)
    acc = torch.zeros((2, n), dtype=torch.float64, device=dev)
    length = torch.zeros(n, dtype=torch.float64, device=dev)
    generator = torch.Generator(device=dev); generator.manual_seed(int(seed))
    chunk = int(env.episode_len)
    for s0 in range(0, steps, chunk):
        buf = collect(env, policies, min(chunk, steps - s0), generator, seed=int(seed), step0=s0, deterministic=deterministic)
        for t in range(buf['rewards'].shape[0]):
            acc[0] += buf['rewards'][t]; acc[1] += buf['info'][t, :, 0]; length += 1
            d = buf['dones'][t].bool() & (count < rounds)
            row = count.clamp(max=rounds - 1)
            new = torch.stack([acc[0], acc[1] / length, buf['info'][t, :, 1].double()])
            rec[:, row, ar] = torch.where(d, new, rec[:, row, ar])
            count += d.long()
            keep = 1.0 - buf['dones'][t].double()
            acc *= keep; length *= keep
    valid = (torch.arange(rounds, device=dev)[:, None] < count[None]).cpu()
    rec = rec.cpu()
    out = dict(episodes=int(valid.sum()))
    for k, name in enumerate(('reward', 'force', 'task_success')):
        v = rec[k][valid]
        out[name + '_mean'] = float(v.mean()) if v.numel() else float('nan')
        out[name + '_std'] = float(v.std(unbiased=False)) if v.numel() else float('nan')
    return out
