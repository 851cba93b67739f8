"""The PPO learner, its checkpoints, the evaluator and the command line on the CPU (assistive_gym_amd/ppo.py, learn.py), and what can be checked of
agx_policy_act / agx_gae without a device: their argument checks and the noise recipe the device test (test_gpu_policy_kernel.py) holds the kernel to."""
import copy
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from policy_recipe import policy_eps            # noqa: E402  (tests/policy_recipe.py: the numpy restatement of the kernel's noise)


class ToyEnv:
    """64 envs; the observation is a target uniform in [-1, 1]^2, redrawn every step as a function of (seed, step index); reward
    -||clip(a, -1, 1) - obs||^2; done every 8 steps.  The surface of a vec env that rollout.collect / ppo read."""
    episode_len = 8

    def __init__(self, n_envs=64, seed=0):
        self.n_envs, self.device, self.obs_dim, self.act_dim, self.seed, self.env_offset = n_envs, torch.device('cpu'), 2, 2, seed, 0
        self.t = 0
        self.obs = self._draw()

    def _draw(self):
        g = torch.Generator(); g.manual_seed(self.seed * 1000003 + self.t)
        return torch.rand((self.n_envs, 2), generator=g) * 2.0 - 1.0

    def reset(self):
        self.obs = self._draw()      # the target of the current step once more: a reset does not move the env in time
        return self.obs

    def step(self, actions):
        reward = -((actions.clamp(-1.0, 1.0) - self.obs) ** 2).sum(-1)
        self.t += 1
        done = torch.full((self.n_envs,), 1 if self.t % self.episode_len == 0 else 0, dtype=torch.uint8)
        info = torch.zeros((self.n_envs, 8))
        info[:, 0] = -reward                                   # 'total_force_on_human'
        info[:, 1] = (reward > -0.5).float()                   # 'task_success'
        self.obs = self._draw()
        return self.obs, reward, done, info


def _toy_cfg():
    from assistive_gym_amd.ppo import PPOConfig
    return PPOConfig(horizon=8, num_sgd_iter=8, sgd_minibatch_size=128, lr=1e-3)


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
def test_ppo_loss_matches_the_formulas_in_float64():
    from assistive_gym_amd.ppo import PPOConfig, ppo_loss
    from assistive_gym_amd.rollout import GaussianMLPPolicy
    torch.manual_seed(3)
    cfg = PPOConfig()
    pi = GaussianMLPPolicy(3, 2, hidden=(5, 4)).double()
    with torch.no_grad():
        pi.pi[-1].weight.mul_(100.0)                           # undo the small final layer: means and log_stds of some size
        pi.pi[-1].bias.copy_(torch.tensor([0.2, -0.1, -0.3, 0.4], dtype=torch.float64))
    obs = torch.randn(6, 3, dtype=torch.float64)
    with torch.no_grad():
        mean, log_std, v = pi(obs)
    # the behaviour policy: shifted means and log_stds (non-zero KL), actions placed so that the ratios fall on both sides of the clip range
    old_mean, old_log_std = mean + torch.tensor([[0.3, -0.2]], dtype=torch.float64), log_std + torch.tensor([[0.1, -0.15]], dtype=torch.float64)
    z = torch.tensor([[0.1, 0.2], [2.5, -2.0], [-1.5, 1.0], [0.0, 0.0], [3.0, 3.0], [-0.5, 0.4]], dtype=torch.float64)
    actions = mean + log_std.exp() * z
    logp_old = (-0.5 * ((actions - old_mean) / old_log_std.exp()) ** 2 - old_log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    adv = torch.tensor([1.0, -2.0, 0.5, -0.3, 1.5, -1.0], dtype=torch.float64)
    values = v + torch.tensor([0.5, -0.5, 25.0, 0.1, -0.2, 0.3], dtype=torch.float64)    # the third: a value error beyond vf_clip_param = 10
    ret = v + torch.tensor([1.0, -30.0, 2.0, 0.0, 0.5, -0.5], dtype=torch.float64)
    batch = dict(obs=obs, actions=actions, logp=logp_old, adv=adv, ret=ret, values=values, old_mean=old_mean, old_log_std=old_log_std)
    loss, terms = ppo_loss(pi, batch, cfg, 0.2)
    # numpy, from the formulas
    m, ls, vv, a = mean.numpy(), log_std.numpy(), v.numpy(), actions.numpy()
    om, ols = old_mean.numpy(), old_log_std.numpy()
    logp = (-0.5 * ((a - m) / np.exp(ls)) ** 2 - ls - 0.5 * np.log(2 * np.pi)).sum(-1)
    ratio = np.exp(logp - logp_old.numpy())
    assert (ratio > 1.0 + cfg.clip_param).any() and (ratio < 1.0 - cfg.clip_param).any() and ((ratio > 0.7) & (ratio < 1.3)).any()
    surrogate = np.minimum(adv.numpy() * ratio, adv.numpy() * np.clip(ratio, 1 - cfg.clip_param, 1 + cfg.clip_param)).mean()
    kl = (ls - ols + (np.exp(2 * ols) + (om - m) ** 2) / (2 * np.exp(2 * ls)) - 0.5).sum(-1).mean()
    assert kl > 1e-3
    vf1 = (vv - ret.numpy()) ** 2
    diff = vv - values.numpy()
    assert (np.abs(diff) > cfg.vf_clip_param).any()
    vf2 = (values.numpy() + np.clip(diff, -cfg.vf_clip_param, cfg.vf_clip_param) - ret.numpy()) ** 2
    vf = np.maximum(vf1, vf2).mean()
    ent = (ls + 0.5 * np.log(2 * np.pi * np.e)).sum(-1).mean()
    want = -surrogate + 0.2 * kl + cfg.vf_loss_coeff * vf - cfg.entropy_coeff * ent
    assert abs(float(loss.detach()) - want) < 1e-6
    for k, w in (('surrogate', surrogate), ('kl', kl), ('vf_loss', vf), ('entropy', ent)):
        assert abs(float(terms[k].detach()) - w) < 1e-6, k
    # the same in float32, the learner's precision (looser: float32 rounding of six-sample means of O(100) terms)
    loss32, _ = ppo_loss(copy.deepcopy(pi).float(), {k: x.float() for k, x in batch.items()}, cfg, 0.2)
    assert abs(float(loss32.detach()) - want) < 1e-3 * max(1.0, abs(want))


def test_kl_coefficient_adapts_in_both_directions():
    from assistive_gym_amd.ppo import PPOConfig, adapt_kl_coeff
    cfg = PPOConfig()
    assert cfg.kl_coeff == 0.2 and cfg.kl_target == 0.01 and cfg.lr == 5e-5 and cfg.clip_param == 0.3 and cfg.lam == 0.95 and cfg.gamma == 0.99
    assert (cfg.num_sgd_iter, cfg.sgd_minibatch_size, cfg.train_batch_size) == (50, 128, 19200) and cfg.vf_clip_param == 10.0
    assert adapt_kl_coeff(0.2, 0.021, cfg) == pytest.approx(0.3)
    assert adapt_kl_coeff(0.2, 0.0049, cfg) == pytest.approx(0.1)
    assert adapt_kl_coeff(0.2, 0.01, cfg) == 0.2 and adapt_kl_coeff(0.2, 0.02, cfg) == 0.2 and adapt_kl_coeff(0.2, 0.005, cfg) == 0.2
    b = PPOConfig.batched(4096)
    assert b.steps_per_iteration(4096) * 4096 == b.train_batch_size and b.sgd_minibatch_size > 128 and b.num_sgd_iter < 50


# ---- learning ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_learns_the_toy_environment(seed):
    """mean step reward over the last 3 of 30 iterations >= -0.3 (the untrained policy scores about -1.5)"""
    from assistive_gym_amd.ppo import PPOTrainer
    torch.set_num_threads(min(4, torch.get_num_threads()))
    tr = PPOTrainer(ToyEnv(64, seed), _toy_cfg(), seed=seed)
    means = []
    for _ in range(30):
        r = tr.train()
        means.append(r['episode_reward_mean'] / ToyEnv.episode_len)
    print('seed %d: mean step reward, first iteration %.3f, last three %.3f' % (seed, means[0], np.mean(means[-3:])))
    assert means[0] < -1.0
    assert r['timesteps_total'] == 30 * 64 * 8 and r['training_iteration'] == 30
    assert np.mean(means[-3:]) >= -0.3


def test_checkpoint_round_trip_is_bit_identical(tmp_path):
    from assistive_gym_amd.ppo import PPOTrainer, latest_checkpoint, checkpoint_dir, remove_checkpoint
    a = PPOTrainer(ToyEnv(64, 5), _toy_cfg(), seed=7)
    for _ in range(2):
        a.train()
    a.kl_coeffs[0] = 0.45                                     # something a fresh trainer does not have
    d = checkpoint_dir(str(tmp_path), 'ppo', 'Toy-v1')
    path = a.save(d)
    assert path == os.path.join(str(tmp_path), 'ppo', 'Toy-v1', 'checkpoint_2', 'checkpoint-2.pt') and os.path.isfile(path)
    assert latest_checkpoint(str(tmp_path), 'ppo', 'Toy-v1') == path and latest_checkpoint(path) == path
    env_b = copy.deepcopy(a.env)
    b = PPOTrainer(env_b, _toy_cfg(), seed=99)               # another seed: everything that matters must come from the checkpoint
    b.restore(path)
    for pa, pb in zip(a.policies.parameters(), b.policies.parameters()):
        assert torch.equal(pa, pb)
    assert b.kl_coeff == 0.45 and (b.training_iteration, b.timesteps_total, b.steps_done) == (2, 1024, 16) and b.time_total_s == a.time_total_s
    assert b.seed == a.seed
    ra, rb = a.train(), b.train()
    for pa, pb in zip(a.policies.parameters(), b.policies.parameters()):
        assert torch.equal(pa, pb)
    for k in ('training_iteration', 'timesteps_total', 'episode_reward_mean', 'episode_reward_min', 'episode_reward_max'):
        assert ra[k] == rb[k], k
    assert ra['learner'] == rb['learner'] and a.kl_coeff == b.kl_coeff
    # the newest checkpoint of a directory is found, the previous one removed (learn.py:49-56,89-93)
    path3 = a.save(d)
    assert latest_checkpoint(str(tmp_path), 'ppo', 'Toy-v1') == path3
    remove_checkpoint(path)
    assert not os.path.exists(os.path.dirname(path)) and os.path.isfile(path3)


def test_evaluate_scripted_policy():
    """a policy whose mean is the constant (0.25, -2) -- clipped to (0.25, -1) by the env -- evaluated deterministically: the statistics by hand"""
    from assistive_gym_amd.ppo import evaluate
    from assistive_gym_amd.rollout import GaussianMLPPolicy
    pi = GaussianMLPPolicy(2, 2)
    with torch.no_grad():
        for p in pi.parameters():
            p.zero_()
        pi.pi[-1].bias.copy_(torch.tensor([0.25, -2.0, 0.0, 0.0]))
    env = ToyEnv(64, 11)
    stats = evaluate(env, pi, 100, seed=0, deterministic=True)            # 100 episodes on 64 envs: two whole episodes of every env
    ref = ToyEnv(64, 11)
    a = torch.tensor([0.25, -1.0])
    rew = np.zeros((16, 64)); succ = np.zeros((16, 64))
    for t in range(16):
        r = -((a - ref.obs) ** 2).sum(-1)
        rew[t], succ[t] = r.numpy(), (r > -0.5).numpy()
        ref.step(torch.tensor([[0.25, -2.0]]).expand(64, 2))
    ep = rew.reshape(2, 8, 64).sum(1).reshape(-1)
    force = (-rew).reshape(2, 8, 64).mean(1).reshape(-1)
    last = succ.reshape(2, 8, 64)[:, -1].reshape(-1)
    assert stats['episodes'] == 128
    for name, v in (('reward', ep), ('force', force), ('task_success', last)):
        assert stats[name + '_mean'] == pytest.approx(v.mean(), abs=1e-5), name
        assert stats[name + '_std'] == pytest.approx(v.std(), abs=1e-5), name
    assert 0.0 < stats['task_success_mean'] < 1.0 and stats['reward_std'] > 0.1


# ---- command line --------------------------------------------------------------------------------------------------------------------------
def test_command_line_parses_the_reference_flags():
    from assistive_gym_amd.learn import build_parser
    a = build_parser().parse_args(['--env', 'FeedingJaco-v1', '--algo', 'ppo', '--seed', '3', '--train', '--evaluate', '--train-timesteps', '5000', '--save-dir', '/x',
                                   '--load-policy-path', '/y', '--eval-episodes', '7', '--verbose', '--n-envs', '64', '--reset', 'device', '--deterministic'])
    assert (a.env, a.algo, a.seed, a.train, a.evaluate, a.train_timesteps, a.save_dir, a.load_policy_path, a.eval_episodes, a.verbose) == \
        ('FeedingJaco-v1', 'ppo', 3, True, True, 5000, '/x', '/y', 7, True)
    assert (a.n_envs, a.reset, a.deterministic) == (64, 'device', True)
    d = build_parser().parse_args([])
    assert (d.algo, d.seed, d.train, d.evaluate, d.train_timesteps, d.save_dir, d.load_policy_path, d.eval_episodes) == \
        ('ppo', 1, False, False, 1000000, './trained_models/', './trained_models/', 100)


@pytest.mark.parametrize('module', ['assistive_gym.learn', 'assistive_gym_amd.learn'])
def test_command_line_refuses_what_is_not_built(module):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'assistive_gym_amd', 'shim'), ROOT]))
    for flags, word in ((['--algo', 'sac', '--train'], 'sac'), (['--render'], '--render')):
        p = subprocess.run([sys.executable, '-m', module, '--env', 'FeedingJaco-v1'] + flags, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode != 0
        lines = [ln for ln in p.stderr.strip().splitlines() if ln.strip()]
        assert len(lines) == 1 and word in lines[0] and 'not built' in lines[0], p.stderr


# ---- the C ABI entries without a device -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from assistive_gym_amd.build import build
    build()
    from assistive_gym_amd import libagx
    return libagx.load()


def _act_args(obs=25, ha=100, hb=100, act=7, obs_stride=25, n=4, action_stride=7, null=None):
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    ptrs = {k: (None if k == null else p) for k in ('params', 'obs', 'action', 'logp', 'value')}
    return [ptrs['params'], obs, ha, hb, act, ptrs['obs'], obs_stride, n, 1, 0, 0, 0, ptrs['action'], action_stride, ptrs['logp'], ptrs['value'], None]


def test_policy_act_and_gae_argument_checks(lib):
    """every limit of include/agx.h is checked before any device call: AGX_E_ARG = -1 with or without a GPU; the host pointers of this test
    are never dereferenced"""
    E_ARG = -1
    for bad in (dict(obs=0), dict(obs=129, obs_stride=129), dict(ha=0), dict(ha=129), dict(hb=0), dict(hb=129), dict(act=0), dict(act=33, action_stride=33),
                dict(obs_stride=24), dict(action_stride=6), dict(n=-1), dict(null='params'), dict(null='obs'), dict(null='action'), dict(null='logp'), dict(null='value')):
        assert lib.agx_policy_act(*_act_args(**bad)) == E_ARG, bad
    assert lib.agx_policy_act(*_act_args(n=0)) == 0                      # nothing to do: AGX_OK without a launch
    assert lib.agx_policy_act(*_act_args(obs=128, obs_stride=128, ha=128, hb=128, act=32, action_stride=32, n=0)) == 0
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.agx_gae(p, p, p, -1, 4, 0.99, 0.95, p, p, None) == E_ARG
    assert lib.agx_gae(p, p, p, 4, -1, 0.99, 0.95, p, p, None) == E_ARG
    for k in range(5):
        a = [p] * 5; a[k] = None
        assert lib.agx_gae(a[0], a[1], a[2], 4, 4, 0.99, 0.95, a[3], a[4], None) == E_ARG
    assert lib.agx_gae(p, p, p, 0, 4, 0.99, 0.95, p, p, None) == 0 and lib.agx_gae(p, p, p, 4, 0, 0.99, 0.95, p, p, None) == 0


def test_policy_act_and_gae_have_no_cpu_path(lib):
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    assert lib.agx_policy_act(*_act_args()) == -4                        # AGX_E_NOGPU
    assert lib.agx_gae(p, p, p, 4, 4, 0.99, 0.95, p, p, None) == -4
    from assistive_gym_amd import libagx
    with pytest.raises(libagx.AgxError, match='no HIP device'):
        libagx.gae(torch.zeros(2, 3), torch.zeros(3, 3), torch.zeros(2, 3, dtype=torch.uint8), 0.99, 0.95, torch.zeros(2, 3), torch.zeros(2, 3))


def test_flat_params_layout():
    from assistive_gym_amd.rollout import GaussianMLPPolicy
    torch.manual_seed(0)
    pi = GaussianMLPPolicy(5, 3, hidden=(4, 6))
    with torch.no_grad():
        for p in pi.parameters():
            p.add_(torch.randn_like(p))
    flat = pi.flat_params()
    want = [pi.pi[0].weight, pi.pi[0].bias, pi.pi[2].weight, pi.pi[2].bias, pi.pi[4].weight, pi.pi[4].bias,
            pi.vf[0].weight, pi.vf[0].bias, pi.vf[2].weight, pi.vf[2].bias, pi.vf[4].weight, pi.vf[4].bias]
    assert flat.dtype == torch.float32 and flat.numel() == sum(w.numel() for w in want)
    assert torch.equal(flat, torch.cat([w.detach().reshape(-1) for w in want]))
    assert [tuple(w.shape) for w in want[:6:2]] == [(4, 5), (6, 4), (6, 6)]       # [out][in], the last: 2 x act_dim rows
    assert pi.fits_kernel() and not GaussianMLPPolicy(129, 3).fits_kernel() and not GaussianMLPPolicy(5, 33).fits_kernel() and not GaussianMLPPolicy(5, 3, hidden=(4,)).fits_kernel()


# ---- the noise recipe ----------------------------------------------------------------------------------------------------------------------
def test_noise_recipe_statistics():
    """eps[env, step, k] of the restated recipe over 64 envs x 32 steps x 8 components: standard normal, and uncorrelated along every axis"""
    eps = policy_eps(seed=12345, env_offset=0, n_envs=64, steps=range(32), act_dim=8)          # [64, 32, 8]
    assert eps.shape == (64, 32, 8) and np.isfinite(eps).all()
    n = eps.size
    assert abs(eps.mean()) < 4.0 / math.sqrt(n)
    assert abs(eps.var() - 1.0) < 0.05
    for axis in (2, 1, 0):                                                                     # across k, across step, across envs
        a, b = np.take(eps, range(0, eps.shape[axis] - 1), axis=axis), np.take(eps, range(1, eps.shape[axis]), axis=axis)
        corr = ((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std())
        assert abs(corr) < 4.0 / math.sqrt(a.size), (axis, corr)
    # addressing: env i of a batch at offset o is env o + i of the whole; another seed or step is another stream
    assert np.array_equal(policy_eps(12345, 32, 32, range(32), 8), eps[32:])
    assert not np.array_equal(policy_eps(12346, 0, 64, range(32), 8)[:, 1:], eps[:, 1:])
    assert np.array_equal(policy_eps(12345, 0, 64, [5], 8)[:, 0], eps[:, 5])
