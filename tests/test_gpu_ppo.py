"""The fused rollout (rollout.collect with a seed: one agx_policy_act launch per policy and step), the trainer and the evaluator on the device."""
import numpy as np
import pytest
import torch

from assistive_gym_amd.rollout import GaussianMLPPolicy, collect


@pytest.fixture(scope='module')
def gpu():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()


def _replay(env2, buf):
    """the rollout is what the env produces step by step from the recorded actions"""
    for t in range(buf['obs'].shape[0]):
        assert torch.equal(env2.obs, buf['obs'][t])
        _, rew, _, _ = env2.step(buf['actions'][t].contiguous())
        assert torch.equal(rew, buf['rewards'][t])


@pytest.mark.gpu
def test_fused_collect(gpu):
    from assistive_gym_amd.vec_env import FeedingJacoVecEnv
    n, T = 128, 4
    env = FeedingJacoVecEnv(n, pool_size=32, seed=5)
    env.reset()
    pool = env.pool_host.copy()
    torch.manual_seed(1)
    pi = GaussianMLPPolicy(env.obs_dim, env.act_dim).to(env.device)
    buf = collect(env, pi, T, seed=3)
    assert buf['obs'].shape == (T, n, 25) and buf['actions'].shape == (T, n, 7) and buf['logp'].shape == (T, n) and buf['values'].shape == (T + 1, n)
    assert all(torch.isfinite(buf[k]).all() for k in ('obs', 'actions', 'logp', 'rewards', 'values', 'info'))
    assert float(buf['actions'].std()) > 0.5                                  # sampled (sigma = 1 at initialisation), not the mean
    env2 = FeedingJacoVecEnv(n, pool_size=32, seed=5)
    env2.set_pool(pool)
    env2.reset()
    _replay(env2, buf)
    with torch.no_grad():
        lp, v = pi.log_prob(buf['obs'].reshape(T * n, -1), buf['actions'].reshape(T * n, -1))
    assert float((lp.reshape(T, n) - buf['logp']).abs().max()) < 1e-4
    assert float((v.reshape(T, n) - buf['values'][:T]).abs().max()) < 1e-4
    # the same trajectory whatever the layout: two half batches at env_offset 0 and 64 reproduce the rows of the whole
    for off in (0, 64):
        half = FeedingJacoVecEnv(64, pool_size=32, seed=5)
        half.set_pool(pool)
        half.reset(env_offset=off)
        hb = collect(half, pi, T, seed=3)
        for k in ('obs', 'actions', 'logp', 'rewards'):
            assert torch.equal(hb[k], buf[k][:, off:off + 64]), (off, k)
        assert torch.equal(hb['values'][:T], buf['values'][:T, off:off + 64])
        half.close()
    # another seed: other actions; no seed: the torch path, as before
    env2.reset()
    other = collect(env2, pi, 1, seed=4)
    assert not torch.equal(other['actions'][0], buf['actions'][0]) and torch.equal(other['obs'][0], buf['obs'][0])
    env.close(); env2.close()


@pytest.mark.gpu
def test_trainer_on_feeding_jaco(gpu, tmp_path):
    from assistive_gym_amd.ppo import PPOConfig, PPOTrainer, evaluate, latest_checkpoint, checkpoint_dir
    from assistive_gym_amd.vec_env import FeedingJacoVecEnv
    env = FeedingJacoVecEnv(64, pool_size=32, seed=5)
    cfg = PPOConfig(horizon=8, num_sgd_iter=2, sgd_minibatch_size=256)
    tr = PPOTrainer(env, cfg, seed=2, env_name='FeedingJaco-v1')
    before = [p.detach().clone() for p in tr.policies.parameters()]
    for _ in range(2):
        r = tr.train()
        for terms in r['learner']:
            assert all(np.isfinite(v) for v in terms.values()), terms
    assert r['timesteps_total'] == 1024 and r['training_iteration'] == 2 and r['time_rollout_s'] > 0 and r['time_learn_s'] > 0
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.policies.parameters()))
    path = tr.save(checkpoint_dir(str(tmp_path), 'ppo', 'FeedingJaco-v1'))
    assert latest_checkpoint(str(tmp_path), 'ppo', 'FeedingJaco-v1') == path
    tr2 = PPOTrainer(env, cfg, seed=9, env_name='FeedingJaco-v1')
    tr2.restore(path)
    for a, b in zip(tr.policies.parameters(), tr2.policies.parameters()):
        assert torch.equal(a, b)
    assert tr2.timesteps_total == 1024 and tr2.kl_coeff == tr.kl_coeff and tr2.seed == 2
    stats = evaluate(env, tr2.policies, 1, seed=0)                            # one episode (200 steps) of each of the 64 envs
    assert stats['episodes'] == 64 and all(np.isfinite(v) for v in stats.values()), stats
    assert 0.0 <= stats['task_success_mean'] <= 1.0 and stats['force_mean'] >= 0.0
    env.close()


@pytest.mark.gpu
def test_coop_collect(gpu):
    from assistive_gym_amd.vec_env import ScratchItchPR2HumanVecEnv
    n, T = 64, 3
    env = ScratchItchPR2HumanVecEnv(n, pool_size=32, seed=5)
    env.reset()
    b = env.blob
    o_r, a_r = b.obs_dim_robot, b.act_dim_robot
    torch.manual_seed(1)
    pis = (GaussianMLPPolicy(o_r, a_r).to(env.device), GaussianMLPPolicy(env.obs_dim - o_r, env.act_dim - a_r).to(env.device))
    buf = collect(env, pis, T, seed=3)
    assert buf['actions'].shape == (T, n, env.act_dim) and buf['logp'].shape == (2, T, n) and buf['values'].shape == (2, T + 1, n)
    assert all(torch.isfinite(buf[k]).all() for k in ('obs', 'actions', 'logp', 'rewards', 'values'))
    assert float(buf['actions'][:, :, :a_r].std()) > 0.5 and float(buf['actions'][:, :, a_r:].std()) > 0.5       # both agents' columns are filled
    assert not torch.equal(buf['actions'][:, :, 0], buf['actions'][:, :, a_r])                                    # ... from streams of their own
    for a, (pi, oc, ac) in enumerate(((pis[0], slice(0, o_r), slice(0, a_r)), (pis[1], slice(o_r, None), slice(a_r, None)))):
        with torch.no_grad():
            lp, _ = pi.log_prob(buf['obs'][:, :, oc].reshape(T * n, -1), buf['actions'][:, :, ac].reshape(T * n, -1))
        assert float((lp.reshape(T, n) - buf['logp'][a]).abs().max()) < 1e-4
    env2 = ScratchItchPR2HumanVecEnv(n, pool_size=32, seed=5)
    env2.set_pool(env.pool_host.copy())
    env2.reset()
    _replay(env2, buf)
    env.close(); env2.close()
