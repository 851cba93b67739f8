"""agx_policy_act and agx_gae on the device (csrc/agx_policy.hip) against float64 references, with tolerances propagated from float32 rounding.

Forward: a float64 forward of the same parameters, with a bound carried along: per layer e_out = |W| e_in + (K + 2) u (|W||h| + |b|), u = 2^-24,
K the fan-in, and + 4 u |y| per tanh / exp.  The kernel returns action, logp and value, not mean and log_std themselves, so
  * mean is read from a deterministic call (action == mean there) and held to e_mean, value to e_value;
  * the clamped log_std enters the deterministic logp with coefficient 1 per component (logp = -sum_k log_std_k - A ln(2 pi) / 2), held to
    sum_k e_logstd,k + A 8 u max(1, |logp|), and the sampled action component by component through sigma;
  * eps is the restated recipe's (tests/policy_recipe.py); the kernel's implied eps = (action - mean) / sigma must agree within e_eps = 2e-5
    (r <= 5.9 times a trigonometric argument error of a few roundings of 2 pi 2^-24, plus <= 4 ulp each in log, sqrt, sin, cos) -- plus what the
    division itself amplifies: |eps| e_logstd and the rounding of the two actions over sigma;
  * action within e_mean + sigma (|eps| e_logstd + e_eps) + u |action|, logp within sum_k(|eps_k| e_eps + e_logstd,k) + A 8 u max(1, |logp|).
"""
import math

import numpy as np
import pytest
import torch

from policy_recipe import policy_eps

U = 2.0 ** -24
E_EPS = 2e-5
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


@pytest.fixture(scope='module')
def agx():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()
    return libagx


def _make_params(dims, rng):
    """[(W, b)] x 6 in the order pi.0, pi.2, pi.4, vf.0, vf.2, vf.4 (float32): weights N(0, 1) / sqrt(fan_in); biases of +-25 on the first log_std outputs"""
    o, ha, hb, a = dims
    layers = []
    for out, inp in ((ha, o), (hb, ha), (2 * a, hb), (ha, o), (hb, ha), (1, hb)):
        layers.append(((rng.randn(out, inp) / math.sqrt(inp)).astype(np.float32), (0.1 * rng.randn(out)).astype(np.float32)))
    b = layers[2][1]
    b[a] = 25.0                                   # log_std of component 0: clamped to 2
    if a > 1:
        b[a + 1] = -25.0                          # component 1: clamped to -20
    return layers


def _flat(layers):
    return np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in layers])


def _branch(layers, obs):
    """float64 forward of one branch and the float32 rounding bound of its output"""
    h, e = obs.astype(np.float64), np.zeros_like(obs, dtype=np.float64)
    for i, (w, b) in enumerate(layers):
        w, b, k = w.astype(np.float64), b.astype(np.float64), w.shape[1]
        y = h @ w.T + b
        e = e @ np.abs(w).T + (k + 2) * U * (np.abs(h) @ np.abs(w).T + np.abs(b))
        if i < len(layers) - 1:
            h = np.tanh(y)
            e = e + 4 * U * np.abs(h)             # (tanh is 1-Lipschitz)
        else:
            h = y
    return h, e


def _reference(layers, dims, obs):
    a = dims[3]
    out, e_out = _branch(layers[:3], obs)
    value, e_value = _branch(layers[3:], obs)
    mean, e_mean = out[:, :a], e_out[:, :a]
    log_std, e_ls = np.clip(out[:, a:], -20.0, 2.0), e_out[:, a:] + 4 * U      # (the clamp is 1-Lipschitz; + the rounding of exp, as a log_std error)
    return mean, e_mean, log_std, e_ls, value[:, 0], e_value[:, 0]


def _call(agx, flat, dims, obs, n, seed=7, env_offset=0, step=3, deterministic=False):
    o, ha, hb, a = dims
    action = torch.full((n, a), float('nan'), device='cuda')
    logp, value = torch.full((n,), float('nan'), device='cuda'), torch.full((n,), float('nan'), device='cuda')
    agx.policy_act(flat, o, ha, hb, a, obs, n, seed, env_offset, step, action, logp, value, deterministic=deterministic, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return action.cpu().numpy().astype(np.float64), logp.cpu().numpy().astype(np.float64), value.cpu().numpy().astype(np.float64)


DIMS = [(25, 100, 100, 7), (1, 1, 1, 1), (128, 128, 128, 32), (87, 100, 100, 24), (25, 100, 100, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize('dims', DIMS, ids=lambda d: 'x'.join(map(str, d)))
def test_forward_parity(agx, dims):
    E = agx.POLICY_TILE
    rng = np.random.RandomState(sum(dims))
    layers = _make_params(dims, rng)
    flat = torch.from_numpy(_flat(layers)).cuda()
    seed, step = 1234567, 9
    worst = dict(mean=0.0, value=0.0, logp_det=0.0, eps=0.0, action=0.0, logp=0.0)
    for n in (1, E - 1, E, E + 1, 2 * E + 2):
        obs_h = (3.0 * rng.randn(n, dims[0])).astype(np.float32)              # N(0, 3): the tanh layers saturate
        obs = torch.from_numpy(obs_h).cuda()
        mean, e_mean, log_std, e_ls, value, e_value = _reference(layers, dims, obs_h)
        a = dims[3]
        if a > 1:
            assert (log_std[:, 0] == 2.0).all() and (log_std[:, 1] == -20.0).all()       # both clamps are hit
        sigma = np.exp(log_std)
        eps = policy_eps(seed, 0, n, [step], a)[:, 0]
        # deterministic: action == mean, logp = -sum log_std - A ln(2 pi) / 2
        act_d, logp_d, val_d = _call(agx, flat, dims, obs, n, seed, 0, step, deterministic=True)
        want_ld = -log_std.sum(-1) - a * HALF_LOG_2PI
        tol_ld = e_ls.sum(-1) + a * 8 * U * np.maximum(1.0, np.abs(want_ld))
        act_s, logp_s, val_s = _call(agx, flat, dims, obs, n, seed, 0, step)
        want_a = mean + sigma * eps
        tol_a = e_mean + sigma * (np.abs(eps) * e_ls + E_EPS) + U * np.abs(want_a)
        want_l = (-0.5 * eps * eps - log_std - HALF_LOG_2PI).sum(-1)
        tol_l = (np.abs(eps) * E_EPS + e_ls).sum(-1) + a * 8 * U * np.maximum(1.0, np.abs(want_l))
        implied = (act_s - act_d) / sigma
        tol_e = E_EPS + np.abs(eps) * e_ls + U * (np.abs(act_s) + np.abs(act_d)) / sigma
        checks = dict(mean=(act_d, mean, e_mean), value=(val_d, value, e_value), logp_det=(logp_d, want_ld, tol_ld), eps=(implied, eps, tol_e),
                      action=(act_s, want_a, tol_a), logp=(logp_s, want_l, tol_l))
        for name, (got, want, tol) in checks.items():
            ratio = float((np.abs(got - want) / tol).max())
            worst[name] = max(worst[name], ratio)
            print('%s n=%d %s: max |error| / bound = %.3f (largest bound %.2e)' % ('x'.join(map(str, dims)), n, name, ratio, float(np.max(tol))))
        assert np.array_equal(val_s, val_d)
        for name, (got, want, tol) in checks.items():
            assert np.isfinite(got).all(), name
            assert (np.abs(got - want) <= tol).all(), (name, n, float((np.abs(got - want) / tol).max()))
    assert worst['mean'] > 0.0 or dims == (1, 1, 1, 1)                         # (the comparison is not vacuous: float32 and float64 differ)


@pytest.mark.gpu
def test_strided_slices_leave_other_columns_untouched(agx):
    dims, n = (25, 100, 100, 7), 35
    rng = np.random.RandomState(5)
    flat = torch.from_numpy(_flat(_make_params(dims, rng))).cuda()
    wide_obs = torch.from_numpy((3.0 * rng.randn(n, 40)).astype(np.float32)).cuda()
    obs = wide_obs[:, 5:30]
    a0, l0, v0 = _call(agx, flat, dims, obs.contiguous(), n)
    wide_act = torch.full((n, 20), 123.0, device='cuda')
    logp, value = torch.empty(n, device='cuda'), torch.empty(n, device='cuda')
    agx.policy_act(flat, *dims, obs, n, 7, 0, 3, wide_act[:, 3:10], logp, value, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert obs.data_ptr() != wide_obs.data_ptr() and obs.stride(0) == 40
    w = wide_act.cpu().numpy()
    assert (w[:, :3] == 123.0).all() and (w[:, 10:] == 123.0).all()
    assert np.array_equal(w[:, 3:10].astype(np.float64), a0) and np.array_equal(logp.cpu().numpy().astype(np.float64), l0) and np.array_equal(value.cpu().numpy().astype(np.float64), v0)


@pytest.mark.gpu
def test_noise_is_reproducible_and_addressed_by_the_global_env_index(agx):
    dims, n = (25, 100, 100, 7), 36
    rng = np.random.RandomState(6)
    layers = _make_params(dims, rng)
    layers[2][1][7:9] = 0.0                                                    # no clamped log_std here: every component carries visible noise
    flat = torch.from_numpy(_flat(layers)).cuda()
    obs = torch.from_numpy((3.0 * rng.randn(n, 25)).astype(np.float32)).cuda()
    a0, l0, v0 = _call(agx, flat, dims, obs, n, seed=11, step=4)
    a1, l1, v1 = _call(agx, flat, dims, obs, n, seed=11, step=4)
    assert np.array_equal(a0, a1) and np.array_equal(l0, l1) and np.array_equal(v0, v1)
    h = n // 2
    lo = _call(agx, flat, dims, obs[:h], h, seed=11, env_offset=0, step=4)
    hi = _call(agx, flat, dims, obs[h:], n - h, seed=11, env_offset=h, step=4)
    for whole, x, y in zip((a0, l0, v0), lo, hi):
        assert np.array_equal(whole, np.concatenate([x, y]))
    a2, l2, _ = _call(agx, flat, dims, obs, n, seed=11, step=5)
    a3, l3, _ = _call(agx, flat, dims, obs, n, seed=12, step=4)
    for other_a, other_l in ((a2, l2), (a3, l3)):
        assert (other_a != a0).any(axis=1).all() and (other_l != l0).all()       # every row changes
    ad, ld, vd = _call(agx, flat, dims, obs, n, seed=11, step=4, deterministic=True)
    ad2, _, _ = _call(agx, flat, dims, obs, n, seed=99, step=77, deterministic=True)
    assert np.array_equal(ad, ad2) and np.array_equal(vd, v0)                  # deterministic: no noise, whatever the address


@pytest.mark.gpu
def test_deterministic_action_is_the_mean(agx):
    """deterministic=1 against the float32 torch module the parameters came from: action == mean of the kernel's own forward exactly (eps = 0 adds
    nothing) -- the float64 reference bounds it in test_forward_parity; here: the module's flat_params drive the kernel and the two agree"""
    from assistive_gym_amd.rollout import GaussianMLPPolicy
    torch.manual_seed(0)
    pi = GaussianMLPPolicy(25, 7).cuda()
    obs = torch.randn(33, 25, device='cuda')
    act, logp, value = _call(agx, pi.flat_params(), (25, 100, 100, 7), obs, 33, deterministic=True)
    with torch.no_grad():
        mean, log_std, v = pi(obs)
    np.testing.assert_allclose(act, mean.cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(value, v.cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(logp, (-log_std.sum(-1) - 7 * HALF_LOG_2PI).cpu().numpy(), rtol=0, atol=1e-4)
    # and a sampled action is mean + sigma eps of the recipe, i.e. log_prob of the module reproduces the kernel's logp
    act_s, logp_s, _ = _call(agx, pi.flat_params(), (25, 100, 100, 7), obs, 33, seed=5, step=1)
    with torch.no_grad():
        lp, _ = pi.log_prob(obs, torch.from_numpy(act_s).float().cuda())
    np.testing.assert_allclose(logp_s, lp.cpu().numpy(), rtol=0, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize('T,N', [(1, 1), (12, 65), (7, 130)])
def test_gae_matches_the_python_loop(agx, T, N):
    from assistive_gym_amd.rollout import gae, gae_loop
    rng = np.random.RandomState(T * 1000 + N)
    r, v = rng.randn(T, N).astype(np.float32), (3.0 * rng.randn(T + 1, N)).astype(np.float32)
    d = (rng.rand(T, N) < 0.2).astype(np.uint8)
    d[:, 0] = 1                                                                # done at every step
    if N > 1:
        d[:, 1] = 0                                                            # never done
    gamma, lam = 0.99, 0.95
    want_adv, want_ret = gae_loop(torch.from_numpy(r).double(), torch.from_numpy(v).double(), torch.from_numpy(d), gamma, lam)
    adv, ret = gae(torch.from_numpy(r).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(d).cuda(), gamma, lam)
    assert adv.is_cuda and adv.dtype == torch.float32 and adv.shape == (T, N)
    terms = max(float(np.abs(r).max()), float(np.abs(v).max()), float(want_adv.abs().max()), float(want_ret.abs().max()))
    tol = T * 4 * U * terms
    err = max(float((adv.cpu().double() - want_adv).abs().max()), float((ret.cpu().double() - want_ret).abs().max()))
    print('T=%d N=%d: max |error| %.3e, bound %.3e' % (T, N, err, tol))
    assert err <= tol
    assert torch.equal(adv[:, 0].cpu().double(), (torch.from_numpy(r[:, 0]).double() - torch.from_numpy(v[:-1, 0]).double()).float().double())   # done every step: no bootstrap, no carry
