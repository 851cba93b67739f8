"""-m gpu: the camera on the device -- the frames kernel (agx_collider_frames) against the oracle's forward kinematics within float32 rounding
bounds, the ray caster (agx_render, csrc/agx_render.hip) against the float64 reference of tests/camera_ref.py fed the device's own frames, the
invariances of a render call, the scalar envs' camera calls and the BatchedCamera wrapper.

Worst error / bound ratios measured on an MI355X are recorded in profiles/camera/README.md."""
import numpy as np
import pytest
import torch

import camera_ref as R

pytestmark = pytest.mark.gpu

LIGHT, AMBIENT, DIFFUSE = (0.0, -3.0, 1.0), 0.8, 0.3      # the reference's defaults (env.py:354)


@pytest.fixture(scope='module')
def gpu():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()


_STATES = {}


def _states(model, coop, n, seed=7001):
    """post-reset states from the device's own reset (vec_env.build_reset_pool), once per model -> (blob, states, water or None)"""
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.vec_env import build_reset_pool
    if model not in _STATES:
        blob = ModelBlob.load(model)
        blob = blob.coop() if coop else blob
        st = build_reset_pool(blob, n, seed)
        _STATES[model] = (blob,) + (tuple(st) if isinstance(st, tuple) else (st, None))
    blob, st, extra = _STATES[model]
    assert len(st) >= n
    return blob, st[:n], None if extra is None else extra[:n]


def _mixed_gender_states():
    """FeedingJaco, environment 0 male and environment 1 female, forced through the reset's gender mode"""
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.libagx import Stepper
    if 'mixed' not in _STATES:
        blob = ModelBlob.load('feeding_jaco')
        st = Stepper(blob, 2)
        st.reset(seed=7101, gender='male')
        st.reset(mask=torch.tensor([0, 1], dtype=torch.uint8, device='cuda'), seed=7101, gender='female')
        torch.cuda.synchronize()
        _STATES['mixed'] = (blob, st.get_state(), None)
        st.close()
    return _STATES['mixed']


def _stepper(blob, states, water):
    from assistive_gym_amd.libagx import Stepper
    st = Stepper(blob, len(states))
    st.set_state(states)
    if water is not None:
        st.set_cloth(water)
    return st


def _frames(st, env0=0, count=None):
    count = st.n_envs - env0 if count is None else count
    out = torch.full((count, st.collider_count(), 12), float('nan'), device='cuda')
    st.collider_frames(out, env0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _render(st, h, w, env0=0, count=None, light=LIGHT, which=('depth', 'seg', 'rgba'), pad=1):
    """agx_render into buffers with `pad` extra images behind them, which must come back untouched -> dict of numpy arrays"""
    count = st.n_envs - env0 if count is None else count
    buf = dict(depth=torch.full((count + pad, h, w), -7.0, device='cuda'), seg=torch.full((count + pad, h, w), -7, dtype=torch.int32, device='cuda'),
               rgba=torch.full((count + pad, h, w, 4), 7, dtype=torch.uint8, device='cuda'))
    st.render(env0, count, light, AMBIENT, DIFFUSE, **{k: (buf[k][:count] if k in which else None) for k in buf})
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in buf.items()}
    for k, v in out.items():
        assert np.all(v[count:] == (7 if k == 'rgba' else -7)), 'agx_render wrote behind the last image (%s)' % k
        if k not in which:
            assert np.all(v == (7 if k == 'rgba' else -7)), 'agx_render wrote an output that was not asked for (%s)' % k
    return {k: v[:count] for k, v in out.items()}


# ---- stage A: the frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model,coop,n', [('feeding_jaco', False, 3), ('scratch_itch_pr2', True, 2), ('drinking_jaco', False, 2)], ids=lambda v: str(v))
def test_frames_against_the_oracle(gpu, model, coop, n):
    from oracle_lib import Oracle
    blob, states, water = _states(model, coop, 3 if model == 'feeding_jaco' else 2)
    st = _stepper(blob, states[:n], None if water is None else water[:n])
    assert st.collider_count() == blob.h['NCOLL']
    before = st.state_tensor().clone()
    got = _frames(st)
    assert torch.equal(st.state_tensor().view(torch.int32), before.view(torch.int32))
    part = _frames(st, 1, n - 1)
    assert np.array_equal(part.view(np.uint32), got[1:].view(np.uint32))          # a range is the rows of the whole
    st.close()
    oracle = Oracle(blob)
    worst_p, worst_r, moved = 0.0, 0.0, 0
    for e in range(n):
        want, levels, reach = R.ref_frames(blob, oracle, states[e])
        bp, br = R.frame_bounds(levels, reach)
        dp, dr = np.abs(got[e, :, :3] - want[:, :3]).max(1), np.abs(got[e, :, 3:] - want[:, 3:]).max(1)
        assert np.all(dp <= bp) and np.all(dr <= br), (model, e, float((dp / np.maximum(bp, 1e-300)).max()), float((dr / np.maximum(br, 1e-300)).max()))
        links = levels > 1
        worst_p = max(worst_p, float((dp[links] / bp[links]).max())); worst_r = max(worst_r, float((dr[br > 0] / br[br > 0]).max()))
        moved += int((dp[links] > 0).sum())
    print('%s: worst |frame error| / bound: position %.3g, rotation %.3g' % (model, worst_p, worst_r))
    assert moved > 0                                                              # the comparison saw float32 rounding, not a copy of the reference


# ---- stage B: the images ----------------------------------------------------------------------------------------------------------------------
def _image_case(name):
    if name == 'mixed_gender':
        blob, states, water = _mixed_gender_states()
        return blob, states, water, R.CASES['feeding_jaco']
    coop, n = {'feeding_jaco': (False, 3), 'scratch_itch_pr2': (True, 2), 'drinking_jaco': (False, 2)}[name]
    blob, states, water = _states(name, coop, n)
    return blob, states, water, (R.cup_camera(blob, states[0]) if name == 'drinking_jaco' else R.CASES[name])


@pytest.mark.parametrize('name', ['feeding_jaco', 'scratch_itch_pr2', 'drinking_jaco', 'mixed_gender'])
def test_images_against_the_reference(gpu, name):
    """seg equal, depth within 0.1 max_k |t_k - t_0| + 64 2^-24 max(1, t), rgba within 2 levels on the pixels where the reference's five rays agree;
    at most 5 % unsafe pixels, 10 % creases, at least 25 % hits per image (camera_ref.compare)"""
    from assistive_gym_amd.libagx import camera_colours
    blob, states, water, case = _image_case(name)
    n = len(states)
    st = _stepper(blob, states, water)
    st.camera_set(case['eye'], case['target'], fov=case['fov'], width=case['width'], height=case['height'])
    frames = _frames(st).astype(np.float64)
    img = _render(st, case['height'], case['width'])
    st.close()
    scene, cam, colours = R.Scene.of_blob(blob), R.Camera(**case), camera_colours()
    genders = blob.view(states)['gender']
    if name == 'mixed_gender':
        assert list(genders) == [0, 1]
    worst, seen_water = {}, 0
    for e in range(n):
        w = None if water is None else water[e, 0].astype(np.float64)
        five = R.render_five(scene, cam, frames[e], int(genders[e]), w)
        R.compare(scene, cam, five, colours, LIGHT, AMBIENT, DIFFUSE, img['depth'][e], img['seg'][e], img['rgba'][e], worst, '%s env %d' % (name, e))
        seen_water += int((img['seg'][e] >= scene.ncoll).sum())
        if name == 'mixed_gender':                                                 # each environment shows its own gender's human and not the other's
            rg = blob.meta['ranges']
            own, other = (rg['human_male'], rg['human_female']) if genders[e] == 0 else (rg['human_female'], rg['human_male'])
            s = img['seg'][e]
            assert ((s >= own[0]) & (s < own[1])).sum() > 0 and ((s >= other[0]) & (s < other[1])).sum() == 0
    print('%s: worst error / bound over %d images: depth %.3g, rgba %.3g' % (name, n, worst['depth'], worst['rgba']))
    assert np.all(img['rgba'][..., 3] == 255)
    if name == 'drinking_jaco':
        assert seen_water > 0, 'the camera near the cup sees no water particle'


# ---- invariances -------------------------------------------------------------------------------------------------------------------------------
def test_render_invariances(gpu):
    from assistive_gym_amd.libagx import camera_colours
    blob, states, _ = _states('feeding_jaco', False, 3)
    case = R.CASES['feeding_jaco']
    h, w = case['height'], case['width']
    st = _stepper(blob, states, None)
    st.camera_set(case['eye'], case['target'], fov=case['fov'], width=w, height=h)
    before = st.state_tensor().clone()
    full = _render(st, h, w)
    again = _render(st, h, w)
    part = _render(st, h, w, 1, 2)
    assert torch.equal(st.state_tensor().view(torch.int32), before.view(torch.int32))          # neither kernel writes the state records
    for k in full:
        assert np.array_equal(full[k].view(np.uint8), again[k].view(np.uint8)), k              # two calls are identical
        assert np.array_equal(part[k].view(np.uint8), full[k][1:3].view(np.uint8)), k          # environments [1, 3) = rows 1..2 of all
    for k in full:                                                                             # a null output leaves the others as they are
        one = _render(st, h, w, which=(k,))
        assert np.array_equal(one[k].view(np.uint8), full[k].view(np.uint8)), k
    assert (full['seg'] >= 0).mean() > 0.25 and len(np.unique(full['seg'])) > 5 and len(np.unique(full['rgba'].reshape(-1, 4), axis=0)) > 5
    # looking up at the sky: all background
    st.camera_set((0.0, 0.0, 3.0), (0.0, 0.5, 10.0), fov=40.0, width=w, height=h)
    sky = _render(st, h, w)
    bg = np.append(np.round(255.0 * camera_colours()[11].astype(np.float64)), 255).astype(np.uint8)
    assert np.all(sky['seg'] == -1) and np.all(sky['depth'] == np.float32(100.0))
    assert np.all(sky['rgba'] == sky['rgba'][0, 0, 0]) and np.abs(sky['rgba'][0, 0, 0].astype(int) - bg.astype(int)).max() <= 2      # one colour, the background's within the 2 levels of float32 shading
    # after 20 steps of a constant action the picture has changed
    st.camera_set(case['eye'], case['target'], fov=case['fov'], width=w, height=h)
    n = st.n_envs
    act = torch.full((n, st.act_dim), 0.5, device='cuda')
    obs, rew = torch.zeros((n, st.obs_dim), device='cuda'), torch.zeros(n, device='cuda')
    done, info = torch.zeros(n, dtype=torch.uint8, device='cuda'), torch.zeros((n, 8), device='cuda')
    for _ in range(20):
        st.step_dev(act, obs, rew, done, info)
    torch.cuda.synchronize()
    later = _render(st, h, w)
    for e in range(n):
        assert (later['seg'][e] != full['seg'][e]).sum() + (later['depth'][e] != full['depth'][e]).sum() > 0, e
    st.close()


def test_argument_checks_come_before_any_launch(gpu):
    blob, states, _ = _states('feeding_jaco', False, 3)
    st = _stepper(blob, states, None)
    d = torch.full((3, 36, 48), -7.0, device='cuda')
    v = (np.zeros(3, dtype=np.float32), np.array([0, 1, 0], dtype=np.float32), np.array([0, 0, 1], dtype=np.float32))
    ptr = lambda a: a.ctypes.data
    err = lambda: st.L.agx_last_error()
    assert st.L.agx_render(st.h, 0, 3, ptr(v[2]), 0.8, 0.3, d.data_ptr(), None, None, None) == -1 and b'agx_camera_set first' in err()
    cs = lambda eye, target, up, fov, w, h, near, far: st.L.agx_camera_set(st.h, eye, target, up, fov, w, h, near, far)
    for args, word in (((None, ptr(v[1]), ptr(v[2]), 60.0, 48, 36, 0.01, 100.0), b'null'), ((ptr(v[0]), ptr(v[0]), ptr(v[2]), 60.0, 48, 36, 0.01, 100.0), b'same point'),
                       ((ptr(v[0]), ptr(v[2]), ptr(v[2]), 60.0, 48, 36, 0.01, 100.0), b'up vector'), ((ptr(v[0]), ptr(v[1]), ptr(v[2]), 0.0, 48, 36, 0.01, 100.0), b'fov'),
                       ((ptr(v[0]), ptr(v[1]), ptr(v[2]), 180.0, 48, 36, 0.01, 100.0), b'fov'), ((ptr(v[0]), ptr(v[1]), ptr(v[2]), 60.0, 0, 36, 0.01, 100.0), b'width'),
                       ((ptr(v[0]), ptr(v[1]), ptr(v[2]), 60.0, 48, 9000, 0.01, 100.0), b'width'), ((ptr(v[0]), ptr(v[1]), ptr(v[2]), 60.0, 48, 36, 0.0, 100.0), b'near'),
                       ((ptr(v[0]), ptr(v[1]), ptr(v[2]), 60.0, 48, 36, 1.0, 1.0), b'near'), ((ptr(v[0]), ptr(v[1]), ptr(v[2]), float('nan'), 48, 36, 0.01, 100.0), b'fov')):
        assert cs(*args) == -1 and word in err(), (args, err())
    assert cs(ptr(v[0]), ptr(v[1]), ptr(v[2]), 60.0, 48, 36, 0.01, 100.0) == 0
    rd = lambda env0, count, light, depth: st.L.agx_render(st.h, env0, count, light, 0.8, 0.3, depth, None, None, None)
    for args, word in (((-1, 1, ptr(v[2]), d.data_ptr()), b'range'), ((0, 4, ptr(v[2]), d.data_ptr()), b'range'), ((2, 2, ptr(v[2]), d.data_ptr()), b'range'),
                       ((0, 0, ptr(v[2]), d.data_ptr()), b'range'), ((0, 3, None, d.data_ptr()), b'null light'), ((0, 3, ptr(v[0]), d.data_ptr()), b'light vector'),
                       ((0, 3, ptr(v[2]), None), b'outputs are null')):
        assert rd(*args) == -1 and word in err(), (args, err())
    f = torch.full((3, st.collider_count(), 12), -7.0, device='cuda')
    assert st.L.agx_collider_frames(st.h, 0, 4, f.data_ptr(), None) == -1 and b'range' in err()
    assert st.L.agx_collider_frames(st.h, 0, 3, None, None) == -1 and b'null output' in err()
    torch.cuda.synchronize()
    assert bool((d == -7.0).all()) and bool((f == -7.0).all())
    st.close()


# ---- the scalar envs and the wrapper ------------------------------------------------------------------------------------------------------------
def test_facade_camera(gpu):
    from assistive_gym_amd.envs import make
    env = make('assistive_gym:FeedingJaco-v1')
    env.seed(3)
    env.reset()
    env.setup_camera(camera_width=48, camera_height=36)
    img, depth = env.get_camera_image_depth()
    assert img.shape == (36, 48, 4) and img.dtype == np.uint8 and len(np.unique(img.reshape(-1, 4), axis=0)) > 5 and np.all(img[..., 3] == 255)
    assert depth.shape == (36, 48) and depth.min() >= 0.0 and depth.max() <= 1.0 and (depth < 1.0).sum() > 0.25 * depth.size
    img_dark, _ = env.get_camera_image_depth(light_pos=[0, -3, 1], shadow=True, ambient=0.2, diffuse=0.3, specular=0.5)
    assert img_dark[..., :3].astype(int).sum() < img[..., :3].astype(int).sum()
    env.setup_camera_rpy(camera_width=40, camera_height=30)
    img2, depth2 = env.get_camera_image_depth()
    assert img2.shape == (30, 40, 4) and depth2.shape == (30, 40) and (depth2 < 1.0).sum() > 0.25 * depth2.size and len(np.unique(img2.reshape(-1, 4), axis=0)) > 5
    obs, rew, done, info = env.step(np.zeros(env.action_robot_len))             # the camera does not disturb the environment
    assert np.isfinite(obs).all() and env.render() is None
    env.disconnect()


def test_batched_camera(gpu):
    from assistive_gym_amd.camera import BatchedCamera, collider_info
    from assistive_gym_amd.vec_env import FeedingJacoVecEnv
    env = FeedingJacoVecEnv(64, pool_size=8, seed=5)
    env.reset()
    camera = BatchedCamera(env, 33, 17)
    out = camera.render()
    assert out['depth'].shape == (64, 17, 33) and out['depth'].dtype == torch.float32 and out['seg'].shape == (64, 17, 33) and out['seg'].dtype == torch.int32
    assert out['rgba'].shape == (64, 17, 33, 4) and out['rgba'].dtype == torch.uint8 and all(v.device == env.device for v in out.values())
    sub = camera.render([5, 6, 7, 40, 2])
    assert sub['depth'].shape == (5, 17, 33)
    for k in out:
        assert torch.equal(sub[k], out[k][[5, 6, 7, 40, 2]]), k
    seg = out['seg'].cpu().numpy()
    tags = {collider_info(env.blob, i)[0] for i in np.unique(seg) if i >= 0}
    assert 3 in tags and len(tags) >= 3 and collider_info(env.blob, -1) is None      # the human and at least two other kinds of thing are in the picture
    camera.setup_rpy(distance=2.0)
    far = camera.render(range(2))
    assert far['depth'].shape == (2, 17, 33) and not torch.equal(far['depth'], out['depth'][:2])
    env.close()
