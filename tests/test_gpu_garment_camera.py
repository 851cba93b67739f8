"""-m gpu: the garment of a dressing scene in the camera's images (agx_camera_garment, agx_render_garment_kernel of csrc/agx_render.hip) against the
float64 reference of tests/garment_ref.py fed the device's own collider frames: the gown of two records of the committed dressing trajectory under
the sleeve camera, synthetic sheets placed by hand (free, half behind colliders, folded, through the near plane, degenerate, sub-pixel with list
flushes, an image whose tiles end inside it), the invariances of a render call with the garment on and off, a record the cloth kernel has just
written, and the Python surface.  tests/test_garment_cpu.py checks the caps of every comparison here on the reference alone.

Worst error / bound ratios measured on an MI355X are recorded in profiles/garment_camera/README.md."""
import os

import numpy as np
import pytest
import torch

import camera_ref as R
import garment_ref as G
from test_gpu_camera import AMBIENT, DIFFUSE, LIGHT, _frames, _render

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FACES = 7673


@pytest.fixture(scope='module')
def gpu():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()


@pytest.fixture(scope='module')
def dr():
    from assistive_gym_amd.blob import ModelBlob
    return ModelBlob.load('dressing_baxter')


def _stepper(blob, states, cloth):
    from assistive_gym_amd.libagx import Stepper
    st = Stepper(blob, len(states))
    st.set_state(np.ascontiguousarray(states, dtype=np.float32))
    st.set_cloth(cloth)
    return st


def _gender(blob, state):
    return int(blob.view(np.asarray(state, dtype=np.float32).reshape(1, -1))['gender'][0])


# ---- 1. the real garment -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('record', [0, 5])
def test_gown_against_the_reference(gpu, dr, record):
    """face-exact: seg equal, depth within 0.1 max_k |t_k - t_0| + 64 2^-24 max(1, t), rgba within 2 levels on the pixels where the reference's five
    rays agree on the segmentation value, a face index included (garment_ref.compare)"""
    g = np.load(os.path.join(GOLDEN, 'bridge_dump_dressingbaxter.npz'))
    state, cloth = g['states'][record].copy(), g['cloth'][record].copy()
    case = G.sleeve_camera(dr, cloth[0])
    st = _stepper(dr, state[None], cloth[None])
    st.camera_set(case['eye'], case['target'], fov=case['fov'], width=case['width'], height=case['height'])
    st.camera_garment(True)
    frames = _frames(st).astype(np.float64)
    img = _render(st, case['height'], case['width'])
    tris = st.garment_faces()
    st.close()
    assert np.array_equal(tris, G.faces(dr)) and len(tris) == FACES
    scene, cam = R.Scene.of_blob(dr), R.Camera(**case)
    five = G.render_five(scene, cam, frames[0], _gender(dr, state), cloth[0], tris)
    worst = {}
    G.compare(scene, cam, five, LIGHT, AMBIENT, DIFFUSE, img['depth'][0], img['seg'][0], img['rgba'][0], worst, 'gown record %d' % record)
    assert (img['seg'] >= scene.ncoll).mean() > 0.10 and img['seg'].max() < scene.ncoll + FACES and np.all(img['rgba'][..., 3] == 255)


# ---- 2. synthetic sheets -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', G.SHEETS)
def test_sheets_against_the_reference(gpu, name):
    s = G.sheet_setup(name)
    blob, view, x = s['blob'], s['view'], s['x']
    cloth = np.zeros((1, 2, len(x), 3), dtype=np.float32)      # velocities 0, nothing stepped
    cloth[0, 0] = x
    st = _stepper(blob, s['state'][None], cloth)
    st.camera_set(view['eye'], view['target'], fov=view['fov'], width=view['width'], height=view['height'], near=s['near'])
    off = _render(st, view['height'], view['width'])
    st.camera_garment(True)
    frames = _frames(st).astype(np.float64)
    img = _render(st, view['height'], view['width'])
    assert np.array_equal(st.garment_faces(), s['tris'])
    st.close()
    ncoll = blob.h['NCOLL']
    assert off['seg'].max() < ncoll
    if name == 'line':      # zero-area faces: the image is the garment-off image, bit for bit
        for k in img:
            assert np.array_equal(img[k].view(np.uint8), off[k].view(np.uint8)), k
        return
    scene, cam = R.Scene.of_blob(blob), R.Camera(near=s['near'], **view)
    five = G.render_five(scene, cam, frames[0], _gender(blob, s['state']), x, s['tris'])
    worst = {}
    G.compare(scene, cam, five, LIGHT, AMBIENT, DIFFUSE, img['depth'][0], img['seg'][0], img['rgba'][0], worst, name, s['subpixel'])
    seg, depth = img['seg'][0], img['depth'][0]
    assert seg.max() < ncoll + len(s['tris']) and (seg >= ncoll).mean() >= G.MIN_GARMENT
    assert np.all(depth[seg >= ncoll] >= np.float32(s['near']))                                # no hit before the near plane
    keep = seg < ncoll                                                                          # where no face won, the rigid image is untouched
    assert np.array_equal(seg[keep], off['seg'][0][keep]) and np.array_equal(depth[keep].view(np.uint32), off['depth'][0][keep].view(np.uint32))
    assert np.all(depth[~keep] <= off['depth'][0][~keep])


# ---- 3. invariances ----------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_garment_invariances(gpu, dr):
    from assistive_gym_amd.vec_env import build_reset_pool
    states, cloth = build_reset_pool(dr, 3, 7301)
    cloth = np.ascontiguousarray(cloth[:3], dtype=np.float32)
    st = _stepper(dr, states[:3], cloth)
    ncoll, h, w = dr.h['NCOLL'], 36, 48
    st.camera_set((0.5, -0.75, 1.5), (-0.2, 0.0, 0.75), fov=60.0, width=w, height=h)
    state0, cloth0 = st.state_tensor().clone(), st.cloth_tensor().clone()
    off = _render(st, h, w)
    st.camera_garment(True)
    on = _render(st, h, w)
    st.camera_garment(False)
    assert _same(_render(st, h, w), off)                                                       # off again: bit-equal to before the first switch
    st.camera_garment(True)
    assert _same(_render(st, h, w), on)
    rigid, gar = on['seg'] < ncoll, on['seg'] >= ncoll
    assert gar.reshape(3, -1).any(1).all() and on['seg'].max() < ncoll + FACES and off['seg'].max() < ncoll
    for k in on:                                                                               # a pixel no face won is the garment-off pixel
        assert np.array_equal(on[k][rigid].view(np.uint8), off[k][rigid].view(np.uint8)), k
    assert np.all(on['depth'][gar] <= off['depth'][gar])                                       # a face wins only by being nearer
    part = _render(st, h, w, 1, 2)
    for k in on:
        assert np.array_equal(part[k].view(np.uint8), on[k][1:3].view(np.uint8)), k            # environments [1, 3) = rows 1..2 of all
    for k in on:                                                                               # outputs not asked for and the padding stay untouched (_render)
        one = _render(st, h, w, which=(k,))
        assert np.array_equal(one[k].view(np.uint8), on[k].view(np.uint8)), k
    assert torch.equal(st.state_tensor().view(torch.int32), state0.view(torch.int32)) and torch.equal(st.cloth_tensor().view(torch.int32), cloth0.view(torch.int32))
    # environment 1's garment 1 km away: no garment pixel there, nothing changes in the others
    moved = cloth.copy()
    moved[1, 0] += np.float32(1000.0)
    st.set_cloth(moved)
    away = _render(st, h, w)
    assert (away['seg'][1] >= ncoll).sum() == 0 and _same({k: v[1] for k, v in away.items()}, {k: v[1] for k, v in off.items()})
    assert _same({k: v[[0, 2]] for k, v in away.items()}, {k: v[[0, 2]] for k, v in on.items()})
    # NaN in a handful of environment 2's nodes: the call returns, the others are bit-equal, environment 2 stays finite and in range
    broken = cloth.copy()
    nodes = np.unique(on['seg'][2][on['seg'][2] >= ncoll] - ncoll)[:3]                         # faces that are in the picture
    tris = st.garment_faces()
    broken[2, 0, tris[nodes].reshape(-1)[:5]] = np.nan
    broken[2, 0, 7] = np.inf
    st.set_cloth(broken)
    nan = _render(st, h, w)
    assert _same({k: v[:2] for k, v in nan.items()}, {k: v[:2] for k, v in on.items()})
    assert np.isfinite(nan['depth'][2]).all() and nan['seg'][2].min() >= -1 and nan['seg'][2].max() < ncoll + FACES
    hit_faces = np.unique(nan['seg'][2][nan['seg'][2] >= ncoll] - ncoll)
    assert np.isfinite(broken[2, 0][tris[hit_faces]]).all()                                    # no face with a node that is not finite is hit
    assert (nan['seg'][2] >= ncoll).sum() > 0 and not np.array_equal(nan['seg'][2], on['seg'][2])
    st.close()


# ---- 4. a record the cloth kernel has just written -----------------------------------------------------------------------------------------------
def test_live_record_after_a_step(gpu, dr):
    from assistive_gym_amd.vec_env import DressingBaxterVecEnv
    env = DressingBaxterVecEnv(2, pool_size=2, seed=7401)
    env.reset()
    st = env.stepper
    before = st.get_cloth()
    case = G.sleeve_camera(dr, before[0, 0])
    st.camera_set(case['eye'], case['target'], fov=case['fov'], width=case['width'], height=case['height'])
    st.camera_garment(True)
    pre = _render(st, case['height'], case['width'])
    act = torch.zeros((2, st.act_dim), device=env.device)
    act[:, :3] = 1.0
    env.step(act)
    torch.cuda.synchronize()
    after, states = st.get_cloth(), st.get_state()
    assert np.abs(after[:, 0] - before[:, 0]).max() > 1e-4
    post = _render(st, case['height'], case['width'])
    assert not np.array_equal(post['depth'][0], pre['depth'][0]) and not np.array_equal(post['seg'][0], pre['seg'][0])      # the picture follows the record
    scene, tris, worst = R.Scene.of_blob(dr), st.garment_faces(), {}
    for e in range(2):      # each environment under the sleeve camera of its own garment
        case = G.sleeve_camera(dr, after[e, 0])
        st.camera_set(case['eye'], case['target'], fov=case['fov'], width=case['width'], height=case['height'])
        frames = _frames(st, e, 1).astype(np.float64)
        img = _render(st, case['height'], case['width'], e, 1)
        five = G.render_five(scene, R.Camera(**case), frames[0], _gender(dr, states[e]), after[e, 0], tris)
        G.compare(scene, R.Camera(**case), five, LIGHT, AMBIENT, DIFFUSE, img['depth'][0], img['seg'][0], img['rgba'][0], worst, 'live env %d' % e)
    env.close()


# ---- 5. the surface --------------------------------------------------------------------------------------------------------------------------------
def test_batched_camera_and_scalar_env(gpu, dr):
    from assistive_gym_amd.camera import BatchedCamera, collider_info
    from assistive_gym_amd.envs import make
    from assistive_gym_amd.libagx import camera_garment_colour
    from assistive_gym_amd.vec_env import DressingBaxterVecEnv
    env = DressingBaxterVecEnv(2, pool_size=2, seed=7501)
    env.reset()
    ncoll = dr.h['NCOLL']
    plain = BatchedCamera(env, 64, 48).render()
    assert int((plain['seg'] >= ncoll).sum()) == 0                                              # the default: no garment
    camera = BatchedCamera(env, 64, 48, garment=True)
    out = camera.render()
    seg = out['seg'].cpu().numpy()
    assert out['seg'].shape == (2, 48, 64) and (seg >= ncoll).reshape(2, -1).any(1).all() and seg.max() < ncoll + FACES
    assert collider_info(dr, int(seg.max())) == ('garment', int(seg.max()) - ncoll, -1)
    camera.set_garment(False)
    assert all(torch.equal(v, plain[k]) for k, v in camera.render().items())
    assert int((BatchedCamera(env, 64, 48, garment=False).render()['seg'] >= ncoll).sum()) == 0
    env.close()
    # the scalar env: the gown's colour, at the shades of the camera's formula, is in the frame with garment=True and not without
    col = camera_garment_colour().astype(np.float64)
    shades = {tuple(np.round(255.0 * np.minimum(1.0, col * (0.8 + 0.3 * k / 3000.0))).astype(int)) for k in range(3001)}
    count = lambda img: sum(tuple(int(v) for v in p) in shades for p in img[..., :3].reshape(-1, 3))
    scalar = make('assistive_gym:DressingBaxter-v1')
    scalar.seed(9)
    scalar.reset()
    scalar.setup_camera(camera_width=64, camera_height=48)
    without, _ = scalar.get_camera_image_depth()
    scalar.setup_camera(camera_width=64, camera_height=48, garment=True)
    img, depth = scalar.get_camera_image_depth()
    assert img.shape == (48, 64, 4) and count(img) > 20 and count(without) == 0
    scalar.setup_camera_rpy(camera_width=40, camera_height=30, garment=True)
    assert count(scalar.get_camera_image_depth()[0]) > 0
    scalar.disconnect()


def test_models_without_a_garment_and_argument_checks(gpu, dr):
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.libagx import AgxError, Stepper
    for model in ('feeding_jaco', 'drinking_jaco'):
        st = Stepper(ModelBlob.load(model), 1)
        assert st.garment_faces().shape == (0, 3)                                               # needs no camera
        st.camera_set((0.5, -0.75, 1.5), (-0.2, 0.0, 0.75), width=16, height=12)
        with pytest.raises(AgxError, match=r'\(-1\).*no garment'):
            st.camera_garment(True)
        st.camera_garment(False)                                                                # switching off what is off is no error
        st.close()
    st = Stepper(dr, 1)
    assert np.array_equal(st.garment_faces(), G.faces(dr))                                      # before any camera
    with pytest.raises(AgxError, match=r'\(-1\).*agx_camera_set first'):
        st.camera_garment(True)
    with pytest.raises(AgxError, match=r'\(-1\).*agx_camera_set first'):
        st.camera_garment(False)
    assert st.L.agx_garment_faces(st.h, None, None) == -1 and b'null count' in st.L.agx_last_error()
    st.close()
