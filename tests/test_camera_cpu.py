"""The camera without a device: the view and ray conventions (assistive_gym_amd/camera.py), the float64 ray caster the device images are held to
(tests/camera_ref.py) on scenes with known answers, its caps on the three task scenes, the host-side plane builder (csrc/agx_hull.h) against
model/cloth.py hull_planes, and the argument checks of the C ABI entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_ref as R
from assistive_gym_amd import camera as cam
from assistive_gym_amd.blob import ModelBlob
from assistive_gym_amd.model.cloth import hull_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


# ---- view and rays -----------------------------------------------------------------------------------------------------------------------------
def test_view_matrix_closed_forms():
    b = cam.view_from_eye((0, -2, 1), (0, 0, 1))                   # looking along +y, z up
    assert np.allclose(b, [[1, 0, 0], [0, 0, 1], [0, 1, 0]], atol=1e-15)
    b = cam.view_from_eye(cam.DEFAULT_EYE, cam.DEFAULT_TARGET)
    f = np.array(cam.DEFAULT_TARGET) - np.array(cam.DEFAULT_EYE)
    assert np.allclose(b[2], f / np.linalg.norm(f)) and np.allclose(b @ b.T, np.eye(3), atol=1e-14)
    assert abs(b[0][2]) < 1e-15 and b[1][2] > 0 and np.allclose(np.cross(b[0], b[1]), -b[2])      # right is horizontal, up points up, right-handed with -forward
    # yaw, pitch, roll: yaw 0 looks along +y from behind; pitch -90 looks straight down from above; yaw 90 turns the camera to look along -x
    eye, target, up = cam.view_from_rpy((1, 2, 3), 2.0, 0, 0, 0)
    assert np.allclose(eye, (1, 0, 3)) and np.allclose(up, (0, 0, 1)) and np.allclose(target, (1, 2, 3))
    eye, target, up = cam.view_from_rpy((1, 2, 3), 2.0, 0, -90, 0)
    assert np.allclose(eye, (1, 2, 5)) and np.allclose(up, (0, 1, 0))
    eye, target, up = cam.view_from_rpy((0, 0, 0), 1.0, 90, 0, 0)
    assert np.allclose(eye, (1, 0, 0)) and np.allclose(up, (0, 0, 1))
    eye, target, up = cam.view_from_rpy((-0.2, 0, 0.75), 1.5, 40, -35, 0)                          # the reference's default (env.py:348)
    assert np.isclose(np.linalg.norm(eye - target), 1.5) and np.isclose(eye[2] - 0.75, 1.5 * np.sin(np.radians(35)))


def test_pixel_rays_and_depth_buffer():
    b = cam.view_from_eye((0, -2, 1), (0, 0, 1))
    w, h, fov = 6, 4, 60.0
    d = cam.pixel_rays(b, fov, w, h)
    t = np.tan(np.radians(30.0))
    assert d.shape == (h, w, 3)
    for i, j in ((0, 0), (5, 3), (2, 1)):
        want = ((2 * (i + 0.5) / w - 1) * t * w / h) * b[0] + ((1 - 2 * (j + 0.5) / h) * t) * b[1] + b[2]
        assert np.allclose(d[j, i], want, atol=1e-15)
    assert np.allclose(d @ b[2], 1.0)                              # the depth along the view direction is the ray parameter
    assert d[0, 0] @ b[1] > 0 > d[3, 0] @ b[1] and d[0, 0] @ b[0] < 0 < d[0, 5] @ b[0]      # row 0 is the top, column 0 the left
    assert np.allclose(cam.pixel_rays(b, fov, w, h, di=0.5)[:, :-1], 0.5 * (d[:, :-1] + d[:, 1:]))
    assert cam.bullet_depth(cam.NEAR) == 0.0 and np.isclose(cam.bullet_depth(cam.FAR), 1.0) and 0 < cam.bullet_depth(1.0) < 1
    assert np.isclose(cam.bullet_depth(2.0), 100.0 * 1.99 / (2.0 * 99.99))


# ---- the reference on scenes with known answers -----------------------------------------------------------------------------------------------
def _frames(*positions):
    return np.array([np.concatenate([np.asarray(p, dtype=np.float64), np.eye(3).reshape(9)]) for p in positions])


def _col(verts, radius, tag=1):
    return dict(verts=np.asarray(verts, dtype=np.float64).reshape(-1, 3), radius=radius, tag=tag, body=-1)


def _centre_and_grid(n=41):
    c = R.Camera((0, -2, 0), (0, 0, 0), fov=60.0, width=n, height=n)
    return c, c.rays().reshape(n, n, 3)


def test_reference_sphere():
    c, d = _centre_and_grid()
    sc = R.Scene([_col([[0, 0, 0]], 0.25)])
    t, idx, nrm, face = R.cast(sc, _frames((0, 0, 0)), 0, c.eye, d.reshape(-1, 3))
    t, idx, nrm = t.reshape(41, 41), idx.reshape(41, 41), nrm.reshape(41, 41, 3)
    assert idx[20, 20] == 0 and np.isclose(t[20, 20], 1.75) and np.allclose(nrm[20, 20], (0, -1, 0))
    # every hit lies on the sphere, with the outward normal; a ray hits iff it passes within the radius of the centre
    hit = idx >= 0
    x = c.eye + t[..., None] * d
    assert np.allclose(np.linalg.norm(x[hit], axis=1), 0.25) and np.allclose(nrm[hit], x[hit] / 0.25)
    dist = np.linalg.norm(np.cross(d, -c.eye), axis=2) / np.linalg.norm(d, axis=2)
    assert np.array_equal(hit, dist <= 0.25) and 0 < hit.sum() < hit.size
    assert np.all(t[~hit] == c.far)
    # seen from inside the near plane's reach: the eye inside the sphere sees its far side, the normal still outward
    t2, idx2, n2, _ = R.cast(sc, _frames((0, -2, 0)), 0, c.eye, d[20, 20][None])
    assert idx2[0] == 0 and np.isclose(t2[0], 0.25) and np.allclose(n2[0], (0, 1, 0))


def test_reference_capsule_side_on_and_end_on():
    c, d = _centre_and_grid()
    side = R.Scene([_col([[-0.3, 0, 0], [0.3, 0, 0]], 0.1)])
    t, idx, nrm, _ = R.cast(side, _frames((0, 0, 0)), 0, c.eye, d.reshape(-1, 3))
    t, idx, nrm = t.reshape(41, 41), idx.reshape(41, 41), nrm.reshape(41, 41, 3)
    assert idx[20, 20] == 0 and np.isclose(t[20, 20], 1.9) and np.allclose(nrm[20, 20], (0, -1, 0))
    x = c.eye + t[..., None] * d
    hit = idx >= 0
    seg_dist = np.linalg.norm(x - np.clip(x * [1, 0, 0], -0.3, 0.3), axis=2)          # distance from the segment
    assert np.allclose(seg_dist[hit], 0.1) and hit[20].sum() > hit[:, 20].sum() > 0      # wider than tall
    end = R.Scene([_col([[0, -0.3, 0], [0, 0.3, 0]], 0.1)])
    t, idx, nrm, _ = R.cast(end, _frames((0, 0, 0)), 0, c.eye, d.reshape(-1, 3))
    t, idx = t.reshape(41, 41), idx.reshape(41, 41)
    assert idx[20, 20] == 0 and np.isclose(t[20, 20], 2.0 - 0.3 - 0.1)                  # the near cap
    hit = idx >= 0
    assert abs(int(hit[20].sum()) - int(hit[:, 20].sum())) <= 0 and np.array_equal(hit, hit.T)      # a disc
    x = c.eye + t[..., None] * d
    assert np.allclose(np.linalg.norm((x - np.clip(x * [0, 1, 0], -0.3, 0.3))[hit], axis=1), 0.1)


def test_reference_box_face_on_and_inside_the_near_plane():
    c, d = _centre_and_grid()
    corners = [[sx * 0.3, sy * 0.2, sz * 0.1] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    box = R.Scene([_col(corners, 0.01)])
    assert len(box.planes[0]) == 6
    t, idx, nrm, face = R.cast(box, _frames((0, 0, 0)), 0, c.eye, d.reshape(-1, 3))
    hit = idx >= 0
    # the face towards the camera is the plane y = -0.21 (pushed out by the radius): constant depth 1.79 wherever the front face is what is seen
    front = hit & (np.abs(nrm[:, 1] + 1) < 1e-12)
    assert front.sum() > 20 and np.allclose(t[front], 1.79) and len(set(face[front])) == 1
    x = c.eye + t[:, None] * d.reshape(-1, 3)
    assert np.all(np.abs(x[front, 0]) <= 0.31 + 1e-12) and np.all(np.abs(x[front, 2]) <= 0.11 + 1e-12)
    # the projected rectangle: |x| <= 0.31, |z| <= 0.11 at depth 1.79
    dd = d.reshape(-1, 3)
    assert np.array_equal(front, (np.abs(dd[:, 0]) * 1.79 <= 0.31) & (np.abs(dd[:, 2]) * 1.79 <= 0.11))
    # a flat vertex set is its bounding box
    flat = R.Scene([_col([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], 0.05)])
    assert len(flat.planes[0]) == 6
    # the hull reaches through the near plane: the eye is inside the box, the hit is where the ray leaves it, with that face's outward normal
    t, idx, nrm, face = R.cast(box, _frames((0, -2.0, 0)), 0, c.eye, d[20, 20][None])
    assert idx[0] == 0 and np.isclose(t[0], 0.21) and np.allclose(nrm[0], (0, 1, 0))
    # ... and a box that starts behind the near plane but before the eye's depth 0.01: entry below near, so the exit is the hit
    t, idx, nrm, face = R.cast(box, _frames((0, -2.0 + 0.215, 0)), 0, c.eye, d[20, 20][None])
    assert idx[0] == 0 and np.isclose(t[0], 0.425) and np.allclose(nrm[0], (0, 1, 0))
    # ties go to the lower index; a gender mask hides a collider
    two = R.Scene([_col([[0, 0, 0]], 0.25), _col([[0, 0, 0]], 0.25)], genders=[2, 3])
    assert R.cast(two, _frames((0, 0, 0), (0, 0, 0)), 1, c.eye, d[20, 20][None])[1][0] == 0
    assert R.cast(two, _frames((0, 0, 0), (0, 0, 0)), 0, c.eye, d[20, 20][None])[1][0] == 1


# ---- the caps of the image comparison, on the reference alone ------------------------------------------------------------------------------
def _golden_state(model):
    if model == 'drinking_jaco':
        g = np.load(os.path.join(GOLDEN, 'bridge_dump_drinkingjaco.npz'))
        return ModelBlob.load(model), g['states'][0].copy(), g['cloth'][0, 0].astype(np.float64)
    if model == 'scratch_itch_pr2':
        g = np.load(os.path.join(GOLDEN, 'scratch_itch_pr2_coop_oracle_traj.npz'))
        return ModelBlob.load(model).coop(), g['state0'].copy(), None
    g = np.load(os.path.join(GOLDEN, 'feeding_jaco_oracle_traj.npz'))
    return ModelBlob.load(model), g['state0'].copy(), None


@pytest.mark.parametrize('model', ['feeding_jaco', 'scratch_itch_pr2', 'drinking_jaco'])
def test_caps_hold_on_the_reference_alone(model):
    """the cameras and sizes of tests/test_gpu_camera.py on a committed state of each scene: unsafe pixels, creases and hits within the caps"""
    from oracle_lib import Oracle
    blob, state, water = _golden_state(model)
    frames, _, _ = R.ref_frames(blob, Oracle(blob), state)
    scene = R.Scene.of_blob(blob)
    c = R.Camera(**(R.cup_camera(blob, state) if model == 'drinking_jaco' else R.CASES[model]))
    gender = int(blob.view(state.reshape(1, -1))['gender'][0])
    five = R.render_five(scene, c, frames, gender, water)
    R.check_caps(five, model)
    if water is not None:
        assert (five[0][1] >= scene.ncoll).sum() > 0, 'no water particle is visible'


# ---- the host plane builder --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planes_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp('camera_planes')
    so = str(d / 'libplanes.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-I' + os.path.join(ROOT, 'assistive_gym_amd', 'csrc'), '-o', so,
                           os.path.join(ROOT, 'tests', 'camera_planes', 'planes_main.cpp')])
    L = C.CDLL(so)
    L.agx_test_hull_planes.restype = C.c_int
    L.agx_test_grown_bound.restype = C.c_double
    return L


def _cxx_planes(L, verts):
    v = np.ascontiguousarray(verts, dtype=np.float32)
    out = np.zeros((512, 4))
    n = L.agx_test_hull_planes(v.ctypes.data_as(C.c_void_p), C.c_int(len(v)), out.ctypes.data_as(C.c_void_p), C.c_int(512))
    assert 0 < n <= 512
    return out[:n].copy()


def _hulls(model):
    blob = ModelBlob.load(model)
    return [blob.collider(c) for c in range(blob.h['NCOLL']) if len(blob.collider(c)['verts']) >= 3]


# two planes are the same plane when they agree within twice the grid hull_planes itself merges facets on (normals to 1e-5, offsets to 1e-6)
N_TOL, OFF_TOL = 2e-5, 2e-6


@pytest.mark.parametrize('model', ['feeding_jaco', 'dressing_baxter'])
def test_plane_builder_matches_hull_planes(planes_lib, model):
    hulls = _hulls(model)
    assert len(hulls) > 20
    boxes = 0
    for k, col in enumerate(hulls):
        want, got = hull_planes(col['verts']), _cxx_planes(planes_lib, col['verts'])
        for a, b, what in ((want, got, 'missing'), (got, want, 'extra')):
            for p in a:
                near = (np.abs(b[:, :3] - p[:3]).max(1) <= N_TOL) & (np.abs(b[:, 3] - p[3]) <= OFF_TOL)
                assert near.any(), (model, k, what, p)
        assert np.allclose(np.linalg.norm(got[:, :3], axis=1), 1.0, atol=1e-12)
        v = col['verts']
        assert np.all(v @ got[:, :3].T - got[:, 3] <= 1e-7 * max(1.0, np.abs(v).max()))      # every vertex behind every plane
        boxes += len(want) == 6 and np.allclose(np.abs(want[:, :3]).max(1), 1.0) and len(v) <= 4
        # the bounding radius of the grown polytope holds the vertices grown by the radius
        centre = 0.5 * (v.min(0) + v.max(0))
        vf = np.ascontiguousarray(v, dtype=np.float32)
        b = planes_lib.agx_test_grown_bound(vf.ctypes.data_as(C.c_void_p), C.c_int(len(vf)), C.c_double(col['radius']), centre.ctypes.data_as(C.c_void_p))
        assert b >= np.linalg.norm(v - centre, axis=1).max() + col['radius'] - 1e-9
    print('%s: %d hulls, %d of them flat (bounding boxes)' % (model, len(hulls), boxes))


def test_plane_builder_degenerate_sets(planes_lib):
    flat = [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]]
    for verts in (flat, flat[:3], [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]):
        got, want = _cxx_planes(planes_lib, verts), hull_planes(verts)
        assert len(want) == 6 and np.allclose(got, want)
    tet = _cxx_planes(planes_lib, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    assert len(tet) == 4
    cube = _cxx_planes(planes_lib, [[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    assert len(cube) == 6                                        # the two triangles of every face are one plane


def test_plane_builder_under_sanitizers(tmp_path):
    """the same header in a program of its own, built with AddressSanitizer and UBSan, run once over every hull of the two models"""
    exe, data = str(tmp_path / 'planes_asan'), str(tmp_path / 'hulls.bin')
    hulls = _hulls('feeding_jaco') + _hulls('dressing_baxter')
    with open(data, 'wb') as f:
        f.write(np.int32(len(hulls)).tobytes())
        for col in hulls:
            v = np.ascontiguousarray(col['verts'], dtype=np.float32)
            f.write(np.int32(len(v)).tobytes() + np.float32(col['radius']).tobytes() + (0.5 * (v.min(0) + v.max(0))).astype(np.float32).tobytes() + v.tobytes())
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DPLANES_MAIN',
                           '-I' + os.path.join(ROOT, 'assistive_gym_amd', 'csrc'), '-o', exe, os.path.join(ROOT, 'tests', 'camera_planes', 'planes_main.cpp')])
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    assert r.stdout.startswith('hulls %d planes ' % len(hulls))


# ---- the C ABI entries without a device --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from assistive_gym_amd.build import build
    build()
    from assistive_gym_amd import libagx
    return libagx.load()


def test_camera_entries_refuse_bad_arguments_without_a_device(lib):
    E_ARG = -1
    v = (C.c_float * 3)(0.0, 0.0, 1.0)
    p = C.cast(v, C.c_void_p)
    n = C.c_int(-7)
    for call, word in ((lambda: lib.agx_camera_set(None, p, p, p, 60.0, 48, 36, 0.01, 100.0), b'agx_camera_set'),
                       (lambda: lib.agx_render(None, 0, 1, p, 0.8, 0.3, p, None, None, None), b'agx_render'),
                       (lambda: lib.agx_collider_frames(None, 0, 1, p, None), b'agx_collider_frames'),
                       (lambda: lib.agx_collider_count(None, C.byref(n)), b'agx_collider_count'),
                       (lambda: lib.agx_camera_colours(None), b'agx_camera_colours')):
        assert call() == E_ARG and word in lib.agx_last_error(), lib.agx_last_error()
    assert n.value == -7
    from assistive_gym_amd.libagx import camera_colours
    col = camera_colours()
    assert col.shape == (12, 3) and col.min() >= 0.0 and col.max() <= 1.0 and len({tuple(c) for c in col}) == 12      # one colour per tag, none repeated
    assert np.allclose(col[11], (0.8, 0.9, 1.0))


def test_collider_info():
    blob = ModelBlob.load('drinking_jaco')
    ncoll = blob.h['NCOLL']
    assert cam.collider_info(blob, -1) is None and cam.collider_info(blob, ncoll + 5) == ('water', 5, -1)
    c = blob.collider(0)
    assert cam.collider_info(blob, 0) == (c['tag'], c['body'], c['link'])
    tags = {cam.collider_info(blob, i)[0] for i in range(ncoll)}
    assert {1, 2, 3} <= tags                                     # robot, tool (the cup), human
