"""The camera's garment kernel without a device: the host-side triangle-table builder (csrc/agx_garment.h) against the numpy derivation of
tests/garment_ref.py, on the gown, on synthetic garments and on malformed sections, also under the sanitizers in a program of its own; the float64
reference on triangles with known answers; its caps on what tests/test_gpu_garment_camera.py renders (the gown of two fixture records under the
sleeve camera, the synthetic sheets); collider_info and the argument checks of the C ABI entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camera_ref as R
import cloth_cases as CC
import garment_ref as G
from assistive_gym_amd import camera as cam
from assistive_gym_amd.blob import ModelBlob
from assistive_gym_amd.model import compiler as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SRC = os.path.join(ROOT, 'tests', 'garment_faces', 'faces_main.cpp')
INC = '-I' + os.path.join(ROOT, 'assistive_gym_amd', 'csrc')
RECORDS = (0, 5)      # of tests/golden/bridge_dump_dressingbaxter.npz


# ---- the table builder -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def faces_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('garment_faces') / 'libfaces.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', INC, '-o', so, SRC])
    lib = C.CDLL(so)
    lib.agx_test_garment_faces.restype = C.c_int
    return lib


def _words(blob):
    return np.ascontiguousarray(blob.words).view(np.int32).copy()


def _cxx_faces(lib, words):
    """-> int [faces, 3], or the builder's message for a refused section"""
    out, msg = np.full((20000, 3), -1, dtype=np.int32), C.create_string_buffer(256)
    n = lib.agx_test_garment_faces(words.ctypes.data_as(C.c_void_p), C.c_int(len(words)), out.ctypes.data_as(C.c_void_p), C.c_int(len(out)), msg, C.c_int(256))
    return msg.value.decode() if n < 0 else out[:n].astype(int)


@pytest.fixture(scope='module')
def garments():
    dr = ModelBlob.load('dressing_baxter')
    return {'gown': dr, '6x5': G.sheet_setup('free')['blob'], '40x30': G.sheet_setup('subpixel')['blob']}


@pytest.mark.parametrize('name,count', [('gown', 7673), ('6x5', 40), ('40x30', 2262)])
def test_table_builder_matches_the_numpy_derivation(faces_lib, garments, name, count):
    blob = garments[name]
    want, got = G.faces(blob), _cxx_faces(faces_lib, _words(blob))
    assert want.shape == (count, 3) and np.array_equal(got, want)                    # identical order
    if name == 'gown':
        assert blob.meta['cloth']['faces'] == count
    nn = int(blob.i[blob.h['OFF_CLOTH'] + L.CL['NN']])
    assert want.min() >= 0 and want.max() < nn                                       # every node index below NN
    ent = {tuple(e) for e in G.entries(blob)}
    assert len(ent) == 3 * count
    for a, b, c in want:                                                             # a face's three rotations are among the blob's entries
        assert (a, b, c) in ent and (b, c, a) in ent and (c, a, b) in ent
    assert len({tuple(sorted(f)) for f in want}) == count                            # and no face twice


def test_blobs_without_a_garment_have_no_faces(faces_lib):
    for model in ('drinking_jaco', 'feeding_jaco'):
        blob = ModelBlob.load(model)
        got = _cxx_faces(faces_lib, _words(blob))
        assert isinstance(got, np.ndarray) and len(got) == 0 and len(G.faces(blob)) == 0, model


def _corrupt(blob):
    """copies of the blob's words with one word of the cloth section changed -> {what: (words, word of the refusal)}"""
    w = _words(blob)
    oc = blob.h['OFF_CLOTH']
    nn, o_node, o_face = (int(w[oc + L.CL[k]]) for k in ('NN', 'OFF_NODE', 'OFF_FACE'))
    out = {}
    for what, index, value, word in (('face offset beyond the section', oc + L.CL['OFF_FACE'], len(w) - oc - 5, 'outside the section'),
                                     ('node offset beyond the section', oc + L.CL['OFF_NODE'], len(w) - oc - 5, 'outside the section'),
                                     ('negative offset', oc + L.CL['OFF_FACE'], -7, 'outside the section'),
                                     ('node index = NN', oc + o_face + 4, nn | (1 << 16), '>= NN'),
                                     ('node index = NN in the high half', oc + o_face + 4, 1 | (nn << 16), '>= NN'),
                                     ('entry count not a multiple of 3', oc + o_node + 2 * nn, int(w[oc + o_node + 2 * nn]) - 1, 'multiple of 3'),
                                     ('entry count beyond the section', oc + o_node + 2 * nn, 3 * (1 << 28), 'outside the section'),
                                     ('a node range running backwards', oc + o_node + 2 * 3, int(w[oc + o_node + 2 * 4]) + 3, 'entry range')):
        c = w.copy()
        c[index] = value
        out[what] = (c, word)
    c = w[:oc + L.CL['HDR'] - 2].copy()
    c[L.H['NWORDS']] = len(c)
    out['blob ends inside the section header'] = (c, 'header')
    return out


def test_malformed_sections_are_refused(faces_lib, garments):
    for name in ('gown', '6x5'):
        for what, (words, word) in _corrupt(garments[name]).items():
            got = _cxx_faces(faces_lib, words)
            assert isinstance(got, str) and word in got, (name, what, got if isinstance(got, str) else len(got))


def test_table_builder_under_sanitizers(tmp_path, garments):
    """the same header in a program of its own, built with AddressSanitizer and UBSan, run once over the garments, two blobs without one and the
    corrupt copies; every blob is handed over as a heap block of exactly its size"""
    exe, data = str(tmp_path / 'faces_asan'), str(tmp_path / 'blobs.bin')
    items = [(_words(garments['gown']), 7673), (_words(garments['6x5']), 40), (_words(garments['40x30']), 2262),
             (_words(ModelBlob.load('drinking_jaco')), 0), (_words(ModelBlob.load('feeding_jaco')), 0)]
    items += [(w, -1) for name in ('gown', '6x5') for w, _ in _corrupt(garments[name]).values()]
    with open(data, 'wb') as f:
        f.write(np.int32(len(items)).tobytes())
        for w, expect in items:
            f.write(np.int32(len(w)).tobytes() + np.int32(expect).tobytes() + w.tobytes())
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DFACES_MAIN', INC, '-o', exe, SRC])
    r = subprocess.run([exe, data], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    assert r.stdout.strip() == 'blobs %d faces %d refused %d' % (len(items), 7673 + 40 + 2262, len(items) - 5)


# ---- Python and the C ABI without a device -------------------------------------------------------------------------------------------------------
def test_collider_info_names_garment_faces(garments):
    blob = garments['gown']
    ncoll = blob.h['NCOLL']
    assert cam.collider_info(blob, ncoll) == ('garment', 0, -1) and cam.collider_info(blob, ncoll + 7672) == ('garment', 7672, -1)
    assert cam.collider_info(blob, -1) is None and cam.collider_info(blob, ncoll - 1)[0] != 'garment'
    water = ModelBlob.load('drinking_jaco')
    assert cam.collider_info(water, water.h['NCOLL'] + 5) == ('water', 5, -1)


@pytest.fixture(scope='module')
def lib():
    from assistive_gym_amd.build import build
    build()
    from assistive_gym_amd import libagx
    return libagx.load()


def test_garment_entries_refuse_bad_arguments_without_a_device(lib):
    n = C.c_int(-7)
    buf = (C.c_int * 3)(-7, -7, -7)
    for call, word in ((lambda: lib.agx_camera_garment(None, 1), b'agx_camera_garment'), (lambda: lib.agx_camera_garment(None, 0), b'agx_camera_garment'),
                       (lambda: lib.agx_garment_faces(None, C.byref(n), C.cast(buf, C.c_void_p)), b'agx_garment_faces'),
                       (lambda: lib.agx_camera_garment_colour(None), b'agx_camera_garment_colour')):
        assert call() == -1 and word in lib.agx_last_error(), lib.agx_last_error()
    assert n.value == -7 and list(buf) == [-7, -7, -7]
    from assistive_gym_amd.libagx import camera_colours, camera_garment_colour
    col = camera_garment_colour()
    assert col.dtype == np.float32 and np.array_equal(col, (np.array([139, 195, 74], dtype=np.float32) / np.float32(256)))
    assert camera_colours().shape == (12, 3) and not any(np.array_equal(col, c) for c in camera_colours())      # next to the table, not in it


# ---- the reference on triangles with known answers -----------------------------------------------------------------------------------------------
TRI = np.array([[0, 1, 2]])


def _one(x, d=(0.0, 1.0, 0.0), eye=(0.0, -2.0, 0.0), near=R.NEAR, far=R.FAR):
    t, f, n = G.cast_garment(np.array(eye), np.array([d], dtype=np.float64), np.array(x, dtype=np.float32), TRI, near, far)
    return float(t[0]), int(f[0]), n[0]


def test_reference_triangle_closed_forms():
    face_on = [[-1, 0.5, -1], [1, 0.5, -1], [0, 0.5, 1]]                              # in the plane y = 0.5, seen from (0, -2, 0) along +y
    t, f, n = _one(face_on)
    assert f == 0 and t == 2.5 and np.allclose(n, (0, -1, 0))                         # t = its distance; the normal faces the eye
    t2, f2, n2 = _one([face_on[0], face_on[2], face_on[1]])                           # the other winding: the back side is visible, the normal flipped
    assert f2 == 0 and t2 == 2.5 and np.allclose(n2, (0, -1, 0))
    t3, f3, n3 = _one(face_on, eye=(0.0, 3.0, 0.0), d=(0.0, -1.0, 0.0))               # ... and from behind
    assert f3 == 0 and t3 == 2.5 and np.allclose(n3, (0, 1, 0))
    assert _one(face_on, d=(0.0, 1.0, 0.3))[1] == 0 and _one(face_on, d=(0.0, 1.0, 0.45))[1] == -1     # meets the plane at z = 0.75 and at z = 1.125: the apex is at z = 1
    t4, f4, _ = _one(face_on, d=(0.1, 1.0, 0.0))                                       # d is not normalised: t is the depth along y, not the distance
    assert f4 == 0 and np.isclose(t4, 2.5)
    assert _one([[0, -1, -1], [0, 1, -1], [0, 0, 1]])[1] == -1                         # edge on (det = 0): not hit
    assert _one([[-1, 0.5, 0], [1, 0.5, 0], [3, 0.5, 0]])[1] == -1                     # zero area: never hit
    assert _one(face_on, near=2.6)[1] == -1 and _one(face_on, far=2.4)[1] == -1 and _one(face_on, near=2.5, far=2.5)[1] == 0
    # straddling the near plane: a triangle along the view direction, from behind the eye to 3 m before it, 10 cm below the eye
    along = [[-1, -3, -0.1], [1, -3, -0.1], [0, 1, -0.1]]
    eye = np.array([0.0, -2.0, 0.0])
    for dz, hit in ((-0.5, False), (-0.11, False), (-0.09, True), (-0.05, True)):      # the ray meets z = -0.1 at depth 0.1 / |dz|; near = 1
        t, f, n = _one(along, d=(0.0, 1.0, dz), near=1.0)
        assert (f == 0) == hit and (not hit or (np.isclose(t, 0.1 / -dz) and t >= 1.0 and np.allclose(n, (0, 0, 1)))), (dz, t, f)
    # two layers along the ray: the nearer one wins whatever its index; equal depth: the lower face
    x = np.array([[-1, 0.5, -1], [1, 0.5, -1], [0, 0.5, 1], [-1, 0.3, -1], [1, 0.3, -1], [0, 0.3, 1]], dtype=np.float32)
    t, f, _ = G.cast_garment(eye, np.array([[0.0, 1.0, 0.0]]), x, np.array([[0, 1, 2], [3, 4, 5]]))
    assert f[0] == 1 and np.isclose(t[0], 2.3)
    t, f, _ = G.cast_garment(eye, np.array([[0.0, 1.0, 0.0]]), x, np.array([[3, 4, 5], [0, 1, 2], [3, 5, 4]]))
    assert f[0] == 0
    # the merge: the smaller t wins, a collider keeps a tie
    rigid = (np.array([2.5, 2.5, 100.0]), np.array([4, 4, -1]), np.zeros((3, 3)), np.array([-1, -1, -1]))
    tm, im, _, _ = G.merge(rigid, (np.array([2.5, 2.4, 2.5]), np.array([0, 0, 7]), np.zeros((3, 3))), 10, 100.0)
    assert list(im) == [4, 10, 17] and list(tm) == [2.5, 2.4, 2.5]


def test_reference_with_and_without_the_screen_boxes_agree():
    s = G.sheet_setup('folded')
    c = R.Camera(near=s['near'], **s['view'])
    a = G.cast_garment(c.eye, c.rays(), s['x'], s['tris'], c.near, c.far)
    b = G.cast_garment(c.eye, c.rays(), s['x'], s['tris'], c.near, c.far, c.basis)
    assert all(np.array_equal(p, q) for p, q in zip(a, b)) and (a[1] >= 0).sum() > 100


# ---- the caps of the image comparison, on the reference alone -------------------------------------------------------------------------------
_REF = {}


def _oracle_frames(blob, state):
    from oracle_lib import Oracle
    key = state.tobytes()
    if key not in _REF:
        _REF[key] = R.ref_frames(blob, Oracle(blob), state)[0]
    return _REF[key]


def _gown_five(record):
    """the sleeve camera on a record of the committed dressing trajectory, the rigid scene included (frames from the oracle)"""
    if ('gown', record) not in _REF:
        g = np.load(os.path.join(GOLDEN, 'bridge_dump_dressingbaxter.npz'))
        blob = ModelBlob.load('dressing_baxter')
        state, x = g['states'][record].copy(), g['cloth'][record, 0]
        scene, c, gender = R.Scene.of_blob(blob), R.Camera(**G.sleeve_camera(blob, x)), int(blob.view(state.reshape(1, -1))['gender'][0])
        _REF[('gown', record)] = (scene, c, _oracle_frames(blob, state), gender, G.render_five(scene, c, _oracle_frames(blob, state), gender, x, G.faces(blob)))
    return _REF[('gown', record)]


@pytest.mark.parametrize('record', RECORDS)
def test_caps_hold_on_the_reference_alone_gown(record):
    scene, c, _, _, five = _gown_five(record)
    shares = G.check_caps(five, scene.ncoll, 'gown record %d' % record)
    assert shares['garment'] > 0.5 and (five[0][1] < scene.ncoll).sum() > 0      # the gown fills most of the view; the rigid scene shows through its openings


def _sheet_five(name):
    if name not in _REF:
        s = G.sheet_setup(name)
        scene, c = R.Scene.of_blob(s['blob']), R.Camera(near=s['near'], **s['view'])
        gender = int(s['blob'].view(s['state'].reshape(1, -1))['gender'][0])
        _REF[name] = (s, scene, c, G.render_five(scene, c, _oracle_frames(s['blob'], s['state']), gender, s['x'], s['tris']), gender)
    return _REF[name]


@pytest.mark.parametrize('name', [n for n in G.SHEETS if n != 'line'])
def test_caps_hold_on_the_reference_alone_sheets(name):
    s, scene, c, five, _ = _sheet_five(name)
    G.check_caps(five, scene.ncoll, name, s['subpixel'])


def _visible_ties(scene, c, frames, gender, five):
    safe = R.masks(five)[0]
    return [(int(p % c.width), int(p // c.width)) for p in G.rigid_ties(scene, c, frames, gender) if safe[p] and five[0][1][p] < scene.ncoll]


def test_no_view_shows_two_colliders_within_the_floor_of_each_other():
    """a safe pixel that shows a collider with a second collider within 64 2^-24 max(1, t) behind it would test how float32 orders a tie inside the
    rigid scene, not the garment: the views of the device tests have none (garment_ref.SHEET_VIEW says how they were chosen)"""
    for name in (n for n in G.SHEETS if n != 'line'):
        s, scene, c, five, gender = _sheet_five(name)
        assert _visible_ties(scene, c, _oracle_frames(s['blob'], s['state']), gender, five) == [], name
    for record in RECORDS:
        scene, c, frames, gender, five = _gown_five(record)
        assert _visible_ties(scene, c, frames, gender, five) == [], record


def test_the_sheets_show_what_their_cases_are_about():
    # (b) occlusion both ways: the sheet hides colliders other than the ground, and colliders hide part of the sheet
    s, scene, c, five, gender = _sheet_five('occluded')
    alone = G.cast_garment(c.eye, c.rays(), s['x'], s['tris'], c.near, c.far)
    rigid = R.cast(scene, _oracle_frames(s['blob'], s['state']), gender, c.eye, c.rays(), c.near, c.far)
    seg = five[0][1]
    ground = scene.ncoll - 1
    assert ((seg >= scene.ncoll) & (rigid[1] >= 0) & (rigid[1] != ground)).sum() >= 20 and ((alone[1] >= 0) & (seg < scene.ncoll)).sum() >= 20
    # (c) two layers along the ray: where the rays meet the far layer (columns 3..5 of the grid) too, the near layer is what is seen
    s, scene, c, five, _ = _sheet_five('folded')
    far_layer = np.array([bool((s['ij'][f, 0] >= 3).all()) for f in s['tris']])
    near_layer = np.array([bool((s['ij'][f, 0] <= 2).all()) for f in s['tris']])
    behind = G.cast_garment(c.eye, c.rays(), s['x'], s['tris'][far_layer], c.near, c.far)
    front = G.cast_garment(c.eye, c.rays(), s['x'], s['tris'][near_layer], c.near, c.far)
    both = (behind[1] >= 0) & (front[1] >= 0)
    seg = five[0][1] - scene.ncoll
    assert both.sum() >= 30 and np.all(front[0][both] < behind[0][both]) and np.all(near_layer[seg[both]]) and (far_layer[seg[seg >= 0]]).sum() >= 10
    # (d) nodes behind the eye and before the near plane; rays that meet the sheet's plane before the near plane show no garment
    s, scene, c, five, _ = _sheet_five('near_plane')
    z = (s['x'].astype(np.float64) - c.eye) @ c.basis[2]
    assert (z < 0).sum() >= 5 and ((z > 0) & (z < c.near)).sum() == 0 and np.float32(c.near) == np.float32(0.05)
    everything = G.cast_garment(c.eye, c.rays(), s['x'], s['tris'], 1e-9, c.far)
    seg, t = five[0][1], five[0][0]
    assert np.all(t[seg >= scene.ncoll] >= c.near) and ((everything[1] >= 0) & (everything[0] < c.near)).sum() >= 50
    assert np.all(seg[(everything[1] >= 0) & (everything[0] < c.near)] < scene.ncoll)
    # (e) all nodes on one line: no face is hit
    s = G.sheet_setup('line')
    c = R.Camera(**s['view'])
    assert np.all(G.cast_garment(c.eye, c.rays(), s['x'], s['tris'], c.near, c.far)[1] == -1) and np.ptp(s['x'], 0).max() > 0.1
    # (f) exactly planar, every face far smaller than a pixel, all inside the rows 4..8 of the image: one tile
    s, scene, c, five, _ = _sheet_five('subpixel')
    assert len(np.unique(s['x'][:, 2])) == 1 and len(s['tris']) == 2262
    pc = (s['x'].astype(np.float64) - c.eye) @ c.basis.T
    ty = np.tan(0.5 * np.radians(c.fov))
    px, py = (pc[:, 0] / pc[:, 2] / (ty * c.width / c.height) + 1) / 2 * c.width, (1 - pc[:, 1] / pc[:, 2] / ty) / 2 * c.height
    assert px.min() > 0 and px.max() < 16 and py.min() > 4 and py.max() < 8
    assert len(s['tris']) / ((five[0][1] >= scene.ncoll).sum()) > 20                 # faces per garment pixel
