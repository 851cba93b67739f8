"""The closest-point query without a GPU: the reference of tests/proximity_ref.py against closed forms, the selectors and the pair expansion of
assistive_gym_amd/proximity.py, the argument checks of the new ABI entries, and the kernel's wave body (csrc/agx_proximity.h) on the CPU wave
emulator -- tests/emu/emu_proximity.cpp -- over all cross-body pairs of six stored scenes, judged by the function that judges the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import narrowphase_cases as NC
import proximity_ref as PR
from assistive_gym_amd.model import compiler as L

PROX_CPP = os.path.join(emu_lib.EMU, 'emu_proximity.cpp')
_LIBS = {}


def prox_lib(kind='feeding'):
    """tests/emu/emu_proximity.cpp (which includes emu_main.cpp) with the -D flags of an emulator kind, as emu_lib.lib builds emu_main.cpp"""
    if kind not in _LIBS:
        so = os.path.join(emu_lib.EMU, 'libagx_emu_proximity_%s.so' % kind)
        deps = [PROX_CPP] + [os.path.join(emu_lib.EMU, f) for f in ('emu_main.cpp', 'agx_wave.h')] + \
               [os.path.join(emu_lib.CSRC, f) for f in sorted(os.listdir(emu_lib.CSRC)) if f.endswith(('.h', '.def'))] + [os.path.join(emu_lib.ROOT, 'include', 'agx_blob.h')]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import fcntl
            with open(so + '.lock', 'w') as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                tmp = '%s.%d.tmp' % (so, os.getpid())
                subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-I' + emu_lib.EMU, '-I' + emu_lib.CSRC] + emu_lib.kind_defs(kind) + ['-o', tmp, PROX_CPP])
                os.replace(tmp, so)
        _LIBS[kind] = C.CDLL(so)
    return _LIBS[kind]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def emu_proximity(blob, states, pairs, nqueries, max_distance, env0=0, count=None):
    """(records [count, npairs, 12], nearest [count, nqueries, 12]) of the emulated kernel; the frames come from the emulated frames kernel"""
    Lb = prox_lib()
    words, states = np.ascontiguousarray(blob.words), np.ascontiguousarray(states, dtype=np.float32)
    n, ncoll = len(states), blob.h['NCOLL']
    count = n - env0 if count is None else count
    frames = np.zeros((n, ncoll, 12), dtype=np.float32)
    for e in range(n):
        assert Lb.agx_emu_collider_frames(_p(words), _p(states[e]), _p(frames[e])) == 0
    p4 = np.zeros((len(pairs), 4), dtype=np.int32)
    p4[:, :3] = pairs
    flags = PR.collider_flags(blob)
    rec, near = np.full((count, len(pairs), 12), np.nan, dtype=np.float32), np.full((count, nqueries, 12), np.nan, dtype=np.float32)
    rc = Lb.agx_emu_proximity(_p(words), _p(states), C.c_int(states.shape[1]), _p(frames), _p(p4), _p(flags), C.c_int(len(pairs)), C.c_int(nqueries), C.c_int(env0), C.c_int(count),
                              C.c_float(max_distance), _p(rec), _p(near))
    assert rc == 0, 'wave emulator reported divergent control flow: a collective that not all lanes take'
    return rec, near


# ---------------------------------------------------------------------------------------------------- 1. the reference against closed forms
PAR = dict(tol=1e-6, dirs=np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float32))
IDENT = np.concatenate([np.zeros(3), np.eye(3).reshape(-1)])


def _col(verts, radius, body=200, face_box=False):
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    return dict(body=body, verts=v, radius=float(radius), friction=np.float32(1), face_box=face_box, box_c=(lo + hi) / 2, box_h=(hi - lo) / 2, tag=0)


def _at(p):
    return np.concatenate([np.asarray(p, dtype=np.float64), np.eye(3).reshape(-1)])


BOX = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-0.5, 0.5) for z in (-0.25, 0.0)])


def test_reference_two_spheres():
    a, b = _col([[0, 0, 0]], 0.03), _col([[0, 0, 0]], 0.05, body=201)
    e = PR.expected(a, b, _at([0.3, 0.4, 0.0]), IDENT, PAR, 1.0, limits=False)
    assert e['kind'] == 1 and abs(e['dist'] - (0.5 - 0.08)) < 1e-14
    assert np.allclose(e['n'], [0.6, 0.8, 0.0], atol=1e-14) and np.allclose(e['pa'], np.array([0.3, 0.4, 0]) - 0.03 * e['n'], atol=1e-14) and np.allclose(e['pb'], 0.05 * e['n'], atol=1e-14)
    assert PR.expected(a, b, _at([0.3, 0.4, 0.0]), IDENT, PAR, 0.42 - 1e-9, limits=False)['kind'] == 0      # points closer than the distance only
    assert PR.expected(a, b, _at([np.nan, 0.4, 0.0]), IDENT, PAR, 1.0, limits=False)['kind'] == 0


@pytest.mark.parametrize('centre, want', [((0.2, 0.1, 0.3), 0.3), ((1.3, 0.0, 0.4), 0.5), ((1.3, 0.9, 0.4), np.sqrt(0.09 + 0.16 + 0.16))], ids=['face', 'edge', 'corner'])
@pytest.mark.parametrize('box_first', [False, True])
def test_reference_sphere_over_box(centre, want, box_first):
    s, box = _col([[0, 0, 0]], 0.02), _col(BOX, 0.0, body=L.BODY_WORLD, face_box=True)
    e = PR.expected(box, s, IDENT, _at(centre), PAR, 1.0, limits=False) if box_first else PR.expected(s, box, _at(centre), IDENT, PAR, 1.0, limits=False)
    assert e['kind'] == 1 and e['swapped'] == box_first and abs(e['dist'] - (want - 0.02)) < 1e-12
    clamp = np.clip(centre, BOX.min(0), BOX.max(0))
    assert np.allclose(e['pb'], clamp, atol=1e-9) and np.allclose(e['n'], (np.array(centre) - clamp) / want, atol=1e-9)


def test_reference_parallel_capsules():
    a, b = _col([[-0.2, 0, 0], [0.2, 0, 0]], 0.01), _col([[-0.1, 0, 0], [0.3, 0, 0]], 0.02, body=201)
    e = PR.expected(a, b, _at([0, 0.05, 0.12]), IDENT, PAR, 1.0, limits=False)
    assert e['kind'] == 1 and abs(e['dist'] - (0.13 - 0.03)) < 1e-12 and np.allclose(e['n'], [0, 5 / 13, 12 / 13], atol=1e-9)
    o = PR.expected(a, b, _at([0, 0, 0]), IDENT, PAR, 1.0, limits=False)      # the segments overlap: the sampler, the first direction of smallest depth
    assert o['kind'] == 2 and o['ndir'] == 0 and abs(o['dist'] + 0.03) < 1e-12


def test_reference_clipped_box_is_the_whole_box_within_reach():
    rng = np.random.RandomState(5)
    box = _col(BOX, 0.0, body=L.BODY_WORLD, face_box=True)
    empty = 0
    for _ in range(300):
        a = _col(rng.uniform(-0.05, 0.05, (rng.randint(1, 6), 3)), rng.uniform(0, 0.01))
        fa = _at(rng.uniform(-1.6, 1.6, 3) * [1, 1, 0.5])
        g = rng.uniform(0.0, 0.4)
        A = PR.world_verts(a, fa)
        d = NC.hull_distance(A, BOX)[0]
        ext = PR.clipped_box(a, fa, BOX, g)
        if ext is None:
            empty += 1
            assert d > g      # empty only beyond g
        elif d <= g:
            assert abs(NC.hull_distance(A, ext)[0] - d) <= 1e-12      # within g the clipped box answers as the whole box
        assert d <= PR.reach_bound(a, fa, BOX) + 1e-12      # the bound the kernel clips by holds the distance: that clip answers as the whole box, always
        assert abs(NC.hull_distance(A, PR.clipped_box(a, fa, BOX, PR.reach_bound(a, fa, BOX)))[0] - d) <= 1e-12
    assert empty > 10


# ---------------------------------------------------------------------------------------------------- 2. selectors and pair expansion
def test_selectors_and_expansion(blob):
    from assistive_gym_amd import proximity as P
    n = blob.h['NCOLL']
    sets = {t: P.colliders(blob, t) for t in P.TAGS}
    assert sorted(P.TAGS) == sorted(['robot', 'tool', 'human', 'food', 'bowl', 'table', 'plane', 'wheelchair', 'bed'])
    assert sorted(c for s in sets.values() for c in s) == list(range(n)), 'the tags partition the colliders'
    assert all(len(sets[t]) for t in ('robot', 'tool', 'human', 'food', 'table'))
    for t, s in sets.items():
        assert all(blob.collider(c)['tag'] == L.TAG[t.upper()] for c in s)
    links = sorted({blob.collider(c)['link'] for c in sets['robot']})
    some = P.colliders(blob, 'robot', links[-2:])
    assert some and set(some) < set(sets['robot']) and all(blob.collider(c)['link'] in links[-2:] for c in some)
    assert P.colliders(blob, 'robot', links[0]) == [c for c in sets['robot'] if blob.collider(c)['link'] == links[0]]
    with pytest.raises(ValueError):
        P.colliders(blob, 'spoon')
    pairs = P.expand(blob, [('tool', 'human'), (('robot', links[-2:]), 'table'), (sets['robot'][:3], sets['robot'])])
    assert pairs.dtype == np.int32 and pairs.shape[1] == 3 and len(pairs)
    body = [blob.collider(c)['body'] for c in range(n)]
    assert all(a != b and body[a] != body[b] for a, b, _ in pairs), 'no pair on one body, no collider with itself'
    q0 = [(a, b) for a, b, q in pairs if q == 0]
    assert q0 == [(a, b) for a in sets['tool'] for b in sets['human'] if body[a] != body[b]], 'the cross product, a major, query ids set'
    assert {int(q) for q in pairs[:, 2]} == {0, 1, 2} and all((a in some and b in sets['table']) for a, b, q in pairs if q == 1)
    assert len([1 for a, b, q in pairs if q == 2]) < 3 * len(sets['robot'])      # the same-body pairs of the third query are gone
    both = {bool(f & 1) for f in PR.collider_flags(blob)[sets['human']]} | {bool(f & 2) for f in PR.collider_flags(blob)[sets['human']]}
    assert both == {True, False}, 'the human colliders of both genders are selected'


# ---------------------------------------------------------------------------------------------------- 3. argument checks
def test_null_handle_is_refused():
    from assistive_gym_amd.build import build
    build()
    from assistive_gym_amd import libagx
    lib = libagx.load()
    pairs = np.array([[0, 1, 0]], dtype=np.int32)
    n, q = C.c_int(7), C.c_int(7)
    for call, name in ((lambda: lib.agx_proximity_set(None, _p(pairs), 1, 1), b'agx_proximity_set:'), (lambda: lib.agx_proximity_pairs(None, C.byref(n), C.byref(q)), b'agx_proximity_pairs:'),
                       (lambda: lib.agx_proximity(None, 0, 1, 0.1, None, None, None), b'agx_proximity:')):
        assert call() == -1 and lib.agx_last_error().startswith(name) and b'null handle' in lib.agx_last_error()


# ---------------------------------------------------------------------------------------------------- 4. the kernel body on the wave emulator
@pytest.mark.parametrize('name', PR.SCENES)
def test_emulated_kernel_on_stored_scene(name):
    blob, states, table, par = PR.scene(name)
    pairs = PR.cross_body_pairs(table)
    exp = PR.scene_expected(name, pairs, 0.1)
    rec, near = emu_proximity(blob, states, pairs, 1, 0.1)
    assert not np.isnan(rec[..., :10]).any() and not np.isnan(near[..., :10]).any()      # (words 10 and 11 are integers: pair -1 has a NaN's bits)
    bad, skipped, total = PR.judge_records(rec, exp, pairs, table, par)
    nbad, loose = PR.judge_nearest(near, exp, pairs, 1)
    kinds = np.bincount(rec.view(np.int32)[:, :, 10].reshape(-1), minlength=3)
    print('proximity %-10s emulator: %d records (kind 0 / 1 / 2: %d / %d / %d), %d skipped (cap %d); nearest: %d by dist alone' % (name, total, *kinds[:3], skipped, PR.cap(total), loose))
    assert not bad, '%d violations, e.g. %s' % (len(bad), bad[:5])
    assert not nbad, '%d violations, e.g. %s' % (len(nbad), nbad[:5])
    assert skipped <= PR.cap(total)
    assert np.array_equal(near.view(np.int32), PR.nearest_of(rec, pairs, 1).view(np.int32)), 'the nearest records are not those of the rule over the records'
