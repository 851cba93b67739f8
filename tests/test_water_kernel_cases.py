"""The particle-exact water cases (tests/golden/water_kernel_cases.npz, tests/water_cases.py) on the CPU:
  * the committed generator reproduces the stored fixture;
  * the oracle's water_substep agrees with the numpy restatement on every stored substep, determined or not (both are float64);
  * the kernel SOURCE (csrc/agx_water.h) on the wave emulator is judged by the comparison and the limits the device is judged by;
  * that comparison accepts the float32 restatement and rejects it with one planted error at a time.
tests/test_gpu_water_kernel.py runs the HIP kernel on the same cases."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import water_cases as WC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'diag'))

SCENES = ('ww_free_1', 'ww_free_2', 'ww_free_63', 'ww_free_64', 'ww_pile', 'ww_cup_rest', 'ww_cap_a', 'ww_cap_b', 'ww_chunks', 'ww_planes', 'ww_cores', 'ww_gender',
          'ww_friction', 'ww_hit_last')
# share of the tried substeps that may be left out as undetermined: half -- a scene that loses more than that to its thresholds is about
# its thresholds, not about the path it was built for -- except in the shaken pile of 64 in the real cup, where some of ~500 pairs and ~300
# particle-piece distances is within a band in almost every substep (measured: 10 of 159 determined)
MAX_LEFT_OUT = 0.5
MAX_LEFT_OUT_CUP = 0.95


@pytest.fixture(scope='module')
def cases():
    return WC.load_cases()


def test_fixture_conditions(cases):
    assert sorted(WC.scenes(cases)) == sorted(SCENES)
    for name in SCENES:
        rec, mask, det = cases[name + '/recipe'], cases[name + '/mask'], cases[name + '/det']
        assert det.sum() >= 10 and mask.sum() >= 10 and rec['determined'] == mask.sum() and rec['tried'] == len(mask), name
        assert (~mask).sum() <= (MAX_LEFT_OUT_CUP if name == 'ww_cup_rest' else MAX_LEFT_OUT) * len(mask), name
    assert os.path.getsize(WC.GOLDEN) < 512 * 1024
    assert [len(cases['ww_free_%d/xin' % n][0]) for n in (1, 2, 63, 64)] == [1, 2, 63, 64] and len(cases['ww_free_64/recipe']['parked']) == 2
    assert len(cases['ww_chunks/recipe']['splice']['shape_ids']) == 192 and cases['ww_chunks/recipe']['touched_at'] == [0, 63, 64, 127, 128, 191]
    assert cases['ww_cup_rest/det'].all()                     # determined substeps only
    assert len(cases['ww_cup_rest/xin'][0]) == 64 and len(cases['ww_cap_a/recipe']['splice']['shape_ids']) == 14
    sh = WC.shape_table(WC.case_blob(cases['ww_planes/recipe']))
    assert [len(s['planes']) for s in sh] == [8, 8, 8, 124] and sorted(cases['ww_planes/recipe']['splice']['keep_planes'].values()) == [5, 7, 8]
    assert cases['ww_hit_last/recipe']['nsub'] == 4


@pytest.fixture(scope='module')
def world():
    """the settled state record and water the generator starts every scene from (50 settle steps of the oracle: once)"""
    import make_water_kernel_cases as G
    dk = G.load()
    state, water = G.settled(dk)
    return dk, G.World(dk, state), water


@pytest.mark.parametrize('name', SCENES)
def test_generator_reproduces_the_fixture(cases, world, name):
    """every scene, every array, bit for bit (float arrays compared as their bits: a state record holds integer words as well)"""
    import make_water_kernel_cases as G
    out = G.make_scene(*world, name, log=lambda *a: None)
    assert sorted(out) == sorted(k for k in cases if k.startswith(name + '/'))
    for key, val in out.items():
        if key.endswith('/recipe'):
            assert json.loads(str(val)) == cases[key]
        else:
            bits = lambda a: a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == 'f' else a
            assert val.dtype == cases[key].dtype and val.shape == cases[key].shape and np.array_equal(bits(val), bits(cases[key])), key


def _oracle(cases, name):
    from oracle_lib import Oracle
    blob = WC.case_blob(cases[name + '/recipe'])
    return blob, Oracle(blob)


@pytest.mark.parametrize('name', SCENES)
def test_oracle_agrees_with_the_restatement(cases, name):
    """every stored substep, determined or not.  Both sides compute in float64 from the same float32 inputs; what separates them is what
    crosses the ctypes boundary and the fixture's storage: the oracle returns x and v rounded to float32 (half an ulp of each), the fixture
    holds x as float32 input + float32 difference (half an ulp of the difference) and v as float32 (half an ulp).  The launch of four
    substeps replays frames that went through the float32 trace (half an ulp of a frame coordinate, 6e-8 m, per substep, and 1 / dt of it in v)"""
    blob, o = _oracle(cases, name)
    subs = WC.stored_substeps(cases, name, determined_only=False)
    assert len(subs) >= 10
    nsub = cases[name + '/recipe']['nsub']
    shapes, t = WC.shape_table(blob), WC.tables(blob)
    for s in subs:
        state, water = s['state'].copy(), np.stack([s['xin'], s['vin']])
        o.settle_cloth(state, water, 1)
        half = lambda a: 0.5 * WC.ulp32(a)
        frames = nsub * half(np.ones(1)) if nsub > 1 else 0.0
        lim_x = half(s['x']) + half(s['x'] - s['xin']) + frames + 1e-12
        lim_v = 2 * half(s['v']) + frames / WC.DT + 1e-9
        assert np.abs(water[0] - s['x']).max() <= lim_x and np.abs(water[1] - s['v']).max() <= lim_v, (name, s['sub'], np.abs(water[0] - s['x']).max(), lim_x, np.abs(water[1] - s['v']).max(), lim_v)
        got = {(int(i), shapes[int(sh)]['same']) for i, sh in zip(o.cloth_contact_nodes(), o.cloth_contact_shapes())}
        if s['det']:      # (the twins of a touched shape are touched or not by rounding: water_cases._twin)
            fr = _frames(blob, o, s['state'], s['xin'], s['vin'], nsub, np.float64)
            lucky = WC.substeps(t, shapes, fr, s['xin'].astype(np.float64), s['vin'].astype(np.float64), gender=_gender(blob, s['state']))[4]['lucky']
            assert s['hits'] <= got <= s['hits'] | lucky, (name, s['sub'], sorted(got ^ s['hits'])[:6])


def _gender(blob, state):
    return int(blob.view(state[None])['gender'][0])


def _frames(blob, o, state, x, v, nsub, dtype):
    if nsub > 1:
        trace, _ = WC.oracle_trace(blob, o, state, np.stack([x, v]), nsub)
        return [WC.body_frames(blob, state, WC.moving_of_trace(trace, k), dtype) for k in range(nsub)]
    return [WC.body_frames(blob, state, WC.moving_of_state(blob, o, state), dtype)]


# ---- the kernel source on the wave emulator
@pytest.mark.parametrize('name', SCENES)
def test_kernel_source_on_the_emulator(cases, name):
    """csrc/agx_water.h as the device compiles it, run lane by lane on the CPU (tests/emu) over the oracle's trace of each stored determined
    substep: the same judge, the same limits as tests/test_gpu_water_kernel.py"""
    from emu_lib import lib, _p
    E = lib('feeding')
    blob, o = _oracle(cases, name)
    words = np.ascontiguousarray(blob.words)
    nsub = cases[name + '/recipe']['nsub']
    res = []
    for s in WC.stored_substeps(cases, name):
        trace, _ = WC.oracle_trace(blob, o, s['state'], np.stack([s['xin'], s['vin']]), nsub)
        w = np.ascontiguousarray(np.stack([s['xin'], s['vin']]))
        report = np.full(64, -1, np.int32)
        assert E.agx_emu_water(_p(words), _p(s['state']), _p(trace), _p(w), _p(report), C.c_int(nsub)) == 0
        res.append((w[0], w[1], report))
    m, lim, bad = WC.judge(cases, name, res)
    print('water kernel source %-12s limit x %.3g v %.3g | emulator x %.3g v %.3g | parked: limit x %.3g v %.3g | emulator x %.3g v %.3g | person flags %d'
          % (name, lim['x'], lim['v'], m['x'], m['v'], lim['far_x'], lim['far_v'], m['far_x'], m['far_v'], m['hits']))
    assert not bad, bad


# ---- the comparison can fail
def _restated(cases, name, plant=None):
    """the float32 restatement (optionally with a planted error) on the stored determined substeps, in the form judge() takes"""
    blob, o = _oracle(cases, name)
    t, shapes = WC.tables(blob), WC.shape_table(blob)
    nsub = cases[name + '/recipe']['nsub']
    res = []
    for s in WC.stored_substeps(cases, name):
        fr = _frames(blob, o, s['state'], s['xin'], s['vin'], nsub, np.float32)
        x, v, hits, _, _ = WC.substeps(t, shapes, fr, s['xin'], s['vin'], gender=_gender(blob, s['state']), dtype=np.float32, plant=plant)
        res.append((x, v, hits))
    return res


PLANTS = {
    'cap 11 instead of 12': ('ww_cap_b', 'cap11'),
    'the last 12 candidates in shape order kept': ('ww_cap_b', 'last12'),
    'the plane taken at the predicted position': ('ww_cores', 'plane_at_prediction'),
    'no division by cnt when cnt is 2 either (the split one count late)': ('ww_pile', 'split_at_two'),
    'coincident centres split with the sign reversed': ('ww_pile', 'coincident_sign'),
    'friction uncapped': ('ww_friction', 'friction_uncapped'),
    '(1 - kDP) dropped': ('ww_free_64', 'no_kdp'),
    'gender filter ignored': ('ww_gender', 'no_gender'),
    'hit flag OR-ed over all substeps': ('ww_hit_last', 'hit_or'),
    'trace slot off by one': ('ww_hit_last', 'trace_slot'),
    'reach without the |v| dt term': ('ww_cores', 'reach_without_v'),
    'no 500 m cut-off': ('ww_free_64', 'no_far_cutoff'),
}


@pytest.mark.parametrize('name', ['ww_free_64', 'ww_pile', 'ww_cap_b', 'ww_cores', 'ww_gender', 'ww_friction', 'ww_hit_last'])
def test_comparison_accepts_the_float32_restatement(cases, name):
    m, lim, bad = WC.judge(cases, name, _restated(cases, name))
    assert not bad, bad


@pytest.mark.parametrize('what', list(PLANTS))
def test_comparison_rejects_a_planted_error(cases, what):
    name, plant = PLANTS[what]
    res = _restated(cases, name, {plant: True})
    m, lim, bad = WC.judge(cases, name, res)
    assert bad, (what, m, lim)
    if plant == 'hit_or':      # what the device reports: the flags, not the set
        shapes = WC.shape_table(WC.case_blob(cases[name + '/recipe']))
        flags = [(x, v, np.concatenate([WC.person_flags(h, shapes, len(x)), np.zeros(64 - len(x), np.int32)])) for x, v, h in res]
        assert WC.judge(cases, name, flags)[2]


def test_division_by_a_count_of_one_is_no_error(cases):
    """"division by cnt also when cnt == 1" cannot be rejected by any comparison: x / 1 is x, bit for bit, in every IEEE type -- the kernel's
    `if (cnt > 1)` only saves three divisions.  Planted all the same: the result must be the unplanted one to the bit (the split that CAN be
    wrong, one count late, is among PLANTS)"""
    for (x, v, h), (xp, vp, hp) in zip(_restated(cases, 'ww_pile'), _restated(cases, 'ww_pile', dict(divide_single=True))):
        assert np.array_equal(x.view(np.int32), xp.view(np.int32)) and np.array_equal(v.view(np.int32), vp.view(np.int32)) and h == hp
