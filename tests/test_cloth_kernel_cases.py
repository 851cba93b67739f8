"""The node-exact cloth cases (tests/golden/cloth_kernel_cases.npz, tests/cloth_cases.py) on the CPU:
  * the committed generator reproduces the stored fixture;
  * the oracle's cloth_substep agrees with the numpy restatement on every stored substep -- capsules, a hull, the two-contact cap in the overlap
    of three shapes, a shape of the other gender -- and on the free flights up to the 4,096-node garment;
  * the comparison the device tests judge by (cloth_cases.judge_forced / judge_free) accepts the float32 restatement and rejects it with one
    planted error at a time.
tests/test_gpu_cloth_kernel.py runs the HIP kernel on the same cases."""
import os
import sys

import numpy as np
import pytest

import cloth_cases as CC

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'diag'))

FORCED = ('fs_A_slide', 'fs_A_drop', 'fs_B_slide', 'fs_B_drop', 'fs_hull', 'fs_overlap', 'fs_gender', 'fs_first_touch')
MIN_CONTACTS = dict(fs_first_touch=10)      # one contact per substep: the node that arrives
FREE = ('ff_A_k1', 'ff_A_k0_clamp', 'ff_B', 'ff_C_clamp', 'ff_D')
GRAVITY = -9.81


@pytest.fixture(scope='module')
def cases():
    return CC.load_cases()


def test_fixture_conditions(cases):
    """what the generator asserted when it chose the placements, read back from the stored file"""
    for name in FORCED:
        rec, mask, det = cases[name + '/recipe'], cases[name + '/mask'], cases[name + '/det']
        assert (len(mask) >= 40 or name in MIN_CONTACTS) and det.sum() >= 10 and mask.sum() >= 10, name
        assert sum(len(s['con']) for s in CC.forced_substeps(cases, name)) >= MIN_CONTACTS.get(name, 50), name
        assert (~mask).sum() <= 0.75 * len(mask), name
        assert rec['determined'] == mask.sum()
    assert cases['fs_overlap/recipe']['triple_nodes'] >= 5
    assert cases['ff_A_k0_clamp/recipe']['clamp_fired'] > 0 and cases['ff_C_clamp/recipe']['clamp_fired'] > 0
    assert cases['ff_A_k1/recipe']['cross_classes'] == 0 and cases['ff_B/recipe']['cross_classes'] >= 3 and cases['ff_D/recipe']['nodes'] == 4096
    assert os.path.getsize(CC.GOLDEN) < 512 * 1024


@pytest.mark.parametrize('name', ['ff_A_k1', 'fs_A_drop'])
def test_generator_reproduces_the_fixture(cases, name):
    import make_cloth_kernel_cases as G
    out = G.make([name], log=lambda *a: None)
    for key, val in out.items():
        if key == 'state':
            assert np.allclose(val, cases[key], rtol=0, atol=1e-6)
        elif key.endswith('/recipe'):
            assert __import__('json').loads(str(val)) == cases[key]
        elif val.dtype.kind in 'biu':
            assert np.array_equal(val, cases[key]), key
        else:      # the rigid scene's frames come from the C oracle (libm): allow the last bits of a float64
            assert val.shape == cases[key].shape and np.allclose(val, cases[key], rtol=1e-3 if key.endswith('/dev') else 1e-6, atol=1e-9), key


def _oracle_contacts(o):
    con, nodes = o.cloth_contacts(), o.cloth_contact_nodes()
    out, seen = {}, {}
    for c, i in zip(con, nodes):
        slot = seen.get(int(i), 0)
        seen[int(i)] = slot + 1
        out[(int(i), slot)] = (c[:3], float(np.linalg.norm(c[3:])))
    return out


@pytest.mark.parametrize('name', FORCED)
def test_oracle_agrees_with_the_restatement_forced(cases, name):
    """every stored substep, determined or not (both sides are float64), at the tolerances of tests/test_cloth_oracle.py"""
    from oracle_lib import Oracle
    o = Oracle(CC.one_substep_blob(CC.case_blob(cases[name + '/recipe'])))
    subs = CC.forced_substeps(cases, name, determined_only=False)
    assert len(subs) >= 10
    for s in subs:
        state, cloth = s['state'].copy(), np.stack([s['xin'], s['vin']])
        o.settle_cloth(state, cloth, 1)
        assert np.abs(cloth[0] - s['x']).max() < 5e-6 and np.abs(cloth[1] - s['v']).max() < 2e-3, (name, s['sub'])
        got = _oracle_contacts(o)
        assert set(got) == set(s['con']), (name, s['sub'])
        for k, f in s['con'].items():
            assert np.allclose(got[k][0], s['x'][k[0]], atol=5e-6) and np.isclose(got[k][1], f, rtol=2e-3, atol=3e-5), (name, s['sub'], k)


@pytest.mark.parametrize('name', FREE)
def test_oracle_agrees_with_the_restatement_free_flight(cases, name):
    from oracle_lib import Oracle
    rec = cases[name + '/recipe']
    blob = CC.case_blob(rec)
    x, v = CC.free_input(CC.tables(blob), rec)
    state, cloth = cases['state'].copy(), np.stack([x, v])
    Oracle(blob).settle_cloth(state, cloth, 1)
    want_x = x.astype(np.float64) + cases[name + '/dx'].astype(np.float64)
    assert np.abs(cloth[0] - want_x).max() < 2e-6 and np.abs(cloth[1] - cases[name + '/v']).max() < 2e-4


# ---- the comparison can fail
def _restated_forced(cases, name, plant=None, plant_for=None):
    """the float32 restatement (optionally with a planted error) on the stored determined substeps, in the form the device test hands to judge_forced"""
    from oracle_lib import Oracle
    blob = CC.one_substep_blob(CC.case_blob(cases[name + '/recipe']))
    o, t, shapes = Oracle(blob), CC.tables(blob), CC.shape_table(blob)
    res = []
    for s in CC.forced_substeps(cases, name):
        frames = CC.body_frames(blob, o, s['state'], shapes)
        anchor, _ = o.ee_pose(s['state'])
        pl = plant_for(t, shapes, s) if plant_for else plant
        x, v, con, _, _ = CC.substep(t, shapes, frames, s['xin'], s['vin'], GRAVITY, CC.DT, anchor, gender=0, dtype=np.float32, plant=pl)
        res.append((x, v, con, None))
    return blob, res


def _restated_free(cases, name, plant=None):
    from oracle_lib import Oracle
    rec = cases[name + '/recipe']
    blob = CC.case_blob(rec)
    t, shapes = CC.tables(blob), CC.shape_table(blob)
    frames = CC.body_frames(blob, Oracle(blob), cases['state'], shapes)
    x, v = CC.free_input(t, rec)
    x, v, _, _ = CC.free_flight(t, shapes, frames, x, v, GRAVITY, np.array(rec['ee']), np.float32, plant=plant)
    return t, x, v


def _most_strained_cross_link(t, rec):
    """a link of the first cross-patch class, the one the seeded velocities stretch most in the first substep"""
    x, v = CC.free_input(t, rec)
    ls = np.nonzero(t['cls'] == t['first_cross'])[0]
    dv = np.linalg.norm(v[t['a'][ls]] - v[t['b'][ls]], axis=1)
    return int(ls[np.argmax(dv)])


PLANTS = {
    'one link dropped from a cross-patch class': ('ff_B', 'drop_link'),
    'one class relaxed before its predecessor': ('ff_B', 'swap_classes'),
    'the friction factor 1 - fc where 0 belongs': ('fs_A_drop', dict(friction=True)),
    'the third contact kept instead of the second': ('fs_overlap', dict(third_contact=True)),
    'an anchored node allowed to collide': ('fs_gender', dict(anchored_collide=True)),
    "one plane's normal negated": ('fs_hull', 'negate_plane'),
    'the report slot of contact 1 written to slot 0': ('fs_overlap', dict(slot1_to_slot0=True)),
}


@pytest.mark.parametrize('name', ['ff_B', 'fs_A_drop', 'fs_overlap', 'fs_gender', 'fs_hull'])
def test_comparison_accepts_the_float32_restatement(cases, name):
    if name.startswith('ff'):
        t, x, v = _restated_free(cases, name)
        m, lim, bad = CC.judge_free(cases, name, t, x, v)
    else:
        blob, res = _restated_forced(cases, name)
        m, lim, bad = CC.judge_forced(cases, name, blob, res)
    assert not bad, bad


@pytest.mark.parametrize('what', list(PLANTS))
def test_comparison_rejects_a_planted_error(cases, what):
    name, plant = PLANTS[what]
    if name.startswith('ff'):
        rec = cases[name + '/recipe']
        t = CC.tables(CC.case_blob(rec))
        plant = dict(drop_link=_most_strained_cross_link(t, rec)) if plant == 'drop_link' else dict(swap_classes=t['first_cross'])
        t, x, v = _restated_free(cases, name, plant)
        m, lim, bad = CC.judge_free(cases, name, t, x, v)
    else:
        plant_for = None
        if plant == 'negate_plane':      # the top face of the arm rest (a world body: its plane normals are world normals)
            plant, plant_for = None, lambda t, shapes, s: dict(negate_plane=(0, int(np.argmax(shapes[0]['planes'][:, 2]))))
        blob, res = _restated_forced(cases, name, plant, plant_for)
        m, lim, bad = CC.judge_forced(cases, name, blob, res)
    assert bad, (what, m, lim)
