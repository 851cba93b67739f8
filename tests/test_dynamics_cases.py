"""The dynamics cases (tests/dynamics_cases.py, tests/golden/dynamics_cases.npz) on the CPU: the float64 reference against closed forms, the
oracle's minv / aba / fk against the reference, the wave emulator's debug records and stored states against the stored scenes -- ALL stored
poses, maxima against the stored limits --, the stored file against a fresh run of the generator, and the comparison itself against planted
errors.  tests/test_gpu_dynamics_cases.py holds the device to the same scenes."""
import os
import sys

import numpy as np
import pytest

import dynamics_cases as DC
from dynamics_cases import LK, FB

SCENES = ('dy_chain', 'dy_tree', 'dy_star', 'dy_two', 'dy_frozen', 'dy_far', 'dy_ratio', 'dy_ratio_up', 'dy_fast', 'dy_free', 'dy_block12', 'dy_block16', 'dy_block22', 'dy_cols')
ORACLE_MEASURED = dict(minv=6.9e-7, qdd=6.4e-7, fk=2.2e-7)      # the largest deviations seen over all stored poses (profiles/dynamics_cases/README.md)
ORACLE_BOUND = {k: min(10 * v, 1e-6) for k, v in ORACLE_MEASURED.items()}


@pytest.fixture(scope='module')
def cases():
    return DC.load_cases()


# ---------------------------------------------------------------------------------------------------- the reference itself
PAR0 = dict(DT=0.02, LIN_DAMP=0.0, ANG_DAMP=0.0, ROBOT_GRAVITY_Z=-9.81, HUMAN_GRAVITY_Z=-9.81)
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _link(parent=-1, jtype=0, tpos=(0, 0, 0), tquat=(0, 0, 0, 1), axis=(0, 1, 0), com=(0, 0, 0), mass=1.0, inertia=(0, 0, 0, 0, 0, 0), jdamp=0.0):
    r = np.zeros(DC.LINK_COLS)
    r[LK['parent']], r[LK['jtype']], r[LK['mass']], r[LK['jdamp']] = parent, jtype, mass, jdamp
    r[LK['tpos']:LK['tpos'] + 3], r[LK['tquat']:LK['tquat'] + 4], r[LK['axis']:LK['axis'] + 3], r[LK['com']:LK['com'] + 3], r[LK['inertia']:LK['inertia'] + 6] = tpos, tquat, axis, com, inertia
    return r


def _ref(rows, q, qd, par=PAR0, base=IDENT, **kw):
    rows = np.array(rows)
    return DC.reference(np.stack([rows, rows]), None, par, len(rows), dict(q=np.array(q, dtype=float), qd=np.array(qd, dtype=float), base=base, hbase=IDENT, free=np.zeros((0, 13)), gender=0, frozen=0), **kw)


def _close(a, b, rel=1e-9):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= rel * max(np.abs(np.asarray(b)).max(), 1e-300)


def test_pendulums():
    """a point mass on a massless rod: qdd = -(g / l) sin q whatever the speed; a body with inertia I about its centre of mass: -m g l sin q / (I + m l^2)"""
    g, l, m, I = 9.81, 0.37, 1.7, 0.05
    for q, qd in ((0.3, 0.0), (-2.1, 1.5), (3.0, -4.0)):
        r = _ref([_link(com=(0, 0, -l), mass=m)], [q], [qd])
        assert _close(r['qdd'], [-(g / l) * np.sin(q)]) and _close(r['minv'], [[1 / (m * l * l)]])
        r = _ref([_link(com=(0, 0, -l), mass=m, inertia=(0.02, I, 0.03, 0, 0, 0))], [q], [qd])
        assert _close(r['qdd'], [-m * g * l * np.sin(q) / (I + m * l * l)])


def test_prismatic_joint_falls_along_its_axis():
    rng = np.random.RandomState(3)
    for _ in range(5):
        a = rng.randn(3); a /= np.sqrt(a @ a)
        tq = rng.randn(4)
        r = _ref([_link(jtype=1, axis=a, tquat=tq, com=rng.randn(3), mass=2.3, inertia=(0.1, 0.2, 0.15, 0.01, 0, 0))], [0.4], [1.1])
        az = (DC.quat_mat(tq) @ a)[2]
        assert _close(r['qdd'], [-9.81 * az]) and _close(r['minv'], [[1 / 2.3]])


def test_planar_double_pendulum():
    """the textbook mass matrix and accelerations in relative angles"""
    m1, m2, l1, l2, g = 1.3, 0.7, 0.5, 0.3, 9.81
    rows = [_link(com=(0, 0, -l1), mass=m1), _link(parent=0, tpos=(0, 0, -l1), com=(0, 0, -l2), mass=m2)]
    for (q1, q2), (w1, w2) in (((0.4, -0.9), (0.0, 0.0)), ((2.2, 1.4), (1.5, -2.5)), ((-1.0, 3.0), (-3.0, 0.7))):
        r = _ref(rows, [q1, q2], [w1, w2])
        M = np.array([[(m1 + m2) * l1 ** 2 + m2 * l2 ** 2 + 2 * m2 * l1 * l2 * np.cos(q2), m2 * l2 ** 2 + m2 * l1 * l2 * np.cos(q2)], [m2 * l2 ** 2 + m2 * l1 * l2 * np.cos(q2), m2 * l2 ** 2]])
        h = np.array([-m2 * l1 * l2 * np.sin(q2) * (2 * w1 * w2 + w2 ** 2) + (m1 + m2) * g * l1 * np.sin(q1) + m2 * g * l2 * np.sin(q1 + q2),
                      m2 * l1 * l2 * np.sin(q2) * w1 ** 2 + m2 * g * l2 * np.sin(q1 + q2)])
        assert _close(r['M'], M) and _close(r['h'], h) and _close(r['qdd'], np.linalg.solve(M, -h)) and _close(r['minv'], np.linalg.inv(M))


def _random_tree(rng, n=6, jdamp=0.0):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'diag'))
    import make_dynamics_cases as G
    par = [-1] + [int(rng.randint(-1, d)) for d in range(1, n)]
    return [G.link_row(rng, par[d], int(rng.rand() < 0.3), False, jdamp=jdamp * rng.rand()) for d in range(n)]


@pytest.mark.parametrize('forces', [False, True])
def test_power_balance(forces):
    """d/dt of the kinetic energy, qd'M qdd + qd'(dM/dt) qd / 2, is the power of gravity and the dampings -- nothing where both are off"""
    rng = np.random.RandomState(11)
    par = dict(PAR0, LIN_DAMP=0.3, ANG_DAMP=0.2) if forces else dict(PAR0, ROBOT_GRAVITY_Z=0.0)
    for _ in range(4):
        rows = np.array(_random_tree(rng, jdamp=0.5 if forces else 0.0))
        q, qd = rng.uniform(-3, 3, 6), rng.uniform(-3, 3, 6)
        r = _ref(rows, q, qd, par)
        m = DC.model_of(rows, None, par, 6)
        Z = (q + 1j * DC.STEP * qd)[None]
        P, R = DC.fk(m, Z, IDENT, IDENT)
        Mdot = DC.mass_matrix(m, *DC.jacobians(m, P, R)[:3])[0].imag / DC.STEP
        P, R = DC.fk(m, q[None], IDENT, IDENT)
        Jv, Jw, Iw, _ = DC.jacobians(m, P, R)
        v, w = np.einsum('dki,k->di', Jv[0], qd), np.einsum('dki,k->di', Jw[0], qd)
        power = 0.0
        if forces:
            sl, sa = 0.3 + 0.3 * np.sqrt((v * v).sum(1)), 0.2 + 0.2 * np.sqrt((w * w).sum(1))
            power = (m['mass'] * -9.81 * v[:, 2]).sum() - (m['mass'] * sl * (v * v).sum(1)).sum() - (sa * np.einsum('di,dij,dj->d', w, Iw[0], w)).sum() - (m['jdamp'] * qd * qd).sum()
        got = qd @ r['M'] @ r['qdd'] + qd @ Mdot @ qd / 2
        scale = np.abs(qd) @ np.abs(r['M']) @ np.abs(r['qdd'])
        assert abs(got - power) <= 1e-9 * scale, (got, power)


def test_complex_step_sizes_agree():
    rng = np.random.RandomState(5)
    rows = np.array(_random_tree(rng))
    q, qd = rng.uniform(-3, 3, 6), rng.uniform(-20, 20, 6)
    a, b = _ref(rows, q, qd, step=1e-20)['C'], _ref(rows, q, qd, step=1e-30)['C']
    assert _close(a, b) and np.abs(a).max() > 1.0


def test_invariance_under_a_motion_of_the_base():
    """a turn about the vertical and any translation of the base leave qdd and M^-1 as they are; without gravity any rigid motion does"""
    rng = np.random.RandomState(8)
    rows = np.array(_random_tree(rng))
    q, qd = rng.uniform(-3, 3, 6), rng.uniform(-3, 3, 6)
    for par, quat in ((PAR0, (0, 0, np.sin(0.6), np.cos(0.6))), (dict(PAR0, ROBOT_GRAVITY_Z=0.0, LIN_DAMP=0.1, ANG_DAMP=0.1), rng.randn(4))):
        a = _ref(rows, q, qd, par)
        b = _ref(rows, q, qd, par, base=np.concatenate([[3.0, -7.0, 2.0], quat]))
        assert _close(a['qdd'], b['qdd']) and _close(a['minv'], b['minv'])


def test_free_body_against_eulers_equations():
    """no damping, no gravity: I dw/dt = -w x I w in the body frame, and a spin about a principal axis stays as it is"""
    rng = np.random.RandomState(2)
    par = dict(PAR0, DT=1e-3)
    I = np.array([0.02, 0.05, 0.03])
    fb = np.array([[1.0, *I, 0.0]])
    m = DC.model_of(np.array([_link()]), fb, par, 1)
    for k in range(4):
        quat = rng.randn(4); quat /= np.sqrt(quat @ quat)
        wb = rng.uniform(-5, 5, 3) if k else np.array([0, 4.0, 0])
        R = DC.quat_mat(quat)
        st = dict(free=np.concatenate([rng.randn(3), quat, rng.randn(3), R @ wb])[None])
        out = DC.free_dynamics(m, st)[0]
        want = R @ (wb + 1e-3 * (-np.cross(wb, I * wb) / I))
        assert _close(out[10:13], want, 1e-12) and _close(out[7:10], st['free'][0, 7:10], 1e-15) and _close(out[:3], st['free'][0, :3] + 1e-3 * st['free'][0, 7:10], 1e-15)
        th = np.sqrt(want @ want) * 1e-3      # the new attitude: the old one turned by |w'| dt about w'
        Rn = DC.quat_mat(out[3:7])
        u = want / np.sqrt(want @ want)
        K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
        assert np.abs(Rn - (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K) @ R).max() < 1e-12
        assert abs(np.sqrt(out[3:7] @ out[3:7]) - 1) < 1e-15


# ---------------------------------------------------------------------------------------------------- the scenes
def _scene_ok(cases, name):
    assert name + '/recipe' in cases, 'scene %s is not in the stored file' % name
    rec = cases[name + '/recipe']
    assert 10 <= len(cases[name + '/q']) <= 64 and 2 * rec['rejected'] <= rec['drawn']


@pytest.mark.parametrize('name', SCENES)
def test_oracle_scene(cases, name):
    """agxo_minv, agxo_aba with the velocity damping and agxo_fk on every stored pose, relative to the block's largest entry (positions: metres)"""
    from oracle_lib import Oracle
    _scene_ok(cases, name)
    blob = DC.scene_blob(cases, name)
    rec = cases[name + '/recipe']
    o = Oracle(blob)
    worst = dict(minv=0.0, qdd=0.0, fk=0.0)
    for p, s in enumerate(DC.scene_states(cases, name)):
        w = DC.stored_result(cases, name, p)
        mi, qdd = o.minv(s.copy()), o.aba(s.copy(), damping=True)
        for b0, b1 in DC._blocks(rec['ndof'], rec['nrobot']):
            if b1 > b0:
                if np.abs(w['minv'][b0:b1, b0:b1]).max() > 0:
                    worst['minv'] = max(worst['minv'], np.abs(mi - w['minv'])[b0:b1, b0:b1].max() / np.abs(w['minv'][b0:b1, b0:b1]).max())
                else:
                    assert (mi[b0:b1, b0:b1] == 0).all()
                if np.abs(w['qdd'][b0:b1]).max() > 0:
                    worst['qdd'] = max(worst['qdd'], np.abs(qdd - w['qdd'])[b0:b1].max() / np.abs(w['qdd'][b0:b1]).max())
                else:
                    assert (qdd[b0:b1] == 0).all()
        st = DC.pose_of(cases, name, p)
        ref = DC.reference(cases[name + '/links'], None, rec['params_all'], rec['nrobot'], st)
        pos, rot = o.fk(s.copy())
        worst['fk'] = max(worst['fk'], np.abs(pos - ref['pos']).max() / max(1.0, np.abs(ref['pos']).max()), np.abs(rot - ref['rot']).max())
    print('dynamics %-10s oracle   M^-1 %.3g  qdd %.3g  link frames %.3g (relative)' % (name, worst['minv'], worst['qdd'], worst['fk']))
    assert all(worst[k] <= ORACLE_BOUND[k] for k in worst), worst


_EMU = {}


def _emulate(cases, name):
    if name not in _EMU:
        from emu_lib import Emu
        blob = DC.scene_blob(cases, name)
        e = Emu(blob)
        lay = [e.DEBUG_WORDS, e.DBG_CON, e.DBG_MINV, e.MINV_STRIDE, e.DBG_HDR, e.DBG_LAM, e.DBG_TIME, e.DBG_QDD]
        res = []
        for s in DC.scene_states(cases, name):
            s2 = s.copy()
            res.append(DC.result_of(e.settle(s2, 1, debug=True), lay, s2, blob))
        _EMU[name] = res
    return _EMU[name]


@pytest.mark.parametrize('name', SCENES)
def test_emulator_scene(cases, name):
    from assistive_gym_amd import variants
    _scene_ok(cases, name)
    rec = cases[name + '/recipe']
    assert variants.pick(DC.scene_blob(cases, name)).name == rec['variant']
    res = _emulate(cases, name)
    m, bad = DC.judge(cases, name, res)
    print(DC.say(name, 'emulator', m))
    assert not bad, bad[:10]
    assert m['n'] == len(cases[name + '/q'])
    dt = np.float32(rec['dt'])
    for p, r in enumerate(res):      # the emulator rounds twice: the product, then the sum
        st = DC.pose_of(cases, name, p)
        qd = st['qd'].astype(np.float32) + dt * r['qdd']
        assert qd.dtype == np.float32 and np.array_equal(qd.view(np.int32), r['qd'].view(np.int32))
        assert np.array_equal((st['q'].astype(np.float32) + dt * qd).view(np.int32), r['q'].view(np.int32))


@pytest.mark.parametrize('name', ['dy_chain', 'dy_tree'])
def test_emulator_four_substeps(cases, name):
    """the reference iterated four times against four substeps of the emulator"""
    from emu_lib import Emu
    steps = cases[name + '/recipe']['steps']
    blob = DC.scene_blob(cases, name)
    e = Emu(blob)
    res = []
    for s in DC.scene_states(cases, name):
        s2 = s.copy()
        e.settle(s2, steps)
        v = blob.view(s2.reshape(1, -1))
        res.append((v['q'][0].copy(), v['qd'][0].copy()))
    m, bad = DC.judge_iterated(cases, name, res)
    print('dynamics %-10s emulator %d substeps, poses %3d | q %.3g rad, %.2f of its limit at most | qd %.3g, %.2f of its limit' % (name, steps, m['n'], m['q'], m['q_of'], m['qd'], m['qd_of']))
    assert steps == 4 and not bad, bad[:10]
    assert m['n'] == len(cases[name + '/q'])


def _oracle_frames(cases, name):
    """(collider frames [poses, ncoll, 12], end-effector poses [poses, 7]) as the device reports them, from the oracle's fk and ee_pose"""
    from oracle_lib import Oracle
    blob = DC.scene_blob(cases, name)
    o = Oracle(blob)
    states = DC.scene_states(cases, name)
    cf, ee = np.zeros((len(states), blob.h['NCOLL'], 12), dtype=np.float32), np.zeros((len(states), 7), dtype=np.float32)
    for p, s in enumerate(states):
        pos, rot = o.fk(s.copy())
        for c in range(blob.h['NCOLL']):
            b = blob.collider(c)['body']
            if 0 <= b < blob.ndof:
                cf[p, c, :3], cf[p, c, 3:] = pos[b], rot[b].reshape(-1)
        ee[p, :3], ee[p, 3:] = o.ee_pose(s.copy())
    return blob, cf, ee


@pytest.mark.parametrize('name', ['dy_tree', 'dy_far'])
def test_oracle_frames(cases, name):
    """the stored link and end-effector frames (what agx_collider_frames and agx_ee_pose are held to on the device) against the oracle's fk and
    ee_pose rounded to float32, at the limits the device gets; and the comparison rejects a frame off by a millimetre or a milliradian"""
    blob, cf, ee = _oracle_frames(cases, name)
    m, bad, n = DC.judge_frames(cases, name, blob, cf, ee)
    print('dynamics %-10s oracle   frames of %d colliders and the end effector | position %.3g m, %.2f of its limit | rotation %.3g, %.2f of its limit' % (name, n, m['pos'], m['pos_of'], m['rot'], m['rot_of']))
    assert not bad, bad[:10]
    assert n >= 10 * len(cases[name + '/q'])
    c = next(c for c in range(blob.h['NCOLL']) if 0 <= blob.collider(c)['body'] < blob.nrobot)
    for plant in ('pos', 'rot', 'ee'):
        cf2, ee2 = cf.copy(), ee.copy()
        if plant == 'pos':
            cf2[3, c, 1] += 1e-3
        elif plant == 'rot':
            cf2[3, c, 3:] = (cf2[3, c, 3:].reshape(3, 3) @ DC.axis_rot(np.array([0, 0, 1.0]), np.array([1e-3]))[0]).reshape(-1)
        else:
            ee2[3, :3] = cf[3, c, :3]
        bad = DC.judge_frames(cases, name, blob, cf2, ee2)[1]
        assert len(bad) == 1 and bad[0].startswith('pose 3, ' + ('end effector' if plant == 'ee' else 'collider %d' % c)), bad


def test_quaternion_of_a_rotation():
    rng = np.random.RandomState(4)
    for _ in range(50):
        q = rng.randn(4); q /= np.sqrt(q @ q)
        if rng.rand() < 0.5:
            q[3] *= 1e-3; q /= np.sqrt(q @ q)      # half a turn: the branches without the trace
        assert np.abs(DC.quat_mat(DC.mat_quat(DC.quat_mat(q))) - DC.quat_mat(q)).max() < 1e-14


def test_scene_coverage(cases):
    """what the scenes are for is in them"""
    from assistive_gym_amd import variants
    want = dict(dy_chain='feeding', dy_block12='feeding_l', dy_block16='feeding_m', dy_block22='arm_manipulation_l', dy_cols='bed_settle')
    for name, v in want.items():
        assert cases[name + '/recipe']['variant'] == v
    row = next(r for r in variants.VARIANTS if r.name == 'bed_settle')
    assert cases['dy_cols/recipe']['ndof'] > (row.max_dof + 1) // 2 > 0 and cases['dy_cols/recipe']['ndof'] > 32      # two batches of columns, two mask words
    assert cases['dy_block22/recipe']['nrobot'] == 22 and cases['dy_block16/recipe']['nrobot'] == 16
    lk = cases['dy_tree/links'][0]
    par, jt = lk[:10, LK['parent']].astype(int), lk[:10, LK['jtype']].astype(int)
    assert any(jt[p] == 1 and (par == p).sum() >= 2 for p in range(10)) and (par == -1).sum() >= 2
    assert (cases['dy_star/links'][0, :10, LK['parent']] == -1).all()
    two = cases['dy_two/recipe']
    assert two['params']['HUMAN_GRAVITY_Z'] != two['params']['ROBOT_GRAVITY_Z'] and set(cases['dy_two/env'][:, 0]) == {0, 1} and (cases['dy_two/env'][:, 1] == 0).all()
    assert not np.array_equal(cases['dy_two/links'][0, 10:], cases['dy_two/links'][1, 10:]) and len(np.unique(cases['dy_two/hbase'], axis=0)) == len(cases['dy_two/hbase'])
    fz = cases['dy_frozen/env'][:, 1]
    assert len(set(fz)) == 5 and (np.abs(cases['dy_frozen/qd']) > 0).all() and cases['dy_frozen/links'][0, 9, LK['mass']] == 0 and cases['dy_frozen/dead'][:, 9].all()
    assert {n for n in cases['dy_far/recipe']['notes']} == {'0.1 m', '3 m', '30 m'} and 'fpos_hi' in ' '.join(k for k in cases if k.startswith('dy_far/')) and 'dy_tree/fquat_hi' in cases
    m = cases['dy_ratio/links'][0, :10, LK['mass']]
    assert m.max() / m.min() >= 9999 and cases['dy_ratio/recipe']['measures']['cond'][0] > 1e5
    assert np.abs(cases['dy_fast/qd']).max() > 15 and cases['dy_fast/recipe']['params']['ROBOT_GRAVITY_Z'] == 0 and cases['dy_fast/links'][0, :, LK['jdamp']].max() > 0.1
    assert 'rest' in cases['dy_chain/recipe']['notes']
    fr, fb = cases['dy_free/free'], cases['dy_free/freeb']
    w = np.sqrt((fr[:, :, 10:13] ** 2).sum(2))
    dt = cases['dy_free/recipe']['dt']      # the substep
    assert (w == 0).any() and ((w > 0) & (w * dt < DC.SMALL_ANGLE)).any() and ((w * dt > DC.SMALL_ANGLE) & (w < 1e-9)).any() and w.max() > 25
    assert (fb[:, FB['inertia']:FB['inertia'] + 3] == 0).sum() == 1 and len(set(fb[:, FB['gravity']])) == len(fb) and np.abs(fr[:, :, 7:10]).max() > 2
    assert {int(x) for x in cases['dy_cols/env'][:, 1]} - {0} and all(int(x) < 2 ** 32 for x in cases['dy_cols/env'][:, 1])


# ---------------------------------------------------------------------------------------------------- the file is what the generator writes
def test_stored_file_is_fresh(cases):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'diag'))
    import make_dynamics_cases as G
    assert set(G.SCENES) == set(SCENES) == set(DC.scenes(cases))
    fresh = G.generate()      # every scene: about a minute
    assert set(fresh) == set(cases)
    for k, v in fresh.items():
        if k.endswith('/recipe'):
            a, b = __import__('json').loads(str(v)), cases[k]
            ma, mb = a.pop('measures'), dict(b).pop('measures')
            assert a == {x: y for x, y in b.items() if x != 'measures'}
            assert all(np.allclose(ma[x], mb[x], rtol=1e-6) for x in ma)
        elif k.endswith('_lo'):      # what float32 leaves of M^-1, in steps of 2e-10 of its largest entry: the same to a step
            assert v.shape == cases[k].shape and (np.abs(v.astype(int) - cases[k]) <= 1).all(), k
        elif v.dtype == np.float64 or k.endswith(('/e', '/eq', 'lim', 'lim4')):
            assert v.shape == cases[k].shape and np.allclose(v, cases[k], rtol=1e-6, atol=1e-300), k
        else:
            assert np.array_equal(v, cases[k]), k
    assert os.path.getsize(DC.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(DC.GOLDEN), 'narrowphase_cases.npz'))


# ---------------------------------------------------------------------------------------------------- the comparison rejects planted errors
PLANTS = ('no_velocity_products', 'human_gravity', 'sibling_on_brother', 'prismatic_as_revolute', 'inertia_product_sign', 'com_inertia', 'cross_block_leak', 'frozen_live',
          'jdamp', 'columns_swapped', 'gender0', 'tquat_transposed', 'small_angle', 'linear_damping')
POSES = 4      # of every scene, the first so many


def _planted(cases, name, plant, p):
    """the record of a device with the planted error at stored pose p, or None where the scene has nothing the error could touch"""
    rec = cases[name + '/recipe']
    n, nr = rec['ndof'], rec['nrobot']
    links = cases[name + '/links'].copy()
    st = DC.pose_of(cases, name, p)
    par0, jt = links[0, :, LK['parent']].astype(int), links[0, :, LK['jtype']].astype(int)
    flaws = ()
    if plant in ('cross_block_leak', 'columns_swapped'):
        r = DC.perfect(cases, name, p)
        if plant == 'cross_block_leak':
            if nr in (0, n):
                return None
            r['minv'][0, nr] = 1e-6
        else:
            if n <= 24:
                return None
            r['minv'][:, [3, 27]] = r['minv'][:, [27, 3]]
        return r
    if plant == 'sibling_on_brother':
        d = next((d for d in range(1, n) if any(par0[c] == par0[d] and (c < nr) == (d < nr) for c in range(d))), None)
        if d is None:
            return None
        links[:, d, LK['parent']] = next(c for c in range(d) if par0[c] == par0[d] and (c < nr) == (d < nr))
    elif plant == 'prismatic_as_revolute':
        if not (jt == 1).any():
            return None
        links[:, int(np.argmax(jt == 1)), LK['jtype']] = 0
    elif plant == 'inertia_product_sign':      # the least conspicuous one: the product that is smallest next to its link's moments
        I = links[0, :, LK['inertia']:LK['inertia'] + 6].astype(np.float64)
        rel = np.where(np.abs(I[:, 3:]) > 0, np.abs(I[:, 3:]) / np.maximum(I[:, :3].sum(1, keepdims=True), 1e-300), np.inf)
        d, k = np.unravel_index(int(np.argmin(rel)), rel.shape)
        links[:, d, LK['inertia'] + 3 + k] *= -1
    elif plant in ('com_inertia', 'jdamp'):      # of one link: the one whose offset (joint damping) is the smallest that is not zero
        size = np.sqrt((links[0, :, LK['com']:LK['com'] + 3].astype(np.float64) ** 2).sum(1)) * (links[0, :, LK['mass']] > 0) if plant == 'com_inertia' else links[0, :, LK['jdamp']].astype(np.float64)
        if not (size > 0).any():
            return None
        flaws = ('%s:%d' % (plant, int(np.argmin(np.where(size > 0, size, np.inf)))),)
    elif plant == 'tquat_transposed':
        links[:, n // 2, LK['tquat']:LK['tquat'] + 3] *= -1
    elif plant == 'gender0':
        if st['gender'] == 0 or nr == n:
            return None
        flaws = ('gender0',)
    elif plant == 'frozen_live':
        if st['frozen'] == 0:
            return None
        flaws = ('frozen_live',)
    else:
        flaws = (plant,)
    fb = cases[name + '/freeb'] if rec['nfree'] else None
    ref = DC.reference(links, fb, rec['params_all'], nr, st, flaws=flaws)
    ref['dead'] = cases[name + '/dead'][p].astype(bool)
    return DC.perfect(cases, name, p, ref)


_REJECTS = {}


def _rejections(cases, loose=False):
    """{(plant, scene)}: the planted errors the comparison rejects, over the first POSES poses of every scene"""
    key = bool(loose)
    if key not in _REJECTS:
        out = set()
        for name in SCENES:
            clean = [DC.perfect(cases, name, p) for p in range(len(cases[name + '/q']))]
            assert not DC.judge(cases, name, clean)[1], 'the exact records of %s do not pass' % name
            for plant in PLANTS:
                res, touched = list(clean), set()
                for p in range(POSES):
                    r = _planted(cases, name, plant, p)
                    if r is not None:
                        res[p] = r
                        touched.add(p)
                if touched and DC.judge(cases, name, res, only=touched, loose=loose)[1]:
                    out.add((plant, name))
        _REJECTS[key] = out
    return _REJECTS[key]


def test_comparison_rejects_planted_errors(cases):
    """every planted error is rejected by at least one scene, every scene rejects at least one"""
    rej = _rejections(cases)
    for plant in PLANTS:
        print('%-22s rejected by %s' % (plant, ' '.join(s for s in SCENES if (plant, s) in rej) or '-'))
    assert all(any((plant, s) in rej for s in SCENES) for plant in PLANTS)
    assert all(any((plant, s) in rej for plant in PLANTS) for s in SCENES)
    assert ('human_gravity', 'dy_two') in rej and ('columns_swapped', 'dy_cols') in rej and ('small_angle', 'dy_free') in rej and ('jdamp', 'dy_fast') in rej


def test_tightened_limits_are_what_rejects(cases):
    """with every limit put back to CAP x scale -- the bound the suite held before -- a scene that rejects the planted sign of an inertia product
    accepts it.  The centre of mass left out of one link's inertia and one joint's damping dropped are rejected at CAP as well, each planted
    on the link where it is smallest: every link of these scenes has its centre of mass centimetres off its joint frame, and dy_fast, the
    one scene with joint damping, turns every joint at radians per second (printed; profiles/dynamics_cases/README.md)"""
    tight, loose = _rejections(cases), _rejections(cases, loose=True)
    passed = {}
    for plant in ('inertia_product_sign', 'com_inertia', 'jdamp'):
        passed[plant] = [s for s in SCENES if (plant, s) in tight and (plant, s) not in loose]
        print('%-22s at 1e-4: accepted by %s' % (plant, ' '.join(passed[plant]) or '-'))
    assert passed['inertia_product_sign']


def test_a_small_error_in_qdd_is_rejected(cases):
    """the error the suite could not see before these cases -- 3e-5 of the block's largest |qdd|, on one DoF -- against the stored limits, on
    every live DoF of every stored pose in turn"""
    share = {}
    for name in SCENES:
        hit = tot = 0
        for p in range(len(cases[name + '/q'])):
            lim, scale = DC.qdd_limits(cases, name, p)
            live = ~cases[name + '/dead'][p].astype(bool) & (scale > 0)
            want = DC.stored_qdd(cases, name, p)
            got = (want + 3e-5 * scale).astype(np.float32).astype(np.float64)
            hit, tot = hit + int((np.abs(got - want) > lim)[live].sum()), tot + int(live.sum())
        print('%-12s a qdd off by 3e-5 of the scale is rejected on %4d of %4d live DoFs of its poses' % (name, hit, tot))
        share[name] = (hit, tot)
    assert all(h > 0 for h, t in share.values()), share
