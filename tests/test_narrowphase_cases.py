"""The narrowphase cases (tests/narrowphase_cases.py, tests/golden/narrowphase_cases.npz) on the CPU: the float64 reference against pairs whose
distance is known by construction, the oracle's gjk against the reference, the oracle's and the wave emulator's contact records against the
stored scenes -- ALL contacts of ALL stored poses, maxima against the stored per-contact limits --, the stored file against a fresh run of the
generator, and the comparison itself against planted errors.  tests/test_gpu_narrowphase_cases.py holds the device to the same scenes."""
import os
import sys

import numpy as np
import pytest

import narrowphase_cases as NC
from narrowphase_cases import CON

SCENES = ('np_counts', 'np_served', 'np_flat', 'np_far', 'np_pen', 'np_micron', 'np_grid', 'np_keep', 'np_wide', 'np_table')


@pytest.fixture(scope='module')
def cases():
    return NC.load_cases()


# ---------------------------------------------------------------------------------------------------- the reference itself
def _frame(rng):
    q = rng.randn(4)
    return NC.quat_to_mat(q), rng.uniform(-1, 1, 3)


def _feature(rng, kind, above):
    """vertices whose support feature towards the plane z = 0 is a vertex, an edge or a face through the origin region, the rest of them
    `above` (+1) or below (-1) the plane by at least a centimetre"""
    base = {'vertex': np.zeros((1, 3)), 'edge': np.array([[-0.03, 0.002, 0], [0.03, -0.002, 0]]),
            'face': np.array([[-0.03, -0.02, 0], [0.03, -0.02, 0], [0.0, 0.03, 0]])}[kind]
    rest = rng.uniform(-0.05, 0.05, (rng.randint(0, 12), 3))
    rest[:, 2] = above * rng.uniform(0.01, 0.06, len(rest))
    return np.concatenate([base, rest])


@pytest.mark.parametrize('ka', ['vertex', 'edge', 'face'])
@pytest.mark.parametrize('kb', ['vertex', 'edge', 'face'])
def test_reference_against_closed_forms(ka, kb):
    """A's support feature at height 0, B's at height d with overlapping projections (both contain the z axis' neighbourhood: the origin
    is a point of each feature), both then turned and moved together: the distance is d, the normal the plane's"""
    rng = np.random.RandomState(['vertex', 'edge', 'face'].index(ka) * 3 + ['vertex', 'edge', 'face'].index(kb))
    for d in (1e-7, 1e-5, 1e-3, 0.0123, 0.04, 0.7):
        A = _feature(rng, ka, -1)
        B = _feature(rng, kb, +1) + (0, 0, d)
        R, p = _frame(rng)
        Aw, Bw = A @ R.T + p, B @ R.T + p
        dist, pa, pb, _ = NC.hull_distance(Aw, Bw)
        assert abs(dist - d) <= 1e-12 * max(1.0, d / 1e-3) + 1e-9 * d
        n = (pb - pa) / dist
        assert np.abs(n - R[:, 2]).max() < 1e-6 * max(1.0, 1e-5 / d)
        # the points are points of the hulls, d apart
        assert NC.point_hull_distance(pa, Aw) < 1e-12 and NC.point_hull_distance(pb, Bw) < 1e-12
        assert abs(NC.point_hull_distance(pa, Bw) - d) <= 1e-9 * d + 1e-12 and abs(NC.point_hull_distance(Aw[0], Aw)) < 1e-15


def test_reference_overlap_and_sampler():
    """overlapping hulls have distance 0; the sampler over the axes returns the smallest axis overlap, that axis, and A's vertex there"""
    A = np.array([[x, y, z] for x in (0, 1.0) for y in (0, 1.0) for z in (0, 1.0)])
    B = A * 0.5 + (0.9, 0.2, 0.3)
    assert NC.hull_distance(A, B)[0] < 1e-12
    dirs = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    dep, k, va, lead, vlead = NC.sampler(A, B, dirs)
    # along d the need is max_B(x.d) - min_A(x.d): 1.4, 0.1, 0.7, 0.8, 0.8, 0.7 for the six axes; A's vertices with x = 1 tie
    assert k == 1 and abs(dep - 0.1) < 1e-15 and va[0] == 1.0 and abs(lead - 0.6) < 1e-12 and vlead == 0.0


def test_oracle_gjk_against_reference():
    """the oracle's float64 gjk on random separated pairs of 1 to 64 vertices: the reference's distance to 1e-9 m"""
    from assistive_gym_amd.blob import ModelBlob
    from oracle_lib import Oracle
    o = Oracle(ModelBlob.load('feeding_jaco'))
    rng = np.random.RandomState(7)
    worst, n = 0.0, 0
    for k in range(100):
        na, nb = rng.randint(1, 65), rng.randint(1, 65)
        A = rng.randn(na, 3) * rng.uniform(0.005, 0.05)
        B = rng.randn(nb, 3) * rng.uniform(0.005, 0.05) + rng.randn(3) * (0.15, 0.05)[k % 2]      # far apart, and close (some overlap)
        d, pa, pb, _ = NC.hull_distance(A, B)
        pen, do, pao, pbo, it = o.gjk(A, B)
        if d < 1e-6:
            assert pen or do < 1e-6
            continue
        assert not pen
        worst, n = max(worst, abs(do - d)), n + 1
        assert abs(np.sqrt(((pao - pbo) ** 2).sum()) - do) < 1e-9
    print('oracle gjk against the reference: %d separated pairs, largest difference %.3g m' % (n, worst))
    assert n > 60 and worst < 1e-9


def test_stored_closed_forms(cases):
    """np_flat is built around its separating planes: the stored reference distances are the clearances, to what rounding the pose to float32 leaves"""
    con, closed = cases['np_flat/con'], cases['np_flat/closed']
    brk = NC.params(NC.scene_blob(cases, 'np_flat'))['brk']
    seen = 0
    for p, a, b, c in closed:
        row = con[(con[:, CON['pose']] == p) & (con[:, CON['ca']] == a) & (con[:, CON['cb']] == b)]
        assert len(row) == (1 if c < brk else 0), (p, c)
        if len(row):
            assert abs(row[0, CON['dist']] - c) < 2e-7
            seen += 1
    assert seen >= 12 and len(closed) == len(cases['np_flat/free'])


# ---------------------------------------------------------------------------------------------------- the scenes
def _scene_ok(cases, name):
    assert name + '/recipe' in cases, 'scene %s is not in the stored file' % name
    assert len(cases[name + '/free']) >= 10
    assert 10 <= len(cases[name + '/free']) <= 64


@pytest.mark.parametrize('name', SCENES)
def test_oracle_scene(cases, name):
    from oracle_lib import Oracle
    _scene_ok(cases, name)
    o = Oracle(NC.scene_blob(cases, name))
    res = [NC.records_of_oracle(o.substep_debug(s.copy())) for s in NC.scene_states(cases, name)]
    m, bad = NC.judge(cases, name, res, full=False)
    print(NC.say(name, 'oracle', m))
    assert not bad, bad[:10]


def _emulate(cases, name):
    from emu_lib import Emu
    e = Emu(NC.scene_blob(cases, name))
    dbg = [e.settle(s.copy(), 1, debug=True) for s in NC.scene_states(cases, name)]
    return e, dbg


@pytest.mark.parametrize('name', SCENES)
def test_emulator_scene(cases, name):
    _scene_ok(cases, name)
    e, dbg = _emulate(cases, name)
    m, bad = NC.judge(cases, name, [NC.records_of_debug(d, e.DBG_CON) for d in dbg])
    print(NC.say(name, 'emulator', m))
    assert not bad, bad[:10]
    if name == 'np_served':      # the pass holds what the scene says it holds: 1, 16, 17 pairs with the big hull, one pass
        notes = cases[name + '/recipe']['notes']
        assert {n for n in notes} == {'1 lanes', '16 lanes', '17 lanes'}
        for d, note in zip(dbg, notes):
            assert int(d[e.DBG_TIME + 13]) == int(note.split()[0]) and int(d[e.DBG_TIME + 14]) == 1
    if name == 'np_grid':      # flushes: the pose beyond the cap runs several passes and drops what the file says
        k = cases[name + '/recipe']['notes'].index('overflow')
        assert cases[name + '/overflow'][k] >= 20 and int(dbg[k][e.DBG_TIME + 13]) >= 200 and int(dbg[k][e.DBG_TIME + 14]) >= 4


def test_scene_coverage(cases):
    """what the scenes are for is in them"""
    c = cases['np_counts/recipe']
    a0, a1, b0, b1 = c['groups'][0][:4]
    na = {x['nvert'] for x in c['colliders'] if a0 <= x['col'] < a1}
    nb = {x['nvert'] for x in c['colliders'] if b0 <= x['col'] < b1}
    assert na == {1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 28} and nb == {1, 2, 8, 32, 33, 63, 64}
    con = cases['np_counts/con']
    assert set(con[:, CON['corral']].astype(int)) >= {1, 2, 3}      # closest features of every kind: vertices, an edge, a face
    radii = {x['radius'] > 0 for x in c['colliders']}
    assert radii == {True, False}
    assert len({n.split()[0] for n in cases['np_far/recipe']['notes']}) == 3
    mc = cases['np_micron/con']
    assert (mc[:, CON['kind']] == 1).sum() >= 5 and (mc[:, CON['kind']] == 0).sum() >= 5
    assert ((mc[:, CON['kind']] == 0) <= (np.abs(mc[:, CON['core']] - 1e-5) < 1e-6)).all()
    assert (cases['np_pen/con'][:, CON['kind']] == 1).all() and len(cases['np_pen/con']) >= 20
    for name, least in (('np_grid', 10), ('np_wide', 9)):
        per = np.bincount(cases[name + '/con'][:, CON['pose']].astype(int))
        assert per.max() == 64 and sum(15 <= n <= 63 for n in per) >= least and cases[name + '/overflow'].max() >= 20
    assert cases['np_wide/recipe']['model'] == 'feeding_sawyer'
    from assistive_gym_amd import variants
    assert variants.pick(NC.scene_blob(cases, 'np_wide')).name == 'feeding_l' and variants.pick(NC.scene_blob(cases, 'np_grid')).name == 'feeding'
    t = cases['np_table/con']
    notes = cases['np_table/recipe']['notes']
    assert {'face', 'tilt', 'edge', 'corner', 'over'} <= set(notes)
    assert (t[:, CON['kind']] == 2).sum() >= 100 and (t[:, CON['kind']] == 0).sum() >= 10
    per_pair = [int(((t[:, CON['pose']] == p) & (t[:, CON['ca']] == a)).sum()) for p in range(len(notes)) for a in set(t[:, CON['ca']])]
    assert {1, 2, 4} <= set(per_pair)      # a vertex alone, a capsule's two ends, a face with its three extra points
    assert len({int(a) for a in t[:, CON['ca']]}) == 6


def test_keep_scene_is_about_velocities_and_ranks(cases):
    """np_keep would not notice a missing velocity term or a missing cut if its contacts were those of the bodies at rest, or of keep = 0"""
    name = 'np_keep'
    blob = NC.scene_blob(cases, name)
    par, table, rows = NC.params(blob), NC.scene_table(cases, name), NC.group_rows(blob)
    assert [(g[4], g[5]) for g in rows] == [(0, 4), (0, 2), (0, 1)]
    con, states = cases[name + '/con'], NC.scene_states(cases, name)
    at_rest = uncut = approaching = receding = 0
    for p in range(0, len(states), 2):
        free = blob.view(states[p:p + 1])['free'][0]
        want = [(int(r[CON['ca']]), int(r[CON['cb']])) for r in con[con[:, CON['pose']] == p]]
        got = [(k['ca'], k['cb']) for k in NC.contact_list(table, rows, free, par)[0]]
        assert got == want
        still = free.copy()
        still[:, 7:] = 0
        at_rest += [(k['ca'], k['cb']) for k in NC.contact_list(table, rows, still, par)[0]] != want
        uncut += len(NC.contact_list(table, [g[:5] + (0,) for g in rows], free, par)[0]) > len(want)
    d = con[:, CON['dist']]
    approaching, receding = int((d > par['slack'] + 1e-4).sum()), len(states) * 8 * 3 - len(con)
    print('np_keep: of %d poses looked at, %d have other contacts at rest, %d more contacts without the cut; %d contacts farther than the slack' % (len(states[::2]), at_rest, uncut, approaching))
    assert at_rest >= 4 and uncut >= 4 and approaching >= 20


# ---------------------------------------------------------------------------------------------------- the file is what the generator writes
def test_stored_file_is_fresh(cases):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'diag'))
    import make_narrowphase_cases as G
    fresh = G.generate(['np_flat', 'np_micron'])
    for k, v in fresh.items():
        if k.endswith('/recipe'):
            assert __import__('json').loads(str(v)) == cases[k]
        elif k.endswith('/con'):
            assert v.shape == cases[k].shape and np.allclose(v, cases[k], rtol=1e-9, atol=1e-12), k
        else:
            assert np.array_equal(v, cases[k]), k
    assert os.path.getsize(NC.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(NC.GOLDEN), 'cloth_kernel_cases.npz'))


# ---------------------------------------------------------------------------------------------------- the comparison rejects planted errors
def _perfect(cases, name):
    """records as a device that computes the reference exactly (rounded to float32) would write them"""
    blob = NC.scene_blob(cases, name)
    table = NC.scene_table(cases, name)
    par = NC.params(blob)
    con, out = cases[name + '/con'], []
    for p in range(len(cases[name + '/free'])):
        want = con[con[:, CON['pose']] == p]
        rec = np.zeros((len(want), 16), dtype=np.float32)
        ri = rec.view(np.int32)
        for r, ii, w in zip(rec, ri, want):
            a, b = table[int(w[CON['ca']])], table[int(w[CON['cb']])]
            ii[NC.C_CA], ii[NC.C_CB], ii[NC.C_BA], ii[NC.C_BB] = w[CON['ca']], w[CON['cb']], a['body'], b['body']
            r[NC.C_PA:NC.C_PA + 3], r[NC.C_PB:NC.C_PB + 3], r[NC.C_DIST] = w[CON['pa']:CON['pa'] + 3], w[CON['pb']:CON['pb'] + 3], w[CON['dist']]
            r[NC.C_N:NC.C_N + 3] = par['dirs'][int(w[CON['ndir']])] if w[CON['kind']] == 1 else w[CON['n']:CON['n'] + 3]
            r[NC.C_MU] = a['friction'] * b['friction']
        out.append([len(rec), rec, int(cases[name + '/overflow'][p])])
    return out


def _perp(n):
    t = np.cross(n, [1.0, 0, 0] if abs(n[0]) < 0.9 else [0, 1.0, 0])
    return t / np.sqrt(t @ t)


_CLEAN = {}
PLANTS = ('dropped', 'swapped', 'dist', 'normal', 'point', 'radius_sign', 'beyond_limit', 'mu', 'overflow')


@pytest.mark.parametrize('plant', PLANTS)
def test_comparison_rejects(cases, plant):
    """one planted error in otherwise exact records of np_served (np_counts for the pair beyond the limit): the comparison names it"""
    name = 'np_counts' if plant == 'beyond_limit' else 'np_served'
    res = _perfect(cases, name)
    if name not in _CLEAN:      # the exact records pass, every pose of them: once per scene
        _CLEAN[name] = NC.judge(cases, name, res)[1]
    assert not _CLEAN[name], _CLEAN[name][:5]
    con = cases[name + '/con']
    table = NC.scene_table(cases, name)
    if plant == 'beyond_limit':      # a pose whose pair is beyond the break distance, reported all the same
        p = next(p for p in range(len(res)) if res[p][0] == 0)
        rec = _perfect(cases, name)[next(q for q in range(len(res)) if res[q][0] == 1)][1]
        res[p][0], res[p][1] = 1, rec
    else:
        p = next(p for p in range(len(res)) if res[p][0] >= 3)
        want = con[con[:, CON['pose']] == p]
        rec = res[p][1]
        # a contact whose limits are tight enough for the planted size: a one-vertex core for the point
        i = next(i for i, w in enumerate(want) if w[CON['lim_pt']] < 5e-6 and w[CON['kind']] == 0) if plant == 'point' else 1
        w = want[i]
        n = rec[i, NC.C_N:NC.C_N + 3].astype(np.float64)
        ra = table[int(w[CON['ca']])]['radius']
        if plant == 'dropped':
            res[p][0], res[p][1] = len(rec) - 1, np.delete(rec, i, 0)
        elif plant == 'swapped':
            rec[[i, i + 1]] = rec[[i + 1, i]]
        elif plant == 'dist':      # twice its limit, the points moved with it: nothing else is wrong with the record
            e = 2 * w[CON['lim_dist']]
            rec[i, NC.C_DIST] = np.float32(w[CON['dist']] + e)
            rec[i, NC.C_PA:NC.C_PA + 3] = (w[CON['pa']:CON['pa'] + 3] + e * n).astype(np.float32)
            assert rec[i, NC.C_DIST] != np.float32(w[CON['dist']])
        elif plant == 'normal':
            ang = 2 * w[CON['lim_ang']]
            n2 = np.cos(ang) * n + np.sin(ang) * _perp(n)
            rec[i, NC.C_N:NC.C_N + 3] = n2.astype(np.float32)
            rec[i, NC.C_PB:NC.C_PB + 3] = (rec[i, NC.C_PA:NC.C_PA + 3].astype(np.float64) - w[CON['dist']] * n2).astype(np.float32)
        elif plant == 'point':      # both points 1e-5 m along the normal towards B: A's leaves its core
            rec[i, NC.C_PA:NC.C_PA + 3] = (w[CON['pa']:CON['pa'] + 3] - 1e-5 * n).astype(np.float32)
            rec[i, NC.C_PB:NC.C_PB + 3] = (w[CON['pb']:CON['pb'] + 3] - 1e-5 * n).astype(np.float32)
        elif plant == 'radius_sign':      # pa = ca + r_a n instead of ca - r_a n, dist to match
            assert ra > 0
            rec[i, NC.C_PA:NC.C_PA + 3] = (w[CON['pa']:CON['pa'] + 3] + 2 * ra * n).astype(np.float32)
            rec[i, NC.C_DIST] = np.float32(w[CON['dist']] + 2 * ra)
        elif plant == 'mu':
            rec[i, NC.C_MU] = np.nextafter(rec[i, NC.C_MU], np.float32(2))
        elif plant == 'overflow':
            res[p][2] += 1
    m, bad = NC.judge(cases, name, res, only={p})
    assert bad, 'the comparison accepts the planted error'
    assert len(bad) <= 2 and all(b.startswith('pose %d:' % p) for b in bad), bad
    word = dict(dropped='pairs differ', swapped='pairs differ', dist='dist off', normal='n turned', point='off their cores', radius_sign='dist off', beyond_limit='pairs differ',
                mu='mu', overflow='dropped at the cap')[plant]
    assert any(word in b for b in bad), bad
