"""The closest-point query on the device (agx_proximity_set / agx_proximity, csrc/agx_proximity.hip) through the C ABI, against the float64
reference and the derived limits of tests/proximity_ref.py: the stored poses of tests/golden/narrowphase_cases.npz as the environments of one
handle, every record and every nearest record judged; the launch shapes, the threshold, pairs turned round, an articulated scene with both
genders, a state that is not finite, the argument checks and the scalar facade."""
import ctypes as C

import numpy as np
import pytest

import narrowphase_cases as NC
import proximity_ref as PR

pytestmark = pytest.mark.gpu
DIST = 0.1
ART_DIST = 0.5      # the articulated scene: after a reset the arm is 11 cm and the spoon 45 cm from the person, so 0.1 would report nothing


@pytest.fixture(scope='module')
def gpu():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


class Run:
    """one handle whose environments are the given states, and the query calls on it"""

    def __init__(self, blob, states):
        from assistive_gym_amd.libagx import Stepper
        self.blob, self.states = blob, np.ascontiguousarray(states, dtype=np.float32)
        self.st = Stepper(blob, len(self.states))
        self.st.set_state(self.states)
        self.n = len(self.states)

    def query(self, max_distance=DIST, env0=0, count=None, records=True, nearest=True):
        import torch
        npairs, nq = self.st.proximity_pairs()
        count = self.n - env0 if count is None else count
        rec = torch.full((count, npairs, 12), float('nan'), dtype=torch.float32, device='cuda:0') if records else None
        near = torch.full((count, nq, 12), float('nan'), dtype=torch.float32, device='cuda:0') if nearest else None
        self.st.proximity(max_distance, rec, near, env0=env0)
        self.st.synchronize()
        return (rec.cpu().numpy() if records else None), (near.cpu().numpy() if nearest else None)


_RUNS = {}


def scene_run(name):
    if name not in _RUNS:
        blob, states, table, par = PR.scene(name)
        _RUNS[name] = (Run(blob, states), table, par)
    return _RUNS[name]


def grid_pairs(table):
    """np_grid: a seeded choice of 200 of its cross-body pairs -- more than 64, no multiple of 64"""
    pairs = PR.cross_body_pairs(table)
    return pairs[np.sort(np.random.RandomState(7).choice(len(pairs), 200, replace=False))]


def check_scene(name, pairs, run, table, par, nqueries=1):
    exp = PR.scene_expected(name, pairs, DIST)
    run.st.proximity_set(pairs, nqueries)
    rec, near = run.query()
    assert not np.isnan(rec[..., :10]).any() and not np.isnan(near[..., :10]).any()      # (words 10 and 11 are integers: pair -1 has a NaN's bits)
    bad, skipped, total = PR.judge_records(rec, exp, pairs, table, par)
    nbad, loose = PR.judge_nearest(near, exp, pairs, nqueries)
    kinds = np.bincount(rec.view(np.int32)[:, :, 10].reshape(-1), minlength=3)
    print('proximity %-10s device: %d records (kind 0 / 1 / 2: %d / %d / %d), %d skipped (cap %d); nearest: %d by dist alone' % (name, total, *kinds[:3], skipped, PR.cap(total), loose))
    assert not bad, '%d violations, e.g. %s' % (len(bad), bad[:5])
    assert not nbad, '%d violations, e.g. %s' % (len(nbad), nbad[:5])
    assert skipped <= PR.cap(total)
    assert np.array_equal(bits(near), bits(PR.nearest_of(rec, pairs, nqueries))), 'the nearest records are not those of the rule over the records'
    return rec, near


# ---------------------------------------------------------------------------------------------------- scenes
@pytest.mark.parametrize('name', PR.SCENES)
def test_stored_scene(gpu, name):
    """all cross-body pairs, every other one turned round (a world box on either side), max_distance 0.1: records and nearest records"""
    run, table, par = scene_run(name)
    check_scene(name, PR.cross_body_pairs(table), run, table, par)


def test_grid_of_200_pairs(gpu):
    """more than 64 pairs: one environment per wave, in rounds of 64 with a partly idle last round; three queries"""
    run, table, par = scene_run('np_grid')
    pairs = grid_pairs(table)
    pairs[:, 2] = np.arange(len(pairs)) % 3
    check_scene('np_grid', pairs, run, table, par, nqueries=3)


# ---------------------------------------------------------------------------------------------------- shapes
def test_launch_shapes(gpu):
    run, table, par = scene_run('np_table')
    full_pairs = PR.cross_body_pairs(table)
    run.st.proximity_set(full_pairs, 1)
    rec, near = run.query()
    again = run.query()
    assert np.array_equal(bits(rec), bits(again[0])) and np.array_equal(bits(near), bits(again[1])), 'the same call twice'
    assert np.array_equal(bits(run.query(nearest=False)[0]), bits(rec)) and np.array_equal(bits(run.query(records=False)[1]), bits(near)), 'records only, nearest only'
    for env0, count in ((run.n - 1, 1), (5, 17), (0, 3)):
        r, m = run.query(env0=env0, count=count)
        assert np.array_equal(bits(r), bits(rec[env0:env0 + count])) and np.array_equal(bits(m), bits(near[env0:env0 + count])), 'a sub-range is the same rows of the full run'
    # one pair; three pairs x 40 environments: 16 environments per wave, the last wave partly idle
    exp = PR.scene_expected('np_table', full_pairs, DIST)
    for sel in ([4], [0, 5, 9]):
        run.st.proximity_set(full_pairs[sel], 1)
        assert run.st.proximity_pairs() == (len(sel), 1)
        r, m = run.query()
        want = rec[:, sel].copy()
        want.view(np.int32)[:, :, 11] = np.arange(len(sel))
        assert np.array_equal(bits(r), bits(want)), 'a record does not depend on the pairs around it'
        assert np.array_equal(bits(m), bits(PR.nearest_of(r, full_pairs[sel], 1)))
        assert not PR.judge_records(r, [[e[k] for k in sel] for e in exp], full_pairs[sel], table, par)[0]
    # two queries over the same pairs, split differently: each agrees with the records
    for split in (np.arange(len(full_pairs)) % 2, (np.arange(len(full_pairs)) >= 3).astype(int)):
        pairs = full_pairs.copy()
        pairs[:, 2] = split
        run.st.proximity_set(pairs, 2)
        r, m = run.query()
        assert np.array_equal(bits(r), bits(rec)) and np.array_equal(bits(m), bits(PR.nearest_of(rec, pairs, 2)))
        assert not PR.judge_nearest(m, exp, pairs, 2)[0]


# ---------------------------------------------------------------------------------------------------- threshold
@pytest.mark.parametrize('name', ['np_table', 'np_served', 'np_micron'])
def test_threshold(gpu, name):
    """max_distance 0.02: bit for bit the 0.1 run on every record that is determined and below 0.02, kind 0 elsewhere"""
    run, table, par = scene_run(name)
    pairs = PR.cross_body_pairs(table)
    run.st.proximity_set(pairs, 1)
    wide, _ = run.query(DIST)
    tight, _ = run.query(0.02)
    exp = PR.scene_expected(name, pairs, 0.02, limits=False)
    below = same = 0
    for p in range(run.n):
        for k in range(len(pairs)):
            if not exp[p][k]['determined']:
                continue
            if exp[p][k]['kind'] != 0:
                below += 1
                same += np.array_equal(bits(tight[p, k]), bits(wide[p, k]))
                assert wide[p, k, 0] < 0.02
            else:
                assert tight[p, k].view(np.int32)[10] == 0 and np.isposinf(tight[p, k, 0]) and not tight[p, k, 1:10].any()
    print('proximity %-10s threshold: %d records below 0.02, %d bit-equal to the 0.1 run' % (name, below, same))
    assert below > 0 and same == below


# ---------------------------------------------------------------------------------------------------- swap
@pytest.mark.parametrize('name', ['np_table', 'np_far'])
def test_pairs_turned_round(gpu, name):
    """(b, a) for (a, b): dist within the limit, n negated, the points exchanged -- within the limits, not bit for bit.  Closest points
    (kind 1); an overlap's points are anchored on A's vertex by definition and do not turn with the pair: dist and n are compared"""
    run, table, par = scene_run(name)
    pairs = PR.cross_body_pairs(table)
    turned = pairs.copy()
    turned[:, 0], turned[:, 1] = pairs[:, 1], pairs[:, 0]
    exp = PR.scene_expected(name, pairs, DIST)
    run.st.proximity_set(pairs, 1)
    rec, _ = run.query()
    run.st.proximity_set(turned, 1)
    rev, _ = run.query()
    assert not PR.judge_records(rev, PR.scene_expected(name, turned, DIST), turned, table, par)[0]
    n = 0
    for p in range(run.n):
        for k, (a, b, _) in enumerate(pairs):
            e = exp[p][k]
            if not e['determined'] or e['kind'] == 0:
                continue
            back = PR.unswap(rev[p, k])
            assert abs(float(back[0]) - float(rec[p, k, 0])) <= 2 * e['lim'][0]
            if e['kind'] == 2:
                assert np.array_equal(bits(back[7:10]), bits(rec[p, k, 7:10]))
                continue
            assert not PR.judge_record(back, e, table[int(a)], table[int(b)], par)[0], 'the record of (b, a), turned back, is within the limits of (a, b)'
            n += 1
    assert n > 0


# ---------------------------------------------------------------------------------------------------- an articulated scene
@pytest.fixture(scope='module')
def jaco(gpu):
    """8 states of the FeedingJaco trajectory fixture: its first and last state, stepped 0 to 3 times with its actions, both genders"""
    from assistive_gym_amd.blob import ModelBlob
    blob = ModelBlob.load('feeding_jaco')
    z = np.load(NC.GOLDEN.replace('narrowphase_cases.npz', 'feeding_jaco_oracle_traj.npz'))
    run = Run(blob, np.stack([z['state0'], z['state_end']] * 4))
    for k in range(3):
        act = np.where((np.arange(8) // 2 > k)[:, None], z['actions'][k], 0.0).astype(np.float32)
        run.st.step_host(act)
    states = run.st.get_state()
    blob.view(states)['gender'][:] = [0, 0, 1, 1, 0, 1, 0, 1]
    run.st.set_state(states)
    run.states = states
    return run


def test_articulated_scene(jaco):
    """robot x human and tool x human on FeedingJaco; the reference is fed the device's own collider frames, so the query kernel is judged
    alone.  Colliders of the other gender report nothing in exactly the environments of that gender"""
    import torch
    from assistive_gym_amd import proximity as P
    blob, st = jaco.blob, jaco.st
    pairs = P.expand(blob, [('robot', 'human'), ('tool', 'human')])
    st.proximity_set(pairs, 2)
    rec, near = jaco.query(ART_DIST)
    frames = torch.zeros((jaco.n, st.collider_count(), 12), dtype=torch.float32, device='cuda:0')
    st.collider_frames(frames)
    st.synchronize()
    frames = frames.cpu().numpy().astype(np.float64)
    table, par, flags = PR.collider_table(blob, sorted(set(pairs[:, 0]) | set(pairs[:, 1]))), NC.params(blob), PR.collider_flags(blob)
    gender = blob.view(jaco.states)['gender']
    exp, absent = [], 0
    for e in range(jaco.n):
        row = []
        for k, (a, b, _) in enumerate(pairs):
            if not (flags[a] & flags[b] & (1 << int(gender[e] == 1))):
                row.append(PR._nothing())
                absent += 1
                assert rec[e, k].view(np.int32)[10] == 0
            else:
                row.append(PR.expected(table[int(a)], table[int(b)], frames[e, a], frames[e, b], par, ART_DIST, seed=1000 * e + k))
        exp.append(row)
    assert 0 < absent < jaco.n * len(pairs)
    bad, skipped, total = PR.judge_records(rec, exp, pairs, table, par)
    nbad, loose = PR.judge_nearest(near, exp, pairs, 2)
    kinds = np.bincount(rec.view(np.int32)[:, :, 10].reshape(-1), minlength=3)
    print('proximity feeding_jaco device: %d records (kind 0 / 1 / 2: %d / %d / %d; %d of the other gender), %d skipped (cap %d); nearest: %d by dist alone'
          % (total, *kinds[:3], absent, skipped, PR.cap(total), loose))
    assert not bad, '%d violations, e.g. %s' % (len(bad), bad[:5])
    assert not nbad, '%d violations, e.g. %s' % (len(nbad), nbad[:5])
    assert skipped <= PR.cap(total) and kinds[1] > 100 and (near.view(np.int32)[:, :, 10] != 0).any()
    assert np.array_equal(bits(near), bits(PR.nearest_of(rec, pairs, 2)))


def test_read_only_and_not_finite(jaco):
    """the query leaves the state records alone; an environment with a NaN in a free body's position reports nothing for the pairs of that
    body, writes no NaN, and leaves every other environment's records bit for bit as they were"""
    from assistive_gym_amd import proximity as P
    blob, st = jaco.blob, jaco.st
    pairs = P.expand(blob, [('tool', 'human'), ('robot', 'human')])
    st.proximity_set(pairs, 2)
    before = st.get_state()
    rec, near = jaco.query(ART_DIST)
    assert np.array_equal(bits(st.get_state()), bits(before)), 'get_state before and after'
    tool_body = blob.collider(P.colliders(blob, 'tool')[0])['body']
    assert 200 <= tool_body < 300, 'the tool is a free body'
    broken = before.copy()
    blob.view(broken)['free'][3, tool_body - 200, 1] = np.nan
    st.set_state(broken)
    try:
        r2, n2 = jaco.query(ART_DIST)
    finally:
        st.set_state(before)
    assert not np.isnan(r2[..., :10]).any() and not np.isnan(n2[..., :10]).any()      # (words 10 and 11 are integers: pair -1 has a NaN's bits)
    others = [e for e in range(jaco.n) if e != 3]
    assert np.array_equal(bits(r2[others]), bits(rec[others])) and np.array_equal(bits(n2[others]), bits(near[others]))
    on_tool = np.array([blob.collider(int(a))['body'] == tool_body or blob.collider(int(b))['body'] == tool_body for a, b, _ in pairs])
    assert on_tool.any() and (rec[3, on_tool].view(np.int32)[:, 10] != 0).any() and (r2[3, on_tool].view(np.int32)[:, 10] == 0).all() and np.isposinf(r2[3, on_tool, 0]).all() and not r2[3, on_tool, 1:10].any()
    assert np.array_equal(bits(r2[3, ~on_tool]), bits(rec[3, ~on_tool]))
    assert np.array_equal(bits(n2), bits(PR.nearest_of(r2, pairs, 2)))


# ---------------------------------------------------------------------------------------------------- errors
def test_argument_checks(gpu):
    import torch
    from assistive_gym_amd import libagx
    from assistive_gym_amd.blob import ModelBlob
    blob = ModelBlob.load('feeding_jaco')
    st = libagx.Stepper(blob, 4)
    lib, h, ncoll = st.L, st.h, blob.h['NCOLL']
    out = torch.zeros((4, 2, 12), dtype=torch.float32, device='cuda:0')

    def refused(rc, text, code=-1):
        assert rc == code and text in lib.agx_last_error(), (rc, lib.agx_last_error())

    def set_(rows, nq=1, n=None):
        a = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 3)
        return lib.agx_proximity_set(h, a.ctypes.data_as(C.c_void_p), len(a) if n is None else n, nq)
    n, q = C.c_int(7), C.c_int(7)
    assert lib.agx_proximity_pairs(h, C.byref(n), C.byref(q)) == 0 and (n.value, q.value) == (0, 0)
    refused(lib.agx_proximity(h, 0, 4, 0.1, out.data_ptr(), None, None), b'agx_proximity_set first')
    refused(lib.agx_proximity_set(h, None, 1, 1), b'null pair list')
    refused(set_([[0, 1, 0]], n=0), b'npairs')
    refused(set_([[0, 1, 0]], nq=0), b'nqueries outside 1..16')
    refused(set_([[0, 1, 0]], nq=17), b'nqueries outside 1..16')
    refused(set_([[0, ncoll, 0]]), b'outside [0, ncoll)')
    refused(set_([[-1, 1, 0]]), b'outside [0, ncoll)')
    refused(set_([[5, 5, 0]]), b'with itself')
    refused(set_([[0, 1, 1]]), b'query id outside')
    refused(set_([[0, 1, -1]]), b'query id outside')
    refused(set_(np.tile([[0, 1, 0]], (8193, 1))), b'8,192', code=-5)
    assert lib.agx_proximity_pairs(h, C.byref(n), C.byref(q)) == 0 and (n.value, q.value) == (0, 0), 'a refused list sets nothing'
    assert set_([[0, 20, 0], [1, 20, 0]]) == 0 and lib.agx_proximity_pairs(h, C.byref(n), C.byref(q)) == 0 and (n.value, q.value) == (2, 1)
    for env0, count in ((-1, 2), (0, 0), (0, 5), (3, 2)):
        refused(lib.agx_proximity(h, env0, count, 0.1, out.data_ptr(), None, None), b'not a range')
    for d in (-0.1, float('nan'), float('inf')):
        refused(lib.agx_proximity(h, 0, 4, d, out.data_ptr(), None, None), b'max_distance')
    refused(lib.agx_proximity(h, 0, 4, 0.1, None, None, None), b'both outputs')
    refused(lib.agx_proximity(h, 0, 4, 0.1, out.data_ptr() + 4, None, None), b'aligned')
    assert lib.agx_proximity(h, 0, 4, 0.1, out.data_ptr(), None, None) == 0
    st.synchronize()
    st.close()


# ---------------------------------------------------------------------------------------------------- the facade
def test_scalar_facade(gpu):
    from assistive_gym_amd import proximity as P
    from assistive_gym_amd.envs import make
    from assistive_gym_amd.proximity import ProximityQuery
    env = make('FeedingJaco-v1')
    env.seed(3)
    env.reset()
    out = env.tool.get_closest_points(env.human, distance=5.0)
    assert len(out) == 5 and len({len(x) for x in out}) == 1 and len(out[0]) > 0
    assert all(len(p) == 3 for p in out[2] + out[3]) and all(d < 5.0 for d in out[4])
    q = ProximityQuery(env._ensure_stepper(), [('tool', 'human')], distance=5.0)
    near = q.nearest()
    assert float(near['distance'][0, 0]) == np.float32(min(out[4])) and int(near['kind'][0, 0]) != 0
    k = int(near['pair'][0, 0])
    assert q.blob.collider(int(q.pairs[k, 0]))['tag'] == 2 and q.blob.collider(int(q.pairs[k, 1]))['tag'] == 3
    link = env.blob.collider(P.colliders(env.blob, 'robot')[-1])['link']
    some = env.robot.get_closest_points(env.human, distance=0.5, linkA=link)
    assert len(some) == 5 and set(some[0]) <= {link}
    assert env.tool.get_closest_points(env.human, distance=5.0)[4] == out[4], 'another query in between does not change the answer'
    with pytest.raises(NotImplementedError):
        env.robot.get_pos_orient(3)
    env.disconnect()
