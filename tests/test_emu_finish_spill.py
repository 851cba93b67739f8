"""The finish kernel's spill query (csrc/agx_task.h, env_finish_feeding) on the CPU wave emulator: the default build proves "some spoon piece is
within SPILL_DIST of this particle" from the collider AABBs where that is decided by more than a millimetre and runs the narrowphase for the rest;
-DAGX_FINISH_SPILL_GJK runs the narrowphase for every live particle, as the kernel did before.  Both must end every env step in the SAME BITS:
observation, reward, done, info and the whole state record (alive / active masks, RNG words, success counter included).
The -DAGX_EMU_TRACE_GJK twins of both builds show which path ran: a narrowphase pass of the finish is one whose recorded limit exceeds 0.1 m
(SPILL_DIST + radii; the build kernel's speculative limits are centimetres)."""
import ctypes as C
import os

import numpy as np
import pytest

import emu_lib
from assistive_gym_amd.host.reset import make_states

emu_lib.derive('feeding_finish_gjk', 'feeding', ['-DAGX_FINISH_SPILL_GJK'])
emu_lib.derive('feeding_trace_finish_gjk', 'feeding', ['-DAGX_EMU_TRACE_GJK', '-DAGX_FINISH_SPILL_GJK'])
BUILDS = ('feeding', 'feeding_finish_gjk')              # the default (shortcut) and the switch
TRACED = {'feeding': 'feeding_trace', 'feeding_finish_gjk': 'feeding_trace_finish_gjk'}
N_STATES, N_STEPS = 6, 30
FAR_MARGIN_UM = 100                             # GJK_FAR_MARGIN (csrc/agx_collide.h): the traced limit is SPILL_DIST + radii + this


@pytest.fixture(scope='module')
def settled(blob, oracle):
    """settled start states: the food rests on the spoon (the pool's 25 settle substeps)"""
    st, _ = make_states(blob, N_STATES, seed=4242)
    for i in range(N_STATES):
        oracle.settle(st[i], 25)
    assert (blob.view(st)['food_alive'] == (1 << blob.nfood) - 1).all(), 'fixture: every particle must be alive after the settle'
    return st


@pytest.fixture(scope='module')
def cases():
    """the crafted placements of particle 0 (tests/diag/make_finish_spill_cases.py wrote them, and says how)"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'finish_spill_cases.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def emus(blob):
    """12 solver sweeps instead of 50, as tests/test_emu_parity.py: the finish does not look at the solver, and a step emulates in a third of the time"""
    b12 = blob.set_param('NITER', 12)
    return {k: emu_lib.Emu(b12, kind=k) for k in BUILDS + tuple(TRACED.values())}


def _step(e, state, action):
    """one env step from a copy of `state` without warm-start memory -> every output and the new record, as raw words"""
    s = state.copy()
    e.forget_warm()
    obs, rew, done, info, _ = e.step(s, action)
    return dict(obs=obs.view(np.uint32), reward=np.float32(rew).view(np.uint32), done=np.uint8(done), info=info.view(np.uint32), state=s.view(np.uint32)), s


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), '%s: %s differs between the default build and -DAGX_FINISH_SPILL_GJK' % (what, k)


def finish_trace(e, state, action):
    """(narrowphase passes of the finish, surface separation in metres of the first such pass: the smallest any of its lanes reported, every
    output as raw words) of one env step on a traced build"""
    tr = (C.c_int * (1 << 22)).in_dll(e.L, 'g_gjk_trace'); n = C.c_int.in_dll(e.L, 'g_gjk_n')
    n.value = 0
    out, _ = _step(e, state, action)
    t = np.frombuffer(tr, dtype=np.int32, count=n.value).reshape(-1, 9)
    f = t[t[:, 8] > 100000]
    f0 = f[f[:, 0] == f[0, 0]] if len(f) else f          # the first of them: the lowest live particle that was not proven near
    sep = ((f0[:, 7] - (f0[:, 8] - 100000 - FAR_MARGIN_UM)).min() * 1e-6) if len(f0) else None      # core distance - radii
    return len(np.unique(f[:, 0])), sep, out


def _both(blob, emus, state, what):
    """one zero-action step of `state` through the default build and the switch build: the same bits; -> the new record"""
    a = np.zeros(blob.act_dim, dtype=np.float32)
    ref, s1 = _step(emus['feeding'], state, a)
    _same(ref, _step(emus['feeding_finish_gjk'], state, a)[0], what)
    return ref, blob.view(s1)


def test_resting_food_is_proven_near(blob, emus, cases):
    """(a) food resting on the spoon: the default build runs NO narrowphase pass in the finish, the switch build one per live particle"""
    a = np.zeros(blob.act_dim, dtype=np.float32)
    passes, _, out = finish_trace(emus['feeding_trace'], cases['resting'], a)
    passes_gjk, sep, out_gjk = finish_trace(emus['feeding_trace_finish_gjk'], cases['resting'], a)
    assert passes == 0 and passes_gjk == blob.nfood, (passes, passes_gjk)
    assert sep < 0.02                                    # touching, give or take: decided by centimetres
    _same(out, out_gjk, 'resting (traced builds)')
    ref, v1 = _both(blob, emus, cases['resting'], 'resting')
    _same(ref, out, 'resting (traced against plain)')
    assert int(v1['food_alive'][0]) == (1 << blob.nfood) - 1


@pytest.mark.parametrize('case, near', [('shell_in', True), ('shell_out', False)])
def test_shell_around_the_limit_takes_the_narrowphase(blob, emus, cases, case, near):
    """(b) 0.095-0.105 m from the nearest spoon piece, either side of SPILL_DIST: the bound cannot decide, the narrowphase does, in both builds"""
    a = np.zeros(blob.act_dim, dtype=np.float32)
    passes, sep, out = finish_trace(emus['feeding_trace'], cases[case], a)
    assert passes >= 1
    assert (0.095 < sep < 0.1) if near else (0.1 < sep < 0.105), sep
    ref, v1 = _both(blob, emus, cases[case], case)
    _same(ref, out, case + ' (traced against plain)')
    assert bool(int(v1['food_alive'][0]) & 1) == near          # 2 mm inside the limit it stays, 2 mm outside it is spilled


def test_far_particle_is_spilled(blob, emus, cases):
    """(c) more than 0.3 m from the spoon"""
    _, v1 = _both(blob, emus, cases['far'], 'far')
    assert int(v1['food_alive'][0]) == (1 << blob.nfood) - 2


def test_eaten_particle_draws_from_the_rng(blob, emus, cases):
    """(d) within MOUTH_DIST of the target after the step's free fall: eaten, teleported with three draws -- the particles after it in the loop
    see the same RNG and the same poses in both builds"""
    v = blob.view(cases['mouth'].copy())
    _, v1 = _both(blob, emus, cases['mouth'], 'mouth')
    assert int(v1['task_success'][0]) == int(v['task_success'][0]) + 1 and int(v1['food_alive'][0]) == (1 << blob.nfood) - 2
    assert not np.array_equal(v1['rng'][0], v['rng'][0]) and (v1['free'][0, blob.h['FOOD0'], :3] >= 1000.0).all()


def test_rollouts_bit_identical(blob, emus, settled):
    """6 settled states x 30 random-action steps, every third action three times as large (food leaves the spoon): the same bits after every step"""
    from concurrent.futures import ThreadPoolExecutor
    rng = np.random.RandomState(13)          # (a sequence after which four of the six states have lost food: the spilled branch is in the comparison)
    lost = 0
    pool = ThreadPoolExecutor(2)                  # the two builds are two libraries with their own emulator state: they step side by side
    for i in range(N_STATES):
        sa, sb = settled[i].copy(), settled[i].copy()
        emus['feeding'].forget_warm(); emus['feeding_finish_gjk'].forget_warm()
        for k in range(N_STEPS):
            a = (rng.uniform(-1, 1, blob.act_dim) * (3.0 if k % 3 == 2 else 1.0)).astype(np.float32)
            fa, fb = pool.submit(emus['feeding'].step, sa, a), pool.submit(emus['feeding_finish_gjk'].step, sb, a)
            oa, ob = fa.result(), fb.result()
            what = 'state %d step %d' % (i, k)
            assert np.array_equal(oa[0].view(np.uint32), ob[0].view(np.uint32)), what + ': observation'
            assert np.float32(oa[1]).view(np.uint32) == np.float32(ob[1]).view(np.uint32) and oa[2] == ob[2], what + ': reward / done'
            assert np.array_equal(oa[3].view(np.uint32), ob[3].view(np.uint32)), what + ': info'
            assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), what + ': state record'
        lost += blob.nfood - bin(int(blob.view(sa)['food_alive'][0])).count('1')
    pool.shutdown()
    assert lost > 0, 'the rollouts must contain particles that left the spoon'
