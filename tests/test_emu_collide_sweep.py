"""The windowed sweep of collide() (csrc/agx_collide.h, AGX_FRONT_SWEEP) on the CPU wave emulator.  The default build sweeps a window of consecutive
live pair groups at once: level 1 over the concatenated collider ranges, one level-2 pair grid over the concatenated pair counts, the survivors
appended by ballot rank; -DAGX_FRONT_SWEEP=0 alone sweeps one live group at a time, as the kernel did before the switch existed.  The worklist is
defined as the overlapping pairs in enumeration order and the units are flushed where the serial loop flushes them, so both must end every env step
in the SAME BITS: observation, reward, done, info, the state record and the debug record of the first substep (the words of
tests/test_emu_collide_front.py).  Further kinds cut the windows short -- a small list area (-DAGX_SWEEP_TEST_LIST), at most 1 or 2 groups per
window (-DAGX_SWEEP_TEST_WINDOW) -- and are compared with the same serial kind.  The debug words DBG_TIME + 20 .. 23 (sweeps = windows of the
substep, level-2 rounds, level-1 rounds, live groups) show that the default really merges groups and that the cut kinds really cut."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import emu_lib
from assistive_gym_amd.blob import ModelBlob
from test_emu_collide_front import _states, _words

# A list area of 100 indices instead of 256: the lists of an ordinary FeedingJaco substep (some 270 indices over 12 to 14 live groups) are cut
# into four windows or more.  A group whose own two lists exceeded the area would be swept with what fits and counted as overflow, which the
# serial kind does not do: the comparison would fail, and the overflow count is asserted to be zero besides.
LIST = 100
G_STRIDE, G_B0F = 8, 4      # include/agx_blob.h: words of a pair-group record, its female B range (-1: none)
FEMALE_GROUPS = [2, 9, 10, 11, 28]      # the groups of feeding_jaco whose B range depends on the gender


def _kinds(b, cuts):
    """the default kind, the serial kind, and one kind per entry of `cuts` (tag, flags)"""
    base = emu_lib.variants.pick(b).name
    serial = 'sweep_serial_%s' % base
    emu_lib.derive(serial, base, ['-DAGX_FRONT_SWEEP=0'])
    out = {'default': base, 'serial': serial}
    for tag, flags in cuts:
        out[tag] = 'sweep_%s_%s' % (tag, base)
        emu_lib.derive(out[tag], base, flags)
    return out


def _rollout(b, states, kinds, steps, what):
    """random-action rollouts (every third action three times as large) of every state through all kinds side by side; every kind agrees with
    the serial one in every word after every step.  -> per kind, the (windows, level-2 rounds, level-1 rounds, live groups) of every step's
    first substep, and the overflow counts"""
    E = {t: emu_lib.Emu(b, kind=k) for t, k in kinds.items()}
    T = E['default'].DBG_TIME
    rng = np.random.RandomState(13)
    stat, over = {t: [] for t in E}, []
    with ThreadPoolExecutor(len(E)) as pool:
        for i, s0 in enumerate(states):
            s = {t: s0.copy() for t in E}
            for t in E:
                E[t].forget_warm()
            for j in range(steps):
                a = (rng.uniform(-1, 1, b.act_dim) * (3.0 if j % 3 == 2 else 1.0)).astype(np.float32)
                fut = {t: pool.submit(E[t].step, s[t], a, True) for t in E}
                raw = {t: fut[t].result() for t in E}
                ref = _words(E['serial'], raw['serial'], s['serial'])
                for t in E:
                    if t == 'serial':
                        continue
                    out = _words(E[t], raw[t], s[t])
                    for k in ref:
                        assert np.array_equal(out[k], ref[k]), '%s state %d step %d: %s differs between the %s kind and -DAGX_FRONT_SWEEP=0' % (what, i, j, k, t)
                for t in E:
                    stat[t].append([int(x) for x in raw[t][4][T + 20:T + 24]])
                over.append(int(raw['serial'][4][2]))
    return {t: np.array(v) for t, v in stat.items()}, over


@pytest.fixture(scope='module')
def settled(blob, oracle):
    """two settled start states of FeedingJaco (the pool's 25 settle substeps), one of each gender"""
    from assistive_gym_amd.host.reset import make_states
    st, _ = make_states(blob, 8, seed=4242)
    gender = blob.view(st)['gender']
    pick = [int(np.flatnonzero(gender == 0)[0]), int(np.flatnonzero(gender == 1)[0])]
    out = []
    for i in pick:
        oracle.settle(st[i], 25)
        out.append(st[i].copy())
    return out


def test_feeding_jaco_windows_merge_and_cut_windows_agree(blob, settled):
    """(a) 2 settled states x 10 steps, both genders: the female state takes the female B range of groups 2, 9, 10, 11 and 28.
    (b) the same rollout with a list area of LIST indices, and with at most 1 and 2 groups per window.
    (c) the default has fewer windows per substep than live groups; the cut kinds have more windows than the default."""
    gender = [int(blob.view(s)['gender'][0]) for s in settled]
    assert sorted(gender) == [0, 1], 'fixture: one state of each gender, got %s' % gender
    og = blob.h['OFF_GROUP']
    female = [g for g in range(blob.h['NGROUP']) if int(blob.i[og + G_STRIDE * g + G_B0F]) >= 0]
    assert female == FEMALE_GROUPS, 'the groups with a female B range: %s' % female
    b = blob.set_param('NITER', 12)          # 12 solver sweeps instead of 50, as the other emulator tests
    kinds = _kinds(b, [('list%d' % LIST, ['-DAGX_SWEEP_TEST_LIST=%d' % LIST]), ('window1', ['-DAGX_SWEEP_TEST_WINDOW=1']), ('window2', ['-DAGX_SWEEP_TEST_WINDOW=2'])])
    stat, over = _rollout(b, settled, kinds, 10, 'feeding_jaco')
    assert max(over) == 0, 'nothing overflows in these rollouts, the lists of a group under the short list area included'
    d = stat['default']
    print('feeding_jaco, first substeps: live groups %.1f; windows default %.1f, list area %d: %.1f, one group %.1f, two groups %.1f, serial sweeps %.1f; level-2 rounds default %.1f, serial %.1f; level-1 rounds default %.1f, serial %.1f'
          % (d[:, 3].mean(), d[:, 0].mean(), LIST, stat['list%d' % LIST][:, 0].mean(), stat['window1'][:, 0].mean(), stat['window2'][:, 0].mean(), stat['serial'][:, 0].mean(),
             d[:, 1].mean(), stat['serial'][:, 1].mean(), d[:, 2].mean(), stat['serial'][:, 2].mean()))
    assert (d[:, 3] >= 8).all(), 'the rollout must keep the arm among the table and wheelchair groups: live groups %s' % d[:, 3]
    assert (d[:, 0] < d[:, 3]).all(), 'the default must merge groups: windows %s, live groups %s' % (d[:, 0], d[:, 3])
    for t in ('list%d' % LIST, 'window1', 'window2'):
        assert (stat[t][:, 3] == d[:, 3]).all()
        assert (stat[t][:, 0] > d[:, 0]).all(), 'the %s kind must cut the windows of every substep: %s against %s' % (t, stat[t][:, 0], d[:, 0])
    assert (stat['window1'][:, 0] >= d[:, 3]).all() and (stat['serial'][:, 0] >= d[:, 3]).all(), 'one group per window: a sweep per live group at least'


@pytest.mark.parametrize('name, module, coop', [('feeding_stretch', 'reset', False), ('scratch_itch_pr2', 'reset_scratch', True)], ids=['feeding_stretch', 'scratch_itch_pr2'])
def test_other_models_bit_identical(name, module, coop):
    """feeding_stretch: a robot standing on the ground plane -- several face groups (every pair enumerated 1 + AGX_FACE_EXTRA times) in one window;
    scratch_itch_pr2 with an active human.  2 states x 6 steps each."""
    b = ModelBlob.load(name)
    b = (b.coop() if coop else b).set_param('NITER', 12)
    stat, over = _rollout(b, _states(b, module, 2, 7001), _kinds(b, []), 6, name)
    d = stat['default']
    print('%s: live groups %.1f, windows %.1f, serial sweeps %.1f, overflow %d' % (name, d[:, 3].mean(), d[:, 0].mean(), stat['serial'][:, 0].mean(), sum(over)))
    assert (d[:, 0] < d[:, 3]).all(), 'the default must merge groups: windows %s, live groups %s' % (d[:, 0], d[:, 3])
