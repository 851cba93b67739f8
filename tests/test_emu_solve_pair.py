"""Two environments per wavefront in the solve kernel (csrc/agx_pgs_lvw.h pgs_lvw_pair, csrc/agx_env.h env_solve_pair; -DAGX_SOLVE_PAIR, the default of the
feeding variant): the C++ twin of the paired sweep on the CPU wave emulator against two single env_solve runs, BIT FOR BIT -- state records and scratch
records (the solved impulses of the contacts) after every substep of an env.step().  Each environment of a pair visits its rows in the order it
would alone (rows of a step share no velocity slot), so not a bit may move.  tests/emu/emu_pair.cpp hosts the two environments in one emulated wavefront."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from assistive_gym_amd.host.reset import make_states

import emu_lib

PAIR_CPP = os.path.join(emu_lib.EMU, 'emu_pair.cpp')
emu_lib.derive('feeding_pair_40steps', 'feeding', ['-DAGX_LVW_MAX_STEPS=40'])      # the scheduler gives up beyond 40 steps per part: a settled scene overflows it two rows wide, a fresh one fits
_LIBS = {}


def pair_lib(kind):
    """tests/emu/emu_pair.cpp (which includes emu_main.cpp) with the -D flags of an emulator kind, as emu_lib.lib builds emu_main.cpp"""
    if kind not in _LIBS:
        so = os.path.join(emu_lib.EMU, 'libagx_emu_pair_%s.so' % kind)
        deps = [PAIR_CPP] + [os.path.join(emu_lib.EMU, f) for f in ('emu_main.cpp', 'agx_wave.h')] + \
               [os.path.join(emu_lib.CSRC, f) for f in sorted(os.listdir(emu_lib.CSRC)) if f.endswith(('.h', '.def'))] + [os.path.join(emu_lib.ROOT, 'include', 'agx_blob.h')]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import fcntl
            with open(so + '.lock', 'w') as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                tmp = '%s.%d.tmp' % (so, os.getpid())
                subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-I' + emu_lib.EMU, '-I' + emu_lib.CSRC] + emu_lib.kind_defs(kind) + ['-o', tmp, PAIR_CPP])
                os.replace(tmp, so)
        _LIBS[kind] = C.CDLL(so)
    return _LIBS[kind]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class PairEmu:
    def __init__(self, blob, kind='feeding'):
        self.blob, self.L, self.words = blob, pair_lib(kind), np.ascontiguousarray(blob.words)
        self.scr_words = self.L.agx_emu_pair_scr_words()
        m = (C.c_int * 4)(); self.L.agx_emu_pair_meta(m)
        self.o_nrows, self.o_ncon, self.max_steps, self.compiled = list(m)
        self.nsub = int(blob.param('FRAME_SKIP')) * max(1, int(blob.h['SIM_SUBSTEPS']))

    def step(self, states, actions, paired, present=3):
        """the substeps of one env.step() of two environments (states [2, sw] in place) -> (scratch records after the last substep, paired-sweep flags per substep, rows per substep)"""
        assert states.dtype == np.float32 and states.flags.c_contiguous and states.shape[0] == 2
        scr = np.zeros((2, self.scr_words), dtype=np.float32)
        took, rows = [], []
        for k in range(self.nsub):
            for e in range(2):
                if present >> e & 1:
                    act = np.ascontiguousarray(actions[e], dtype=np.float32) if k == 0 else None
                    assert self.L.agx_emu_pair_build(_p(self.words), _p(states[e]), _p(act), _p(scr[e])) == 0
            rows.append([int(scr[e, self.o_nrows:self.o_nrows + 1].view(np.int32)[0]) for e in range(2)])
            rc = self.L.agx_emu_pair_solve(_p(self.words), _p(states), C.c_int(states.shape[1]), _p(scr), C.c_int(k), C.c_int(1 if paired else 0), C.c_int(present))
            assert rc >= 0, 'wave emulator reported divergent control flow'
            took.append(rc)
        return scr, took, rows

    def schedule_steps(self, state, width):
        """steps of the two list schedules (non-contact + normal rows, friction rows) of a state's first substep, `width` rows per step; -1 = does not fit"""
        s = np.ascontiguousarray(state, dtype=np.float32).copy()
        scr = np.zeros(self.scr_words, dtype=np.float32)
        assert self.L.agx_emu_pair_build(_p(self.words), _p(s), None, _p(scr)) == 0
        out = (C.c_int * 5)()
        assert self.L.agx_emu_pair_schedule(_p(scr), C.c_int(width), out, None, None) == 0
        return out[0], out[1]


@pytest.fixture(scope='module')
def scenes(blob):
    """a fresh FeedingJaco state (bowl and food in the air: few rows) and two settled ones (food on the spoon: many rows), shared by the cases below"""
    from emu_lib import Emu
    e = Emu(blob)
    st, _ = make_states(blob, 3, seed=3711)
    fresh = st[0].copy()
    settled = []
    for i in (1, 2):
        s = st[i].copy(); e.settle(s, 8); settled.append(s)
    for s in [fresh] + settled:
        s.setflags(write=False)
    return fresh, settled[0], settled[1]


def _compare(pe, sa, sb, present=3, steps=2, seed=5):
    """`steps` env.step()s of the two states, paired against single: every bit of the states and the scratch records.  Returns the paired-sweep flags and row counts."""
    rng = np.random.RandomState(seed)
    sp = np.ascontiguousarray(np.stack([sa, sb])).astype(np.float32); ss = sp.copy()
    took, rows = [], []
    for k in range(steps):
        a = rng.uniform(-1, 1, (2, pe.blob.act_dim)).astype(np.float32)
        scr_p, t, r = pe.step(sp, a, True, present)
        scr_s, t0, _ = pe.step(ss, a, False, present)
        assert not any(t0)
        assert np.array_equal(sp.view(np.uint32), ss.view(np.uint32)), (k, 'states')
        assert np.array_equal(scr_p.view(np.uint32), scr_s.view(np.uint32)), (k, 'scratch records')
        took += t; rows += r
    return took, rows


def test_paired_sweep_is_compiled_for_the_feeding_variant(blob):
    assert PairEmu(blob).compiled == 1


def test_an_ordinary_pair(blob, scenes):
    """two settled scenes (food on the spoon): every substep takes the paired sweep"""
    took, rows = _compare(PairEmu(blob), scenes[1], scenes[2])
    assert all(took), took
    assert min(min(r) for r in rows) > 40, rows      # (contacts on both sides: a real sweep)


def test_very_different_row_counts(blob, scenes):
    """a fresh scene beside a settled one, in both orders: the shorter lists end in idle rows"""
    pe = PairEmu(blob)
    for a, b in ((scenes[0], scenes[1]), (scenes[1], scenes[0])):
        took, rows = _compare(pe, a, b, steps=1)
        assert all(took), took
        assert max(abs(r[0] - r[1]) for r in rows) >= 30, rows


def test_two_friction_directions(blob, scenes):
    took, _ = _compare(PairEmu(blob.set_param('FRICTION_DIRS', 2.0)), scenes[1], scenes[0], steps=1)
    assert all(took), took


def test_far_rows_in_both_halves(blob, scenes):
    """a 300-pair LDS window: most rows of both environments read their pairs from their scratch records"""
    took, _ = _compare(PairEmu(blob, 'feeding_lvw_cap'), scenes[1], scenes[2], steps=1)
    assert all(took), took


def test_one_side_overflows_the_scheduler(blob, scenes):
    """a build whose scheduler gives up at 40 steps per part: a settled scene (42 steps and more) does not fit, so the pair goes through env_solve one after the other
    (the fresh scene, 35 steps, fits: a pair of two fresh scenes still takes the paired sweep)"""
    pe = PairEmu(blob, 'feeding_pair_40steps')
    assert pe.max_steps == 40
    full = PairEmu(blob)
    fresh, settled = full.schedule_steps(scenes[0], 2), full.schedule_steps(scenes[1], 2)
    assert 0 < max(fresh) <= 40 < max(settled) <= 64, (fresh, settled)      # (the premise of this case, from the scheduler itself, two rows wide)
    assert pe.schedule_steps(scenes[0], 2) == fresh and pe.schedule_steps(scenes[1], 2)[0] == -1
    took, _ = _compare(pe, scenes[0], scenes[1], steps=1)
    assert took[0] == 0, took
    took, _ = _compare(pe, scenes[0], scenes[0], steps=1)
    assert took[0] == 1, took


def test_a_missing_partner(blob, scenes):
    """only one environment of the workgroup takes part (the end of a launch, the `active` mask): the other's records keep their bits"""
    pe = PairEmu(blob)
    for present in (1, 2):
        took, _ = _compare(pe, scenes[1], scenes[2], present=present, steps=1)
        assert not any(took)
        sp = np.ascontiguousarray(np.stack([scenes[1], scenes[2]])); before = sp.copy()
        pe.step(sp, np.zeros((2, blob.act_dim), dtype=np.float32), True, present)
        absent = 1 if present == 1 else 0
        assert np.array_equal(sp[absent].view(np.uint32), before[absent].view(np.uint32))
        assert not np.array_equal(sp[1 - absent].view(np.uint32), before[1 - absent].view(np.uint32))


def test_switched_off_by_the_blob(blob, scenes):
    """AGX_P_SOLVE_WIDE = 0: both environments go through the narrow sweep inside the paired kernel"""
    took, _ = _compare(PairEmu(blob.set_param('SOLVE_WIDE', 0)), scenes[1], scenes[2], steps=1)
    assert not any(took)
