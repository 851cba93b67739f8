"""End-effector control without a GPU: the device's math (csrc/agx_ik.h, compiled with g++ through tests/emu/ik_host.cpp) against the float64 reference
of tests/ee_ref.py (RobotKin.fk / ee_jacobian, RobotKin.ik's update over one chain's seven DoFs), within the float32 rounding bounds derived there;
the argument checks of the C entries that need no device; the command line's flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
from ee_ref import ArmRef, U, check_one_iteration, check_pose, delta_command, reachable_target

from assistive_gym_amd.blob import ModelBlob

IK_CPP = os.path.join(emu_lib.EMU, 'ik_host.cpp')
_LIB = []


def ik_lib():
    if not _LIB:
        so = os.path.join(emu_lib.EMU, 'libagx_ik_host.so')
        deps = [IK_CPP, os.path.join(emu_lib.EMU, 'agx_wave.h'), os.path.join(emu_lib.CSRC, 'agx_ik.h'), os.path.join(emu_lib.CSRC, 'agx_math.h'),
                os.path.join(emu_lib.ROOT, 'include', 'agx_blob.h')]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import fcntl
            with open(so + '.lock', 'w') as lock:
                fcntl.flock(lock, fcntl.LOCK_EX)
                tmp = '%s.%d.tmp' % (so, os.getpid())
                subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-I' + emu_lib.EMU, '-I' + emu_lib.CSRC, '-o', tmp, IK_CPP])
                os.replace(tmp, so)
        L = C.CDLL(so)
        L.ik_host_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.ik_host_ik.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        _LIB.append(L)
    return _LIB[0]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_pose(blob, state, arm):
    out = np.zeros(7, dtype=np.float32)
    ik_lib().ik_host_pose(_p(np.ascontiguousarray(blob.words)), _p(state), arm, _p(out))
    return out.astype(np.float64)


def host_ik(blob, state, arm, target, frame, iters, damping=0.05, gain=10.0):
    """-> (q_out[7], err[2], action row pre-filled with 123)"""
    q, err, act = np.zeros(7, dtype=np.float32), np.zeros(2, dtype=np.float32), np.full(blob.act_dim, 123.0, dtype=np.float32)
    ik_lib().ik_host_ik(_p(np.ascontiguousarray(blob.words)), _p(state), arm, _p(np.ascontiguousarray(target, dtype=np.float32)),
                        {'absolute': 0, 'delta': 1}[frame], iters, damping, gain, _p(q), _p(err), _p(act))
    return q.astype(np.float64), err.astype(np.float64), act.astype(np.float64)


def _arm_manipulation_states(robot, seeds):
    """Emu(blob).sample(seed) of an arm-manipulation blob reads the rag doll's and the fall model's records: a few oracle steps each (tests/test_reset_arm_device.py)"""
    import sys
    sys.path.insert(0, os.path.join(emu_lib.ROOT, 'oracle'))
    import reset_oracle as ro
    from emu_lib import Emu
    from oracle_lib import Oracle
    from test_reset_arm_device import chain
    out = []
    for seed in seeds:
        sblob, b, fb, rag, _ = chain(robot, seed, rag_steps=3, fall_steps=2)
        fell, _ = ro.ResetOracle(fb.words).sample(seed, impairment_mode=ro.MODE_NO_TREMOR, settled=rag)
        fell = fell.copy(); Oracle(fb).settle(fell, 2)
        out.append(Emu(b).sample(seed, impairment_mode=ro.MODE_NO_TREMOR, settled=rag, fell=fell)[0])
    return out


@pytest.fixture(scope='module')
def cases():
    """[(name, blob, state records)]: FeedingJaco, a left arm (ScratchItchPR2) and two arms (ArmManipulationBaxter), every record from the reset generator on the wave emulator"""
    from emu_lib import Emu
    out = []
    for name, seeds in (('feeding_jaco', range(4100, 4106)), ('scratch_itch_pr2', (4200, 4201))):
        blob = ModelBlob.load(name)
        emu = Emu(blob)
        out.append((name, blob, [emu.sample(s)[0] for s in seeds]))
    out.append(('arm_manipulation_baxter', ModelBlob.load('arm_manipulation_baxter'), _arm_manipulation_states('baxter', (4300,))))
    return out


def _arms(blob):
    from assistive_gym_amd.model import compiler as L
    return 2 if int(blob.i[blob.h['OFF_RESET'] + L.X_['FLAGS']]) & 512 else 1


def test_pose_and_one_iteration_match_robotkin(cases):
    worst = {}
    rng = np.random.RandomState(11)
    for name, blob, states in cases:
        for arm in range(_arms(blob)):
            ref = ArmRef(blob, arm)
            for k, st in enumerate(states):
                label = '%s env %d arm %d' % (name, k, arm)
                check_pose(ref, st, host_pose(blob, st, arm), worst, label)
                # a reachable target a few centimetres away (the pose of q + delta), and a Cartesian delta command
                for frame, cmd in (('absolute', reachable_target(ref, st, rng)), ('delta', delta_command(rng))):
                    q1, err, act = host_ik(blob, st, arm, cmd, frame, 1)
                    cols = check_one_iteration(ref, st, cmd, frame, q1, err, act, 10.0, worst, label)
                    assert all(act[c] == 123.0 for c in range(blob.act_dim) if c not in cols)          # the other arm's columns stay the caller's
        print('%s: worst |error| / bound so far (kappa, b_q: the largest condition number and q_out bound met): %s' % (name, {k: '%.3g' % v for k, v in worst.items()}))
    assert all(worst[k] > 0.0 for k in ('pos', 'quat', 'q_out', 'action'))                      # (not vacuous: float32 and float64 differ)


def test_convergence_where_the_reference_converges(cases):
    rng = np.random.RandomState(12)
    total = converged = 0
    for name, blob, states in cases:
        for arm in range(_arms(blob)):
            ref = ArmRef(blob, arm)
            for st in states:
                bp, bq, qr, qc = ref.split(st)
                cmd = reachable_target(ref, st, rng)
                tp, tq = ref.target(bp, bq, qr, qc, cmd, 'absolute')
                e = ref.error(bp, bq, qr, ref.ik(bp, bq, qr, qc, tp, tq, 50), tp, tq)
                total += 1
                if not (np.linalg.norm(e[:3]) < 1e-4 and np.linalg.norm(e[3:]) < 1e-4):
                    continue
                converged += 1
                q1, err, _ = host_ik(blob, st, arm, cmd, 'absolute', 100)
                b_pos, b_quat = ref.fk_bounds(bp, q1)
                e1 = ref.error(bp, bq, qr, q1, tp, tq)
                assert np.linalg.norm(e1[:3]) <= 1e-4 + 2 * b_pos + 4 * U and np.linalg.norm(e1[3:]) <= 1e-4 + 4 * b_quat + 16 * U, (name, arm, e1, err)
                assert (q1 >= ref.lower - 1e-6).all() and (q1 <= ref.upper + 1e-6).all()
    print('%d of %d targets: the float64 reference converges in 50 iterations' % (converged, total))
    assert converged >= 0.9 * total


def test_a_state_that_is_not_finite_gives_a_zero_action(cases):
    _, blob, states = cases[0]
    ref = ArmRef(blob, 0)
    for bad, cmd in ((float('nan'), [0.0] * 6), (float('inf'), [0.0] * 6), (None, [float('nan')] + [0.0] * 5)):
        st = states[0].copy()
        if bad is not None:
            blob.view(st)['q'][0, ref.chain[2]] = bad
        q1, err, act = host_ik(blob, st, 0, cmd, 'delta', 3)
        assert all(act[c] == 0.0 for c in ref.cols) and np.isinf(err).all() and (err > 0).all()
        assert np.array_equal(q1.astype(np.float32), blob.view(st)['q'][0, ref.chain], equal_nan=True)


def test_null_handles_are_refused_without_a_device():
    from assistive_gym_amd.build import build
    build()
    from assistive_gym_amd import libagx
    L = libagx.load()
    arms = C.c_int(7)
    assert L.agx_ee_arms(None, C.byref(arms)) == -1 and b'agx_ee_arms' in L.agx_last_error()
    assert L.agx_ee_pose(None, None, None) == -1 and b'agx_ee_pose' in L.agx_last_error()
    assert L.agx_ee_ik(None, None, 7, 0, 8, 0.05, 10.0, None, None, 0, None, None) == -1 and b'agx_ee_ik' in L.agx_last_error()


def test_parser_accepts_ee_actions():
    from assistive_gym_amd.learn import build_parser
    assert build_parser().parse_args([]).ee_actions is False
    assert build_parser().parse_args(['--env', 'FeedingJaco-v1', '--train', '--ee-actions']).ee_actions is True
