"""Writes tests/golden/finish_spill_cases.npz: the crafted FeedingJaco states of tests/test_emu_finish_spill.py and tests/test_gpu_step_tail.py.
Each is a settled state (the pool's 25 settle substeps: the food rests on the spoon) with the free-body words of particle 0 edited:
  resting   untouched;
  shell_in  / shell_out   released at rest straight above where it lay, from the height at which -- after the free fall of one env step with a
            zero action -- it ends 0.098 m / 0.102 m (+- 1.5 mm) from the nearest spoon piece: either side of SPILL_DIST, where only the
            narrowphase can decide.  The height is found with the traced all-narrowphase emulator build, which reports that separation;
  far       0.5 m above the spoon;
  mouth     4.5 cm above the mouth target: within MOUTH_DIST after the step's free fall, so it is eaten and draws from the RNG.
Not a test; run by hand:  python tests/diag/make_finish_spill_cases.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from assistive_gym_amd.blob import ModelBlob
from assistive_gym_amd.host.reset import make_states
from oracle_lib import Oracle
import test_emu_finish_spill as T


def place(blob, state, k, pos):
    """particle k of a copy of `state` at rest at `pos`"""
    s = state.copy()
    r = blob.view(s)['free'][0, blob.h['FOOD0'] + k]
    r[:3] = pos; r[3:7] = (0.0, 0.0, 0.0, 1.0); r[7:13] = 0.0
    return s


def above_spoon(blob, traced_gjk, state, want):
    a = np.zeros(blob.act_dim, dtype=np.float32)
    p0 = blob.view(state.copy())['free'][0, blob.h['FOOD0'], :3].astype(np.float64)
    h = want + 0.06
    for _ in range(6):
        s = place(blob, state, 0, p0 + np.array([0.0, 0.0, h]))
        _, sep, _ = T.finish_trace(traced_gjk, s, a)
        if abs(sep - want) < 1.5e-3:
            return s
        h += want - sep
    raise RuntimeError('no placement %.3f m from the spoon found (last separation %.4f)' % (want, sep))


def main():
    blob = ModelBlob.load('feeding_jaco')
    st, _ = make_states(blob, 4, seed=4242)
    o = Oracle(blob)
    for i in range(4):
        o.settle(st[i], 25)
    traced_gjk = T.emu_lib.Emu(blob, kind='feeding_trace_finish_gjk')
    up = np.array([0.0, 0.0, 0.5], dtype=np.float32)
    cases = dict(resting=st[0].copy(), shell_in=above_spoon(blob, traced_gjk, st[1], 0.098), shell_out=above_spoon(blob, traced_gjk, st[1], 0.102),
                 far=place(blob, st[2], 0, blob.view(st[2].copy())['free'][0, blob.h['FOOD0'], :3] + up),
                 mouth=place(blob, st[3], 0, blob.view(st[3].copy())['target'][0] + np.array([0.0, 0.0, 0.045], dtype=np.float32)))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'finish_spill_cases.npz')
    np.savez(out, **cases)
    print('wrote', out, {k: v.shape for k, v in cases.items()})


if __name__ == '__main__':
    main()
