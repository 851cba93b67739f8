"""-m gpu: the windowed sweep of collide() fills the worklist with the same pairs in the same order as the serial one.
The default build sweeps a window of consecutive live pair groups at once (csrc/agx_collide.h, AGX_FRONT_SWEEP); lib/variants/sweepserial.so
(-DAGX_FRONT_SWEEP=0, built by __graft_entry__.build() for the FEEDING and FEEDING_M kernel variants) sweeps one live group at a time, as the kernel
did before the switch existed.  A rollout from the reset pool with random actions through both libraries, each in a process of its own (AGX_LIB;
the rollout tool of tests/test_gpu_face_proof.py): the pool, every output and every state record after every step, and the first substep's debug
record (contact records included), are BIT-IDENTICAL.  FeedingJaco is the headline scene; FeedingStretch stands on the ground plane, so several
face groups (every pair enumerated 1 + AGX_FACE_EXTRA times) share a window.
(tests/test_emu_collide_sweep.py does the same on the CPU, also with windows cut short.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'gpu_face_proof_bits.py')
SERIAL = os.path.join(ROOT, 'assistive_gym_amd', 'lib', 'variants', 'sweepserial.so')


def _rollout(model, n, steps, out, env):
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, TOOL, model, str(n), str(steps), out], capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-1500:]
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('model, n, steps', [('feeding_jaco', 128, 20), ('feeding_stretch', 64, 10)])
def test_windowed_sweep_bit_identical(tmp_path, model, n, steps):
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()
    assert os.path.exists(SERIAL), 'lib/variants/sweepserial.so is missing: run __graft_entry__.build()'
    new, old = _rollout(model, n, steps, str(tmp_path / 'default.npz'), {}), _rollout(model, n, steps, str(tmp_path / 'sweepserial.npz'), {'AGX_LIB': SERIAL})
    assert set(new) == set(old) and 'debug' in new
    for k in ('pool', 'debug', 'obs', 'reward', 'done', 'info', 'state'):
        rows = np.where((new[k] != old[k]).reshape(new[k].shape[0], new[k].shape[1], -1).any(axis=2))
        assert np.array_equal(new[k], old[k]), '%s differs: (step, environment) %s' % (k, list(zip(*rows))[:8])
    assert (new['debug'][0][:, 0].view(np.float32) > 0).all(), 'the rollout is one with contacts in it: every environment\'s first substep has some'
