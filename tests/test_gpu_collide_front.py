"""-m gpu: the front end of collide() decides the same groups and the same contact slots as before.
The default build makes the union boxes of the group cull from block boxes and selects the contacts of a flush in one pass (csrc/agx_collide.h,
AGX_COLLIDE_FRONT); lib/variants/frontplain.so (-DAGX_COLLIDE_FRONT=0, built by __graft_entry__.build() for the FEEDING, FEEDING_L and BED_BATHING
kernel variants) walks the collider ranges and the segments one by one, as the kernel did before the switch existed.  A rollout from the reset
pool with random actions through both libraries, each in a process of its own (AGX_LIB; the rollout tool of tests/test_gpu_face_proof.py): the
pool, every output and every state record after every step, and the first substep's debug record (contact records included), are BIT-IDENTICAL.
FeedingJaco runs three chunks and late enough for food to have fallen, so that the segments differ between environments; FeedingSawyer is the
320-collider variant with 16-bit lists; BedBathingSawyer carries the wiping pad's query points.
(tests/test_emu_collide_front.py does the same on the CPU, also with a short worklist and a crafted tie.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, 'tools', 'gpu_face_proof_bits.py')
FRONTPLAIN = os.path.join(ROOT, 'assistive_gym_amd', 'lib', 'variants', 'frontplain.so')


def _rollout(model, n, steps, out, env):
    e = dict(os.environ); e.update(env)
    r = subprocess.run([sys.executable, TOOL, model, str(n), str(steps), out], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-1500:]
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('model, n, steps', [('feeding_jaco', 192, 40), ('feeding_sawyer', 96, 20), ('bed_bathing_sawyer', 96, 20)])
def test_front_end_bit_identical(tmp_path, model, n, steps):
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()
    assert os.path.exists(FRONTPLAIN), 'lib/variants/frontplain.so is missing: run __graft_entry__.build()'
    new, old = _rollout(model, n, steps, str(tmp_path / 'default.npz'), {}), _rollout(model, n, steps, str(tmp_path / 'frontplain.npz'), {'AGX_LIB': FRONTPLAIN})
    assert set(new) == set(old) and 'debug' in new
    for k in ('pool', 'debug', 'obs', 'reward', 'done', 'info', 'state'):
        rows = np.where((new[k] != old[k]).reshape(new[k].shape[0], new[k].shape[1], -1).any(axis=2))
        assert np.array_equal(new[k], old[k]), '%s differs: (step, environment) %s' % (k, list(zip(*rows))[:8])
    if model == 'feeding_jaco':      # the rollout is one with contacts in it: every environment's first substep has some
        assert (new['debug'][0][:, 0].view(np.float32) > 0).all()
