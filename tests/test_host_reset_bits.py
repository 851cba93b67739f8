"""The numpy samplers of assistive_gym_amd/host against records kept from before the reset layer was rebuilt on shared pieces
(tests/golden/host_reset_records.npz, written by tests/diag/reset_layer_bits.py --write-golden: seed 77, two states per model, no settler,
no checker; the garment / water array as a hash).  The integer words of a record -- env and task words, the frozen mask, the rng words, gender,
iteration -- must be equal; the float words agree to 1e-6 absolute, which covers another libm or BLAS under numpy (on the machine that
recorded them they are equal to the bit: profiles/reset_layer)."""
import hashlib
import os
import sys

import numpy as np
import pytest

from conftest import full

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'diag'))
import reset_layer_bits as bits      # noqa: E402

# one model per sampler, and the two feeding paths without IK restarts (base pose search, placement draws); the other mounts with AGX_FULL_TESTS=1
LEAN = ('feeding_jaco', 'feeding_sawyer', 'feeding_stretch', 'drinking_jaco', 'scratch_itch_pr2', 'bed_bathing_sawyer', 'dressing_baxter', 'arm_manipulation_sawyer')
INT_FIELDS = ('gender', 'food_alive', 'food_active', 'iteration', 'task_success', 'rng', 'total_food', 'frozen', 'task')


@pytest.fixture(scope='module')
def golden():
    with np.load(bits.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('model', [m if m in LEAN else pytest.param(m, marks=full) for m in bits.MODELS])
def test_sampler_reproduces_the_recorded_states(model, golden):
    from assistive_gym_amd.blob import ModelBlob
    blob = ModelBlob.load(model)
    states, extra, _ = bits.sample(model, bits.GOLDEN_STATES, bits.GOLDEN_SEED)
    want = golden[model + '/states'].view(np.float32)
    assert states.shape == want.shape and states.dtype == np.float32
    got_v, want_v = blob.view(states), blob.view(want.copy())
    marks = blob.new_state(len(states))          # which words of a record the integer fields cover, through the same named views
    mv = blob.view(marks)
    for k in INT_FIELDS:
        assert np.array_equal(got_v[k], want_v[k]), k
        mv[k][...] = 1
    floats = marks.view(np.int32) == 0            # every other word is a float (the float targets some tasks keep in task words were compared as bits above)
    assert floats.sum() > 0.5 * floats.size and np.isfinite(states[floats]).all()
    err = np.abs(states[floats].astype(np.float64) - want[floats].astype(np.float64))
    assert err.max() <= 1e-6, float(err.max())
    if extra is not None:
        # the garment / water is the rest grid shifted by one float64 offset and rounded to float32: a hash, as recorded
        assert hashlib.sha256(np.ascontiguousarray(extra).tobytes()).digest() == golden[model + '/extra_sha256'].tobytes()
