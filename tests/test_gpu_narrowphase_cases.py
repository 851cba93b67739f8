"""-m gpu: the build kernel's collision front end (csrc/agx_collide.h, csrc/agx_gjk.h) pair by pair, through the C ABI, on the small synthetic
collider pairs of tests/narrowphase_cases.py.

Everything expected comes from tests/golden/narrowphase_cases.npz (tests/diag/make_narrowphase_cases.py): the contacts of a float64 reference
written from the definitions (Wolfe's minimum-norm point over the difference vertices, brute force over all pairs of every row), which
tests/test_narrowphase_cases.py checks against closed forms, pins the oracle to, and judges the kernel source on the wave emulator by.  No numpy
physics runs here: the comparison (narrowphase_cases.judge) only measures the device's records against the stored values.

  scenes   all stored poses of a scene as the environments of ONE handle, one agx_settle_debug(1): the contact records of the first substep.
           Compared on ALL contacts of ALL poses, maxima: the (ca, cb) list in order, the count and the contacts dropped at the cap, bodies,
           mu bit-equal to the float32 product of the two frictions, dist and n against the stored per-contact limits, the points by what holds
           without uniqueness.
  bits     a pose of np_grid and of np_served as environment 0 and as environment 5 of a six-environment handle, and that handle twice.

Limits: narrowphase_cases (LIMITS at its top), stored per contact.  Measured values: profiles/narrowphase_cases/README.md."""
import numpy as np
import pytest

import narrowphase_cases as NC

pytestmark = pytest.mark.gpu

SCENES = ('np_counts', 'np_served', 'np_flat', 'np_far', 'np_pen', 'np_micron', 'np_grid', 'np_keep', 'np_wide', 'np_table')


@pytest.fixture(scope='module')
def cases():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()
    return NC.load_cases()


def _run(blob, states):
    """one substep of len(states) environments: (debug records [n, words], offset of the contacts in them)"""
    import torch
    from assistive_gym_amd.libagx import Stepper
    st = Stepper(blob, len(states))
    try:
        st.set_state(np.ascontiguousarray(states))
        lay = st.debug_layout()
        dbg = torch.zeros((len(states), lay[0]), device=torch.device('cuda', 0))
        st.settle_debug(1, dbg); st.synchronize()
        torch.cuda.synchronize()
        out = dbg.cpu().numpy()
    finally:
        st.close()
    return out, lay[1]


@pytest.mark.parametrize('name', SCENES)
def test_scene(cases, name):
    states = NC.scene_states(cases, name)
    assert 10 <= len(states) <= 64
    dbg, o_con = _run(NC.scene_blob(cases, name), states)
    m, bad = NC.judge(cases, name, [NC.records_of_debug(d, o_con) for d in dbg])
    print(NC.say(name, 'device', m))
    assert not bad, bad[:10]
    assert m['n'] == len(cases[name + '/con']) > 0


@pytest.mark.parametrize('name', ['np_grid', 'np_served'])
def test_bit_reproducible(cases, name):
    """ballot ranks, the served scan's wave-wide maximum and the one-pass selection are where a lane-dependent order or a missing barrier shows
    as variation: a pose as environment 0 and as environment 5 of a handle whose other environments hold other poses, and all of it twice"""
    states = NC.scene_states(cases, name)[[0, 1, 2, 3, 4, 0]]
    dbg, o_con = _run(NC.scene_blob(cases, name), states)
    part = lambda d: np.concatenate([d[:, :5], d[:, o_con:o_con + NC.MAX_CON * 16]], 1).view(np.int32)      # counts and contact records; not the cycle counters
    a = part(dbg)
    assert a[0, 0] != 0 and np.array_equal(a[0], a[5])
    assert not np.array_equal(a[0], a[1])
    again, _ = _run(NC.scene_blob(cases, name), states)
    assert np.array_equal(a, part(again))
