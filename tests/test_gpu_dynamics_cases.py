"""-m gpu: the dynamics phase of the build kernel (csrc/agx_dyn.h) and the integration of the solve kernel (csrc/agx_env.h) joint by joint,
through the C ABI, on the small synthetic link trees of tests/dynamics_cases.py.

Everything expected comes from tests/golden/dynamics_cases.npz (tests/diag/make_dynamics_cases.py): M^-1, qdd and the free bodies' records of a
float64 reference written from the definitions (link Jacobians at the centres of mass, Lagrange's equations, a dense inverse), which
tests/test_dynamics_cases.py checks against closed forms, pins the oracle to, and judges the kernel source on the wave emulator by.  No numpy
physics runs here: the comparison (dynamics_cases.judge) only measures the device's records against the stored values.

  scenes   all stored poses of a scene as the environments of ONE handle, one agx_settle_debug(1): M^-1 and qdd of the debug record, the state
           record after the substep.  Compared in ALL environments, maxima: every entry of each block and its asymmetry against the stored limits,
           zeros across the blocks and on frozen DoFs exactly, qd' and q' as the float32 update of the device's own qdd, the free bodies.
  four     dy_chain and dy_tree for four substeps (agx_settle) against the reference iterated four times: q and qd of every DoF.
  frames   agx_collider_frames (dy_tree, dy_far) and agx_ee_pose (dy_far) against the reference's link and end-effector frames.
  bits     a pose of dy_tree and of dy_cols as environment 0 and as environment 5 of a six-environment handle, and that handle twice.

Limits: dynamics_cases (LIMITS at its top), stored per environment.  Measured values: profiles/dynamics_cases/README.md."""
import numpy as np
import pytest

import dynamics_cases as DC

pytestmark = pytest.mark.gpu

SCENES = ('dy_chain', 'dy_tree', 'dy_star', 'dy_two', 'dy_frozen', 'dy_far', 'dy_ratio', 'dy_ratio_up', 'dy_fast', 'dy_free', 'dy_block12', 'dy_block16', 'dy_block22', 'dy_cols')


@pytest.fixture(scope='module')
def cases():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()
    return DC.load_cases()


def _run(blob, states):
    """one substep of len(states) environments: (debug records [n, words], their layout, the state records afterwards)"""
    import torch
    from assistive_gym_amd.libagx import Stepper
    st = Stepper(blob, len(states))
    try:
        st.set_state(np.ascontiguousarray(states))
        lay = st.debug_layout()
        dbg = torch.zeros((len(states), lay[0]), device=torch.device('cuda', 0))
        st.settle_debug(1, dbg); st.synchronize()
        torch.cuda.synchronize()
        out, after = dbg.cpu().numpy(), st.get_state()
    finally:
        st.close()
    return out, lay, after


@pytest.mark.parametrize('name', SCENES)
def test_scene(cases, name):
    states = DC.scene_states(cases, name)
    assert 10 <= len(states) <= 64
    blob = DC.scene_blob(cases, name)
    dbg, lay, after = _run(blob, states)
    m, bad = DC.judge(cases, name, [DC.result_of(d, lay, s, blob) for d, s in zip(dbg, after)])
    print(DC.say(name, 'device', m))
    assert not bad, bad[:10]
    assert m['n'] == len(cases[name + '/q']) > 0


@pytest.mark.parametrize('name', ['dy_chain', 'dy_tree'])
def test_four_substeps(cases, name):
    """the reference iterated four times against four substeps of the device"""
    from assistive_gym_amd.libagx import Stepper
    steps = cases[name + '/recipe']['steps']
    blob = DC.scene_blob(cases, name)
    states = DC.scene_states(cases, name)
    st = Stepper(blob, len(states))
    try:
        st.set_state(np.ascontiguousarray(states))
        st.settle(steps); st.synchronize()
        v = blob.view(st.get_state())
    finally:
        st.close()
    m, bad = DC.judge_iterated(cases, name, list(zip(v['q'], v['qd'])))
    print('dynamics %-10s device   %d substeps, poses %3d | q %.3g rad, %.2f of its limit at most | qd %.3g, %.2f of its limit' % (name, steps, m['n'], m['q'], m['q_of'], m['qd'], m['qd_of']))
    assert steps == 4 and not bad, bad[:10]
    assert m['n'] == len(states)


@pytest.mark.parametrize('name', ['dy_tree', 'dy_far'])
def test_frames(cases, name):
    """the other two kinematics walks: agx_collider_frames on every collider of a robot link and agx_ee_pose against the reference's frames.
    dy_far's robot is a serial chain, which agx_ee_pose serves; dy_tree's is not (agx_ee_arms is 0 and says so)"""
    import torch
    from assistive_gym_amd.libagx import Stepper
    blob = DC.scene_blob(cases, name)
    states = DC.scene_states(cases, name)
    st = Stepper(blob, len(states))
    try:
        st.set_state(np.ascontiguousarray(states))
        cf = torch.zeros((len(states), st.collider_count(), 12), device=torch.device('cuda', 0))
        st.collider_frames(cf); st.synchronize()
        arms = st.ee_arms()
        assert arms == (1 if name == 'dy_far' else 0)
        ee = None
        if arms:
            ee = torch.zeros((len(states), arms, 7), device=torch.device('cuda', 0))
            st.ee_pose(ee); st.synchronize()
        torch.cuda.synchronize()
        cf, ee = cf.cpu().numpy(), None if ee is None else ee.cpu().numpy()[:, 0]
    finally:
        st.close()
    m, bad, n = DC.judge_frames(cases, name, blob, cf, ee)
    print('dynamics %-10s device   frames of %d colliders%s | position %.3g m, %.2f of its limit | rotation %.3g, %.2f of its limit' % (name, n, ' and the end effector' if arms else '', m['pos'], m['pos_of'], m['rot'], m['rot_of']))
    assert not bad, bad[:10]
    assert n >= 10 * len(states)


@pytest.mark.parametrize('name', ['dy_tree', 'dy_cols'])
def test_bit_reproducible(cases, name):
    """the chain walks publish through lane 0 between barriers and the columns of M^-1 come in lane batches: a missing barrier or a lane-dependent
    order shows as variation.  A pose as environment 0 and as environment 5 of a handle whose other environments hold other poses, and all of it twice"""
    states = DC.scene_states(cases, name)[[0, 1, 2, 3, 4, 0]]
    blob = DC.scene_blob(cases, name)

    def part():      # counts, M^-1, qdd and the state; not the cycle counters
        dbg, lay, after = _run(blob, states)
        return np.concatenate([dbg[:, :5], dbg[:, lay[2]:lay[2] + lay[3] * lay[3]].reshape(6, lay[3], lay[3])[:, :blob.ndof, :blob.ndof].reshape(6, -1),
                               dbg[:, lay[7]:lay[7] + blob.ndof], after], 1).view(np.int32)
    a = part()
    assert np.array_equal(a[0], a[5])
    assert not np.array_equal(a[0], a[1])
    assert np.array_equal(a, part())
