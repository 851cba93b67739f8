"""-m gpu: the cloth kernel (csrc/agx_cloth.h) node by node, through the C ABI, on the small synthetic garments of tests/cloth_cases.py.

Everything expected comes from tests/golden/cloth_kernel_cases.npz (tests/diag/make_cloth_kernel_cases.py): float64 results of the numpy
restatement that tests/test_cloth_kernel_cases.py pins the oracle to.  No numpy physics runs here.

  forced substeps   all determined substeps of a scene in ONE handle, one environment per substep (each with its own state record, garment,
                    trace and report), one settle(1) of the blob with SIM_SUBSTEPS = 1 and DT / 8: exactly one cloth substep, whose forces
                    the report holds (the cloth kernel writes its report on the settle path as well).  Compared on ALL nodes, maximum not
                    percentile: x, v, the set of (node, slot) contacts, |force| per contact, the reported node height.
  free flight       one settle(1) of the ordinary 8-substep blob: 30 nodes (no cross-patch class) to 4,096 (the kernel's limit).
  bits              the same scene twice, and as environment 0 and 5 of a 6-environment handle: identical bits.

Limits (cloth_cases.limits): 4 x the float32 restatement's own deviation from the float64 result, stored with each scene; floors of one float32
ulp of the coordinate magnitude for x, that / dt for v, that / (dt^2 im) for a force.  The contact set must be equal.  The restatement's force
deviation includes the shapes' frames moved by one float32 ulp: a force answers to the shape's position with 1 / (dt^2 im) = 6.5 N/m, and the
device's frames come from the rigid kernels' float32 forward kinematics (with the frames rounded to nearest alone, one environment of
fs_first_touch measured 7.37e-07 N against a limit of 7.25e-07 N).  Measured values and both findings: profiles/cloth_kernel_tests/README.md."""
import numpy as np
import pytest

import cloth_cases as CC

pytestmark = pytest.mark.gpu

FORCED = ('fs_A_slide', 'fs_A_drop', 'fs_B_slide', 'fs_B_drop', 'fs_hull', 'fs_overlap', 'fs_gender', 'fs_first_touch')
MIN_CONTACTS = dict(fs_first_touch=10)      # one contact per substep: the node that arrives
FREE = ('ff_A_k1', 'ff_A_k0_clamp', 'ff_B', 'ff_C_clamp', 'ff_D')


@pytest.fixture(scope='module')
def cases():
    from assistive_gym_amd import libagx
    if libagx.load().agx_device_count() <= 0:
        __import__('conftest').no_gpu()
    return CC.load_cases()


def _run(blob, states, cloth):
    """one settle(1) of len(states) environments: garments and reports after it"""
    from assistive_gym_amd.libagx import Stepper
    st = Stepper(blob, len(states))
    assert st.cloth_nodes() == cloth.shape[2]
    st.set_state(np.ascontiguousarray(states)); st.set_cloth(cloth)
    st.settle(1); st.synchronize()
    out, rep = st.get_cloth(), st.get_cloth_report()
    assert st.overflow_count() == 0
    st.close()
    return out, rep


def _say(name, m, lim):
    print('cloth kernel %-14s limit x %.3g v %.3g f %.3g | device x %.3g v %.3g f %.3g | contacts compared %d'
          % (name, lim['x'], lim['v'], lim['f'], m['x'], m['v'], m['f'], m['contacts']))


@pytest.mark.parametrize('name', FORCED)
def test_forced_substeps(cases, name):
    blob = CC.one_substep_blob(CC.case_blob(cases[name + '/recipe']))
    subs = CC.forced_substeps(cases, name)
    assert len(subs) >= 10
    nn = subs[0]['xin'].shape[0]
    out, rep = _run(blob, np.stack([s['state'] for s in subs]), np.stack([np.stack([s['xin'], s['vin']]) for s in subs]))
    res = []
    for e in range(len(subs)):
        con, heights = CC.report_contacts(rep[e], nn)
        res.append((out[e, 0], out[e, 1], con, heights))
    m, lim, bad = CC.judge_forced(cases, name, blob, res)
    _say(name, m, lim)
    assert m['contacts'] >= MIN_CONTACTS.get(name, 50)
    assert not bad, bad


@pytest.mark.parametrize('name', FREE)
def test_free_flight(cases, name):
    rec = cases[name + '/recipe']
    blob = CC.case_blob(rec)
    t = CC.tables(blob)
    x, v = CC.free_input(t, rec)
    out, rep = _run(blob, cases['state'][None], np.stack([x, v])[None])
    con, _ = CC.report_contacts(rep[0], t['nn'])
    assert not con
    m, lim, bad = CC.judge_free(cases, name, t, out[0, 0], out[0, 1])
    _say(name, m, lim)
    assert not bad, bad


def test_bit_reproducible(cases):
    """cross-patch classes are where a missing barrier shows as run-to-run variation: the 1,040-node free flight (4 cross classes) twice, and a
    forced substep of the 272-node patch as environment 0 and environment 5 of a handle whose other environments hold other substeps"""
    rec = cases['ff_C_clamp/recipe']
    blob = CC.case_blob(rec)
    x, v = CC.free_input(CC.tables(blob), rec)
    a = _run(blob, cases['state'][None], np.stack([x, v])[None])
    b = _run(blob, cases['state'][None], np.stack([x, v])[None])
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    name = 'fs_B_slide'
    blob = CC.one_substep_blob(CC.case_blob(cases[name + '/recipe']))
    subs = CC.forced_substeps(cases, name)
    order = [0, 1, 2, 3, 4, 0]
    out, rep = _run(blob, np.stack([subs[k]['state'] for k in order]), np.stack([np.stack([subs[k]['xin'], subs[k]['vin']]) for k in order]))
    assert np.array_equal(out[0].view(np.int32), out[5].view(np.int32)) and np.array_equal(rep[0].view(np.int32), rep[5].view(np.int32))
    assert not np.array_equal(out[0], out[1])
    again, rep2 = _run(blob, np.stack([subs[k]['state'] for k in order]), np.stack([np.stack([subs[k]['xin'], subs[k]['vin']]) for k in order]))
    assert np.array_equal(out.view(np.int32), again.view(np.int32)) and np.array_equal(rep.view(np.int32), rep2.view(np.int32))
