"""The task layer (csrc/agx_task.h) on the CPU wave emulator, as raw words: for a refactor of the observation writers and the finish functions that
must not change a bit.  Steps the emulator build of every task family (dressing WITHOUT a cloth report: Emu.step passes none, so its sleeve points are zeros and its
cloth-force loop does not run -- only its rigid half, the observation, the force sum and the frame are reached here) through
  * every case of tests/golden/ref_steps.npz (113 cases, all six tasks; drinking through step_water),
  * the five placements of tests/golden/finish_spill_cases.npz (FeedingJaco, zero action),
  * the co-op flavour (blob.coop()) of one model per task and arm_manipulation_baxter (the dual-arm branch), three random-action steps each,
and keeps obs, reward, done, info, the state record after the step and the observe kernel's view of that record as uint32.  The emulator
reports divergent control flow through the assertions of emu_lib.Emu.  Run it in two trees and compare:
usage: python tests/diag/task_layer_bits.py out.npz [processes];  python tests/diag/task_layer_bits.py --compare a.npz b.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

COOP_MODELS = ('feeding_jaco', 'drinking_jaco', 'bed_bathing_sawyer', 'scratch_itch_pr2', 'arm_manipulation_sawyer', 'dressing_baxter')
SPILL = ('resting', 'shell_in', 'shell_out', 'far', 'mouth')


def _words(e, s, out, water=None):
    obs, rew, done, info = out[:4]
    r = dict(obs=obs.view(np.uint32), reward=np.array([rew], dtype=np.float32).view(np.uint32), done=np.array([done], dtype=np.uint32),
             info=info.view(np.uint32), state=s.view(np.uint32).copy(), observe=e.observe(s.copy()).view(np.uint32))
    if water is not None:
        r['water'] = water.view(np.uint32).copy()
    return r


def _start(model):
    """a start state of `model`: the first case of the reference fixture that has one (with its water), else the host sampler's"""
    from test_reference_pinned import NAMES, case
    for n in NAMES:
        c = case(n)
        if c['model'] == model:
            return c['state'].copy(), None if c['cloth'] is None else c['cloth'].copy()
    from assistive_gym_amd.blob import ModelBlob
    from assistive_gym_amd.host.reset_arm import make_states
    return make_states(ModelBlob.load(model), 1, seed=1001)[0][0].copy(), None


def run(job):
    from emu_lib import Emu
    from assistive_gym_amd.blob import ModelBlob
    kind, name = job
    out = {}
    if kind == 'ref':
        from refcases import variant_blob
        from test_reference_pinned import case
        c = case(name)
        b = variant_blob(c['model'], c['coop'], c['variant'])
        e = Emu(b)
        s = c['state'].copy()
        if c['model'].startswith('drinking'):
            w = c['cloth'].copy()
            out[''] = _words(e, s, e.step_water(s, w, c['action']), w)
        else:
            out[''] = _words(e, s, e.step(s, c['action']))
    elif kind == 'spill':
        b = ModelBlob.load('feeding_jaco')
        e = Emu(b)
        s = np.load(os.path.join(TESTS, 'golden', 'finish_spill_cases.npz'))[name].copy()
        out[''] = _words(e, s, e.step(s, np.zeros(b.act_dim, dtype=np.float32)))
    else:           # 'rollout': three random-action steps of the co-op flavour / of the dual-arm robot
        model, coop = name.split(':')[0], name.endswith(':coop')
        b = ModelBlob.load(model)
        b = b.coop() if coop else b
        e = Emu(b)
        s, w = _start(model)
        rng = np.random.RandomState(5)
        for k in range(3):
            a = rng.uniform(-1, 1, b.act_dim).astype(np.float32)
            out['/%d' % k] = _words(e, s, e.step_water(s, w, a), w) if model.startswith('drinking') else _words(e, s, e.step(s, a))
    return {'%s/%s%s/%s' % (kind, name, step, k): v for step, r in out.items() for k, v in r.items()}


def main():
    if sys.argv[1] == '--compare':
        a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
        bad = [k for k in sorted(set(a.files) | set(b.files)) if k not in a.files or k not in b.files or not np.array_equal(a[k], b[k])]
        for k in bad[:40]:
            print('differs:', k)
        print('%d arrays, %d words: %s' % (len(a.files), sum(a[k].size for k in a.files), 'IDENTICAL' if not bad else 'DIFFERENT (%d arrays)' % len(bad)))
        sys.exit(1 if bad else 0)
    from multiprocessing import Pool
    with np.load(os.path.join(TESTS, 'golden', 'ref_steps.npz')) as z:          # (the workers open the fixture themselves: a forked file handle would be shared)
        NAMES = [str(n) for n in z['names']]
    jobs = [('ref', n) for n in NAMES] + [('spill', n) for n in SPILL] + [('rollout', m + ':coop') for m in COOP_MODELS] + [('rollout', 'arm_manipulation_baxter')]
    jobs.sort(key=lambda j: not ('dressing' in j[1] or 'drinking' in j[1]))          # the long ones (40 / 20 substeps per step) first
    with Pool(int(sys.argv[2]) if len(sys.argv) > 2 else 8) as pool:
        res = {}
        for r in pool.imap_unordered(run, jobs):
            res.update(r)
    np.savez(sys.argv[1], **res)
    print('wrote %s: %d jobs, %d arrays, no divergent control flow' % (sys.argv[1], len(jobs), len(res)))


if __name__ == '__main__':
    main()
