"""What does it cost to sweep TWO environments in one wavefront of the solve kernel (csrc/agx_pgs_lvw.h pgs_lvw_pair)?

Each environment of a pair list-schedules its rows on two lane groups instead of four, and every part of every sweep runs as many steps as the longer
of the two partners' lists.  On the CPU wave emulator (variant 'feeding_trace_sched', as tests/diag/solve_schedule_study.py: the DoF mask of every row and,
per sweep and part, the rows the no-op rule lets through) this script takes ENVS settled FeedingJaco states x STEPS random-policy steps and reports
  * steps per sweep of an environment alone, four rows wide (today's kernel) and two rows wide,
  * steps per sweep of every pairing of two environments, two rows wide, each part padded to the longer partner, relative to the mean of the two alone
    four rows wide: mean, p90, maximum over the pairings,
  * how many substeps have a part that does not fit 64 steps two rows wide (such a pair takes env_solve, one environment after the other).
Output: one JSON object.  usage: [ENVS=8] [STEPS=4] python tests/diag/solve_pair_study.py"""
import ctypes as C, itertools, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from assistive_gym_amd.blob import ModelBlob
from assistive_gym_amd.host.reset import make_states
from emu_lib import Emu
from solve_schedule_study import schedule

MAX_STEPS = 64


def per_sweep_steps(trace, width):
    """-> [substep][sweep] = (steps of the non-contact + normal part, steps of the friction part) of the static schedule `width` rows wide (a step is
    executed when one of its rows is active), and the number of substeps with a part of more than MAX_STEPS steps"""
    out = []; over = 0
    i = 0; n = len(trace)
    while i < n:
        assert trace[i] == -1
        R, nnc, nc = (int(x) for x in trace[i + 1:i + 4]); i += 4
        masks = []
        for r in range(R):
            lo, hi, m2 = (int(x) & 0xffffffff for x in trace[i:i + 3]); i += 3
            masks.append(lo | hi << 32 | m2 << 64)
        nA = nnc + nc
        stA, nsA = schedule(range(nA), masks, width); stF, nsF = schedule(range(nA, nA + nc), masks, width)
        over += int(nsA > MAX_STEPS or nsF > MAX_STEPS)
        sweeps = []
        while i < n and trace[i] != -1:
            a0 = (int(trace[i + 1]) & 0xffffffff) | (int(trace[i + 2]) & 0xffffffff) << 32
            a1 = (int(trace[i + 4]) & 0xffffffff) | (int(trace[i + 5]) & 0xffffffff) << 32
            td = (int(trace[i + 7]) & 0xffffffff) | (int(trace[i + 8]) & 0xffffffff) << 32
            assert trace[i] == -2 and trace[i + 3] == -3 and trace[i + 6] == -4
            i += 9
            actA = [r for r in range(nA) if ((a0 >> r) & 1 if r < 64 else (a1 >> (r - 64)) & 1)]
            actF = [nA + k for k in range(nc) if (td >> k) & 1]
            sweeps.append((len({stA[r] for r in actA}), len({stF[r] for r in actF})))
        out.append(sweeps)
    return out, over


if __name__ == '__main__':
    blob = ModelBlob.load('feeding_jaco')
    emu = Emu(blob, 'feeding_trace_sched')
    tr = (C.c_int * (1 << 24)).in_dll(emu.L, 'g_sched_trace'); cnt = C.c_int.in_dll(emu.L, 'g_sched_n')
    nenv, nstep = int(os.environ.get('ENVS', 8)), int(os.environ.get('STEPS', 4))
    st, _ = make_states(blob, nenv, seed=1001)
    rng = np.random.RandomState(0)
    w2, w4 = [], []; over2 = 0; substeps = 0
    for e in range(nenv):
        s = st[e].copy(); emu.settle(s, 25)
        cnt.value = 0
        for k in range(nstep):
            emu.step(s, rng.uniform(-1, 1, blob.act_dim).astype(np.float32))
        trace = np.ctypeslib.as_array(tr)[:cnt.value].copy()
        a, o = per_sweep_steps(trace, 2); b, _ = per_sweep_steps(trace, 4)
        w2.append(a); w4.append(b); over2 += o; substeps += len(a)
    total = lambda env: sum(x + y for sub in env for (x, y) in sub)
    sweeps = sum(len(sub) for sub in w4[0])
    alone4 = [total(e) for e in w4]; alone2 = [total(e) for e in w2]
    ratios = []
    for i, j in itertools.combinations(range(nenv), 2):
        padded = sum(max(x0, x1) + max(y0, y1) for s0, s1 in zip(w2[i], w2[j]) for (x0, y0), (x1, y1) in zip(s0, s1))
        ratios.append(padded / (0.5 * (alone4[i] + alone4[j])))
    ratios = np.array(ratios)
    print(json.dumps(dict(envs=nenv, steps=nstep, substeps=substeps, pairings=len(ratios),
                          steps_per_sweep_alone_width4=float(np.mean(alone4)) / sweeps, steps_per_sweep_alone_width2=float(np.mean(alone2)) / sweeps,
                          width2_over_width4=float(np.sum(alone2) / np.sum(alone4)),
                          paired_over_alone_width4=dict(mean=float(ratios.mean()), p90=float(np.percentile(ratios, 90)), max=float(ratios.max())),
                          substeps_over_64_steps_at_width2=over2), indent=1))
