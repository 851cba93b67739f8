"""GPU box: what do the pairs of the paired solve kernel (csrc/agx_pgs_lvw.h pgs_lvw_pair) lose to their longer partner late in a rollout?
A random-policy rollout of FeedingJaco environments; at the given steps a debug launch (one environment per workgroup) leaves per environment the steps its
sweeps executed in the first substep (debug word DBG_TIME + 16, as tools/gpu_solve_streams.py reads it).  The pairs of a step launch are the environments
(2 b, 2 b + 1) of every chunk; a pair runs at least max(a, b) steps where the two alone run a and b.  The debug record holds a substep's TOTAL, not the
steps of each part of each sweep, so this is a LOWER bound of the padding (the maximum is taken per part of a sweep: tests/diag/solve_pair_study.py has
that on the emulator); random pairs of the same batch stand beside the consecutive ones.  Prints one JSON line per sampled step.
usage: python tools/gpu_solve_pair_padding.py [n_envs] [step ...]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from assistive_gym_amd import vec_env
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
at = [int(x) for x in sys.argv[2:]] or [4, 64]
env = getattr(vec_env, os.environ.get('AGX_BITS_ENV', 'FeedingJacoVecEnv'))(n, pool_size=256, seed=1001)      # AGX_BITS_ENV: another VecEnv class of the feeding variant
env.reset()
lay = env.stepper.debug_layout(); T = lay[6]
nch = env.stepper.n_chunks(); per = (n + nch - 1) // nch
g = torch.Generator(device='cuda'); g.manual_seed(1)
dbg = torch.zeros((n, lay[0]), device='cuda')
rng = np.random.RandomState(0)
for k in range(1, max(at) + 1):
    a = torch.rand((n, env.act_dim), device='cuda', generator=g) * 2 - 1
    if k not in at:
        env.step(a); continue
    env.stepper.step_dev(a, env.obs, env.reward, env.done, env.info, torch.cuda.current_stream().cuda_stream, debug=dbg)
    env.stepper.reset_done(env.pool, env.pool_size, env.done, torch.cuda.current_stream().cuda_stream)
    s = dbg[:, T + 16].cpu().numpy().astype(np.float64)
    pa, pb = [], []
    for c in range(nch):
        lo, hi = c * per, min(n, (c + 1) * per)
        m = (hi - lo) // 2
        pa += list(range(lo, lo + 2 * m, 2)); pb += list(range(lo + 1, lo + 2 * m, 2))
    pa, pb = np.array(pa), np.array(pb)
    ok = (s[pa] > 0) & (s[pb] > 0)
    lower = np.maximum(s[pa], s[pb])[ok].sum() / (0.5 * (s[pa] + s[pb])[ok].sum())
    perm = rng.permutation(n); qa, qb = perm[:n // 2], perm[n // 2:2 * (n // 2)]
    okr = (s[qa] > 0) & (s[qb] > 0)
    rnd = np.maximum(s[qa], s[qb])[okr].sum() / (0.5 * (s[qa] + s[qb])[okr].sum())
    sweeps = int(env.blob.param('NITER'))
    print(json.dumps(dict(step=k, n_envs=n, chunks=nch, pairs=int(ok.sum()), environments_off_the_wide_sweep=int((s <= 0).sum()), steps_per_sweep_mean=float(s[s > 0].mean()) / sweeps,
                          steps_per_sweep_p10_p90=[float(np.percentile(s[s > 0], 10)) / sweeps, float(np.percentile(s[s > 0], 90)) / sweeps],
                          padding_lower_bound_consecutive_pairs=float(lower), padding_lower_bound_random_pairs=float(rnd))))
